"""The camera row on the host (durf_amd/camera.py) against the header's macros, its one refusal, and the oracle's projection
(tests/camera_ref.py).  CPU only."""
import numpy as np
import pytest

from durf_amd import camera, ops, raygen, trajectory
from tests import camera_ref as C

F64 = np.float64


def _keys(n):
    rng = np.random.default_rng(5)
    return np.stack([C.look_at(rng.uniform(-3, 3, 3), rng.uniform(-1, 1, 3)) for _ in range(n)])


def test_rows_have_the_layout_the_macros_state():
    assert (ops.CAM_FLOATS, ops.CAM_FOCAL, ops.CAM_PPX, ops.CAM_PPY, ops.CAM_H, ops.CAM_W) == (C.FLOATS, C.FOCAL, C.PPX, C.PPY, C.H, C.W)
    assert trajectory.camera_rows is camera.rows and raygen.camera_row is camera.row
    keys = _keys(2)
    rows = camera.rows(keys, 51.5, (17.25, 11.5), 24, 32)
    assert rows.shape == (2, ops.CAM_FLOATS) and rows.dtype == np.float32
    for i in range(2):
        assert np.array_equal(rows[i], camera.row(keys[i], 51.5, (17.25, 11.5), 24, 32))
        assert np.array_equal(rows[i], C.row(keys[i], 51.5, 17.25, 11.5, 24, 32)), 'the oracle builds the same row'
        assert np.array_equal(rows[i, :ops.CAM_FOCAL].reshape(3, 4), keys[i].astype(np.float32))
        assert (rows[i, ops.CAM_FOCAL], rows[i, ops.CAM_PPX], rows[i, ops.CAM_PPY], rows[i, ops.CAM_H], rows[i, ops.CAM_W]) == (51.5, 17.25, 11.5, 24, 32)
        assert camera.size(rows[i]) == (24, 32) and camera.intrinsics(rows[i]) == (51.5, 17.25, 11.5, 24.0, 32.0)
        assert np.array_equal(camera.c2w(rows[i]), keys[i].astype(np.float32))
    td = raygen.TimestepData(keys, [51.5] * 2, [(17.25, 11.5)] * 2, [24] * 2, [32] * 2, device='cpu')
    assert np.array_equal(rows, td.cams), 'the table durf_gen_batch takes'


def test_as_rows_is_the_one_refusal():
    rows = camera.rows(_keys(3), 40.0, (15.5, 11.5), 24, 32)
    got, h, w = camera.as_rows(rows.astype(np.float64).tolist(), 'here')
    assert got.dtype == np.float32 and got.flags['C_CONTIGUOUS'] and np.array_equal(got, rows) and (h, w) == (24, 32)
    assert camera.as_rows(rows[1], 'here')[0].shape == (1, ops.CAM_FLOATS)
    with pytest.raises(ValueError, match=r'here: cams of shape \(3, 17\), expected \[1,17\]'):          # (a caller that takes one camera)
        camera.as_rows(rows, 'here', frames=1)
    with pytest.raises(ValueError, match=r'here: cams of shape \(3, 16\)'):
        camera.as_rows(rows[:, :16], 'here')
    with pytest.raises(ValueError, match='here: .*no camera rows'):
        camera.as_rows(rows[:0], 'here')
    mixed = rows.copy()
    mixed[2, ops.CAM_W] = 33
    with pytest.raises(ValueError, match='here: the cameras of one call share one frame size'):
        camera.as_rows(mixed, 'here')
    assert camera.as_rows(mixed, 'here', one_size=False)[1:] == (24, 32)           # (the library refuses those itself)
    with pytest.raises(ValueError, match=r'there: cams of shape \(3, 17\), expected \[2,17\]'):
        camera.check_shape(rows.shape, 'there', frames=2)


def random_camera(rng, h=48, w=64):
    eye = rng.uniform(-2, 2, 3)
    c2w = C.look_at(eye, eye + rng.normal(size=3), up=rng.normal(size=3))
    # (a float64 row: rounded to fp32 the rotation block is orthonormal to 1e-7 only, and its transpose no inverse to 1e-9)
    return np.concatenate([c2w.reshape(-1), [rng.uniform(30, 90), rng.uniform(20, 40), rng.uniform(15, 30), h, w]])


def test_projection_inverts_the_ray_generator():
    rng = np.random.default_rng(0)
    for _ in range(20):
        cam = random_camera(rng)
        for _ in range(10):
            x, y = float(rng.integers(0, 64)), float(rng.integers(0, 48))
            o, d = C.rays(cam, x, y)
            t = rng.uniform(0.1, 30.0)
            xy, z = C.project(cam[None], (o + t * d)[None], F64)
            assert abs(xy[0, 0] - x) < 1e-9 and abs(xy[0, 1] - y) < 1e-9, (xy, x, y)
            assert abs(z[0] - t) < 1e-9              # the camera-space direction has z = -1: depth is t


def test_float32_projection_stays_by_the_float64_one():
    # 48 points on the rays of random pixels of a 48 x 64 camera, depth 1 .. 20.  Measured worst float32 - float64 difference
    # of camera_ref.project on this input: 6.383853609293055e-06 pixels, 1.8632076432822942e-06 in depth; the bounds are twice that.
    rng = np.random.default_rng(7)
    cam = C.row(C.look_at((1.5, -2.0, 0.75), (0.0, 0.0, 0.0), up=(0.0, 0.0, 1.0)), 52.0, 31.5, 23.5, 48, 64)
    x, y, t = rng.uniform(0, 63, 48), rng.uniform(0, 47, 48), rng.uniform(1.0, 20.0, 48)
    o, d = C.rays(cam, x, y)
    P = (o + t[:, None] * d).astype(np.float32)
    a, za = C.project(cam[None], P[None], np.float32)
    b, zb = C.project(cam[None], P[None], F64)
    assert a.dtype == np.float32 and za.dtype == np.float32
    dxy, dz = float(np.abs(a.astype(F64) - b).max()), float(np.abs(za.astype(F64) - zb).max())
    print('float32 - float64: %r pixels, %r depth' % (dxy, dz))
    assert dxy <= 2 * 6.383853609293055e-06 and dz <= 2 * 1.8632076432822942e-06
    assert np.abs(b[0, :, 0] - x).max() < 1e-4 and np.abs(b[0, :, 1] - y).max() < 1e-4         # (P was rounded to float32)
