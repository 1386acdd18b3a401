"""Motion between frames without a device: the three-way agreement of include/durf_flow.h, durf_amd/_flow_sigs.py and
libdurf_flow.so's symbol table, every refusal of the entry points (they need no device and are read from libdurf_hip.so's
durf_last_error, which names the offending value), the workspace sizer, tests/flow_ref.py on closed forms, and the host side
of durf_amd/flow.py (.flo files, the pairs)."""
import ctypes as C
import re

import numpy as np
import pytest

from durf_amd import _lib, flow, ops
from tests import flow_ref as FR

ENTRY = {'durf_flow_points', 'durf_flow_warp', 'durf_flow_consistency', 'durf_flow_color', 'durf_render_flow',
         'durf_render_flow_workspace_bytes'}
FAKE = 4096              # a non-null, 256-byte aligned address no refused call may touch


def _err():
    return _lib.lib().durf_last_error().decode()


def _cam(h=5, w=13, focal=20.0, o=(0.0, 0.0, 0.0)):
    c2w = np.concatenate([np.eye(3), np.asarray(o, np.float64).reshape(3, 1)], 1)
    return FR.camera_row(c2w, focal, w / 2.0 - 0.25, h / 2.0 - 0.5, h, w)


def _row(cam):
    return (C.c_float * 17)(*np.asarray(cam, np.float32).tolist())


# ---- the library ----------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_bound_and_exported_by_a_library_of_their_own():
    # (header == table == symbol table: tests/test_satellites_host.py; the constants and the scratch macros against the header:
    # tests/test_headers_host.py)
    assert ENTRY == set(_lib.flow_symbols())
    assert len(ops.FLOW_CONS_FIELDS) == ops.FLOW_CONS_FLOATS and FR.CONS_SPAN == ops.FLOW_CONS_SPAN and FR.WHEEL == ops.FLOW_WHEEL
    assert [ops.flow_pose_floats(K) for K in (0, 1, 16)] == [0, 24, 384]
    S = ops.FLOW_CONS_SPAN
    assert [ops.flow_cons_scratch(2, m) for m in (1, S, S + 1)] == [6, 6, 12]


def test_points_refusals_and_zero_work():
    L = _lib.flow_lib()
    cam = _row(_cam())

    def call(n=4, first=0, K=1, znear=1e-2, tol=1e-3, outs=(FAKE,) + (None,) * 6, cams=(cam, cam), hit=FAKE, o_s=FAKE):
        return L.durf_flow_points(None, n, first, K, o_s, FAKE, hit, FAKE, FAKE, cams[0], cams[1], FAKE, FAKE, FAKE, 1, 0.5, znear, tol,
                                  FAKE, *outs)
    assert call(n=0) == 0 and call(n=0, first=65) == 0                          # n == 0: nothing to do
    for kw, text in ((dict(n=-1), 'n = -1'), (dict(first=-2), 'first = -2'), (dict(K=ops.MAX_OBJ + 1), 'K = %d' % (ops.MAX_OBJ + 1)),
                     (dict(K=-1), 'K = -1'), (dict(znear=0.0), 'znear = 0'), (dict(znear=-1.5), 'znear = -1.5'),
                     (dict(znear=float('nan')), 'znear = nan'), (dict(tol=-0.25), 'inside_tol = -0.25'),
                     (dict(n=66), 'n = 66, h w = 65'), (dict(first=64, n=2), 'first = 64, n = 2'),
                     (dict(outs=(None,) * 7), 'at least one output'), (dict(cams=(None, cam)), 'two camera rows'),
                     (dict(hit=None), 'hit, pose_a, pose_b, ext and pose_scratch for K = 1'), (dict(o_s=None), 'origins_s, dirs_s'),
                     (dict(outs=(FAKE + 4,) + (None,) * 6), '8-byte aligned'), (dict(cams=(_row(_cam(w=0)), cam)), 'w = 0')):
        assert call(**kw) != 0 and text in _err(), (kw, _err())


def test_warp_consistency_and_color_refusals():
    L = _lib.flow_lib()
    warp = lambda n=4, h=3, w=5, Cc=3, rel=0.02, ab=0.0, outs=(FAKE, FAKE), tg=FAKE: L.durf_flow_warp(None, n, h, w, Cc, tg, FAKE, FAKE, FAKE,
                                                                                              rel, ab, *outs)
    assert warp(n=0) == 0
    for kw, text in ((dict(n=-3), 'n = -3'), (dict(h=0), 'h = 0'), (dict(w=-1), 'w = -1'), (dict(h=65536, w=65536), 'h = 65536, w = 65536'),
                     (dict(Cc=2), 'C = 2'), (dict(Cc=4), 'C = 4'), (dict(rel=-0.5), 'occ_rel = -0.5'), (dict(ab=-1.0), 'occ_abs = -1'),
                     (dict(outs=(None, None)), 'at least one output'), (dict(tg=None), 'target, valid, img_b and zcam_b')):
        assert warp(**kw) != 0 and text in _err(), (kw, _err())
    cons = lambda P=1, m=8, Cc=3, out=FAKE: L.durf_flow_consistency(None, P, m, Cc, FAKE, FAKE, FAKE, out, FAKE)
    assert cons(P=0) == 0
    for kw, text in ((dict(P=-1), 'P = -1'), (dict(P=65536), 'P = 65536'), (dict(m=0), 'm = 0'), (dict(Cc=2), 'C = 2'),
                     (dict(out=None), 'warped, img_a, mask, out and scratch')):
        assert cons(**kw) != 0 and text in _err(), (kw, _err())
    color = lambda n=4, mm=1.0, outs=(FAKE, None), fl=FAKE: L.durf_flow_color(None, n, fl, mm, *outs)
    assert color(n=0) == 0
    for kw, text in ((dict(n=-1), 'n = -1'), (dict(mm=0.0), 'max_mag = 0'), (dict(mm=-2.0), 'max_mag = -2'), (dict(mm=float('nan')), 'max_mag = nan'),
                     (dict(outs=(None, None)), 'at least one output'), (dict(fl=None), 'flow is given'), (dict(fl=FAKE + 4), '8-byte aligned')):
        assert color(**kw) != 0 and text in _err(), (kw, _err())


def test_render_flow_refusals_need_no_device():
    L = _lib.flow_lib()
    need = int(L.durf_render_flow_workspace_bytes(64, 3))
    # one chunk of rays (12 floats), of origins_s / dirs_s (6), of hit (K ints) and zo, and the pose table
    per_ray = (12 + 6 + 3 + 1) * 4
    assert 64 * per_ray + ops.flow_pose_floats(3) * 4 <= need <= 64 * per_ray + ops.flow_pose_floats(3) * 4 + 12 * 256, need
    F = 3
    cams = np.stack([_cam()] * F)
    rows = lambda c: (C.c_float * c.size)(*c.reshape(-1).tolist())
    ints = lambda p: (C.c_int * len(p))(*p)

    def call(F=F, K=3, P=2, pairs=(0, 1, 1, 2), cams=cams, znear=1e-2, tol=1e-3, chunk=64, outs=(FAKE,) + (None,) * 6, ws=FAKE,
             nbytes=need, dist=FAKE):
        return L.durf_render_flow(None, F, K, rows(cams), FAKE, FAKE, None, dist, FAKE, P, ints(pairs), 0.0, 10.0, chunk, 1, 0.5, znear,
                                  tol, *outs, ws, nbytes)
    odd = cams.copy()
    odd[2, 16] = 14
    cases = [(dict(F=0), 'F = 0'), (dict(F=-2), 'F = -2'), (dict(P=0), 'P = 0'), (dict(P=-1), 'P = -1'),
             (dict(pairs=(0, 1, 1, 3)), 'pair 1 names frame 3 outside [0, 3)'), (dict(pairs=(-1, 1, 1, 2)), 'pair 0 names frame -1'),
             (dict(cams=odd), 'frames of different sizes: frame 2 is 5 x 14, frame 0 is 5 x 13'),
             (dict(K=ops.MAX_OBJ + 1), 'K = %d' % (ops.MAX_OBJ + 1)), (dict(znear=0.0), 'znear = 0'), (dict(znear=-3.0), 'znear = -3'),
             (dict(tol=-1.0), 'inside_tol = -1'), (dict(chunk=0), 'chunk = 0'), (dict(chunk=-8), 'chunk = -8'),
             (dict(outs=(None,) * 7), 'at least one output'), (dict(dist=None), 'distance, acc'), (dict(ws=FAKE + 64), 'aligned to 256'),
             (dict(ws=None), 'aligned to 256')]
    for kw, text in cases:
        assert call(**kw) != 0 and text in _err(), (kw, _err())
    assert call(nbytes=need - 256) != 0
    assert re.search(r'durf_render_flow: workspace of %d bytes, durf_render_flow_workspace_bytes\(64, 3\) = %d' % (need - 256, need), _err()), _err()


def test_workspace_depends_on_the_chunk_and_the_boxes_alone():
    """the sizer takes neither F nor the image (there is nothing to be independent of) and a remainder chunk fits a full one's"""
    f = _lib.flow_lib().durf_render_flow_workspace_bytes
    assert f.argtypes == [C.c_int, C.c_int]
    for K in (0, 1, 3, 16):
        sizes = [int(f(B, K)) for B in (1, 48, 63, 64, 65, 512, 1072, 8192)]
        assert sizes == sorted(sizes) and len(set(sizes)) > 4 and all(s % 256 == 0 for s in sizes), (K, sizes)
    assert int(f(64, 16)) > int(f(64, 1)) >= int(f(64, 0))


# ---- the oracle on closed forms ---------------------------------------------------------------------------------------------
H, W, FOCAL = 9, 16, 20.0
POSE = np.array([[0.4, 0.1, -4.0, 0.0, 0.0, 0.0], [-1.2, -0.3, -5.0, 0.0, 0.3, 0.0]])
EXT = np.array([[0.5, 0.5, 0.5], [0.4, 0.6, 0.4]])
WALL = 8.0


def _flow(cam_a, cam_b, pose_a, pose_b, ext=EXT, skin=0.05, **kw):
    s = FR.plant_scene(cam_a, pose_a, ext, WALL, skin)
    return s, FR.points(s['origins_s'], s['dirs_s'], s['hit'], s['t'], s['acc'], cam_a, cam_b, pose_a if len(pose_a) else None,
                        pose_b if len(pose_b) else None, ext, **kw)


def test_the_analytic_scene_shows_boxes_and_wall():
    s, r = _flow(_cam(H, W, FOCAL), _cam(H, W, FOCAL), POSE, POSE)
    nh = s['hit'].sum(1)
    assert (nh == 1).sum() >= 8 and (nh == 0).sum() >= 8 and set(np.unique(r['moving'])) >= {-1, 0, 1} and r['valid'].all()


def test_identical_cameras_and_poses_give_zero_flow():
    cam = _cam(H, W, FOCAL, o=(0.1, -0.2, 0.3))
    _, r = _flow(cam, cam, POSE, POSE)
    assert r['valid'].all() and np.abs(r['flow']).max() < 1e-5 and np.abs(r['scene_flow']).max() == 0
    # (the planted rays are rounded to fp32, so a pixel's point projects back onto it to ~1e-6 pixels, not to 1e-15)
    x, y = np.arange(H * W) % W, np.arange(H * W) // W
    assert np.abs(r['target'][:, 0] - x).max() < 1e-5 and np.abs(r['target'][:, 1] - y).max() < 1e-5
    assert np.abs(r['zcam'] - r['target'][:, 2]).max() == 0


def test_a_camera_moving_along_its_axis_gives_radial_flow():
    delta = 1.5
    cam_a, cam_b = _cam(H, W, FOCAL), _cam(H, W, FOCAL, o=(0.0, 0.0, -delta))          # the camera looks down -z
    none = np.zeros((0, 6))
    _, r = _flow(cam_a, cam_b, none, none, ext=np.zeros((0, 3)))
    x, y = np.arange(H * W) % W, np.arange(H * W) // W
    ppx, ppy = float(cam_a[13]), float(cam_a[14])
    scale = delta / (WALL - delta)                 # a wall at depth D seen from D - delta: the picture grows by D / (D - delta)
    want = np.stack([(x - ppx) * scale, (y - ppy) * scale], 1)
    assert r['valid'].all() and (r['moving'] == -1).all()
    assert np.abs(r['flow'] - want).max() < 1e-5
    mag = np.linalg.norm(r['flow'], axis=1)
    assert np.abs(mag - np.hypot(x - ppx, y - ppy) * scale).max() < 1e-5
    assert np.abs(r['target'][:, 2] - (WALL - delta)).max() < 1e-5 and np.abs(r['zcam'] - WALL).max() < 1e-5
    assert np.abs(r['scene_flow']).max() == 0


def test_a_translated_box_carries_its_pixels_and_nothing_else():
    cam = _cam(H, W, FOCAL)
    d = np.array([0.3, -0.2, 0.5])
    pose_b = POSE.copy()
    pose_b[0, :3] += d
    s, r = _flow(cam, cam, POSE, pose_b)
    ride0, ride1 = r['moving'] == 0, r['moving'] == 1
    assert ride0.sum() >= 4 and ride1.sum() >= 4 and r['valid'].all()
    assert np.abs(r['scene_flow'][ride0] - d).max() < 1e-6
    assert np.abs(r['scene_flow'][~ride0]).max() == 0, 'the box that stood still and the wall do not move'
    assert (np.abs(r['flow'][~ride0]).max() < 1e-5) and np.abs(r['flow'][ride0]).min() > 0.1
    # a point outside the grown box is scenery seen through it: planted a long way behind the box
    t = s['t'].copy()
    t[ride0] += 3.0
    far = FR.points(s['origins_s'], s['dirs_s'], s['hit'], t, s['acc'], cam, cam, POSE, pose_b, EXT)
    assert (far['moving'][ride0] == -1).all() and np.abs(far['scene_flow'][ride0]).max() == 0
    # two boxes on one ray, too little weight, a target behind the camera: invalid, NaN everywhere
    hit2 = s['hit'].copy()
    hit2[0] = 1
    acc = s['acc'].copy()
    acc[1] = 0.49
    bad = FR.points(s['origins_s'], s['dirs_s'], hit2, s['t'], acc, cam, _cam(H, W, FOCAL, o=(0, 0, -9.0)), POSE, pose_b, EXT)
    assert bad['valid'][:2].tolist() == [0, 0] and bad['moving'][:2].tolist() == [-2, -2] and not bad['valid'].any()
    for k in ('flow', 'scene_flow', 'xyz', 'target', 'zcam'):
        assert np.isnan(bad[k]).all(), k


def test_forward_then_backward_flow_returns_to_the_start():
    """a wall and a box face parallel to the picture, moved so that both shift by whole pixels: the forward target is a pixel of
    the other frame, whose backward flow must lead back"""
    focal = 16.0
    front = 4.0 - 0.5                               # the planted surface of box 0: its front face (no skin: a plane)
    cam_a = _cam(H, W, focal)
    cam_b = _cam(H, W, focal, o=(2.0 * WALL / focal, 0.0, 0.0))                      # the wall shifts by -2 pixels
    pose_a = POSE[:1].copy()
    pose_b = pose_a.copy()
    pose_b[0, 0] += 2.0 * WALL / focal + 3.0 * front / focal                         # the box by +3
    ext = EXT[:1]
    sa, fwd = _flow(cam_a, cam_b, pose_a, pose_b, ext=ext, skin=0.0)
    sb, bwd = _flow(cam_b, cam_a, pose_b, pose_a, ext=ext, skin=0.0)
    own = FR.points(sb['origins_s'], sb['dirs_s'], sb['hit'], sb['t'], sb['acc'], cam_b, cam_b, pose_b, pose_b, ext)['zcam']
    ride = fwd['moving'] == 0
    assert ride.sum() >= 4 and np.abs(fwd['flow'][ride] - [3.0, 0.0]).max() < 1e-4 and np.abs(fwd['flow'][~ride] - [-2.0, 0.0]).max() < 1e-4
    _, vis = FR.warp(fwd['target'], fwd['valid'], np.zeros((H, W, 1)), own.reshape(H, W), occ_rel=0.01)
    vis = vis != 0
    assert 0.5 * H * W < vis.sum() < H * W, 'most pixels come back; those that leave the picture or slide behind the box do not'
    q = np.rint(fwd['target'][vis, 1]).astype(int) * W + np.rint(fwd['target'][vis, 0]).astype(int)
    assert np.abs(fwd['flow'][vis] + bwd['flow'][q]).max() < 1e-4
    hidden = ~vis & (np.rint(fwd['target'][:, 0]) >= 0) & (np.rint(fwd['target'][:, 0]) <= W - 1)
    assert hidden.any() and not ride[hidden].any(), 'wall pixels that land behind the moved box are masked out'


def test_warp_oracle_reproduces_pixels_and_interpolates():
    rs = np.random.default_rng(0)
    h, w = 3, 5
    img = rs.uniform(0, 1, (h, w, 3)).astype(np.float32)
    z = np.full((h, w), 2.0, np.float32)
    tg = np.array([[1, 2, 2.0], [4, 0, 2.0], [1.5, 0.5, 2.0], [4.0001, 0, 2.0], [-0.0, 0, 2.0], [np.nan, 0, 2.0], [2, 1, 2.5], [2, 1, 1.0]])
    wp, mask = FR.warp(tg, np.ones(len(tg), np.int32), img, z, occ_rel=0.1)
    assert mask.tolist() == [1, 1, 1, 0, 1, 0, 0, 1]
    assert wp[0].astype(np.float32).tobytes() == img[2, 1].tobytes() and wp[1].astype(np.float32).tobytes() == img[0, 4].tobytes()
    assert np.allclose(wp[2], img[:2, 1:3].astype(np.float64).mean((0, 1))) and np.isnan(wp[3]).all() and np.isnan(wp[6]).all()
    wp32, mask32 = FR.warp(tg, np.ones(len(tg), np.int32), img, z, occ_rel=0.1, dt=np.float32)
    assert wp32.dtype == np.float32 and mask32.tolist() == mask.tolist() and wp32[0].tobytes() == img[2, 1].tobytes()
    one, m1 = FR.warp(np.array([[0.0, 0.0, 1.0]]), [1], img[:1, :1], z[:1, :1])
    assert m1.tolist() == [1] and one[0].astype(np.float32).tobytes() == img[0, 0].tobytes()


def test_consistency_oracle():
    a = np.zeros((2, 4, 3), np.float32)
    wp = a.copy()
    wp[0, :, :] = 0.5
    wp[0, 3] = np.nan
    mask = np.array([[1, 1, 0, 0], [0, 0, 0, 0]])
    out = FR.consistency(wp, a, mask)
    assert out[0, :3].tolist() == [2.0, 1.5, 3.0] and abs(out[0, 3] - (-10 * np.log10(0.25))) < 1e-12 and np.isnan(out[1, 3])
    assert FR.consistency(a, a, np.ones((2, 4)))[0].tolist() == [4.0, 0.0, 0.0, np.inf]


def test_colour_wheel_and_picture_oracle():
    wheel = FR.colorwheel()
    assert wheel.shape == (55, 3) and wheel[0].tolist() == [255, 0, 0], 'the wheel starts at pure red'
    assert wheel[15].tolist() == [255, 255, 0] and wheel[21].tolist() == [0, 255, 0] and wheel[25].tolist() == [0, 255, 255]
    assert wheel[36].tolist() == [0, 0, 255] and wheel[49].tolist() == [255, 0, 255] and wheel[54].tolist() == [255, 0, 43]
    assert wheel.min() == 0 and wheel.max() == 255 and (np.abs(np.diff(wheel, axis=0)).sum(1) <= 64).all(), 'neighbours are close'
    rgb, _ = FR.color(np.array([[0.0, 0.0], [1.0, 0.0], [2.0, 0.0], [np.nan, 1.0], [1.0, np.inf], [0.5, 0.0]]), 1.0)
    assert rgb[0].tolist() == [1, 1, 1], 'no motion is white'
    assert np.allclose(rgb[1], [1, 0, 0]) and np.allclose(rgb[2], [0.75, 0, 0]), 'motion to the right is red; beyond max_mag, dimmed'
    assert np.allclose(rgb[5], [1, 0.5, 0.5]), 'half the magnitude is half way to white'
    assert rgb[3].tolist() == [0, 0, 0] and rgb[4].tolist() == [0, 0, 0], 'invalid flow is black'
    ang = np.linspace(-np.pi, np.pi, 721)
    fl = np.stack([np.cos(ang), np.sin(ang)], 1) * 0.7
    c64, c32 = FR.color(fl, 1.0)[0], FR.color(fl, 1.0, np.float32)[0]
    assert c32.dtype == np.float32 and 0 < np.abs(c32 - c64).max() < 1e-4
    # continuous in the direction but for the wheel's one seam, where its last entry (255, 0, 43) meets pure red: motion to the
    # right, ang = 0, samples 359 | 360
    step = np.abs(np.diff(c64, axis=0)).max(1)
    assert np.delete(step, 359).max() < 0.02 and abs(step[359] - 0.7 * 43 / 255) < 0.02


# ---- durf_amd/flow.py -----------------------------------------------------------------------------------------------------
def test_flo_round_trip(tmp_path):
    rs = np.random.default_rng(5)
    h, w = 4, 7
    fl = rs.normal(0, 3, (h, w, 2)).astype(np.float32)
    valid = np.ones((h, w), np.int32)
    valid[1, 2] = 0
    fl[2, 3] = np.nan
    path = str(tmp_path / 'a.flo')
    flow.write_flo(path, fl, valid)
    blob = open(path, 'rb').read()
    assert blob[:4] == b'PIEH' and np.frombuffer(blob[4:12], '<i4').tolist() == [w, h] and len(blob) == 12 + h * w * 8
    raw = np.frombuffer(blob, '<f4', offset=12).reshape(h, w, 2)
    assert (raw[1, 2] == np.float32(1e10)).all() and (raw[2, 3] == np.float32(1e10)).all() and raw[0, 1].tobytes() == fl[0, 1].tobytes()
    got, gv = flow.read_flo(path)
    want_valid = valid.copy()
    want_valid[2, 3] = 0
    assert np.array_equal(gv, want_valid) and got.dtype == np.float32
    assert got[gv != 0].tobytes() == fl[want_valid != 0].tobytes() and np.isnan(got[gv == 0]).all()
    flow.write_flo(path, fl[:, :, :], None)
    assert flow.read_flo(path)[1].sum() == h * w - 1
    open(path, 'wb').write(b'PIEX' + blob[4:])
    with pytest.raises(ValueError, match='not a .flo'):
        flow.read_flo(path)
    with pytest.raises(ValueError, match=r'\[h,w,2\]'):
        flow.write_flo(path, fl[0])


def test_pairs_and_required_outputs():
    assert flow.default_pairs(4).tolist() == [[0, 1], [1, 2], [2, 3]]
    assert flow.default_pairs(3, backward=True).tolist() == [[0, 1], [1, 2], [1, 0], [2, 1]]
    assert flow.default_pairs(1).shape == (0, 2)
    with pytest.raises(ValueError, match=r"needs the outputs \['acc', 'poses'\]"):
        flow.render_flow(dict(distance=None), np.zeros((2, 17)), None, near=0.0, far=1.0)
    with pytest.raises(ValueError, match='warp needs'):
        flow.warp(dict(target=None), None, None)
    assert 'READ BACK' in flow.flow_to_color.__doc__
