"""LIDAR sweeps without a device: the three-way agreement of include/durf_lidar.h, durf_amd/_lidar_sigs.py and
libdurf_lidar.so's symbol table, every refusal of the four entry points (they need no device and are read from
libdurf_hip.so's durf_last_error), the zero-work calls, tests/lidar_ref.py on its own, and the host side of durf_amd/lidar.py
(sweep_motion, write_ply, the sensor)."""
import ctypes as C
import math
import re

import numpy as np
import pytest

from durf_amd import _lib, lidar, ops
from tests import lidar_ref as LR

ENTRY = {'durf_lidar_rays', 'durf_lidar_returns', 'durf_lidar_compact', 'durf_render_lidar', 'durf_render_lidar_workspace_bytes'}


def _err():
    return _lib.lib().durf_last_error().decode()


# ---- the library ----------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_bound_and_exported_by_a_library_of_their_own():
    # (header == table == symbol table: tests/test_satellites_host.py; the constants and DURF_LIDAR_COMPACT_SCRATCH against the
    # header: tests/test_headers_host.py)
    assert ENTRY == set(_lib.lidar_symbols())
    assert len(ops.LIDAR_POINT_FIELDS) == ops.LIDAR_POINT_FLOATS
    B = ops.LIDAR_COMPACT_BLOCK
    assert [ops.lidar_compact_scratch(n) for n in (0, 1, B, B + 1)] == [1, 2, 2, 3]


SENSOR = (C.c_float * 6)(4, 8, math.pi, -2 * math.pi, 1.0, 75.0)
SWEEP = (C.c_float * 18)(1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0)
FAKE = 4096              # a non-null, 256-byte aligned address no refused call may touch


def _sensor(H=4, W=8):
    return (C.c_float * 6)(H, W, math.pi, -2 * math.pi, 1.0, 75.0)


def test_rays_refusals_and_zero_work():
    L = _lib.lidar_lib()
    call = lambda sensor, first, count, incl=FAKE: L.durf_lidar_rays(None, sensor, incl, SWEEP, first, count, 0.0, 10.0, FAKE, FAKE, FAKE,
                                                                   FAKE, FAKE, FAKE)
    assert call(SENSOR, 0, 0) == 0 and call(SENSOR, 32, 0) == 0                  # count == 0: nothing to do
    for sensor, first, count, text in ((_sensor(H=0), 0, 1, 'H > 0'), (_sensor(W=0), 0, 1, 'W > 0'), (_sensor(H=-3), 0, 1, 'H > 0'),
                                       (SENSOR, 0, 33, 'inside the sweep'), (SENSOR, -1, 2, 'inside the sweep'),
                                       (SENSOR, 30, 3, 'inside the sweep')):
        assert call(sensor, first, count) != 0 and text in _err(), (text, _err())
    assert call(SENSOR, 0, 4, None) != 0 and 'inclination table' in _err()
    assert L.durf_lidar_rays(None, None, FAKE, SWEEP, 0, 1, 0.0, 10.0, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE) != 0 and 'sensor row' in _err()
    assert L.durf_lidar_rays(None, SENSOR, FAKE, SWEEP, 0, 1, 0.0, 10.0, FAKE, FAKE, None, FAKE, FAKE, FAKE) != 0 and 'six ray fields' in _err()


def test_returns_refusals_and_zero_work():
    L = _lib.lidar_lib()

    def call(n=4, N=64, q=0.5, lo=0.16, hi=0.84, outs=(FAKE,) * 5, w=FAKE, od=(FAKE, FAKE)):
        return L.durf_lidar_returns(None, n, N, w, FAKE, FAKE, od[0], od[1], None, q, lo, hi, 0.5, 75.0, *outs)
    assert call(n=0) == 0
    for kw, text in ((dict(N=0), 'multiple of 32'), (dict(N=48), 'multiple of 32'), (dict(N=288), 'multiple of 32'),
                     (dict(N=16), 'multiple of 32'), (dict(q=0.0), '0 < q < 1'), (dict(q=1.0), '0 < q < 1'),
                     (dict(q=float('nan')), '0 < q < 1'), (dict(lo=0.5, hi=0.5), 'q_lo < q_hi'), (dict(lo=0.9, hi=0.1), 'q_lo < q_hi'),
                     (dict(lo=0.0), 'q_lo < q_hi'), (dict(hi=1.0), 'q_lo < q_hi'), (dict(n=-1), 'n >= 0'),
                     (dict(outs=(None,) * 5), 'at least one output'), (dict(w=None), 'weights, t_vals and acc'),
                     (dict(od=(None, None)), 'xyz needs origins')):
        assert call(**kw) != 0 and text in _err(), (kw, _err())
    assert call(n=0, N=48) != 0, 'an unsupported N is refused whatever the work'


def test_compact_refusals():
    L = _lib.lidar_lib()
    call = lambda n, count=FAKE, scratch=FAKE, points=FAKE, valid=FAKE: L.durf_lidar_compact(None, n, valid, FAKE, FAKE, None, None,
                                                                                         points, FAKE, count, scratch)
    for kw, text in ((dict(n=-1), '0 <= n < 2^27'), (dict(n=1 << 27), '0 <= n < 2^27'), (dict(n=5, count=None), 'count and scratch'),
                     (dict(n=5, scratch=None), 'count and scratch'), (dict(n=5, valid=None), 'valid, xyz, range'),
                     (dict(n=5, points=FAKE + 8), '16-byte aligned')):
        assert call(**kw) != 0 and text in _err(), (kw, _err())


def _forward_args(N=32, K=3, L=2):
    a = ops.ForwardArgs()
    a.N, a.K, a.num_levels, a.B = N, K, L, 64
    a.density_bias, a.resample_padding = -1.0, 0.01
    return a


def test_render_lidar_refusals_need_no_device():
    L = _lib.lidar_lib()
    need = int(L.durf_render_lidar_workspace_bytes(64, 32, 3, 2))
    fwd = int(_lib.lib().durf_forward_workspace_bytes(64, 32, 3))
    # durf_forward's workspace plus one chunk of rays (12 floats) and of per-level outputs (3 + 1 + 1 + 4 N + 1 floats), dyn, zo
    per_ray = 12 * 4 + 2 * (5 + 4 * 32 + 1) * 4 + 8
    assert fwd + 64 * per_ray <= need <= fwd + 64 * per_ray + 40 * 256, (need, fwd)
    assert need == int(L.durf_render_lidar_workspace_bytes(64, 32, 3, 2))

    def call(a=None, F=1, sensor=SENSOR, q=0.5, lo=0.16, hi=0.84, outs=None, ws=FAKE, nbytes=need, chunk=64, args_null=False):
        a = _forward_args() if a is None else a
        outs = (FAKE,) + (None,) * 8 if outs is None else outs
        return L.durf_render_lidar(None, None if args_null else C.byref(a), None, F, sensor, FAKE, SWEEP, FAKE, 0.0, 10.0, chunk, q, lo,
                                   hi, 0.5, *outs, ws, nbytes)
    cases = [(dict(F=0), 'F > 0'), (dict(F=-2), 'F > 0'), (dict(sensor=_sensor(H=0)), 'H > 0'), (dict(sensor=_sensor(W=0)), 'W > 0'),
             (dict(sensor=_sensor(W=-5)), 'W > 0'), (dict(q=0.0), '0 < q < 1'), (dict(q=1.0), '0 < q < 1'), (dict(q=1.5), '0 < q < 1'),
             (dict(lo=0.84, hi=0.16), 'q_lo < q_hi'), (dict(lo=0.3, hi=0.3), 'q_lo < q_hi'),
             (dict(a=_forward_args(K=ops.MAX_OBJ + 1)), 'DURF_MAX_OBJ'), (dict(a=_forward_args(N=48)), 'multiple of 32'),
             (dict(a=_forward_args(N=512)), 'multiple of 32'), (dict(a=_forward_args(L=5)), 'num_levels'),
             (dict(outs=(None,) * 9), 'at least one output'), (dict(chunk=0), 'chunk > 0'), (dict(args_null=True), 'arguments'),
             (dict(ws=FAKE + 64), 'aligned to 256'), (dict(ws=None), 'aligned to 256')]
    for kw, text in cases:
        assert call(**kw) != 0 and text in _err(), (kw, _err())
    assert call(nbytes=need - 256) != 0
    assert re.search(r'durf_render_lidar: workspace of %d bytes, durf_render_lidar_workspace_bytes\(64, 32, 3, 2\) = %d' % (need - 256, need),
                     _err()), _err()
    # the workspace grows with the chunk, not with the sweep: the sizer does not even take H, W or F
    assert int(L.durf_render_lidar_workspace_bytes(128, 32, 3, 2)) > need


def test_forward_workspace_is_monotone_in_the_chunk():
    """a remainder chunk runs in the workspace carved for a full one"""
    f = _lib.lib().durf_forward_workspace_bytes
    for N, K in ((32, 0), (32, 3), (128, 3)):
        sizes = [int(f(B, N, K)) for B in (1, 48, 63, 64, 65, 512, 1072, 8192)]
        assert sizes == sorted(sizes), (N, K, sizes)


# ---- the oracle on its own ------------------------------------------------------------------------------------------------
def _random_ray(rng, N, zeros=0.3):
    w = rng.uniform(0, 1, N) * (rng.uniform(0, 1, N) > zeros)
    t = np.cumsum(rng.uniform(0.05, 1.0, N + 1))
    return w, t


def test_quantile_is_monotone_and_inverts_the_cdf():
    rng = np.random.default_rng(0)
    for N in (32, 96):
        for _ in range(20):
            w, t = _random_ray(rng, N)
            qs = np.linspace(0.01, 0.99, 41)
            r = np.array([LR.quantile(w, t, p)[0] for p in qs])
            assert (np.diff(r) >= 0).all()
            for p, x in zip(qs, r):
                assert abs(LR.cdf(w, t, x) - p * w.sum()) <= 1e-12 * w.sum()
                j = LR.quantile(w, t, p)[1]
                assert w[j] > 0 and t[j] <= x <= t[j + 1]


def test_quantile_limits():
    rng = np.random.default_rng(1)
    w, t = _random_ray(rng, 64)
    w[50:] = 0.0
    last = int(np.nonzero(w > 0)[0][-1])
    r, j = LR.quantile(w, t, 1.0)
    assert j == last and abs(r - t[last + 1]) <= 1e-12, 'q -> 1 reaches the end of the last non-empty bin'
    assert abs(LR.quantile(w, t, 1.0 - 1e-13)[0] - t[last + 1]) <= 1e-9
    for j0 in (0, 17, 63):                       # a single non-zero weight: a point inside that bin, at fraction p of it
        w1 = np.zeros(64)
        w1[j0] = 0.37
        for p in (0.01, 0.5, 0.99):
            r, j = LR.quantile(w1, t, p)
            assert j == j0 and abs(r - (t[j0] + p * (t[j0 + 1] - t[j0]))) <= 1e-12
    assert LR.quantile(np.zeros(32), t[:33], 0.5) == (0.0, -1)
    # two masses with a run of exact zeros between them: the median stays on one of the two surfaces, the mean flies between them
    w2 = np.zeros(64)
    w2[10], w2[40] = 0.6, 0.4
    out = LR.returns(w2[None], t[None], [1.0])
    assert t[10] <= out['range'][0] <= t[11] and t[11] < out['range_mean'][0] < t[40]
    assert out['spread'][0] >= t[40] - t[11]


def test_returns_validity_and_points():
    rng = np.random.default_rng(2)
    n, N = 6, 32
    w = rng.uniform(0.1, 1, (n, N))
    t = np.cumsum(rng.uniform(0.1, 1, (n, N + 1)), 1)
    w[1] = 0.0
    acc = np.array([1.0, 1.0, 0.49, 0.5, 1.0, 1.0])
    raw = LR.returns(w, t, acc)['range_raw']
    out = LR.returns(w, t, acc, max_range=raw[4] - 1e-9, origins=np.ones((n, 3)), directions=np.eye(3)[[0, 1, 2, 0, 1, 2]])
    assert out['valid'].tolist() == [raw[0] <= raw[4] - 1e-9, False, False, raw[3] <= raw[4] - 1e-9, False, raw[5] <= raw[4] - 1e-9]
    assert (out['range'][~out['valid']] == 0).all() and (out['spread'] >= 0).all() and out['spread'][1] == 0
    assert np.allclose(out['xyz'][~out['valid']], 1.0), 'an invalid ray sits at its origin'
    M = np.concatenate([np.eye(3)[[1, 2, 0]], [[1.0], [2.0], [3.0]]], 1)
    got = LR.returns(w, t, acc, origins=np.ones((n, 3)), directions=np.eye(3)[[0, 1, 2, 0, 1, 2]], to_sensor=M)['xyz']
    want = LR.returns(w, t, acc, origins=np.ones((n, 3)), directions=np.eye(3)[[0, 1, 2, 0, 1, 2]])['xyz']
    assert np.allclose(got, want[:, [1, 2, 0]] + [1.0, 2.0, 3.0])
    assert np.abs(LR.xyz_f32(np.ones((n, 3)), np.eye(3)[[0, 1, 2, 0, 1, 2]], want[:, 0] * 0 + 2.5, M) - ([1, 2, 3] + np.array(
        [[1, 1, 3.5], [3.5, 1, 1], [1, 3.5, 1]] * 2))).max() == 0


def test_compaction_oracle():
    n = 9
    xyz, rng_, rgb, dyn = np.arange(3 * n).reshape(n, 3), np.arange(n) + 0.5, np.ones((n, 3)) * 0.25, np.arange(n) % 3
    pts, src, m = LR.compact(np.ones(n, np.int32), xyz, rng_, rgb, dyn)
    assert m == n and src.tolist() == list(range(n)) and pts.shape == (n, 8) and pts.dtype == np.float32
    assert pts[4].tolist() == [12, 13, 14, 4.5, 0.25, 0.25, 0.25, 1]
    pts, src, m = LR.compact(np.zeros(n, np.int32), xyz, rng_, rgb, dyn)
    assert m == 0 and src.shape == (0,) and pts.shape == (0, 8)
    pts, src, m = LR.compact(np.array([0, 1, 0, 0, 1, 1, 0, 0, 7]), xyz, rng_)
    assert m == 4 and src.tolist() == [1, 4, 5, 8] and (pts[:, 4:] == 0).all() and pts[:, 3].tolist() == [1.5, 4.5, 5.5, 8.5]


def test_ray_oracle_and_its_float32_twin():
    sensor = lidar.LidarSensor.uniform(5, math.radians(-20), math.radians(10), 129, az0=math.pi, az_span=-2 * math.pi, radius_scale=2.0)
    pose = np.concatenate([lidar.rodrigues([0.2, -0.4, 1.0]), [[1.0], [-2.0], [0.5]]], 1)
    end = np.concatenate([pose[:, :3] @ lidar.rodrigues([0.1, 0.2, -0.2]), [[1.3], [-2.1], [0.6]]], 1)
    row = lidar.sweep_rows(pose, end)[0]
    r64 = LR.rays(sensor.row(), sensor.inclinations, row, 0.1, 50.0)
    r32 = LR.rays(sensor.row(), sensor.inclinations, row, 0.1, 50.0, np.float32)
    assert r64['directions'].dtype == np.float64 and r32['directions'].dtype == np.float32
    assert np.abs(np.linalg.norm(r64['directions'], axis=1) - 1).max() < 1e-6          # (the pose row is rounded to fp32)
    assert 0 < np.abs(r32['directions'] - r64['directions']).max() < 2e-6
    assert np.abs(r32['origins'] - r64['origins']).max() < 1e-6
    # column 0 starts next to az0, half a step in; the first and last column's poses are half a step inside the sweep
    d = r64['directions'].reshape(5, 129, 3)
    s0 = 0.5 / 129
    want = pose[:, :3].astype(np.float32).astype(np.float64) @ lidar.rodrigues(s0 * row[12:15].astype(np.float64)) @ np.array(
        [math.cos(sensor.inclinations[2]) * math.cos(math.pi - s0 * 2 * math.pi),
         math.cos(sensor.inclinations[2]) * math.sin(math.pi - s0 * 2 * math.pi), math.sin(sensor.inclinations[2])])
    assert np.abs(d[2, 0] - want).max() < 1e-7
    # (the row holds az_span rounded to fp32: the rule is evaluated on that)
    assert abs(r64['radii'][0] / (2.0 * 2 * math.pi / 129 * 2 / math.sqrt(12)) - 1) < 2e-7 and (r64['near'] == np.float32(0.1)).all()
    # a sensor that stands still: one origin, directions that depend on the pose's rotation alone
    still = LR.rays(sensor.row(), sensor.inclinations, lidar.sweep_rows(pose)[0], 0.1, 50.0)
    assert (still['origins'] == still['origins'][0]).all()


# ---- durf_amd/lidar.py ----------------------------------------------------------------------------------------------------
def test_sweep_motion_round_trip():
    rng = np.random.default_rng(3)
    for i in range(200):
        axis = rng.normal(size=3)
        axis /= np.linalg.norm(axis)
        angle = math.radians(170.0) * (1.0 if i < 5 else rng.uniform(0, 1)) * (0.0 if i == 5 else 1.0)
        Rs = lidar.rodrigues(rng.normal(size=3))
        start = np.concatenate([Rs, rng.normal(size=(3, 1))], 1)
        end = np.concatenate([Rs @ lidar.rodrigues(axis * angle), rng.normal(size=(3, 1))], 1)
        om, dp = lidar.sweep_motion(start, end)
        assert np.abs(start[:, :3] @ lidar.rodrigues(om) - end[:, :3]).max() <= 1e-12, (i, angle)
        assert np.abs(start[:, 3] + dp - end[:, 3]).max() <= 1e-15
        assert abs(np.linalg.norm(om) - angle) <= 1e-10
    rows = lidar.sweep_rows(np.stack([start, start]))
    assert rows.shape == (2, 18) and rows.dtype == np.float32 and (rows[:, 12:] == 0).all()
    with pytest.raises(ValueError, match='pose_end'):
        lidar.sweep_rows(np.stack([start, start]), end)


def read_ply(path):
    """a reader by hand: the header line by line, then the packed little-endian records"""
    blob = open(path, 'rb').read()
    head, body = blob.split(b'end_header\n', 1)
    lines = head.decode('ascii').split('\n')
    assert lines[0] == 'ply' and lines[1] == 'format binary_little_endian 1.0'
    m = int(lines[2].split()[2])
    props = [ln.split()[1:] for ln in lines[3:] if ln.startswith('property')]
    assert props == [['float', 'x'], ['float', 'y'], ['float', 'z'], ['uchar', 'red'], ['uchar', 'green'], ['uchar', 'blue'],
                     ['float', 'range'], ['uchar', 'dynamic']]
    rec = np.dtype([(n, '<f4' if t == 'float' else 'u1') for t, n in props])
    assert rec.itemsize == 20 and len(body) == m * 20
    return np.frombuffer(body, rec), m


def test_write_ply_round_trip(tmp_path):
    rng = np.random.default_rng(4)
    n, m = 11, 7
    pts = rng.normal(size=(n, 8)).astype(np.float32)
    pts[:, 4:7] = rng.uniform(0, 1, (n, 3))
    pts[0, 4:7] = [0.0, 1.0, 1.5]                                    # (clipped)
    pts[:, 7] = rng.integers(0, 3, n)
    path = str(tmp_path / 'a.ply')
    assert lidar.write_ply(path, pts, np.array([m], np.int32)) == m
    v, got = read_ply(path)
    assert got == m
    for k, name in enumerate(('x', 'y', 'z')):
        assert v[name].tobytes() == pts[:m, k].tobytes()
    assert v['range'].tobytes() == pts[:m, 3].tobytes()
    assert np.array_equal(np.stack([v['red'], v['green'], v['blue']], 1), np.rint(np.clip(pts[:m, 4:7], 0, 1) * 255).astype(np.uint8))
    assert v['red'][0] == 0 and v['blue'][0] == 255 and np.array_equal(v['dynamic'], pts[:m, 7].astype(np.uint8))
    assert lidar.write_ply(path, pts, 0) == 0 and read_ply(path)[1] == 0


def test_sensors():
    s = lidar.LidarSensor.waymo_top()
    assert s.height == 64 and s.width == 2650 and s.inclinations.shape == (64,) and s.inclinations.dtype == np.float32
    assert abs(s.inclinations[0] - math.radians(2.4)) < 1e-7 and abs(s.inclinations[-1] - math.radians(-17.6)) < 1e-7
    assert (np.diff(s.inclinations) < 0).all() and s.az0 == math.pi and s.az_span == -2 * math.pi and s.max_range == 75.0
    row = s.row()
    assert row.shape == (6,) and row.dtype == np.float32 and row[:2].tolist() == [64, 2650] and row[4] == 1.0
    u = lidar.LidarSensor.uniform(3, -0.2, 0.1, 67, az0=0.0, az_span=1.0)
    assert np.allclose(u.inclinations, [0.1, -0.05, -0.2]) and u.row()[1] == 67
    assert 'calibration' in lidar.LidarSensor.waymo_top.__doc__
