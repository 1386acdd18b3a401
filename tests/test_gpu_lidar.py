"""LIDAR sweeps on the GPU (include/durf_lidar.h, csrc/lidar.hip, durf_amd/lidar.py) against tests/lidar_ref.py.

Rays: per component within 4 x the float32 twin's own largest error against float64 on the same case (the device's sincosf
and operation order differ from numpy's), with a floor of 2^-22 times the field's magnitude; directions == viewdirs and a
window == that slice of the sweep bit for bit; near / far / radii exact.

Returns: the quantile is ill-conditioned across an empty run, so it is held by its residual: the float64 CDF (piecewise
linear over t_vals) at the device's range lies within N 2^-23 W of q W -- any-order fp32 summation of N non-negative terms
errs by at most (N - 1) 2^-24 W, the factor 2 covers the interpolation.  That budget also has to hold the rounding of the
range itself to fp32, w_j ulp(t) / (2 width_j), which is no property of the kernel but of the planted t_vals: they run from
0.05 over N bins of 0.9 .. 1.1 / N, so it is at most 0.6 N 2^-24 w_j.  valid is exact wherever the float64 CDF at max_range
is further than the same N 2^-23 W from q W (the acc and W > 0 tests are exact comparisons of fp32 inputs); the share of
undecided rays is asserted to be at most 2 %.

Compaction and the end-to-end render are bit for bit: count, source and every column against the oracle; rgb / distance / acc
against render_layers on ops.lidar_rays' rays, range / spread / valid against ops.lidar_returns on durf_forward's outputs."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from durf_amd import lidar, ops, utils
from tests import lidar_ref as LR
from tests import test_gpu_trajectory as TT
from tests import test_layers_host as LH
from tests.test_lidar_host import read_ply

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64 = np.float32, np.float64


def _np(t):
    return t.detach().cpu().numpy()


# ---- rays -----------------------------------------------------------------------------------------------------------------
def _pose(rs):
    return np.concatenate([lidar.rodrigues(rs.normal(size=3)), rs.uniform(-20, 20, (3, 1))], 1)


def _ray_case(hw, sign, moving, seed):
    rs = np.random.default_rng(seed)
    H, W = hw
    sensor = lidar.LidarSensor(rs.uniform(-0.4, 0.3, H), W, az0=sign * math.pi, az_span=-sign * 2 * math.pi, radius_scale=1.5)
    start = _pose(rs)
    end = None
    if moving:
        om = rs.normal(size=3)
        om *= 0.3 / np.linalg.norm(om)
        end = np.concatenate([start[:, :3] @ lidar.rodrigues(om), start[:, 3:] + rs.uniform(-0.5, 0.5, (3, 1))], 1)
    return sensor, lidar.sweep_rows(start, end)[0]


RAY_FIELDS = ('origins', 'directions', 'viewdirs', 'radii', 'near', 'far')


@pytest.mark.parametrize('moving', [False, True])
@pytest.mark.parametrize('sign', [1, -1])
@pytest.mark.parametrize('hw', [(1, 1), (3, 67), (16, 64), (5, 129)])
def test_rays_against_the_float64_oracle(cuda, hw, sign, moving):
    sensor, row = _ray_case(hw, sign, moving, seed=hw[1] + 7 * moving + (sign > 0))
    near, far = 0.25, 60.0
    incl = torch.tensor(sensor.inclinations, device=cuda)
    got = dict(zip(RAY_FIELDS, ops.lidar_rays(sensor.row(), incl, row, near, far)))
    r64 = LR.rays(sensor.row(), sensor.inclinations, row, near, far)
    r32 = LR.rays(sensor.row(), sensor.inclinations, row, near, far, F32)
    n = hw[0] * hw[1]
    assert got['origins'].shape == (n, 3) and got['radii'].shape == (n,)
    assert torch.equal(got['directions'].view(torch.int32), got['viewdirs'].view(torch.int32)), 'directions == viewdirs bitwise'
    for name, scale in (('directions', 1.0), ('origins', float(np.abs(r64['origins']).max()))):
        twin = np.abs(r32[name].astype(F64) - r64[name]).max()
        tol = max(4.0 * twin, 2.0 ** -22 * scale)
        err = np.abs(_np(got[name]).astype(F64) - r64[name]).max()
        print('%s %s sign %+d moving %d: error %.3e, twin %.3e, tolerance %.3e' % (hw, name, sign, moving, err, twin, tol))
        assert err <= tol, (name, err, tol)
    assert np.abs(np.linalg.norm(_np(got['directions']).astype(F64), axis=1) - 1).max() < 1e-6
    for name in ('radii', 'near', 'far'):
        assert _np(got[name]).tobytes() == r64[name].tobytes(), name + ' is exact'
    if moving:
        assert not torch.equal(got['origins'][0], got['origins'][-1]) or n == 1
    else:
        assert (got['origins'] == got['origins'][0]).all(), 'a sensor that stands still has one origin'


@pytest.mark.parametrize('count', [1, 63, 64, 65, 255, 257])
def test_a_window_of_rays_is_that_slice_of_the_sweep(cuda, count):
    sensor, row = _ray_case((5, 129), 1, True, seed=3)
    incl = torch.tensor(sensor.inclinations, device=cuda)
    full = ops.lidar_rays(sensor.row(), incl, row, 0.1, 40.0)
    L = ops._lib.lidar_lib()
    import ctypes as C
    for first in (0, 100, 5 * 129 - count):                 # mid-row starts and ends (129 columns), and the sweep's last rays
        f = lambda c: torch.full((count + 8, c), -7.0, device=cuda)          # 8 canary rows behind the window
        bufs = [f(3), f(3), f(3), f(1), f(1), f(1)]
        ops._lib.check(L.durf_lidar_rays(ops._stream(), (C.c_float * 6)(*sensor.row().tolist()), incl.data_ptr(),
                                         (C.c_float * 18)(*row.tolist()), first, count, 0.1, 40.0, *[b.data_ptr() for b in bufs]),
                       'durf_lidar_rays')
        for b, whole, name in zip(bufs, full, RAY_FIELDS):
            want = whole.reshape(5 * 129, -1)[first:first + count]
            assert torch.equal(b[:count].view(torch.int32), want.contiguous().view(torch.int32)), (name, first, count)
            assert (b[count:] == -7.0).all(), name + ': written past the window'


# ---- returns on planted inputs ----------------------------------------------------------------------------------------------
Q, Q_LO, Q_HI, MIN_ACC = 0.5, 0.16, 0.84, 0.5


def planted(n, N, seed):
    """-> weights [n,N], t_vals [n,N+1], acc [n] float32, max_range, kinds [n]"""
    rs = np.random.default_rng(seed)
    t = (0.05 + np.concatenate([np.zeros((n, 1)), np.cumsum(rs.uniform(0.9, 1.1, (n, N)) / N, 1)], 1)).astype(F32)
    w = rs.uniform(0.01, 1.0, (n, N)).astype(F32) * rs.uniform(0.01, 2.0, (n, 1)).astype(F32)
    acc = np.where(rs.uniform(size=n) < 0.5, rs.uniform(0.0, 0.45, n), rs.uniform(0.55, 1.0, n)).astype(F32)
    acc[0] = F32(0.9)                     # (n = 1: the one ray reports a return)
    kinds = np.array(['random'] * n, dtype=object)
    max_range = F32(0.85)                # t runs to ~1.05: the median of a random ray is near 0.55, the late spikes lie beyond
    edge = (22 * N) // 64                 # the first sample of lane 22: edge - 1 is the last of the lane that owns samples before it

    def spike(j, v=0.7):
        x = np.zeros(N, F32)
        x[j] = v
        return x
    two = np.zeros(N, F32)
    two[N // 8], two[N // 2 + 3] = 0.6, 0.4          # (the median lies clearly inside the first mass)
    specials = [('spike_first', spike(0)), ('spike_last', spike(N - 1)), ('spike_lane_end', spike(edge - 1)),
                ('spike_lane_start', spike(edge)), ('two_masses', two), ('zeros', np.zeros(N, F32)),
                ('acc_under', None), ('acc_over', None), ('over_range', None), ('under_range', None)]
    for i, (kind, x) in enumerate(specials):
        r = n - 1 - i                     # from the end: n = 63 and 65 put them on either side of a workgroup's edge
        if r < 1:
            break
        kinds[r] = kind
        acc[r] = 0.9
        if x is not None:
            w[r] = x
        elif kind == 'acc_under':
            acc[r] = np.nextafter(F32(MIN_ACC), F32(0))
        elif kind == 'acc_over':
            acc[r] = np.nextafter(F32(MIN_ACC), F32(1))
        else:                             # a single spike whose bin lies clearly beyond / before max_range
            j = int(np.searchsorted(t[r], max_range * (1.02 if kind == 'over_range' else 0.95)))
            w[r] = spike(min(j, N - 1) if kind == 'over_range' else j - 2)
    return w, t, acc, max_range, kinds


def _neighbour_bins(w, j):
    pos = np.nonzero(w > 0)[0]
    k = int(np.searchsorted(pos, j))
    return int(pos[max(k - 1, 0)]), int(pos[min(k + 1, len(pos) - 1)])


@pytest.mark.parametrize('n', [1, 63, 65, 130])
@pytest.mark.parametrize('N', [32, 64, 96, 256])
def test_returns_on_planted_inputs(cuda, N, n):
    w, t, acc, max_range, kinds = planted(n, N, seed=N + n)
    rs = np.random.default_rng(5)
    o = rs.uniform(-5, 5, (n, 3)).astype(F32)
    d = rs.normal(size=(n, 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F32)
    dev = lambda a: torch.tensor(a, device=cuda)
    kw = dict(q=Q, q_lo=Q_LO, q_hi=Q_HI, min_acc=MIN_ACC, max_range=float(max_range))
    got = {k: _np(v) for k, v in ops.lidar_returns(dev(w), dev(t), dev(acc), dev(o), dev(d), **kw).items()}
    ref = LR.returns(w, t, acc, Q, Q_LO, Q_HI, MIN_ACC, float(max_range))
    tolW = N * 2.0 ** -23 * ref['W']
    undecided = np.zeros(n, bool)
    worst = 0.0
    for r in range(n):
        if ref['W'][r] > 0 and acc[r] >= F32(MIN_ACC):
            undecided[r] = abs(LR.cdf(w[r], t[r], float(max_range)) - Q * ref['W'][r]) <= tolW[r]
    share = undecided.mean()
    print('N = %d, n = %d: %d undecided rays (%.2f %%)' % (N, n, undecided.sum(), 100 * share))
    assert share <= 0.02, 'the inputs leave too many rays on the max_range threshold'
    assert not undecided[kinds != 'random'].any(), 'the planted rays are placed clearly on one side'
    assert np.array_equal(got['valid'][~undecided] != 0, ref['valid'][~undecided]), (kinds[(got['valid'] != 0) != ref['valid']])
    for kind, want in (('acc_under', False), ('acc_over', True), ('over_range', False), ('under_range', True), ('zeros', False)):
        for r in np.nonzero(kinds == kind)[0]:
            assert bool(got['valid'][r]) == want, (kind, r)
    assert (got['range'][got['valid'] == 0] == 0).all(), 'an invalid ray gets range 0'
    # the quantile by its residual, on the rays that report one
    for r in np.nonzero(got['valid'] != 0)[0]:
        x = float(got['range'][r])
        res = abs(LR.cdf(w[r], t[r], x) - Q * ref['W'][r])
        worst = max(worst, res / tolW[r])
        assert res <= tolW[r], (kinds[r], r, res, tolW[r])
        lo, hi = _neighbour_bins(w[r], int(ref['bin'][r]))
        assert t[r, lo] <= x <= t[r, hi + 1], (kinds[r], r, x, int(ref['bin'][r]))
    print('N = %d, n = %d: largest CDF residual %.3f of its tolerance' % (N, n, worst))
    has = ref['W'] > 0
    err = np.abs(got['range_mean'][has] - ref['range_mean'][has]) / ref['range_mean'][has]
    print('N = %d, n = %d: range_mean relative error %.3e (tolerance %.3e)' % (N, n, err.max() if has.any() else 0.0, N * 2.0 ** -23))
    assert (err <= N * 2.0 ** -23).all() and (got['range_mean'][~has] == 0).all()
    assert (got['spread'] >= 0).all() and (got['spread'][~has] == 0).all()
    for r in np.nonzero(np.char.startswith(kinds.astype(str), 'spike') | (kinds == 'over_range') | (kinds == 'under_range'))[0]:
        j = int(np.nonzero(w[r] > 0)[0][0])
        assert got['spread'][r] <= (t[r, j + 1] - t[r, j]) * (1 + 1e-6), (kinds[r], got['spread'][r])
        assert abs(got['spread'][r] - (Q_HI - Q_LO) * (F64(t[r, j + 1]) - F64(t[r, j]))) <= 4 * np.spacing(t[r, j + 1])
    # the point of the device's own range, in fp32: 2 ulp
    want = LR.xyz_f32(o, d, got['range'])
    assert (np.abs(got['xyz'] - want) <= 2 * np.spacing(np.abs(want))).all()
    # ... and in the sensor frame: the float64 point of the device's range, within 4 twin errors
    M = np.concatenate([lidar.rodrigues([0.3, -0.2, 0.5]), [[1.5], [-2.0], [0.25]]], 1).astype(F32)
    gs = _np(ops.lidar_returns(dev(w), dev(t), dev(acc), dev(o), dev(d), to_sensor=M, **kw)['xyz'])
    p64 = (o.astype(F64) + got['range'].astype(F64)[:, None] * d.astype(F64)) @ M[:, :3].astype(F64).T + M[:, 3].astype(F64)
    twin = np.abs(LR.xyz_f32(o, d, got['range'], M).astype(F64) - p64).max()
    tol = max(4 * twin, 2.0 ** -22 * np.abs(p64).max())
    print('N = %d, n = %d: sensor-frame error %.3e, twin %.3e, tolerance %.3e' % (N, n, np.abs(gs - p64).max(), twin, tol))
    assert np.abs(gs - p64).max() <= tol


def test_all_quantiles_of_a_ray_come_out_of_one_launch(cuda):
    """range, spread and range_mean of one call equal those of calls that ask for one plane each (nullable outputs)"""
    import ctypes as C
    w, t, acc, max_range, _ = planted(65, 96, seed=1)
    dev = lambda a: torch.tensor(a, device=cuda)
    W_, T_, A_ = dev(w), dev(t), dev(acc)
    full = ops.lidar_returns(W_, T_, A_, max_range=float(max_range))
    L = ops._lib.lidar_lib()
    for i, name in enumerate(('range', 'range_mean', 'valid', None, 'spread')):
        if name is None:
            continue
        buf = torch.full_like(full[name], 77)
        outs = [None] * 5
        outs[i] = buf.data_ptr()
        ops._lib.check(L.durf_lidar_returns(ops._stream(), 65, 96, W_.data_ptr(), T_.data_ptr(), A_.data_ptr(), None, None, None, 0.5, 0.16,
                                            0.84, 0.5, float(max_range), *outs), 'durf_lidar_returns')
        assert torch.equal(buf, full[name]), name


# ---- compaction -------------------------------------------------------------------------------------------------------------
B = ops.LIDAR_COMPACT_BLOCK


def _mask(kind, n):
    m = np.zeros(n, np.int32)
    if kind == 'all':
        m[:] = 1
    elif kind == 'alternating':
        m[::2] = 1
    elif kind == 'ends':
        m[0] = m[-1] = 1
    elif kind == 'random':
        m[:] = np.random.default_rng(n).integers(0, 2, n) * 5          # (any non-zero value is valid)
    return m


# the scan of the block sums (csrc/scan.h) takes 1024 of them per round: the last size with one round, the first with two (the
# second holds one block of one ray), and one with three
ROUND = 1024 * B


@pytest.mark.parametrize('n,kind', [(n, kind) for kind in ('all', 'none', 'alternating', 'ends', 'random')
                                    for n in (1, B - 1, B, B + 1, 3 * B + 17)] +
                         [(n, kind) for kind in ('all', 'ends', 'random') for n in (ROUND, ROUND + 1, 2 * ROUND + 257)])
def test_compaction_is_exact_and_touches_nothing_else(cuda, n, kind):
    rs = np.random.default_rng(n)
    valid = _mask(kind, n)
    xyz, rng_, rgb = rs.normal(size=(n, 3)).astype(F32), rs.uniform(1, 50, n).astype(F32), rs.uniform(0, 1, (n, 3)).astype(F32)
    dyn = rs.integers(0, 3, n).astype(np.int32)
    dev = lambda a: torch.tensor(a, device=cuda)
    points = torch.full((n, 8), -7.0, device=cuda)
    source = torch.full((n,), -9, dtype=torch.int32, device=cuda)
    p, s, count = ops.lidar_compact(dev(valid), dev(xyz), dev(rng_), dev(rgb), dev(dyn), points=points, source=source)
    assert count.is_cuda and count.dtype == torch.int32, 'the count stays on the device'
    wp, ws, m = LR.compact(valid, xyz, rng_, rgb, dyn)
    assert int(count[0]) == m
    assert _np(p[:m]).tobytes() == wp.tobytes() and _np(s[:m]).tobytes() == ws.tobytes()
    assert (p[m:] == -7.0).all() and (s[m:] == -9).all(), 'rows at and beyond count are left untouched'
    # without colours and box counts the columns are 0
    p2, s2, c2 = ops.lidar_compact(dev(valid), dev(xyz), dev(rng_))
    wp2, _, _ = LR.compact(valid, xyz, rng_)
    assert int(c2[0]) == m and _np(p2[:m]).tobytes() == wp2.tobytes() and torch.equal(s2[:m], s[:m])


def test_compaction_of_no_rays(cuda):
    e = lambda *sh, dt=torch.float32: torch.empty(*sh, dtype=dt, device=cuda)
    p, s, count = ops.lidar_compact(e(0, dt=torch.int32), e(0, 3), e(0))
    assert int(count[0]) == 0 and p.shape == (0, 8)


# ---- end to end -------------------------------------------------------------------------------------------------------------
HW, N, CHUNK = (16, 67), 32, 512
NEAR, FAR, ALPHA = 0.05, 12.0, 6.5
# the trajectory tests' scene: three boxes 3 units along the world's -z, 21 degrees apart.  The sensor sits at the origin with
# its x axis (forward) along -z and sweeps +-0.6 rad of azimuth around it: every box is in the field of view.
SENSOR_POSE = np.array([[0.0, -1.0, 0.0, 0.0], [0.0, 0.0, 1.0, 0.0], [-1.0, 0.0, 0.0, 0.0]])
OUTS = ops.LIDAR_OUTPUTS


def _sensor():
    return lidar.LidarSensor.uniform(HW[0], -0.12, 0.12, HW[1], az0=0.6, az_span=-1.2, max_range=4.0)


@pytest.fixture(scope='module')
def scene(cuda):
    model, variables, init, ext, _ = TT._scene(cuda)
    end = SENSOR_POSE.copy()
    end[:, :3] = SENSOR_POSE[:, :3] @ lidar.rodrigues([0.02, -0.01, 0.05])
    end[:, 3] += [0.05, 0.0, -0.1]
    return dict(model=model, variables=variables, init=init, ext=ext, end=end)


def _sweep(scene, times=(1.0,), chunk=CHUNK, outputs=OUTS, variables=None, ext=None, **kw):
    F = len(times)
    return lidar.render_lidar(scene['model'], scene['variables'] if variables is None else variables, _sensor(),
                              np.stack([SENSOR_POSE] * F), list(times), scene['ext'] if ext is None else ext, False, ALPHA, near=NEAR,
                              far=FAR, pose_end=np.stack([scene['end']] * F), chunk=chunk, min_acc=0.3, outputs=outputs, **kw)


def _bits(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    assert torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)), what


@pytest.mark.parametrize('mask', [None, [1, 0, 1]])
def test_a_sweep_is_the_renderer_on_the_sensors_rays_and_the_return_model_behind_it(cuda, scene, mask):
    model, variables, init, ext = scene['model'], scene['variables'], scene['init'], scene['ext']
    en = None if mask is None else torch.tensor(mask, dtype=torch.int32, device=cuda)
    res = _sweep(scene, box_enable=en)
    n = HW[0] * HW[1]
    assert sorted(res) == sorted(OUTS + ('box_poses',))
    assert res['range'].shape == (1,) + HW and res['xyz'].shape == (1,) + HW + (3,) and res['valid'].dtype == torch.int32
    assert torch.equal(res['box_poses'][0], init[1])
    sensor = _sensor()
    row = lidar.sweep_rows(SENSOR_POSE, scene['end'])[0]
    o, d, v, r, nr, fr = ops.lidar_rays(sensor.row(), torch.tensor(sensor.inclinations, device=cuda), row, NEAR, FAR)
    rays = utils.BoxRays(*[x.reshape(HW + (-1,)) for x in (o, d, v, r, torch.ones(n, device=cuda), nr, fr)])
    want = model.render_layers(variables, rays, init, ext, 1, False, ALPHA, chunk=CHUNK, box_enable=en, pose=res['box_poses'][0],
                               layers=('instance',))
    for name in ('rgb', 'distance', 'acc'):
        _bits(res[name][0], want[name], name + ' against render_layers')
    inst = want['instance'].reshape(-1)
    assert not (inst == -2).any()
    seen = set(int(k) for k in inst[inst >= 0].unique())
    assert seen == ({0, 1, 2} if mask is None else {0, 2}), 'the boxes are in the sweep\'s field of view: %s' % seen
    assert torch.equal(res['dynamic'][0].reshape(-1) > 0, inst >= 0)
    # the return model on durf_forward's last level, chunk by chunk (2 x 512 and a remainder of 48)
    flat = utils.namedtuple_map(lambda x: x.reshape(n, -1), rays)
    for i in range(0, n, CHUNK):
        ck = utils.namedtuple_map(lambda x: x[i:i + CHUNK].contiguous(), flat)
        outs = model.apply_one_call(variables, 0, ck, init, ext, 1, False, False, False, ALPHA, box_enable=en, pose=res['box_poses'][0])
        rgb, depth, acc, weights, t_vals = outs[-1][:5]
        ret = ops.lidar_returns(weights, t_vals, acc.reshape(-1), ck.origins, ck.directions, q=0.5, q_lo=0.16, q_hi=0.84, min_acc=0.3,
                                max_range=4.0)
        sl = slice(i, i + CHUNK)
        for name in ('range', 'range_mean', 'spread', 'valid', 'xyz'):
            _bits(res[name][0].reshape(n, -1)[sl], ret[name].reshape(ret[name].shape[0], -1), '%s of the chunk at %d' % (name, i))
        _bits(res['dynamic'][0].reshape(n, -1)[sl], outs[-1][8].reshape(-1, 1), 'dynamic == dyn_mask')
        _bits(res['distance'][0].reshape(n, -1)[sl], depth.reshape(-1, 1), 'distance of the chunk')
    assert 0 < int(res['valid'].sum()) <= n
    # one chunk for the whole sweep gives the same bits
    whole = _sweep(scene, chunk=HW[0] * HW[1], box_enable=en)
    for name in OUTS:
        _bits(whole[name], res[name], name + ': chunk 1072 against chunk 512')


def test_all_boxes_off_is_the_model_without_boxes(cuda, scene):
    off = _sweep(scene, box_enable=[0, 0, 0])
    sub = LH.reduce_variables(scene['variables'], [])
    bare = _sweep(scene, variables=sub, ext=scene['ext'][:0])
    assert bare['box_poses'].shape == (1, 0, 6)
    for name in OUTS:
        _bits(off[name], bare[name], name)
    assert int(off['dynamic'].sum()) == 0 and not torch.equal(off['rgb'], _sweep(scene, outputs=('rgb',))['rgb'])


def test_fractional_times_take_the_trajectory_calls_poses(cuda, scene):
    times = (0.25, 1.5)
    res = _sweep(scene, times=times, outputs=('range', 'rgb'))
    want = scene['model'].render_trajectory(scene['variables'], None, list(times), scene['ext'], False, ALPHA, near=NEAR, far=FAR,
                                            outputs=())['poses']
    _bits(res['box_poses'], want, 'box_poses')
    assert res['range'].shape == (2,) + HW and sorted(res) == ['box_poses', 'range', 'rgb']
    for f, t in enumerate(times):
        one = _sweep(scene, times=(t,), outputs=('range', 'rgb'))
        _bits(res['range'][f], one['range'][0], 'sweep %d of two against the sweep alone' % f)
        _bits(res['rgb'][f], one['rgb'][0], 'rgb of sweep %d' % f)
    assert not torch.equal(res['rgb'][0], res['rgb'][1]), 'the boxes moved'


def test_an_undersized_workspace_is_refused_before_any_launch(cuda, scene, monkeypatch):
    good = {k: v.clone() for k, v in _sweep(scene).items()}
    need = int(ops._lib.lidar_lib().durf_render_lidar_workspace_bytes(CHUNK, N, 3, 2))
    real = ops._workspace
    assert ops.dispatch_seen() != set(), 'a sweep that runs is seen'
    # (the box poses come from the trajectory call, which sizes a workspace of its own: only the sweep's is cut short)
    monkeypatch.setattr(ops, '_workspace', lambda dev, nb: real(dev, nb)[:nb - 256] if nb == need else real(dev, nb))
    ops.dispatch_reset()
    with pytest.raises(ops._lib.DurfError, match=r'durf_render_lidar: workspace of %d bytes.* = %d' % (need - 256, need)):
        _sweep(scene)
    assert ops.dispatch_seen() == set() and ops.layer_log_seen() <= {'TRAJ_POSE'}, 'refused before any launch of the sweep'
    monkeypatch.setattr(ops, '_workspace', real)
    with pytest.raises(ValueError, match='unknown outputs'):
        _sweep(scene, outputs=('depth',))
    again = _sweep(scene)
    for k in good:
        _bits(again[k], good[k], k)
    ops.dispatch_reset()


def test_point_cloud_of_a_sweep(cuda, scene):
    res = _sweep(scene)
    points, count = lidar.point_cloud(res, 0)
    n = HW[0] * HW[1]
    g = lambda k: _np(res[k][0]).reshape(n, -1)
    wp, _, m = LR.compact(g('valid'), g('xyz'), g('range'), g('rgb'), g('dynamic'))
    assert int(count[0]) == m > 0 and _np(points[:m]).tobytes() == wp.tobytes()
    assert (wp[:, 3] > 0).all() and (wp[:, 3] <= 4.0).all()


# ---- the command ----------------------------------------------------------------------------------------------------------
def test_render_lidar_command_on_the_synthetic_scene(cuda, tmp_path):
    out = str(tmp_path / 'sweeps')
    cmd = [sys.executable, '-m', 'durf_amd.render_lidar', '--synthetic', '--eval_dir', out, '--min_acc', '0.05', '--disable_box', '1',
           '--gin_param', 'MipNerfModel.num_samples = 32', '--gin_param', 'MipNerfModel.no_pose_opt = True',
           '--gin_param', 'MipNerfModel.no_yaw_opt = True']
    p = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)      # a fresh child process
    assert p.returncode == 0, p.stdout.decode()
    H, W = 16, 128
    assert sorted(os.listdir(out)) == sorted('%s_%04d.%s' % (a, f, b) for f in (0, 1) for a, b in
                                             (('range', 'npy'), ('range', 'ppm'), ('sweep', 'ply')))
    total = 0
    for f in (0, 1):
        rng = np.load(os.path.join(out, 'range_%04d.npy' % f))
        assert rng.shape == (H, W) and rng.dtype == np.float32 and np.isfinite(rng).all()
        blob = open(os.path.join(out, 'range_%04d.ppm' % f), 'rb').read()
        header = b'P6\n%d %d\n255\n' % (W, H)
        assert blob[:len(header)] == header and len(blob) == len(header) + H * W * 3
        v, m = read_ply(os.path.join(out, 'sweep_%04d.ply' % f))
        assert m == int((rng > 0).sum()), 'the PLY holds the valid returns: the rays with a range'
        assert np.array_equal(np.sort(v['range']), np.sort(rng[rng > 0]))
        total += m
    assert total > 0 and ('%d returns' % total).encode() in p.stdout
