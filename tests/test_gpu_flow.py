"""Motion between frames on the GPU (include/durf_flow.h, csrc/flow.hip, durf_amd/flow.py) against tests/flow_ref.py.

The yardstick for every float output is the float64 oracle; the allowance is what fp32 in the header's order costs, measured
and not guessed: e = max |twin32 - oracle64| over the test's own planted inputs, on the CPU, and the device may differ from the
oracle by 4 e plus 4 ulp of the value (its sinf / cosf / atan2f and divisions round differently from numpy's; nothing else is
covered).  The e this file was written with, per output, over every case of the parametrised tests below:

    durf_flow_points (point_cases)      flow 4.8e-06   scene_flow 9.9e-07   xyz 1.0e-06   target 4.7e-06   zcam 1.3e-06
    durf_flow_warp (WARP_CASES)         warped 1.1e-07
    durf_flow_color (COLOR_CASES)       rgb 1.3e-06

Each test recomputes its e and fails if it exceeds twice the recorded value (RECORDED), so the yardstick cannot drift silently.
Integer outputs, masks and the placement of NaN are exact; the planted inputs keep every decision (inside / outside a box,
in front of / behind znear, visible / occluded) at least 1e-2 relative away from its boundary, asserted on the oracle's own
numbers, so that no pixel needs to be excluded from a comparison.

durf_flow_consistency's bound is derived, not measured: see test_consistency_against_the_float64_sum."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from durf_amd import flow, ops, raygen
from tests import flow_ref as FR
from tests import test_gpu_trajectory as TT

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64 = np.float32, np.float64
RECORDED = dict(flow=4.8e-06, scene_flow=9.9e-07, xyz=1.0e-06, target=4.7e-06, zcam=1.3e-06, warped=1.1e-07, rgb=1.3e-06)
FLOAT_OUTS = ('flow', 'scene_flow', 'xyz', 'target', 'zcam')


def _np(t):
    return t.detach().cpu().numpy()


def _ulp(x):
    """the spacing of float32 at |x| (of the smallest normal below it)"""
    return np.spacing(np.maximum(np.abs(np.asarray(x, F64)), 2.0 ** -126).astype(F32)).astype(F64)


def _held(got, want, e, what):
    """got (device, fp32) against want (float64 oracle): NaN in the same places, elsewhere within 4 e + 4 ulp of the value"""
    got, want = np.asarray(got, F64), np.asarray(want, F64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(np.isnan(got), np.isnan(want)), what + ': NaN placement'
    ok = ~np.isnan(want)
    if ok.any():
        err, tol = np.abs(got[ok] - want[ok]), 4.0 * e + 4.0 * _ulp(want[ok])
        worst = int(np.argmax(err - tol))
        print('%s: max error %.3e, e %.3e, tolerance there %.3e' % (what, err.max(), e, tol[worst]))
        assert (err <= tol).all(), (what, err[worst], tol[worst])


def _twin_error(r64, r32, names):
    out = {}
    for k in names:
        a, b = np.asarray(r64[k], F64), np.asarray(r32[k], F64)
        assert np.array_equal(np.isnan(a), np.isnan(b)), k + ': the twin puts NaN elsewhere'
        ok = ~np.isnan(a)
        out[k] = float(np.abs(a[ok] - b[ok]).max()) if ok.any() else 0.0
    return out


# ---- durf_flow_points on planted inputs -------------------------------------------------------------------------------------
PH, PW, FIRST = 24, 37, 50                     # the window starts mid-row: 37 does not divide 50
MIN_ACC, ZNEAR, TOL = 0.5, 0.05, 1e-3
POINT_NS, POINT_KS = (1, 63, 64, 65, 257), (0, 1, 3, 16)


def _rot(v):
    return FR.aa2matrix(v).T


def planted_points(n, K, normalise, seed=None):
    """-> dict of the arguments of durf_flow_points as fp32 / int32 arrays, and kinds [n].  The test builds origins_s, dirs_s,
    hit and t itself: no silhouette decision is shared with the code under test."""
    rs = np.random.default_rng(1000 * n + 10 * K + normalise if seed is None else seed)
    cam_a = FR.camera_row(np.concatenate([_rot(rs.normal(0, 0.05, 3)), rs.normal(0, 0.2, (3, 1))], 1), 30.0, PW / 2.0 + 0.25, PH / 2.0 - 0.5, PH, PW)
    cam_b = FR.camera_row(np.concatenate([_rot(rs.normal(0, 0.05, 3)), rs.normal(0, 0.2, (3, 1))], 1), 31.0, PW / 2.0 - 0.5, PH / 2.0 + 0.25, PH, PW)
    pose_a = np.concatenate([rs.uniform(-2, 2, (K, 2)), rs.uniform(-8, -5, (K, 1)), rs.normal(0, 0.6, (K, 3))], 1)
    pose_b = pose_a + np.concatenate([rs.normal(0, 0.3, (K, 3)), rs.normal(0, 0.1, (K, 3))], 1)
    if K:
        pose_a[0, 3:] = 0.0                    # the clamp of aa2matrix: a box that is not rotated
    ext = rs.uniform(0.3, 0.8, (K, 3))
    kinds = rs.choice(['static', 'ride', 'through'] if K else ['static'], n).astype(object)
    specials = (['ride', 'two'] if K >= 2 else ['ride'] if K else ['static']) + ['behind', 'inf', 'static'] + (['through'] if K else [])
    for i, kind in enumerate(specials[:n]):      # from the end: n = 63 and 65 put them on either side of a wave's edge
        kinds[n - 1 - i] = kind
    o_s, d_s, hit = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros((n, K), np.int32)
    tt = rs.uniform(1.0, 5.0, n)
    acc = np.where(rs.uniform(size=n) < 0.3, rs.uniform(0.05, 0.45, n), rs.uniform(0.55, 1.0, n))
    Ra, oa = cam_a[:12].reshape(3, 4)[:, :3].astype(F64), cam_a[:12].reshape(3, 4)[:, 3].astype(F64)
    for i in range(n):
        kind = kinds[i]
        if kind in ('static', 'behind', 'inf'):
            d = Ra @ np.array([rs.uniform(-0.5, 0.5), rs.uniform(-0.3, 0.3), -1.0])
            o_s[i], d_s[i] = oa, d
            tt[i] = rs.uniform(3.0, 9.0) * (-1.0 if kind == 'behind' else 1.0)
        else:
            k = int(rs.integers(K))
            hit[i, k] = 1
            u = rs.uniform(-0.97, 0.97, 3)       # inside: at least 3 % of the half extent from every face
            if kind == 'through':
                j = int(rs.integers(3))
                u[j] = rs.choice([-1.0, 1.0]) * rs.uniform(1.05, 3.0)
            if kind == 'two':
                hit[i, (k + 1 + int(rs.integers(K - 1))) % K] = 1
            d = rs.normal(size=3)
            d /= np.linalg.norm(d)
            # the point is seen from camera a: make sure it also lies in front of camera b by keeping both near the origin
            o_s[i], d_s[i] = u * ext[k] - tt[i] * d, d
    t = tt * acc if normalise else tt
    t[kinds == 'inf'] = np.inf
    acc[(kinds != 'static') & (kinds != 'ride') & (kinds != 'through')] = 0.9        # invalid for its own reason, not for its weight
    f = lambda a: np.ascontiguousarray(a, F32)
    return dict(origins_s=f(o_s), dirs_s=f(d_s), hit=hit, t=f(t), acc=f(acc), cam_a=cam_a, cam_b=cam_b, pose_a=f(pose_a), pose_b=f(pose_b),
                ext=f(ext), kinds=kinds)


def _oracle_points(p, normalise, dt=F64):
    K = p['pose_a'].shape[0]
    return FR.points(p['origins_s'], p['dirs_s'], p['hit'], p['t'], p['acc'], p['cam_a'], p['cam_b'], p['pose_a'] if K else None,
                     p['pose_b'] if K else None, p['ext'], first=FIRST, normalise=normalise, min_acc=MIN_ACC, znear=ZNEAR, inside_tol=TOL,
                     dt=dt)


def point_cases():
    return [(n, K, nm) for n in POINT_NS for K in POINT_KS for nm in (0, 1)]


_POINT_E = {}


def point_yardstick():
    """e per float output over every planted case, computed once (CPU, ~1 s) and shared"""
    if not _POINT_E:
        e = dict.fromkeys(FLOAT_OUTS, 0.0)
        for n, K, nm in point_cases():
            p = planted_points(n, K, nm)
            one = _twin_error(_oracle_points(p, nm), _oracle_points(p, nm, F32), FLOAT_OUTS)
            e = {k: max(e[k], one[k]) for k in e}
        _POINT_E.update(e)
    return _POINT_E


def _device_points(p, cuda, normalise, outputs=ops.FLOW_OUTPUTS):
    d = lambda a: torch.tensor(a, device=cuda)
    return ops.flow_points(d(p['origins_s']), d(p['dirs_s']), d(p['hit']), d(p['t']), d(p['acc']), p['cam_a'], p['cam_b'], d(p['pose_a']),
                           d(p['pose_b']), d(p['ext']), first=FIRST, normalise=bool(normalise), min_acc=MIN_ACC, znear=ZNEAR,
                           inside_tol=TOL, outputs=outputs)


def test_the_point_yardstick_has_not_drifted():
    e = point_yardstick()
    print('e over the planted cases: ' + '   '.join('%s %.2e' % kv for kv in e.items()))
    for k in FLOAT_OUTS:
        assert 0 < e[k] <= 2.0 * RECORDED[k], (k, e[k], RECORDED[k])


@pytest.mark.parametrize('normalise', [0, 1])
@pytest.mark.parametrize('K', POINT_KS)
@pytest.mark.parametrize('n', POINT_NS)
def test_points_against_the_float64_oracle(cuda, n, K, normalise):
    p = planted_points(n, K, normalise)
    want = _oracle_points(p, normalise)
    # the preconditions that make the classification unambiguous, on the oracle's numbers
    one = (want['nh'] == 1) & np.isfinite(want['P']).all(1)
    if one.any():
        k = np.argmax(p['hit'][one] != 0, 1)
        rel = np.abs(np.abs(want['P'][one]) / (p['ext'][k].astype(F64) * (1 + TOL)) - 1.0)
        assert rel.min() >= 1e-2, 'a planted point within 1e-2 ext of its box\'s boundary'
    zb = want['z_b'][np.isfinite(want['z_b'])]
    assert ((zb >= 2 * ZNEAR) | (zb <= 0.5 * ZNEAR)).all() and (np.abs(p['acc'] - MIN_ACC) > 0.04).all()
    got = {k: _np(v) for k, v in _device_points(p, cuda, normalise).items()}
    assert got['flow'].shape == (n, 2) and got['moving'].dtype == np.int32
    assert np.array_equal(got['valid'], want['valid']) and np.array_equal(got['moving'], want['moving'])
    kinds = p['kinds']
    for kind, mv in (('two', -2), ('behind', -2), ('inf', -2)):
        assert (got['moving'][kinds == kind] == mv).all(), kind
    live = want['valid'] != 0
    assert (got['moving'][live & (kinds == 'ride')] >= 0).all() and (got['moving'][live & (kinds != 'ride')] == -1).all()
    if n >= 63:
        assert live.sum() >= n // 3 and (~live).sum() >= 5, 'both classes are present'
    e = point_yardstick()
    for name in FLOAT_OUTS:
        _held(got[name], want[name], e[name], '%s n %d K %d normalise %d' % (name, n, K, normalise))
    still = live & (got['moving'] == -1)
    assert (got['scene_flow'][still] == 0).all(), 'what does not ride a box does not move, exactly'


def test_each_output_alone_gives_the_same_bits(cuda):
    p = planted_points(257, 3, 1)
    full = _device_points(p, cuda, 1)
    for name in ops.FLOW_OUTPUTS:
        alone = _device_points(p, cuda, 1, outputs=(name,))
        assert sorted(alone) == [name]
        assert torch.equal(alone[name].view(torch.int32), full[name].view(torch.int32)), name


# ---- durf_render_flow is the chain it claims to be --------------------------------------------------------------------------
NEAR, FAR, ALPHA = TT.NEAR, TT.FAR, TT.ALPHA
PAIRS = [(0, 1), (3, 2), (4, 4)]


@pytest.fixture(scope='module')
def scene(cuda):
    model, variables, init, ext, _ = TT._scene(cuda)
    frames = {}
    for hw in ((5, 13), (3, 67)):
        cams = TT.scene_arrays(hw)[2]
        out = model.render_trajectory(variables, cams, TT.TIMES, ext, False, ALPHA, near=NEAR, far=FAR, chunk=TT.CHUNK,
                                      outputs=('rgb', 'distance', 'acc'))
        frames[hw] = (cams, out, float(out['acc'].median()))          # (an untrained model accumulates little: half the pixels pass)
    return dict(ext=ext, frames=frames)


def _bits(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    assert torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)), what


def _chain(scene, hw, fa, fb, en, cuda):
    """ops.camera_rays -> ops.ray_setup(_masked) -> durf_flow_points on the whole frame"""
    cams, out, min_acc = scene['frames'][hw]
    rays = raygen.camera_rays(cams[fa], NEAR, FAR, device=cuda)
    o, d = rays.origins.reshape(-1, 3).contiguous(), rays.directions.reshape(-1, 3).contiguous()
    o_s, d_s, hit, _ = ops.ray_setup(o, d, out['poses'][fa], scene['ext'], box_enable=en)
    args = (o_s, d_s, hit, out['distance'][fa].reshape(-1), out['acc'][fa].reshape(-1), cams[fa], cams[fb], out['poses'][fa],
            out['poses'][fb], scene['ext'])
    return args, ops.flow_points(*args, min_acc=min_acc, znear=ZNEAR)


@pytest.mark.parametrize('mask', [None, [1, 0, 1]])
@pytest.mark.parametrize('hw', [(5, 13), (3, 67)])
def test_render_flow_is_rays_box_test_and_flow_points_bit_for_bit(cuda, scene, hw, mask):
    cams, out, min_acc = scene['frames'][hw]
    en = None if mask is None else torch.tensor(mask, dtype=torch.int32, device=cuda)
    kw = dict(near=NEAR, far=FAR, pairs=PAIRS, min_acc=min_acc, znear=ZNEAR, box_enable=en, outputs=ops.FLOW_OUTPUTS)
    res = {ck: flow.render_flow(out, cams, scene['ext'], chunk=ck, **kw) for ck in (64, 65, 4096)}
    first = res[64]
    assert first['flow'].shape == (len(PAIRS),) + hw + (2,) and first['valid'].dtype == torch.int32 and first['pairs'].tolist() == [list(p) for p in PAIRS]
    for ck in (65, 4096):
        for name in ops.FLOW_OUTPUTS:
            _bits(res[ck][name], first[name], '%s: chunk %d against chunk 64' % (name, ck))
    seen = set()
    for p, (fa, fb) in enumerate(PAIRS):
        args, want = _chain(scene, hw, fa, fb, en, cuda)
        for name in ops.FLOW_OUTPUTS:
            _bits(first[name][p].reshape(want[name].shape), want[name], '%s of pair %d -> %d' % (name, fa, fb))
        seen |= set(int(k) for k in first['moving'][p].unique())
    assert 0 < int(first['valid'].sum()) < first['valid'].numel(), 'valid and invalid pixels'
    assert -2 in seen and seen & {-1, 0, 1, 2} and (1 not in seen if mask else True), seen
    # a frame against itself: no flow, and zcam is the depth of xyz in its own camera
    f = PAIRS[2][0]
    args, _ = _chain(scene, hw, f, f, en, cuda)
    host = [_np(a) if torch.is_tensor(a) else a for a in args]
    o64 = FR.points(*host, min_acc=min_acc, znear=ZNEAR)
    e = _twin_error(o64, FR.points(*host, min_acc=min_acc, znear=ZNEAR, dt=F32), ('flow',))['flow']
    got = _np(first['flow'][2]).reshape(-1, 2)
    assert np.array_equal(_np(first['valid'][2]).reshape(-1), o64['valid'])
    _held(got, o64['flow'], e, 'flow of a frame onto itself')
    ok = o64['valid'] != 0
    assert ok.any() and np.abs(got[ok]).max() < 1e-3 and (_np(first['scene_flow'][2]).reshape(-1, 3)[ok] == 0).all()
    cam = cams[f].astype(F64)
    X, zc = _np(first['xyz'][2]).reshape(-1, 3).astype(F64)[ok], _np(first['zcam'][2]).reshape(-1).astype(F64)[ok]
    dX = X - cam[[3, 7, 11]]
    depth = -(dX @ cam[[2, 6, 10]])
    # three subtractions and a three-term product sum in fp32, each rounded once: 6 roundings of at most |R_j| |d_j| each
    assert (np.abs(zc - depth) <= 6 * 2.0 ** -24 * (np.abs(dX) * np.abs(cam[[2, 6, 10]])).sum(1) + _ulp(depth)).all()


def test_an_undersized_workspace_is_refused_before_any_launch(cuda, scene, monkeypatch):
    hw = (5, 13)
    cams, out, min_acc = scene['frames'][hw]
    n = hw[0] * hw[1]
    need = int(ops._lib.flow_lib().durf_render_flow_workspace_bytes(n, 3))
    real = ops._workspace
    canary = {k: torch.full((2, n) + ((c,) if c else ()), -7, dtype=torch.int32 if k in ('moving', 'valid') else torch.float32, device=cuda)
              for k, c in ops._FLOW_COLS.items()}
    call = lambda: ops.render_flow(cams, out['poses'], scene['ext'], out['distance'].reshape(5, n), out['acc'].reshape(5, n), [(0, 1), (1, 2)],
                                   NEAR, FAR, 4096, min_acc=min_acc, outputs=ops.FLOW_OUTPUTS, out=canary)
    monkeypatch.setattr(ops, '_workspace', lambda dev, nb: real(dev, nb)[:nb - 256])
    with pytest.raises(ops._lib.DurfError, match=r'durf_render_flow: workspace of %d bytes, durf_render_flow_workspace_bytes\(65, 3\) = %d' % (need - 256, need)):
        call()
    torch.cuda.synchronize()
    assert all(bool((v == -7).all()) for v in canary.values()), 'refused before any launch: nothing was written'
    monkeypatch.setattr(ops, '_workspace', real)
    with pytest.raises(ValueError, match='unknown outputs'):
        flow.render_flow(out, cams, scene['ext'], near=NEAR, far=FAR, outputs=('depth',))
    with pytest.raises(ops._lib.DurfError, match=r'pair 0 names frame 5 outside \[0, 5\)'):
        flow.render_flow(out, cams, scene['ext'], near=NEAR, far=FAR, pairs=[(5, 0)])
    call()
    assert not any(bool((v == -7).any()) for k, v in canary.items() if k in ('moving', 'valid'))


# ---- durf_flow_warp on planted targets --------------------------------------------------------------------------------------
OCC_REL, OCC_ABS = 0.02, 0.01
WARP_CASES = [(hw, Cc) for hw in ((1, 1), (3, 67), (5, 129)) for Cc in (1, 3)]


def planted_warp(hw, Cc):
    """-> target [n,3], valid [n], img_b [h,w,C], zcam_b [h,w], kinds [n]: every pixel centre, then the edges of the in-frame
    test, then fractional targets; every depth sits 5 % on either side of the occlusion threshold"""
    h, w = hw
    rs = np.random.default_rng(100 * h + w + Cc)
    img = rs.uniform(0.05, 1.0, (h, w, Cc)).astype(F32)
    zc = rs.uniform(2.0, 6.0, (h, w)).astype(F32)
    if h * w > 1:
        zc[rs.integers(h), rs.integers(w)] = np.nan              # a target frame's own invalid pixel
    y, x = np.divmod(np.arange(h * w), w)
    rows = [(float(a), float(b), 'centre') for a, b in zip(x, y)]
    rows += [(-0.0, -0.0, 'centre'), (w - 1.0, h - 1.0, 'centre'), (w - 1 + 1e-3, 0.0, 'out'), (-1e-3, 0.0, 'out'), (0.0, h - 1 + 1e-3, 'out'),
             (0.0, -1e-3, 'out'), (np.nan, 0.0, 'out'), (0.0, np.nan, 'out'), (1e9, 0.0, 'out'), (-np.inf, 0.0, 'out')]
    if w > 1:
        rows += [(rs.uniform(0, w - 1), rs.uniform(0, h - 1), 'between') for _ in range(64)]
        rows += [(w - 1 - 1e-3, h - 1 - 1e-3, 'between'), (w - 1.0, rs.uniform(0, h - 1), 'between'), (rs.uniform(0, w - 1), h - 1.0, 'between'),
                 (0.5, 0.5, 'between'), (1.5, 0.5, 'between')]
    n = len(rows)
    tg = np.zeros((n, 3), F32)
    tg[:, 0], tg[:, 1] = [r[0] for r in rows], [r[1] for r in rows]
    kinds = np.array([r[2] for r in rows], dtype=object)
    xs, ys = np.nan_to_num(tg[:, 0].astype(F64), posinf=0, neginf=0), np.nan_to_num(tg[:, 1].astype(F64), posinf=0, neginf=0)
    xr, yr = np.clip(np.rint(xs), 0, w - 1).astype(int), np.clip(np.rint(ys), 0, h - 1).astype(int)
    zs = np.nan_to_num(zc[yr, xr].astype(F64), nan=4.0)
    front = rs.uniform(size=n) < 0.7
    front[0] = True                              # (pixel 0 is seen whatever the draw: the 1 x 1 picture has little else)
    tg[:, 2] = (zs * (1 + OCC_REL) + OCC_ABS) * np.where(front, rs.uniform(0.5, 0.95, n), rs.uniform(1.05, 1.5, n))
    tg[1 + rs.integers(n - 1), 2] = np.nan
    valid = (rs.uniform(size=n) < 0.85).astype(np.int32)
    valid[0] = 1
    return tg, valid, img, zc, kinds


_WARP_E = {}


def warp_yardstick():
    if not _WARP_E:
        e = 0.0
        for hw, Cc in WARP_CASES:
            tg, valid, img, zc, _ = planted_warp(hw, Cc)
            a, b = FR.warp(tg, valid, img, zc, OCC_REL, OCC_ABS), FR.warp(tg, valid, img, zc, OCC_REL, OCC_ABS, F32)
            assert np.array_equal(a[1], b[1])
            e = max(e, _twin_error(dict(w=a[0]), dict(w=b[0]), ('w',))['w'])
        _WARP_E['warped'] = e
    return _WARP_E['warped']


@pytest.mark.parametrize('hw,Cc', WARP_CASES)
def test_warp_on_planted_targets(cuda, hw, Cc):
    e = warp_yardstick()
    print('e over the planted warp cases: %.2e' % e)
    assert 0 < e <= 2.0 * RECORDED['warped']
    tg, valid, img, zc, kinds = planted_warp(hw, Cc)
    want, wmask = FR.warp(tg, valid, img, zc, OCC_REL, OCC_ABS)
    d = lambda a: torch.tensor(a, device=cuda)
    warped, mask = ops.flow_warp(d(tg), d(valid), d(img), d(zc), OCC_REL, OCC_ABS)
    got, gmask = _np(warped), _np(mask)
    assert got.shape == (len(tg), Cc) and np.array_equal(gmask, wmask), 'the mask is exact'
    assert not gmask[kinds == 'out'].any() and gmask[kinds == 'centre'].any() and not gmask[valid == 0].any()
    _held(got, want, e, 'warped %s C %d' % (hw, Cc))
    vis = (gmask != 0) & (kinds == 'centre')
    xi, yi = np.rint(tg[vis, 0]).astype(int), np.rint(tg[vis, 1]).astype(int)
    assert got[vis].tobytes() == img[yi, xi].tobytes(), 'an integer target reproduces the pixel bit for bit'
    only_mask = ops.flow_warp(d(tg), d(valid), d(img), d(zc), OCC_REL, OCC_ABS, want_warped=False)
    only_warp = ops.flow_warp(d(tg), d(valid), d(img), d(zc), OCC_REL, OCC_ABS, want_mask=False)
    assert only_mask[0] is None and torch.equal(only_mask[1], mask) and only_warp[1] is None
    assert torch.equal(only_warp[0].view(torch.int32), warped.view(torch.int32))


# ---- durf_flow_consistency --------------------------------------------------------------------------------------------------
CONS_MS = (1, 255, 256, 257, 3 * 256 + 17)


def _cons_mask(kind, P, m):
    mk = np.zeros((P, m), np.int32)
    if kind == 'all':
        mk[:] = 1
    elif kind == 'alternating':
        mk[:, ::2] = 1
    elif kind == 'random':
        mk[:] = np.random.default_rng(m + P).integers(0, 2, (P, m)) * 3          # (any non-zero value counts)
    return mk


@pytest.mark.parametrize('kind', ['all', 'none', 'alternating', 'random'])
@pytest.mark.parametrize('m', CONS_MS)
@pytest.mark.parametrize('P', [1, 2])
def test_consistency_against_the_float64_sum(cuda, P, m, kind):
    """The bound the header's order implies, for sums of non-negative terms.  With u = 2^-24: d = fl(warped - a) carries (1 + u);
    d d carries that twice and its own rounding, 3 u in all, |d| carries u.  A thread adds T = ceil(min(m, SPAN) / 256) C terms
    in sequence, the wave's butterfly adds 6 levels, the block 2: a term passes through at most T + 8 fp32 additions, each
    (1 + u).  The second pass adds G = ceil(m / SPAN) partials in double (G 2^-53: nothing) and rounds to float once, u.  So
    |sse - exact| <= ((1 + u)^(T + 12) - 1) exact and |sae - exact| <= ((1 + u)^(T + 10) - 1) exact; the test allows
    (T + 12) u (1 + 1e-3) of the exact sum for both.  count is exact: at most SPAN / 256 = 16 per thread, 4096 per workgroup."""
    for Cc in (1, 3):
        rs = np.random.default_rng(1000 * m + 10 * P + Cc)
        a = rs.uniform(0, 1, (P, m, Cc)).astype(F32)
        wp = (a + rs.normal(0, 0.1, (P, m, Cc))).astype(F32)
        mk = _cons_mask(kind, P, m)
        wp[mk == 0] = np.nan                                       # what the warp leaves where nothing is visible
        want = FR.consistency(wp, a, mk)
        d = lambda x: torch.tensor(x, device=cuda)
        r1 = ops.flow_consistency(d(wp), d(a), d(mk))
        r2 = ops.flow_consistency(d(wp), d(a), d(mk))
        assert torch.equal(r1.view(torch.int32), r2.view(torch.int32)), 'two runs, the same bits'
        got = _np(r1).astype(F64)
        assert got.shape == (P, 4) and np.array_equal(got[:, 0], want[:, 0]), 'count is exact'
        T = -(-min(m, ops.FLOW_CONS_SPAN) // 256) * Cc
        bound = (T + 12) * 2.0 ** -24 * (1 + 1e-3)
        for col, name in ((1, 'sse'), (2, 'sae')):
            err = np.abs(got[:, col] - want[:, col])
            print('P %d m %d C %d %s %s: relative error %.2e, bound %.2e' % (P, m, Cc, kind, name, (err / np.maximum(want[:, col], 1e-300)).max(), bound))
            assert (err <= bound * want[:, col]).all(), (name, err, bound * want[:, col])
        has = want[:, 0] > 0                                       # (a random mask of a single pixel may be empty)
        assert (has.all() if kind in ('all', 'alternating') else True) and (not has.any() if kind == 'none' else True)
        assert np.isnan(got[~has, 3]).all() and (got[~has, :3] == 0).all(), 'nothing visible: PSNR is NaN'
        # d psnr = 10 / ln 10 d sse / sse, and one rounding of the result to float
        assert (np.abs(got[has, 3] - want[has, 3]) <= 10 / np.log(10) * bound + _ulp(want[has, 3])).all()
        same = wp.copy()
        same[mk != 0] = a[mk != 0]
        r = _np(ops.flow_consistency(d(same), d(a), d(mk)))
        assert np.array_equal(r[:, 0], want[:, 0]) and (r[:, 1:3] == 0).all(), 'equal frames: no error'
        assert np.isposinf(r[has, 3]).all() and np.isnan(r[~has, 3]).all(), 'equal frames: +inf where anything is visible'


def test_consistency_over_more_than_one_span(cuda):
    """two workgroups per pair and a second pass that has something to add: m = SPAN + 3"""
    m, P, Cc = ops.FLOW_CONS_SPAN + 3, 2, 3
    rs = np.random.default_rng(7)
    a = rs.uniform(0, 1, (P, m, Cc)).astype(F32)
    wp = (a + rs.normal(0, 0.1, (P, m, Cc))).astype(F32)
    mk = _cons_mask('random', P, m)
    want = FR.consistency(wp, a, mk)
    d = lambda x: torch.tensor(x, device=cuda)
    got = _np(ops.flow_consistency(d(wp), d(a), d(mk))).astype(F64)
    bound = (16 * Cc + 12) * 2.0 ** -24 * (1 + 1e-3)
    assert np.array_equal(got[:, 0], want[:, 0]) and (np.abs(got[:, 1:3] - want[:, 1:3]) <= bound * want[:, 1:3]).all()


# ---- durf_flow_color --------------------------------------------------------------------------------------------------------
MAX_MAG = 3.0
COLOR_CASES = ('one', 'random', 'sweep')


def planted_flow(case):
    rs = np.random.default_rng(len(case))
    if case == 'one':
        return np.array([[1.25, -0.5]], F32)
    if case == 'random':
        fl = rs.normal(0, 2.0, (65, 2)).astype(F32)
        fl[3], fl[17, 1], fl[64, 0], fl[40] = np.nan, np.nan, np.inf, 0.0
        return fl
    ang = np.deg2rad(np.arange(360.0))
    return np.concatenate([np.stack([np.cos(ang), np.sin(ang)], 1) * s for s in (0.0, 0.5 * MAX_MAG, MAX_MAG, 2 * MAX_MAG)]).astype(F32)


_COLOR_E = {}


def color_yardstick():
    if not _COLOR_E:
        e = 0.0
        for case in COLOR_CASES:
            fl = planted_flow(case)
            for dimmed in (False, True):          # (both branches everywhere: the twin's own choice at rad = 1 is no error of fp32)
                e = max(e, float(np.abs(FR.color(fl, MAX_MAG, dimmed=dimmed)[0] - FR.color(fl, MAX_MAG, F32, dimmed=dimmed)[0]).max()))
        _COLOR_E['rgb'] = e
    return _COLOR_E['rgb']


@pytest.mark.parametrize('case', COLOR_CASES)
def test_flow_picture_against_the_oracle(cuda, case):
    e = color_yardstick()
    print('e over the planted flows: %.2e' % e)
    assert 0 < e <= 2.0 * RECORDED['rgb']
    fl = planted_flow(case)
    rgb, rgb8 = ops.flow_color(torch.tensor(fl, device=cuda), MAX_MAG, want_float=True, want_u8=True)
    got, got8 = _np(rgb).astype(F64), _np(rgb8).astype(np.int64)
    assert got.shape == (len(fl), 3) and rgb8.dtype == torch.uint8
    want, want255 = FR.color(fl, MAX_MAG)
    # where rad is 1 to fp32 rounding (the sweep at max_mag) the header's two branches differ by a quarter of the colour and
    # fp32 may take either: such a pixel is held to the nearer of the two; everywhere else to the header's own choice
    f64 = fl.astype(F64)
    rad = np.sqrt((np.nan_to_num(f64, nan=0.0, posinf=0.0, neginf=0.0) ** 2).sum(1)) / MAX_MAG
    edge = np.abs(rad - 1.0) <= 4 * 2.0 ** -24
    assert edge.sum() == (360 if case == 'sweep' else 0)
    alt = {b: FR.color(fl, MAX_MAG, dimmed=b) for b in (False, True)}
    for i in np.nonzero(edge)[0]:
        b = min((False, True), key=lambda b: np.abs(got[i] - alt[b][0][i]).max())
        want[i], want255[i] = alt[b][0][i], alt[b][1][i]
    tol = 4.0 * e + 4.0 * _ulp(want)
    err = np.abs(got - want)
    print('%s: max error %.3e' % (case, err.max()))
    assert (err <= tol).all(), (case, err.max())
    bad = ~np.isfinite(fl).all(1)
    assert (got[bad] == 0).all() and (got8[bad] == 0).all(), 'invalid flow is black'
    level = np.rint(want255).astype(np.int64)
    near_half = np.abs(want255 - np.floor(want255) - 0.5) <= 255.0 * tol
    assert (got8[~near_half] == level[~near_half]).all(), 'rgb8 is exact away from a rounding boundary'
    assert (np.abs(got8 - level) <= 1).all()
    # (the sweep at half of max_mag sits ON a boundary wherever a wheel channel is 0: 1 - 0.5 (1 - 0) = 0.5, level 127.5)
    assert near_half.mean() < (0.15 if case == 'sweep' else 0.05), 'the exception stays an exception'
    if case == 'sweep':
        assert (got8[:360] == 255).all(), 'no motion is white'
        assert got8[360:720].reshape(360, 3).max(0).tolist() == [255, 255, 255] and len(np.unique(got8[360:720], axis=0)) > 100
    only8 = ops.flow_color(torch.tensor(fl, device=cuda), MAX_MAG, want_float=False, want_u8=True)
    assert only8[0] is None and torch.equal(only8[1], rgb8)


# ---- the command ----------------------------------------------------------------------------------------------------------
def test_render_traj_command_writes_flow_files(cuda, tmp_path):
    from durf_amd import render_traj, trajectory
    base = ['--synthetic', '--synthetic_size', '8', '12', '--frames', '3', '--gin_param', 'MipNerfModel.num_samples = 32',
            '--gin_param', 'MipNerfModel.no_pose_opt = True', '--gin_param', 'MipNerfModel.no_yaw_opt = True']
    out = str(tmp_path / 'flow')
    p = subprocess.run([sys.executable, '-m', 'durf_amd.render_traj', '--flow', '--eval_dir', out] + base, cwd=ROOT, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=300)                                        # a fresh child process
    assert p.returncode == 0, p.stdout.decode()
    plain = ['%04d.ppm' % f for f in range(3)] + ['distance.npy']
    assert sorted(os.listdir(out)) == sorted(plain + ['flow_%04d.%s' % (f, x) for f in (0, 1) for x in ('flo', 'ppm')] + ['consistency.json'])
    # the same scene in this process, by the command's own steps
    args = render_traj.build_parser().parse_args(['--eval_dir', out] + base)
    dev, config, dataset = render_traj.open_scene(args)
    model, variables, alpha = render_traj.restore_model(args, config, dataset, dev)
    row = dataset.ts_data[0].cams
    c2w, times = trajectory.make_trajectory([row[0, :12].reshape(3, 4), dataset.ts_data[-1].cams[-1, :12].reshape(3, 4)],
                                            [0.0, float(dataset.T - 1)], 3)
    focal, ppx, ppy, h, w = [float(x) for x in row[0][12:]]
    assert (h, w) == (8, 12)
    cams = trajectory.camera_rows(c2w, focal, (ppx, ppy), 8, 12)
    res = model.render_trajectory(variables, cams, times, dataset.ext, config.white_bkgd, alpha, near=config.near, far=config.far,
                                  outputs=('rgb', 'distance', 'acc'))
    kw = dict(near=config.near, far=config.far)
    fl = flow.render_flow(res, cams, dataset.ext, outputs=('flow', 'valid', 'moving', 'target'), **kw)
    cons = flow.consistency(flow.warp(fl, res['rgb'], flow.frame_depth(res, cams, dataset.ext, **kw)), res['rgb'], fl['pairs'])
    doc = json.load(open(os.path.join(out, 'consistency.json')))
    assert [(r['source'], r['target']) for r in doc['pairs']] == [(0, 1), (1, 2)] and sorted(doc['mean']) == ['count', 'mse', 'psnr']
    same = lambda a, b: a == b or (a != a and b != b)
    for f in (0, 1):
        got, gv = flow.read_flo(os.path.join(out, 'flow_%04d.flo' % f))
        want, wv = _np(fl['flow'][f]), _np(fl['valid'][f])
        assert got.shape == (8, 12, 2) and np.array_equal(gv, wv) and got[gv != 0].tobytes() == want[wv != 0].tobytes()
        assert np.isnan(got[gv == 0]).all() and np.isnan(want[wv == 0]).all()
        blob = open(os.path.join(out, 'flow_%04d.ppm' % f), 'rb').read()
        assert blob[:len(b'P6\n12 8\n255\n')] == b'P6\n12 8\n255\n' and len(blob) == len(b'P6\n12 8\n255\n') + 8 * 12 * 3
        for k in ('count', 'mse', 'psnr'):
            assert same(doc['pairs'][f][k], float(cons[k][f])), (k, doc['pairs'][f][k], float(cons[k][f]))
    # without the flag: none of them
    bare = str(tmp_path / 'bare')
    assert render_traj.main(['--eval_dir', bare] + base) == 0
    assert sorted(os.listdir(bare)) == sorted(plain)
