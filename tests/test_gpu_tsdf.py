"""libdurf_tsdf.so against tests/tsdf_ref on the device: tsdf, weight and colour EQUAL integrate32, compared as int32 bits --
every optional input on and off, launch edges, every skip rule by a voxel built for it, splits, the lattice and the sampler, a
real surface and a moving box end to end, every refusal by its message, and fuse_scene and the command."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from durf_amd import _lib, geometry, mesh, ops, raster, tsdf
from tests import tsdf_ref as R
from tests.test_tsdf_host import SPHERE_FRACTION, tie_scene

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
DT = dict(acc=torch.float32, rgb=torch.float32, label=torch.int32, xform=torch.float32, frame_weight=torch.float32)


def _d(a, cuda, dtype=torch.float32):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a)).to(device=cuda, dtype=dtype).contiguous()


def _device(cuda, state, frame, shape, cams, depth, trunc, **kw):
    """ops.tsdf_integrate on copies of `state` -> the new state as host arrays"""
    st = {k: _d(v, cuda) for k, v in state.items()}
    fr = [frame[k] for k in ('origin', 'du', 'dv', 'dw')]
    kw = {k: (_d(v, cuda, DT[k]) if k in DT else v) for k, v in kw.items()}
    ops.tsdf_integrate(st['tsdf'], st['weight'], st['colour'], shape, *fr, _d(np.asarray(cams).reshape(-1, 17), cuda), _d(depth, cuda), trunc, **kw)
    return {k: (None if v is None else v.cpu().numpy()) for k, v in st.items()}


def _same(got, want, what=''):
    for k in ('tsdf', 'weight', 'colour'):
        if want.get(k) is None:
            assert got.get(k) is None, (what, k)
            continue
        a, b = got[k].reshape(-1).view(np.int32), np.ascontiguousarray(want[k], F32).reshape(-1).view(np.int32)
        assert np.array_equal(a, b), (what, k, int((a != b).sum()), np.argwhere(a != b)[:5].tolist())


def _both(cuda, state, frame, shape, cams, depth, trunc, what='', **kw):
    want = R.integrate32(state, frame, shape, cams, depth, trunc, **kw)
    got = _device(cuda, state, frame, shape, cams, depth, trunc, **kw)
    _same(got, want, what)
    return got, want


def _dirty(shape, rng, colour=True):
    """a state that is not new: what an earlier call left"""
    n = int(np.prod(shape))
    return dict(tsdf=rng.uniform(-1, 1, n).astype(F32), weight=rng.uniform(0, 3, n).astype(F32),
                colour=rng.random((n, 4)).astype(F32) * F32(2.0) if colour else None)


# ---- 1 bits ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def small():
    """9 x 10 x 11 = 990 voxels: three full workgroups and a partial one; F = 3 frames of 24 x 32"""
    return R.random_scene(5, F=3, h=24, w=32, shape=(9, 10, 11), step=0.3, focal=26.0)


OPTIONS = [dict(), dict(acc=1), dict(rgb=1), dict(rgb=1, colour=False), dict(label=1, other_mode=0), dict(label=1, other_mode=1), dict(xform=1),
           dict(frame_weight=1), dict(acc=1, rgb=1, label=1, other_mode=1, xform=1, frame_weight=1), dict(acc=1, rgb=1, label=1, other_mode=0, frame_weight=1)]


@pytest.mark.parametrize('opt', OPTIONS, ids=lambda o: '+'.join(sorted(o)) or 'plain')
def test_bits_with_every_optional_input_on_and_off(cuda, small, opt):
    s = small
    kw = {k: s[k] for k in ('acc', 'rgb', 'label', 'xform', 'frame_weight') if opt.get(k)}
    if 'acc' in kw:
        kw['min_acc'] = 0.25
    if 'label' in kw:
        kw.update(select=1, other_mode=opt['other_mode'])
    rng = np.random.default_rng(1)
    for state in (R.new_state(s['shape'], opt.get('colour', True)), _dirty(s['shape'], rng, opt.get('colour', True))):
        got, want = _both(cuda, state, s['frame'], s['shape'], s['cams'], s['depth'], s['trunc'], what=str(opt), **kw)
    assert (want['why'] == 0).sum() > 300 and len(np.unique(want['why'])) >= 3, np.unique(want['why'])
    untouched = (want['why'] != 0).all(0)
    assert untouched.sum() > 10 and np.array_equal(got['tsdf'][untouched].view(np.int32), state['tsdf'][untouched].view(np.int32))


# ---- 2 launch edges ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', [(2, 2, 2), (3, 5, 17), (4, 8, 8), (2, 2, 65), (2, 3, 257)])
def test_launch_edges(cuda, shape):
    rng = np.random.default_rng(sum(shape))
    h, w = 20, 28
    cams = R.ring_cameras(1, h, w, 14.0, radius=4.0, height=0.7, phase=0.4)
    ex = R.random_extras(rng, 1, h, w)
    step = 2.4 / (max(shape) - 1)
    frame = R.frame_of([-(n - 1) * step / 2.0 for n in shape], step)
    got, want = _both(cuda, _dirty(shape, rng), frame, shape, cams, R.sphere_depth(cams, h, w), 0.4, acc=ex['acc'], min_acc=0.2, rgb=ex['rgb'],
                      frame_weight=ex['frame_weight'])
    assert (want['why'] == 0).sum() >= 2 and (want['why'] != 0).sum() >= 1


# ---- 3 every skip rule -------------------------------------------------------------------------------------------------------------
def test_every_skip_rule_by_a_voxel_built_for_it(cuda):
    """an identity camera with focal 1 and principal point (0, 0): a voxel at (x z, -y z, -z) projects to pixel (x, y) at depth z"""
    h, w = 6, 8
    cams = R.camera(h, w, 1.0, pp=(0.0, 0.0))[None]
    depth = np.full((1, h, w), 2.0, F32)
    acc = np.ones((1, h, w), F32)
    depth[0, 1, 0], depth[0, 1, 1], depth[0, 1, 2], depth[0, 1, 3] = 0.0, np.nan, np.inf, -1.0
    acc[0, 2, 0], acc[0, 2, 1] = 0.5, np.nextafter(F32(0.5), F32(0))
    cases = [('updated', 3.0, 3.0, 1.0), ('behind', 3.0, 3.0, 0.25), ('behind', 3.0, 3.0, -1.0), ('outside', -1.0, 3.0, 1.0), ('outside', 8.0, 3.0, 1.0),
             ('outside', 3.0, -1.0, 1.0), ('outside', 3.0, 6.0, 1.0), ('updated', -0.5, 3.0, 1.0), ('updated', 0.5, 3.0, 1.0), ('updated', 1.5, 3.0, 1.0),
             ('outside', 7.5, 3.0, 1.0), ('updated', 3.0, -0.5, 1.0), ('outside', 3.0, 5.5, 1.0), ('hole', 0.0, 1.0, 1.0), ('hole', 1.0, 1.0, 1.0),
             ('hole', 2.0, 1.0, 1.0), ('hole', 3.0, 1.0, 1.0), ('updated', 0.0, 2.0, 1.0), ('faint', 1.0, 2.0, 1.0), ('updated', 3.0, 3.0, 2.5),
             ('occluded', 3.0, 3.0, 2.75), ('updated', 3.0, 3.0, 1.5), ('updated', 3.0, 3.0, 1.25), ('range', 3.0e6, 3.0, 1.0), ('invalid', np.inf, 3.0, 1.0)]
    # z = 2.5: sdf = -0.5 = -trunc exactly, kept; z = 2.75 is below; z = 1.5: sdf = trunc exactly; z = 1.25: beyond.
    # One call per case: the xform of the call moves voxel (0, 0, 0) to the case's point; the lattice's steps of 1000 put the
    # other seven voxels off the frame or behind the camera.
    frame = R.frame_of([0.0, 0.0, 0.0], axes=((1e3, 0.0, 0.0), (0.0, 1e3, 0.0), (0.0, 0.0, 1e3)))
    small_shape = (2, 2, 2)
    rng = np.random.default_rng(0)
    rgb = rng.random((1, h, w, 3)).astype(F32)
    for name, x, y, z in cases:
        X = np.array([x * z, -y * z, -z], np.float64)
        xf = np.concatenate([np.eye(3), X[:, None]], 1)[None].astype(F32)
        state = _dirty(small_shape, rng)
        got, want = _both(cuda, state, frame, small_shape, cams, depth, 0.5, what='%s %s' % (name, (x, y, z)), acc=acc, min_acc=0.5, rgb=rgb, xform=xf,
                          znear=0.5)
        assert R.RULES[want['why'][0, 0]] == name, (name, x, y, z, R.RULES[want['why'][0, 0]])
        assert (want['why'][0, 1:] != 0).all()                               # the other seven voxels are far off the frame
        for k in ('tsdf', 'weight', 'colour'):
            assert np.array_equal(got[k][1:].view(np.int32), state[k][1:].view(np.int32)), (name, k)
            assert (name != 'updated') == np.array_equal(got[k][0].view(np.int32), state[k][0].view(np.int32)) or k == 'colour', (name, k)
    # sdf == trunc keeps the colour, beyond it does not
    for z, coloured in ((1.5, True), (1.25, False)):
        xf = np.concatenate([np.eye(3), np.array([[9.0], [-9.0], [-3.0]]) * z / 3.0], 1)[None].astype(F32)
        state = R.new_state(small_shape)
        got, _ = _both(cuda, state, frame, small_shape, cams, depth, 0.5, acc=acc, rgb=rgb, xform=xf, znear=0.5)
        assert got['weight'][0] == 1.0 and (got['colour'][0, 3] == 1.0) == coloured
    # a frame weight that is not positive, or not finite, skips the frame
    for wf in (0.0, -1.0, np.nan, np.inf):
        xf = np.concatenate([np.eye(3), np.array([[3.0], [-3.0], [-1.0]])], 1)[None].astype(F32)
        state = _dirty(small_shape, rng)
        got, want = _both(cuda, state, frame, small_shape, cams, depth, 0.5, xform=xf, frame_weight=np.array([wf], F32))
        assert R.RULES[want['why'][0, 0]] == 'weight' and np.array_equal(got['tsdf'].view(np.int32), state['tsdf'].view(np.int32))
    # the label rules: another label skips in mode 0, counts as free space in mode 1 only from sdf >= trunc on, never with colour
    label = np.full((1, h, w), 7, np.int32)
    for z, mode, name in ((1.0, 0, 'other'), (1.0, 1, 'updated'), (1.5, 1, 'updated'), (1.75, 1, 'other')):
        xf = np.concatenate([np.eye(3), np.array([[3.0], [-3.0], [-1.0]]) * z], 1)[None].astype(F32)
        got, want = _both(cuda, R.new_state(small_shape), frame, small_shape, cams, depth, 0.5, xform=xf, label=label, select=1, other_mode=mode, rgb=rgb)
        assert R.RULES[want['why'][0, 0]] == name and got['colour'][0, 3] == 0.0, (z, mode)


def test_rintf_ties_on_the_device(cuda):
    frame, shape, cams, depth = tie_scene(8)
    got, want = _both(cuda, R.new_state(shape, False), frame, shape, cams, depth, 100.0)
    assert want['why'][0].reshape(shape)[0, 0].tolist() == [0] * 8 + [4, 4]


# ---- 4 splits ----------------------------------------------------------------------------------------------------------------------
def test_splits_give_the_same_bits_and_the_clamp_is_reached(cuda):
    s = R.random_scene(7, F=5, h=24, w=32, shape=(9, 10, 11), step=0.3, focal=26.0)
    kw = dict(acc=s['acc'], min_acc=0.1, rgb=s['rgb'], label=s['label'], select=1, other_mode=1, xform=s['xform'], frame_weight=s['frame_weight'],
              max_weight=2.0)
    want = R.integrate32(R.new_state(s['shape']), s['frame'], s['shape'], s['cams'], s['depth'], s['trunc'], **kw)
    assert (want['weight'] == 2.0).sum() > 50
    for cuts in ([0, 5], [0, 2, 5], [0, 1, 2, 3, 4, 5]):
        st = R.new_state(s['shape'])
        for f0, f1 in zip(cuts[:-1], cuts[1:]):
            per = {k: (v[f0:f1] if isinstance(v, np.ndarray) else v) for k, v in kw.items()}
            st = _device(cuda, st, s['frame'], s['shape'], s['cams'][f0:f1], s['depth'][f0:f1], s['trunc'], **per)
        _same(st, want, str(cuts))


# ---- 5 lattice and sample ----------------------------------------------------------------------------------------------------------
def test_lattice_and_sample(cuda):
    rng = np.random.default_rng(11)
    shape = (5, 6, 7)
    frame = R.frame_of([-0.5, 0.25, 1.0], 0.25)                              # exact in float32: q is exact at lattice points
    st = _dirty(shape, rng)
    st['weight'][rng.random(st['weight'].shape) < 0.1] = 0.0                 # unobserved voxels
    st['colour'][rng.random(st['weight'].shape) < 0.1, 3] = 0.0
    st['tsdf'][0] = 0.0
    dev = {k: _d(v, cuda) for k, v in st.items()}
    density, valid, rgb = ops.tsdf_lattice(dev['tsdf'], dev['weight'], dev['colour'], shape, 1.0)
    wd, wv, wr = R.lattice32(st, 1.0)
    assert np.array_equal(density.cpu().numpy().reshape(-1).view(np.int32), wd.view(np.int32)) and np.signbit(density.cpu().numpy().reshape(-1)[0])
    assert np.array_equal(valid.cpu().numpy().reshape(-1), wv) and 0 < wv.sum() < wv.size
    assert np.array_equal(rgb.cpu().numpy().reshape(-1, 3).view(np.int32), wr.view(np.int32))
    assert ops.tsdf_lattice(dev['tsdf'], dev['weight'], None, shape, 1.0)[2] is None
    P = R.voxels(frame, shape, F32)
    lo, hi = P[0], P[-1]
    pts = np.concatenate([P, rng.uniform(lo, hi, (500, 3)).astype(F32), rng.uniform(lo - 0.3, hi + 0.3, (200, 3)).astype(F32),
                          np.array([[np.nan, 0.5, 1.2], [0.0, np.inf, 1.2], hi, lo, [hi[0], lo[1], hi[2]], hi + F32(1e-3), lo - F32(1e-3)], F32)])
    inv = R.inverse_of(frame)
    for trunc, mw in ((0.75, 1.0), (0.5, 0.0)):
        sdf, ok, col = ops.tsdf_sample(dev['tsdf'], dev['weight'], dev['colour'], shape, frame['origin'], inv, trunc, _d(pts, cuda), mw)
        ws, wo, wc = R.sample32(st, frame, shape, trunc, pts, mw)
        assert np.array_equal(ok.cpu().numpy(), wo) and 0 < wo.sum() < wo.size
        assert np.array_equal(sdf.cpu().numpy().view(np.int32), ws.view(np.int32))
        assert np.array_equal(col.cpu().numpy().view(np.int32), wc.view(np.int32))
        assert np.isnan(ws[wo == 0]).all() and np.isfinite(ws[wo == 1]).all()
    # min_weight 0: every inside point is ok; the last faces are inside, a hair beyond is not; NaN and inf are outside
    assert wo[:P.shape[0]].all() and wo[-5:].tolist() == [1, 1, 1, 0, 0] and wo[-7:-5].tolist() == [0, 0]
    # at a lattice point off the last faces, t = 0: D times trunc exactly
    i, j, k = np.meshgrid(*[np.arange(s) for s in shape], indexing='ij')
    inner = ((i < shape[0] - 1) & (j < shape[1] - 1) & (k < shape[2] - 1)).reshape(-1)
    assert np.array_equal(ws[:P.shape[0]][inner].view(np.int32), (st['tsdf'] * F32(0.5))[inner].view(np.int32))
    # beside an unobserved voxel: not ok at min_weight 1
    ws1, wo1, _ = R.sample32(st, frame, shape, 0.75, pts, 1.0)
    assert (wo1[:P.shape[0]][inner & (st['weight'] < 1.0)] == 0).all()
    # the host-side wrapper: host points in, the same answer
    vol = dict(tsdf=dev['tsdf'].reshape(shape), weight=dev['weight'].reshape(shape), colour=dev['colour'].reshape(shape + (4,)), frame=frame, shape=shape,
               trunc=0.75)
    out = tsdf.sample(vol, pts)
    assert np.array_equal(out['ok'].cpu().numpy(), wo1.astype(bool)) and np.array_equal(out['sdf'].cpu().numpy().view(np.int32), ws1.view(np.int32))


# ---- 6 a real surface --------------------------------------------------------------------------------------------------------------
def test_a_sphere_drawn_by_the_rasteriser_is_fused_and_meshed(cuda):
    N = 24
    step = 3.0 / (N - 1)
    v, t = R.icosphere(4)
    cams = R.six_cameras(64, 64, 60.0, 4.0)
    r = raster.render_mesh(dict(vertices=v, triangles=t), cams, attrs=(), label=None)
    vol = tsdf.volume([-1.5] * 3, (N, N, N), step=step, trunc=2.0 * step, colour=False, device=cuda)
    tsdf.integrate(vol, cams, r['depth'])
    want = R.integrate32(R.new_state((N, N, N), False), vol['frame'], (N, N, N), cams, r['depth'].cpu().numpy(), 2.0 * step)
    _same(dict(tsdf=vol['tsdf'].cpu().numpy(), weight=vol['weight'].cpu().numpy()), want)
    m = tsdf.surface(vol)
    X, tri, nrm = m['vertices'].cpu().numpy().astype(np.float64), m['triangles'].cpu().numpy(), m['normals'].cpu().numpy()
    assert tri.shape[0] > 3000 and m['rgb'] is None and int(m['observed']) == int((want['weight'] >= 1).sum())
    assert tri.min() >= 0 and tri.max() < X.shape[0]
    assert np.array_equal(np.unique(tri), np.arange(X.shape[0])), 'every vertex is referenced: the band of two steps leaves no hole in the surface'
    a, b, c = X[tri[:, 0]], X[tri[:, 1]], X[tri[:, 2]]
    fn = np.cross(b - a, c - a)
    big = np.linalg.norm(fn, axis=1) > 1e-9                                   # (a corner exactly at 0 gives zero-area triangles: they stay)
    assert big.sum() > 3000 and (np.einsum('ij,ij->i', fn[big], (a + b + c)[big]) > 0).all(), 'oriented outward'
    assert (np.einsum('ij,ij->i', nrm, X) > 0).all()
    # against a cloud of the sphere: the nearest point of a cloud is farther than the sphere by at most the cloud's covering radius,
    # which for the acute triangles of the icosphere is at most (longest edge) / sqrt(3) (the circumradius of such a triangle)
    rv, rt = R.icosphere(5)                                                  # 10242 points
    edge = max(np.linalg.norm(rv[rt[:, a]].astype(np.float64) - rv[rt[:, b]], axis=1).max() for a, b in ((0, 1), (1, 2), (2, 0)))
    cover = edge / np.sqrt(3.0)
    assert cover < 0.2 * step, 'the cloud is dense enough to say something: %.3f of a step' % (cover / step)
    dist = geometry.cloud_distance(m['vertices'].contiguous(), torch.as_tensor(rv).to(cuda).contiguous(), 1.0, keep=True)['pred_dist'].cpu().numpy()
    radial = np.abs(np.linalg.norm(X, axis=1) - 1.0)
    print('vertices %d, worst radial error %.4f of a step, worst distance to the cloud %.4f, the cloud covers to %.4f'
          % (X.shape[0], radial.max() / step, dist.max() / step, cover / step))
    assert radial.max() <= 2.0 * SPHERE_FRACTION * step
    assert dist.max() <= 2.0 * SPHERE_FRACTION * step + cover
    # a floater: eight voxels in a corner made solid by hand; surface(min_points=) drops it and gives the clean surface back, bit for bit
    vol['tsdf'][1:3, 1:3, 1:3], vol['weight'][1:3, 1:3, 1:3] = -1.0, 1.0
    vol['tsdf'][0:4, 0:4, 0:4] = torch.where(vol['weight'][0:4, 0:4, 0:4] > 0, vol['tsdf'][0:4, 0:4, 0:4], torch.ones(()).to(cuda))
    vol['weight'][0:4, 0:4, 0:4] = 1.0                                       # ... inside a shell of observed free space
    dirty = tsdf.surface(vol)
    assert dirty['vertices'].shape[0] > m['vertices'].shape[0]
    for kw, kept in ((dict(min_points=9), 1), (dict(largest=1), 1), (dict(min_points=8), 2)):
        c = tsdf.surface(vol, **kw)
        assert c['cleaning']['components'] == 2 and c['cleaning']['kept'] == kept and c['rgb'] is None, (kw, c['cleaning'])
        if kept == 1:
            assert c['cleaning']['dropped_points'] == 8 and torch.equal(c['vertices'], m['vertices']) and torch.equal(c['triangles'], m['triangles'])
            assert int(c['component'].max()) == int(c['component'].min())
        else:
            assert c['vertices'].shape[0] == dirty['vertices'].shape[0]


# ---- 7 a moving object -------------------------------------------------------------------------------------------------------------
def test_a_moving_box_is_fused_in_its_own_frame(cuda):
    """A box placed by five different poses in front of one fixed camera -- each pose turns another face (+x, -x, +z, -z, +y)
    towards it, to within 0.03 rad, and shifts the centre -- drawn by the rasteriser together with a small quad of another
    label; the ids are the label, and the box is fused in its own frame with box_xforms.
    Why frontal views: the distance is projective, and a voxel just outside a sharp edge that a camera sees THROUGH the corner
    gets a negative distance (DESIGN.md 12 documents the artefact: on a ring of oblique views the worst vertex of this box is
    1.5 steps off).  Seen face-on, each face is placed by the camera that looks at it, and the bound of the sphere holds:
    measured 0.54 of obj_step (the face nobody looks at, -y, stays open).
    Why the quad stands clear: free space from another label (other_mode = 1) enters the mean of every voxel it is seen behind,
    so it leaves the band around the box alone exactly when the other thing is seen at least trunc clear of the box -- here
    0.4 above its silhouette, 3 behind the lattice.  Then mode 1 observes strictly more voxels and changes none that mode 0
    gave D < 1."""
    half = np.array([0.6, 0.35, 0.45])
    rng = np.random.default_rng(2)
    rv = np.array([(0, np.pi / 2, 0), (0, -np.pi / 2, 0), (0, 0, 0), (0, np.pi, 0), (np.pi / 2, 0, 0)], np.float64)
    F, h, w, dist = len(rv), 96, 96, 8.0
    poses = np.zeros((F, 2, 6))
    poses[:, 1, :3] = rng.uniform(-0.2, 0.2, (F, 3))
    poses[:, 1, 3:] = rv + rng.uniform(-0.03, 0.03, (F, 3))
    xf = tsdf.box_xforms(poses, 1)
    cams = np.stack([R.camera(h, w, 240.0, R.look_at((0, 0, dist), (0, 0, 0)))] * F)
    bv, bt = R.box_mesh(half)
    depth, label = [], []
    for f in range(F):
        world = (xf[f, :, :3].astype(np.float64) @ bv.T.astype(np.float64)).T + xf[f, :, 3]
        s = (dist + 3.0) / dist                                              # the quad at z = -3 as seen in the plane z = 0
        y0, y1 = (world[:, 1].max() + 0.4) * s, (world[:, 1].max() + 0.48) * s
        x0, x1 = (poses[f, 1, 0] - 0.3) * s, (poses[f, 1, 0] + 0.3) * s
        other = np.array([(x0, y0, -3), (x1, y0, -3), (x1, y1, -3), (x0, y1, -3)], F32)
        m = dict(vertices=np.concatenate([world.astype(F32), other]), triangles=np.concatenate([bt, np.array([(8, 9, 10), (8, 10, 11)], np.int32)]),
                 owner=np.concatenate([np.full(8, 1, np.int32), np.zeros(4, np.int32)]))
        r = raster.render_mesh(m, cams[f:f + 1], attrs=(), label='owner')
        depth.append(r['depth']), label.append(r['owner'])
    depth, label = torch.cat(depth), torch.cat(label)
    assert ((label == 1).sum(dim=(1, 2)) > 500).all() and ((label == 0).sum(dim=(1, 2)) > 20).all() and (label == -1).sum() > 1000
    obj_step = 0.1
    frame, _, shape = mesh.object_lattice(np.zeros(3), np.eye(3), half, obj_step, 1.0)
    vols = []
    for carve in (False, True):
        vol = tsdf.volume(frame['origin'], shape, axes=(frame['du'], frame['dv'], frame['dw']), trunc=2.0 * obj_step, colour=False, device=cuda)
        tsdf.integrate(vol, cams, depth, label=label, select=1, carve=carve, xform=xf)
        want = R.integrate32(R.new_state(shape, False), vol['frame'], shape, cams, depth.cpu().numpy(), 2.0 * obj_step, label=label.cpu().numpy(),
                             select=1, other_mode=int(carve), xform=xf)
        _same(dict(tsdf=vol['tsdf'].cpu().numpy(), weight=vol['weight'].cpu().numpy()), want, 'carve %s' % carve)
        vols.append(vol)
    X = tsdf.surface(vols[0])['vertices'].cpu().numpy()
    err = R.box_surface_distance(X, half) / obj_step
    D0, W0, D1, W1 = (vols[i][k].cpu().numpy() for i in (0, 1) for k in ('tsdf', 'weight'))
    near = (W0 > 0) & (D0 < 1.0)
    changed = int((D1[near].view(np.int32) != D0[near].view(np.int32)).sum())
    more = int(((W1 >= 1) & ~(W0 >= 1)).sum())
    print('box: %d vertices, worst %.4f of obj_step (mean %.3f); free space observes %d voxels more and changes %d of %d near ones'
          % (X.shape[0], err.max(), err.mean(), more, changed, near.sum()))
    assert X.shape[0] > 1000 and (np.abs(X).max(0) > 0.9 * half).all()
    assert err.max() <= 2.0 * SPHERE_FRACTION
    assert more > 0 and not ((W0 >= 1) & ~(W1 >= 1)).any(), 'free space observes strictly more'
    assert near.sum() > 500 and changed == 0


# ---- 8 refusals --------------------------------------------------------------------------------------------------------------------
def test_every_refusal_by_its_message_and_nothing_is_written(cuda):
    import ctypes as C
    L = _lib.tsdf_lib()
    shape, F, h, w = (3, 4, 5), 2, 6, 8
    n = 60
    rng = np.random.default_rng(4)
    st = {k: _d(v, cuda) for k, v in _dirty(shape, rng).items()}
    before = {k: v.clone() for k, v in st.items()}
    cams, depth = _d(R.ring_cameras(F, h, w, 8.0), cuda), _d(np.full((F, h, w), 3.0, F32), cuda)
    acc, rgb, label = torch.ones(F, h, w, device=cuda), torch.ones(F, h, w, 3, device=cuda), torch.ones(F, h, w, dtype=torch.int32, device=cuda)
    f3 = lambda *a: (C.c_float * 3)(*a)
    good = dict(stream=None, nu=3, nv=4, nw=5, origin=f3(0, 0, 0), du=f3(1, 0, 0), dv=f3(0, 1, 0), dw=f3(0, 0, 1), F=F, h=h, w=w, cams=cams.data_ptr(),
                depth=depth.data_ptr(), acc=acc.data_ptr(), min_acc=0.5, rgb=rgb.data_ptr(), label=label.data_ptr(), select=1, other_mode=0, xform=None,
                frame_weight=None, trunc=0.5, max_weight=64.0, znear=1e-2, tsdf=st['tsdf'].data_ptr(), weight=st['weight'].data_ptr(),
                colour=st['colour'].data_ptr())
    nan, inf = float('nan'), float('inf')
    cases = [(dict(nu=1), 'nu, nv, nw >= 2'), (dict(nu=1024, nv=1024, nw=128), '2^27 lattice points'), (dict(F=-1), 'F >= 0'), (dict(h=0), '1 <= h, w <= 4096'),
             (dict(w=4097), '1 <= h, w <= 4096'), (dict(F=1 << 20, h=64, w=64), 'F h w < 2^31'), (dict(trunc=0.0), 'trunc > 0 and finite'),
             (dict(trunc=nan), 'trunc > 0 and finite'), (dict(trunc=inf), 'trunc > 0 and finite'), (dict(max_weight=0.0), 'max_weight > 0'),
             (dict(max_weight=nan), 'max_weight > 0'), (dict(znear=0.0), 'znear > 0'), (dict(znear=1e-42), 'znear > 0'), (dict(min_acc=nan), 'min_acc is a number'),
             (dict(other_mode=2), 'other_mode in 0 .. 1'), (dict(other_mode=-1), 'other_mode in 0 .. 1'), (dict(other_mode=1, label=None), 'label with other_mode == 1'),
             (dict(origin=None), 'origin_host'), (dict(du=None), 'du_host'), (dict(dv=None), 'dv_host'), (dict(dw=None), 'dw_host'), (dict(tsdf=None), ': tsdf'),
             (dict(weight=None), ': weight'), (dict(cams=None), 'cams_dev for F = 2'), (dict(depth=None), 'depth for F = 2'),
             (dict(colour=st['colour'].data_ptr() + 4), 'colour aligned to 16 bytes')]
    for change, text in cases:
        rc = L.durf_tsdf_integrate(*dict(good, **change).values())
        msg = _lib.lib().durf_last_error().decode()
        assert rc != 0 and 'durf_tsdf_integrate' in msg and text in msg, (change, msg)
    assert L.durf_tsdf_integrate(*dict(good, F=0, cams=None, depth=None).values()) == 0          # F == 0: success, no launch
    assert L.durf_tsdf_integrate(*dict(good, min_acc=nan, acc=None).values()) == 0               # NaN min_acc matters with acc alone
    torch.cuda.synchronize()
    st2 = {k: before[k].clone() for k in before}
    ops.tsdf_integrate(st2['tsdf'], st2['weight'], st2['colour'], shape, (0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), cams, depth, 0.5, rgb=rgb, label=label,
                       select=1)
    for k in before:                                                         # the one good call above did what this one does; the refusals wrote nothing
        assert torch.equal(st[k], st2[k]), k
    density, valid, out3 = torch.zeros(n, device=cuda), torch.zeros(n, dtype=torch.uint8, device=cuda), torch.zeros(n, 3, device=cuda)
    lat = dict(stream=None, nu=3, nv=4, nw=5, tsdf=st['tsdf'].data_ptr(), weight=st['weight'].data_ptr(), colour=st['colour'].data_ptr(), min_weight=1.0,
               density=density.data_ptr(), valid=valid.data_ptr(), rgb_out=out3.data_ptr())
    for change, text in [(dict(nw=1), 'nu, nv, nw >= 2'), (dict(min_weight=nan), 'min_weight is a number'), (dict(tsdf=None), ': tsdf'), (dict(weight=None), ': weight'),
                         (dict(density=None), ': density'), (dict(valid=None), ': valid'), (dict(colour=None), 'colour with rgb_out'),
                         (dict(colour=st['colour'].data_ptr() + 8), 'colour aligned to 16 bytes')]:
        rc = L.durf_tsdf_lattice(*dict(lat, **change).values())
        msg = _lib.lib().durf_last_error().decode()
        assert rc != 0 and 'durf_tsdf_lattice' in msg and text in msg, (change, msg)
    pts, sdf, ok = torch.zeros(4, 3, device=cuda), torch.full((4,), 7.0, device=cuda), torch.full((4,), 9, dtype=torch.uint8, device=cuda)
    f9 = (C.c_float * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1)
    smp = dict(stream=None, nu=3, nv=4, nw=5, origin=f3(0, 0, 0), inv=f9, tsdf=st['tsdf'].data_ptr(), weight=st['weight'].data_ptr(),
               colour=st['colour'].data_ptr(), trunc=0.5, min_weight=1.0, m=4, points=pts.data_ptr(), sdf=sdf.data_ptr(), ok=ok.data_ptr(), rgb_out=None)
    for change, text in [(dict(nv=0), 'nu, nv, nw >= 2'), (dict(m=-1), 'm >= 0'), (dict(trunc=-1.0), 'trunc > 0 and finite'), (dict(min_weight=nan), 'min_weight is a number'),
                         (dict(origin=None), 'origin_host'), (dict(inv=None), 'inv_host'), (dict(tsdf=None), ': tsdf'), (dict(weight=None), ': weight'),
                         (dict(points=None), 'points for m = 4'), (dict(sdf=None), 'sdf and ok for m = 4'), (dict(ok=None), 'sdf and ok for m = 4'),
                         (dict(colour=None, rgb_out=out3.data_ptr()), 'colour with rgb_out'),
                         (dict(colour=st['colour'].data_ptr() + 12), 'colour aligned to 16 bytes')]:
        rc = L.durf_tsdf_sample(*dict(smp, **change).values())
        msg = _lib.lib().durf_last_error().decode()
        assert rc != 0 and 'durf_tsdf_sample' in msg and text in msg, (change, msg)
    assert L.durf_tsdf_sample(*dict(smp, m=0, points=None, sdf=None, ok=None).values()) == 0
    torch.cuda.synchronize()
    assert (density == 0).all() and (valid == 0).all() and (out3 == 0).all() and (sdf == 7.0).all() and (ok == 9).all()
    # the host side refuses before the device is touched
    vol = tsdf.volume((0, 0, 0), shape, step=1.0, trunc=0.5, device=cuda)
    with pytest.raises(ValueError, match='without label'):
        tsdf.integrate(vol, cams, depth, carve=True)
    with pytest.raises(ValueError, match='points of shape'):
        tsdf.sample(vol, np.zeros((3, 2)))
    assert not vol['weight'].any()


# ---- 9 fuse_scene and the command ------------------------------------------------------------------------------------------------
def test_fuse_scene_and_the_command_on_the_synthetic_scene(cuda, tmp_path):
    out = str(tmp_path / 'fused')
    argv = ['--synthetic', '--objects', '--synthetic_boxes', '2', '--synthetic_size', '16', '24', '--frames', '2', '--grid=-2,-2,-1;12,12,12;0.35',
            '--obj_step', '0.06', '--min_component', '2', '--eval_dir', out, '--gin_param', 'MipNerfModel.num_samples = 32', '--gin_param', 'MipNerfModel.no_pose_opt = True',
            '--gin_param', 'MipNerfModel.no_yaw_opt = True']                  # the one-call inference path (bf16 object MLPs)
    run = subprocess.run([sys.executable, '-m', 'durf_amd.fuse_tsdf'] + argv, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    meta = json.load(open(os.path.join(out, 'tsdf.json')))
    assert meta['frames'] == 2 and (meta['h'], meta['w']) == (16, 24) and meta['background']['shape'] == [12, 12, 12] and len(meta['objects']) == 2
    for name, rec in [('background.ply', meta['background'])] + [('object_%02d.ply' % k, o) for k, o in enumerate(meta['objects'])]:
        m = mesh.read_ply(os.path.join(out, name))
        assert m['vertices'].shape[0] == rec['vertices'] and m['triangles'].shape[0] == rec['triangles'], name
        assert rec['triangles'] == 0 or m['triangles'].max() < rec['vertices']
    poses = np.load(os.path.join(out, 'poses.npy'))
    assert poses.ndim == 3 and poses.shape[1:] == (2, 6)
    # the same scene through fuse_scene: its background volume is a direct integrate of the same render_layers outputs
    from durf_amd import fuse_tsdf, raygen, trajectory
    from durf_amd.render_traj import open_scene, restore_model
    args = fuse_tsdf.build_parser().parse_args(argv)
    origin, shape, step = fuse_tsdf.check_args(args)
    dev, config, dataset = open_scene(args, boxes=args.synthetic_boxes)
    model, variables, alpha = restore_model(args, config, dataset, dev)
    focal, ppx, ppy, h, w = [float(x) for x in dataset.ts_data[0].cams[0][12:]]
    c2w, times = trajectory.make_trajectory([dataset.ts_data[0].cams[0, :12].reshape(3, 4), dataset.ts_data[-1].cams[-1, :12].reshape(3, 4)],
                                            [0.0, float(dataset.T - 1)], 2)
    cams = trajectory.camera_rows(c2w, focal, (ppx, ppy), int(h), int(w))
    s = tsdf.fuse_scene(model, variables, cams, times, dataset.ext, config.white_bkgd, alpha, origin, shape, step, 3.0 * step, obj_step=0.06,
                        near=config.near, far=config.far, batch=1, min_points=2)
    assert int(s['background']['vertices'].shape[0]) == meta['background']['vertices'] and len(s['objects']) == 2
    assert int(s['background']['observed']) == meta['background']['observed'] and s['frame_poses'].shape == (2, 2, 6)
    vol = tsdf.volume(origin, shape, step=step, trunc=3.0 * step, device=dev)
    poses_f = torch.as_tensor(s['frame_poses']).to(dev)
    for f in range(2):
        lay = model.render_layers(variables, raygen.camera_rays(cams[f], config.near, config.far, device=dev), None, dataset.ext, int(np.floor(times[f])),
                                  config.white_bkgd, alpha, pose=poses_f[f], layers=('instance', 'background'))
        tsdf.integrate(vol, cams[f:f + 1], lay['bg_distance'].reshape(1, 16, 24), acc=lay['bg_acc'].reshape(1, 16, 24), rgb=lay['bg_rgb'].reshape(1, 16, 24, 3))
    for k in ('tsdf', 'weight', 'colour'):
        assert torch.equal(vol[k].view(torch.int32), s['volumes']['background'][k].view(torch.int32)), k
    assert bool((vol['weight'] > 0).any())
