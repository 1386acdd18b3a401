"""The iso-surface on the device (include/durf_mesh.h, csrc/mesh.hip, durf_amd/mesh.py) against tests/mesh_ref.py.

The integer side is exact and leaves nobody out: the in / out decision is one comparison of the same float32 values on both
sides, so counts, triangles, vertex_edge, mask, voff and toff equal the oracle's integer for integer on every shape and field.
Shapes are the smallest that can go wrong: one cell, a lattice thinner than a tile, odd sizes, one long column whose offsets
cross every workgroup boundary ((2,2,4097): 65 workgroups of 256 points), and 65 x 66 x 67 = 287430 points = 1123 block sums,
more than the scan's one workgroup of 1024 holds in a round.

The float side is held to the project's gate (tests/test_gpu_flow.py, tests/test_gpu_field.py): four times the float32 twin's
own distance from the float64 oracle plus four ulp -- of the magnitude of the terms a position is summed from, of 1 for a unit
normal, of the larger end for an interpolated attribute, of t itself for t.  Every vertex is compared."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from durf_amd import field, mesh, ops
from tests import field_ref as F
from tests import mesh_ref as M

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I32, U8 = torch.int32, torch.uint8
SHAPES = ((2, 2, 2), (2, 3, 2), (3, 5, 7), (16, 16, 16), (17, 15, 33), (2, 2, 4097), (65, 66, 67))
SIGN_SEED = 1
CANARY = -7


def _d(a, cuda, dtype=torch.float32):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a)).to(device=cuda, dtype=dtype).contiguous()


def _np(t):
    return None if t is None else t.cpu().numpy()


def _frame(shape):
    """an oblique right-handed frame with awkward float32 components"""
    return dict(origin=[-1.3, 0.7, 2.1], du=[0.11, 0.01, 0.0], dv=[-0.01, 0.09, 0.02], dw=[0.0, -0.015, 0.1])


def _run(cuda, d, v, iso, frame, flip=None, normals=True, caps=None, out=None):
    """count + emit on the device -> (counts (V, T), dict of host arrays, (voff, toff, mask) host arrays)"""
    shape = d.shape
    dd, vv = _d(d, cuda), _d(v, cuda, U8)
    counts, ws = ops.mesh_count(dd, vv, shape, iso)
    V, T = (int(x) for x in counts.cpu())
    o, du, dv, dw, A, lh = mesh.host_frame(frame)
    mv, mt = (V, T) if caps is None else caps
    m = ops.mesh_emit(dd, vv, shape, iso, o, du, dv, dw, ws, mv, mt, normal_xform=A if normals else None, flip=lh if flip is None else flip,
                      out=out)
    views = tuple(_np(x) for x in ops.mesh_workspace_views(ws, shape))
    assert tuple(int(x) for x in counts.cpu()) == (V, T), 'emit leaves counts alone'
    return (V, T), {k: _np(x) for k, x in m.items()}, views, (dd, vv, counts, m)


def _sphere(shape, integer=False):
    c = (np.asarray(shape, np.float64) - 1) / 2 + (0.13, -0.21, 0.07)
    R = 0.37 * max(shape) if min(shape) > 2 else 1.7
    d = M.sphere_field(M.unit_frame(), shape, c, R)
    return np.rint(d).astype(np.float32) if integer else d


def _fields(shape):
    return (('signs', M.sign_field(shape, SIGN_SEED), 0.0), ('sphere', _sphere(shape), 0.0), ('all in', np.ones(shape, np.float32), 0.5),
            ('all out', np.zeros(shape, np.float32), 0.5))


# ---- 1. topology, exact ---------------------------------------------------------------------------------------------------------
def test_the_sign_field_holds_every_corner_pattern():
    assert M.corner_patterns(M.sign_field((16, 16, 16), SIGN_SEED), 0.0) == set(range(256))


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: '%dx%dx%d' % s)
def test_topology_is_the_oracles_integer_for_integer(cuda, shape):
    frame = _frame(shape)
    for name, d, iso in _fields(shape):
        want = M.topology(d, None, iso)
        (V, T), got, (voff, toff, mask), _ = _run(cuda, d, None, iso, frame, normals=False)
        assert (V, T) == want['counts'], (name, (V, T), want['counts'])
        assert (mask == want['mask']).all() and (voff == want['voff']).all() and (toff == want['toff']).all(), name
        assert (got['vertex_edge'] == want['vertex_edge']).all(), name
        assert (got['triangles'] == want['triangles']).all(), name
        if name in ('all in', 'all out'):
            assert (V, T) == (0, 0)
        elif name == 'signs':
            assert V > 0 and T > 0
    # nothing is written for an empty surface
    canary = dict(vertices=torch.full((4, 3), float(CANARY), device=cuda), triangles=torch.full((4, 3), CANARY, dtype=I32, device=cuda),
                  vertex_edge=torch.full((4, 2), CANARY, dtype=I32, device=cuda), vertex_t=torch.full((4,), float(CANARY), device=cuda))
    _run(cuda, np.ones(shape, np.float32), None, 0.5, frame, normals=False, caps=(4, 4), out=canary)
    assert all(bool((t == CANARY).all()) for t in canary.values())


def test_the_devices_own_surface_is_closed(cuda):
    for shape in ((16, 16, 16), (17, 15, 33)):
        d = M.sign_field(shape, SIGN_SEED, border=True)
        (V, T), got, _, _ = _run(cuda, d, None, 0.0, _frame(shape))
        assert T > 0 and M.is_closed(got['triangles']), 'every edge in exactly two triangles, with opposite directions'
        assert np.unique(got['triangles']).size == V
        assert M.signed_volume(got['vertices'], got['triangles']) > 0
        left = dict(_frame(shape), dv=_frame(shape)['dw'], dw=_frame(shape)['dv'])
        (_, _), lg, _, _ = _run(cuda, d, None, 0.0, left)
        assert M.is_closed(lg['triangles']) and M.signed_volume(lg['vertices'], lg['triangles']) > 0, 'flip for a left-handed frame'


# ---- 2. positions, t, normals, gathered floats --------------------------------------------------------------------------------
def _gate(got, want, twin, scale, what):
    err = np.abs(np.asarray(got, np.float64) - want)
    bound = 4 * np.abs(np.asarray(twin, np.float64) - want) + 4 * M.ulp32(scale)
    worst = float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0
    print('%s: worst err / bound %.3f over %d values' % (what, worst, err.size))
    assert (err <= bound).all(), what


@pytest.mark.parametrize('kind', ('sphere', 'integer', 'signs', 'holes'))
def test_positions_t_normals_and_attributes_at_the_gate(cuda, kind):
    shape = (17, 15, 33)
    frame = _frame(shape)
    v = None
    if kind == 'signs':
        d = M.sign_field(shape, SIGN_SEED) * np.random.default_rng(5).uniform(0.1, 3.0, shape).astype(np.float32)
    else:
        d = _sphere(shape, integer=kind == 'integer')
    if kind == 'holes':
        v = np.ones(shape, np.uint8)
        v[8, 4:9, 10:20] = 0
        d[3:6, 7, 16] = np.nan
    want = M.surface(d, v, 0.0, frame)
    twin = M.geometry(d, v, 0.0, frame, want['vertex_edge'], np.float32)
    (V, T), got, _, (dd, vv, counts, m) = _run(cuda, d, v, 0.0, frame)
    assert (V, T) == want['counts'] and (got['vertex_edge'] == want['vertex_edge']).all() and (got['triangles'] == want['triangles']).all()
    if kind == 'integer':
        assert (want['t'] == 0).any() and (want['t'] == 1).any(), 'corners with d == iso: t = 0 and t = 1'
    _gate(got['vertex_t'], want['t'], twin[0], want['t'], 't')
    o, du, dv, dw, _, _ = mesh.host_frame(frame)
    g = want['vertex_edge'][:, 0].astype(np.int64)
    q = np.stack([g // (shape[1] * shape[2]), g // shape[2] % shape[1], g % shape[2]], 1) + 1.0
    scale = np.abs(o)[None] + q[:, :1] * np.abs(du)[None] + q[:, 1:2] * np.abs(dv)[None] + q[:, 2:] * np.abs(dw)[None]
    _gate(got['vertices'], want['vertices'], twin[1], scale, 'vertices')
    assert np.isfinite(got['normals']).all()
    _gate(got['normals'], want['normals'], twin[2], 1.0, 'normals')
    # lattice attributes
    n = d.size
    attr = np.random.default_rng(9).normal(size=(n, 3)).astype(np.float32)
    label = np.random.default_rng(10).integers(-1, 2, n).astype(np.int32)
    of, oi = ops.mesh_gather(shape, counts, m['vertex_edge'], m['vertex_t'], attr_f=_d(attr, cuda), attr_i=_d(label, cuda, I32), density=dd,
                             valid=vv, iso=0.0)
    wf = M.gather_float(attr, want['vertex_edge'], got['vertex_t'].astype(np.float64), shape)
    tf = M.gather_float(attr, want['vertex_edge'], got['vertex_t'], shape, np.float32)
    gb = g + np.array([int(np.dot(M.offset(e + 1), (shape[1] * shape[2], shape[2], 1))) for e in want['vertex_edge'][:, 1]])
    _gate(_np(of), wf, tf, np.maximum(np.abs(attr[g]), np.abs(attr[gb])), 'gathered floats')
    assert (_np(oi) == M.gather_label(label, want['vertex_edge'], d, v, 0.0)).all() and set(np.unique(_np(oi))) == {-1, 0, 1}
    if kind == 'holes':
        fwd, bwd, same = M.edge_census(got['triangles'])
        assert (fwd <= 1).all() and (bwd <= 1).all() and (same == 0).all() and ((fwd + bwd) == 1).any(), 'open at the hole, never more than two'
        usable, _ = M.lattice_state(d, v, 0.0)
        ref = np.unique(got['triangles'])
        assert usable.reshape(-1)[g[ref]].all() and usable.reshape(-1)[gb[ref]].all()


def test_labels_are_the_in_ends(cuda):
    shape = (6, 7, 9)
    d = M.sign_field(shape, 3)
    owner = np.where(d > 0, np.random.default_rng(4).integers(0, 2, shape), -1).astype(np.int32)          # in: 0 or 1, out: -1
    (V, T), got, _, (dd, vv, counts, m) = _run(cuda, d, None, 0.0, M.unit_frame(), normals=False)
    _, oi = ops.mesh_gather(shape, counts, m['vertex_edge'], m['vertex_t'], attr_i=_d(owner.reshape(-1), cuda, I32), density=dd, iso=0.0)
    oi = _np(oi)
    assert V > 0 and (oi >= 0).all() and {0, 1} <= set(np.unique(oi)), 'never the out end\'s -1'
    assert (oi == M.gather_label(owner, got['vertex_edge'], d, None, 0.0)).all()


# ---- 3. capacities and determinism --------------------------------------------------------------------------------------------
def _canaries(cuda, V, T):
    return dict(vertices=torch.full((V, 3), float(CANARY), device=cuda), normals=torch.full((V, 3), float(CANARY), device=cuda),
                vertex_edge=torch.full((V, 2), CANARY, dtype=I32, device=cuda), vertex_t=torch.full((V,), float(CANARY), device=cuda),
                triangles=torch.full((T, 3), CANARY, dtype=I32, device=cuda))


def test_capacities_and_two_runs(cuda):
    shape = (17, 15, 33)
    d, frame = _sphere(shape), _frame(shape)
    (V, T), full, _, _ = _run(cuda, d, None, 0.0, frame)
    (V2, T2), again, _, _ = _run(cuda, d, None, 0.0, frame)
    assert (V, T) == (V2, T2) and all(full[k].tobytes() == again[k].tobytes() for k in full), 'two runs, the same bits'
    for mv, mt in ((V - 1, T - 1), (0, 0), (V, 0), (3, T)):
        out = _canaries(cuda, V, T)
        (Vc, Tc), part, _, _ = _run(cuda, d, None, 0.0, frame, caps=(mv, mt), out=out)
        assert (Vc, Tc) == (V, T), 'counts keeps the true totals'
        for k in ('vertices', 'normals', 'vertex_edge', 'vertex_t', 'triangles'):
            cap = mt if k == 'triangles' else mv
            assert part[k][:cap].tobytes() == full[k][:cap].tobytes(), (k, mv, mt)
            assert (part[k][cap:] == CANARY).all(), (k, mv, mt)


# ---- 4. with the model ----------------------------------------------------------------------------------------------------------
def _bits(t):
    return t.contiguous().view(I32) if t.dtype == torch.float32 else t


def _model_scene(cuda):
    from tests import test_gpu_field as TF
    return TF._scene(cuda)


GRID = dict(origin=(-0.2, -0.8, -0.5), shape=(24, 24, 12), step=0.06)


def test_extract_is_surface_of_the_grid_and_its_colours_are_the_query(cuda):
    s = _model_scene(cuda)
    kw = dict(ext=s['ext'], box_enable=s['en'])
    g = field.grid(s['model'], s['variables'], GRID['origin'], GRID['shape'], step=GRID['step'], **kw)
    dens = g['density'][g['valid'] != 0]
    iso = float(dens.median())
    print('density: min %.4f median %.4f max %.4f; owners %s' % (float(dens.min()), iso, float(dens.max()),
                                                                  np.unique(_np(g['owner'])).tolist()))
    a = mesh.surface(g, iso)
    b = mesh.extract(s['model'], s['variables'], GRID['origin'], GRID['shape'], step=GRID['step'], iso=iso, **kw)
    assert a['vertices'].shape[0] > 0 and a['triangles'].shape[0] > 0
    for k in ('vertices', 'normals', 'triangles', 'vertex_edge', 'vertex_t'):
        assert torch.equal(_bits(a[k]), _bits(b[k])), k
    q = field.query(s['model'], s['variables'], b['vertices'], mesh.view_of_normals(b['normals']), **kw)
    assert torch.equal(_bits(q['rgb']), _bits(b['rgb']))
    # (a vertex may itself lie in two boxes, between two lattice points that do not: the field has no colour there)
    assert bool((torch.isfinite(b['rgb']).all(1) == (q['valid'] != 0)).all()) and bool((q['valid'] != 0).any())
    want = M.gather_label(_np(g['owner']), _np(b['vertex_edge']), _np(g['density']), _np(g['valid']), iso)
    assert (_np(b['owner']) == want).all()
    c = mesh.extract(s['model'], s['variables'], GRID['origin'], GRID['shape'], step=GRID['step'], iso=iso, colour='grid', **kw)
    assert torch.equal(_bits(c['vertices']), _bits(b['vertices'])) and tuple(c['rgb'].shape) == tuple(b['rgb'].shape)
    ref = M.topology(_np(g['density']), _np(g['valid']), iso)
    assert (_np(b['triangles']) == ref['triangles']).all() and (_np(b['vertex_edge']) == ref['vertex_edge']).all()


def test_an_object_comes_out_in_its_own_frame(cuda):
    s = _model_scene(cuda)
    k, pad, step, iso = 0, 0.05, 0.05, 1e-3
    o = mesh.extract_object(s['model'], s['variables'], k, s['ext'], step, iso, pad=pad, box_enable=s['en'])
    P = _np(o['vertices']).astype(np.float64)
    assert P.shape[0] > 0 and o['triangles'].shape[0] > 0
    assert (np.abs(P) <= s['ext'][k].astype(np.float64)[None] * (1 + pad)).all()
    assert (_np(o['owner']) == k).all()
    assert M.is_closed(_np(o['triangles'])), 'the object closes at its faces: every lattice point of its grid is usable'
    assert tuple(o['rgb'].shape) == tuple(o['vertices'].shape) and bool(torch.isfinite(o['rgb']).all(1).any())
    # the same lattice meshed in the world frame: its vertices are c + R^T P
    g = o['grid']
    w = mesh.surface(g, iso)
    assert torch.equal(w['triangles'], o['triangles']) and torch.equal(w['vertex_edge'], o['vertex_edge'])
    c, R = o['pose']
    np.testing.assert_allclose(c, s['pose'][k, :3].astype(np.float64), rtol=0, atol=0)
    image = c[None] + P @ R
    d, v = _np(g['density']), _np(g['valid'])
    ve = _np(w['vertex_edge'])
    want = M.geometry(d, v, iso, g['frame'], ve, np.float64, normals=False)[1]
    twin = M.geometry(d, v, iso, g['frame'], ve, np.float32, normals=False)[1]
    twin_obj = M.geometry(d, v, iso, o['frame'], ve, np.float32, normals=False)[1]
    wobj = M.geometry(d, v, iso, o['frame'], ve, np.float64, normals=False)[1]
    # the image inherits the object-frame twin's error (R is orthonormal: no growth) and the rounding of the frames' float32 axes
    scale = np.abs(want).max() + np.abs(wobj).max()
    bound = 4 * (np.abs(twin - want).max() + np.abs(twin_obj - wobj).max()) + 4 * M.ulp32(scale) + np.abs(c[None] + wobj @ R - want).max()
    err = np.abs(image - _np(w['vertices']).astype(np.float64)).max()
    print('object image: err %.3e, bound %.3e' % (err, bound))
    assert err <= bound
    _gate(_np(w['vertices']), want, twin, np.abs(want).max() + 1.0, 'world-frame vertices')


def test_extract_mesh_command_on_the_synthetic_scene(cuda, tmp_path):
    out = str(tmp_path / 'mesh')
    cmd = [sys.executable, '-m', 'durf_amd.extract_mesh', '--synthetic', '--objects', '--eval_dir', out, '--iso', '0.001',
           '--grid=-2,-2,-1;16,16,8;0.25', '--obj_step', '0.1', '--gin_param', 'MipNerfModel.num_samples = 32',
           '--gin_param', 'MipNerfModel.no_pose_opt = True', '--gin_param', 'MipNerfModel.no_yaw_opt = True',
           '--gin_param', 'MipNerfModel.mlp_precision = \'f32\'']
    p = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)      # a fresh child process
    assert p.returncode == 0, p.stdout.decode()
    print(p.stdout.decode()[-400:])
    meta = json.load(open(os.path.join(out, 'mesh.json')))
    K = len(meta['objects'])
    assert K == 3 and sorted(os.listdir(out)) == sorted(['background.ply', 'mesh.json', 'poses.npy'] + ['object_%02d.ply' % k for k in range(K)])
    poses = np.load(os.path.join(out, 'poses.npy'))
    assert poses.ndim == 3 and poses.shape[1:] == (K, 6) and meta['iso'] == 0.001
    for name, rec in [('background.ply', meta['background'])] + [('object_%02d.ply' % k, meta['objects'][k]) for k in range(K)]:
        r = mesh.read_ply(os.path.join(out, name))
        assert r['vertices'].shape[0] == rec['vertices'] and r['triangles'].shape[0] == rec['triangles'], name
        assert r['triangles'].size == 0 or (0 <= r['triangles'].min() and r['triangles'].max() < rec['vertices'])
    assert all(rec['triangles'] > 0 for rec in meta['objects']), 'every box closes at its faces'
