"""libdurf_parts.so on the device against tests/parts_ref.py (include/durf_parts.h in numpy): labels, component numbers, count,
sizes and index bounds, and the compaction of a mesh to the kept components.  Every comparison is integer or bit equality.
The shapes come from the tile extents the header names: one point fewer, the same and one more than a tile, more than one
tile along every axis, k longer than a wave."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from durf_amd import _lib, mesh, ops, parts
from tests import mesh_ref as M
from tests import parts_ref as P

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I32, U8 = torch.int32, torch.uint8
TI, TJ, TK = ops.PARTS_TILE_I, ops.PARTS_TILE_J, ops.PARTS_TILE_K
SHAPES = ((2, 2, 2), (TI, TJ, TK), (TI + 1, TJ + 1, TK + 1), (2 * TI - 1, 3, 2 * TK + 1), (3, 5, 70), (17, 6, 33))
CANARY = -7
_S = {}


def _d(a, cuda, dtype=torch.float32):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a)).to(device=cuda, dtype=dtype).contiguous()


def _np(t):
    return None if t is None else t.cpu().numpy()


def _device(cuda, d, v, iso):
    """label, number, stats through ops -> dict of host arrays as parts_ref.components returns them"""
    shape = d.shape
    dd, vv = _d(d, cuda), _d(v, cuda, U8)
    labels, ws = ops.parts_label(dd, vv, shape, iso)
    comp, count = ops.parts_number(labels, ws)
    c = int(count.cpu())
    size, bbox = ops.parts_stats(comp, shape, c)
    return dict(labels=_np(labels).reshape(shape), comp=_np(comp).reshape(shape), count=c, size=_np(size), bbox=_np(bbox))


def _same(got, want, what):
    assert got['count'] == want['count'], (what, got['count'], want['count'])
    for k in ('labels', 'comp', 'size', 'bbox'):
        assert got[k].dtype == np.int32 and got[k].shape == want[k].shape and (got[k] == want[k]).all(), (what, k)


def _patterns(shape):
    """(name, density, valid, iso): an IN point holds 1, an OUT point 0, iso = 0.5"""
    i, j, k = np.meshgrid(*[np.arange(s) for s in shape], indexing='ij')
    one, zero = np.ones(shape, np.float32), np.zeros(shape, np.float32)
    corner = zero.copy()
    corner[-1, -1, -1] = 1.0
    axis = int(np.argmax(shape))
    plane = [slice(None)] * 3
    plane[axis] = shape[axis] // 2
    plane = tuple(plane)
    out_plane, nan_plane, valid_plane = one.copy(), one.copy(), np.ones(shape, np.uint8)
    out_plane[plane], nan_plane[plane], valid_plane[plane] = 0.0, np.nan, 0
    return (('nothing in', zero, None, 0.5), ('everything in', one, None, 0.5), ('even parity', ((i + j + k) % 2 == 0).astype(np.float32), None, 0.5),
            ('the last corner', corner, None, 0.5), ('two slabs, an OUT plane', out_plane, None, 0.5),
            ('two slabs, a plane of valid = 0', one, valid_plane, 0.5), ('two slabs, a plane of NaN', nan_plane, None, 0.5))


# ---- 1. labels, numbers, sizes, bounds ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: '%dx%dx%d' % s)
def test_patterns_are_the_oracles_integer_for_integer(cuda, shape):
    for name, d, v, iso in _patterns(shape):
        want = P.components(d, v, iso)
        _same(_device(cuda, d, v, iso), want, name)
        if name == 'everything in':
            assert want['count'] == 1 and (want['labels'] == 0).all() and want['size'].tolist() == [d.size]
        if name == 'nothing in':
            assert want['count'] == 0 and (want['labels'] == -1).all()
        if name == 'the last corner':
            assert want['count'] == 1 and want['labels'][-1, -1, -1] == d.size - 1
        if name.startswith('two slabs') and min(shape) > 2:
            assert want['count'] == 2, name


def test_a_serpentine_across_every_tile_border(cuda):
    shape = (2 * TI + 1, 2 * TJ + 1, 2 * TK + 1)
    path = P.serpentine(shape)
    d = np.zeros(shape, np.float32)
    d[tuple(np.array(path).T)] = 1.0
    got = _device(cuda, d, None, 0.5)
    _same(got, P.components(d, None, 0.5), 'the chain')
    assert got['count'] == 1 and got['labels'][path[-1]] == 0 and path[-1] == tuple(s - 1 for s in shape)
    assert (got['labels'][d > 0] == 0).all() and got['size'].tolist() == [len(path)]
    d[path[len(path) // 2]] = 0.0
    got = _device(cuda, d, None, 0.5)
    _same(got, P.components(d, None, 0.5), 'the cut chain')
    assert got['count'] == 2 and got['labels'][path[0]] == 0 and got['labels'][path[-1]] > 0


def _random(p_index):
    """successive draws of default_rng(0) at p = 0.1, 0.2, 0.3, and one valid plane with 10 % zeros"""
    if 'random' not in _S:
        rng = np.random.default_rng(0)
        fields = [(rng.random((17, 6, 33)) < p).astype(np.float32) for p in (0.1, 0.2, 0.3)]
        _S['random'] = fields, (np.random.default_rng(1).random((17, 6, 33)) >= 0.1).astype(np.uint8)
    return _S['random'][0][p_index], _S['random'][1]


@pytest.mark.parametrize('p_index', (0, 1, 2), ids=('p=0.1', 'p=0.2', 'p=0.3'))
def test_random_lattices_with_and_without_valid(cuda, p_index):
    d, valid = _random(p_index)
    for v in (None, valid):
        want = P.components(d, v, 0.5)
        print('%d components, the largest of %d points' % (want['count'], want['size'].max()))
        assert want['count'] > 1
        _same(_device(cuda, d, v, 0.5), want, 'valid' if v is not None else 'no valid')


def test_two_runs_give_the_same_bits_and_no_label_exceeds_its_index(cuda):
    d, _ = _random(2)
    dd = _d(d, cuda)
    a = ops.parts_label(dd, None, d.shape, 0.5)[0]
    b = ops.parts_label(dd, None, d.shape, 0.5)[0]
    assert torch.equal(a, b)
    lab = _np(a)
    assert (lab <= np.arange(lab.size)).all() and ((lab >= 0) == (d.reshape(-1) > 0)).all()


def test_components_past_the_capacity_are_not_written(cuda):
    d, v = _random(1)
    want = P.components(d, v, 0.5)
    c = want['count']
    comp = _d(want['comp'].reshape(-1), cuda, I32)
    size, bbox = torch.full((c,), CANARY, dtype=I32, device=cuda), torch.full((c, 6), CANARY, dtype=I32, device=cuda)
    ops.parts_stats(comp, d.shape, c - 1, size=size, bbox=bbox)
    assert (_np(size)[:c - 1] == want['size'][:c - 1]).all() and (_np(bbox)[:c - 1] == want['bbox'][:c - 1]).all()
    assert _np(size)[c - 1] == CANARY and (_np(bbox)[c - 1] == CANARY).all()
    # rows of numbers no component has: size 0 and the empty bounds
    size, bbox = ops.parts_stats(comp, d.shape, c + 2)
    assert _np(size)[c:].tolist() == [0, 0] and _np(bbox)[c:].tolist() == [[2 ** 31 - 1] * 3 + [-1] * 3] * 2
    assert (_np(size)[:c] == want['size']).all()


def test_a_refused_call_touches_nothing(cuda):
    L = _lib.parts_lib()
    err = lambda: _lib.lib().durf_last_error().decode()
    s = torch.cuda.current_stream().cuda_stream
    n = 64
    d = torch.ones(n, device=cuda)
    ws = torch.full((L.durf_parts_workspace_bytes(4, 4, 4),), 0x5a, dtype=U8, device=cuda)
    out = [torch.full((n,), CANARY, dtype=I32, device=cuda) for _ in range(5)]
    size, bbox, two = torch.full((8,), CANARY, dtype=I32, device=cuda), torch.full((8, 6), CANARY, dtype=I32, device=cuda), \
        torch.full((2,), CANARY, dtype=I32, device=cuda)
    keep, counts = torch.ones(3, dtype=U8, device=cuda), torch.tensor([4, 4], dtype=I32, device=cuda)
    p = lambda t: t.data_ptr()
    lab = lambda shape=(4, 4, 4), dp=p(d), iso=0.5, w=p(ws), nb=ws.numel(), o=p(out[0]): L.durf_parts_label(s, *shape, dp, None, iso, w, nb, o)
    num = lambda m=n, lb=p(out[0]), w=p(ws), nb=ws.numel(), c=p(out[1]), k=p(two): L.durf_parts_number(s, m, lb, w, nb, c, k)
    st = lambda shape=(4, 4, 4), c=p(out[1]), mc=8, sz=p(size), bb=p(bbox): L.durf_parts_stats(s, *shape, c, mc, sz, bb)

    def sel(mv=16, mt=16, nc=3, w=p(ws), nb=ws.numel(), k=p(keep), cout=p(two)):
        return L.durf_parts_select_mesh(s, p(counts), mv, mt, p(out[1]), p(out[2]), k, nc, w, nb, p(out[3]), p(out[4]), p(out[2]), cout)
    cases = ((lab, dict(shape=(1, 4, 4)), 'nu = 1'), (lab, dict(shape=(512, 512, 512)), '512 x 512 x 512'), (lab, dict(iso=float('nan')), 'iso = nan'),
             (lab, dict(dp=None), 'density and labels'), (lab, dict(o=None), 'density and labels'), (lab, dict(w=None), 'workspace aligned'),
             (lab, dict(w=p(ws) + 4), 'workspace aligned'), (lab, dict(nb=ws.numel() - 1), 'durf_parts_workspace_bytes(4, 4, 4) = %d' % ws.numel()),
             (num, dict(m=0), 'n = 0'), (num, dict(lb=None), 'labels, comp and count'), (num, dict(w=p(ws) + 4), 'workspace aligned'),
             (num, dict(nb=ws.numel() - 1), 'workspace of %d bytes' % (ws.numel() - 1)),
             (st, dict(shape=(4, 4, 1)), 'nw = 1'), (st, dict(mc=-1), 'max_components = -1'), (st, dict(c=None), 'comp'),
             (st, dict(sz=None), 'size and bbox'), (sel, dict(mv=-1), 'max_vertices = -1'), (sel, dict(mt=-1), 'max_triangles = -1'),
             (sel, dict(nc=-1), 'n_components = -1'), (sel, dict(k=None), 'keep for n_components = 3'), (sel, dict(cout=None), 'counts and counts_out'),
             (sel, dict(w=p(ws) + 4), 'workspace aligned'), (sel, dict(mt=4096, nb=128), 'workspace of 128 bytes'))
    for fn, kw, text in cases:
        assert fn(**kw) != 0 and text in err(), (kw, err())
    torch.cuda.synchronize()
    assert all(bool((t == CANARY).all()) for t in out + [size, bbox, two]) and bool((ws == 0x5a).all())


# ---- 2. the mesh without its floaters -----------------------------------------------------------------------------------------------
BLOBS_SEED = 3
SMALL = (((2, 2, 2),), ((20, 3, 24), (20, 3, 25)), ((3, 16, 3), (4, 17, 3)), ((21, 16, 20), (22, 17, 21)), ((13, 2, 15),))


def _blobs(cuda):
    """three Gaussian blobs and five of one or two lattice points, a one-point OUT margin all round; at iso = 0.5 eight components"""
    if 'blobs' not in _S:
        shape = (24, 20, 28)
        rng = np.random.default_rng(BLOBS_SEED)
        ijk = np.stack(np.meshgrid(*[np.arange(s) for s in shape], indexing='ij'), -1).astype(np.float64)
        d = np.zeros(shape)
        for c in ((7, 6, 8), (16, 13, 9), (10, 10, 21)):
            d += np.exp(-((ijk - (np.asarray(c) + rng.uniform(-0.3, 0.3, 3))) ** 2).sum(-1) / (2 * 2.5 ** 2))
        for pts in SMALL:
            for q in pts:
                d[q] += 1.0
        d[0] = d[-1] = d[:, 0] = d[:, -1] = d[:, :, 0] = d[:, :, -1] = 0.0
        d = d.astype(np.float32)
        ref = P.components(d, None, 0.5)
        g = dict(density=_d(d, cuda), valid=None, frame=M.unit_frame(0.25, (-3.0, -2.5, -3.5)))
        m = mesh.surface(g, 0.5)
        p = parts.components(g, 0.5)
        _S['blobs'] = dict(d=d, ref=ref, g=g, m=m, p=p, vc=parts.vertex_components(m, g, p))
    return _S['blobs']


def test_components_is_the_oracle_on_the_blobs(cuda):
    s = _blobs(cuda)
    ref, p = s['ref'], s['p']
    assert ref['count'] == 8 and sorted(ref['size'].tolist())[:5] == [1, 1, 2, 2, 2] and min(sorted(ref['size'].tolist())[5:]) >= 90
    assert p['n'] == 8 and int(p['count'].cpu()) == 8 and p['shape'] == (24, 20, 28) and p['iso'] == 0.5
    for k in ('labels', 'comp', 'size', 'bbox'):
        assert p[k].dtype == I32 and (_np(p[k]) == ref[k]).all(), k
    assert not bool(p['touches_border'].any())
    g2 = dict(s['g'], density=s['g']['density'][1:-1, 1:, :-1].contiguous())
    want = P.components(s['d'][1:-1, 1:, :-1], None, 0.99)
    hi = np.array(want['labels'].shape) - 1
    touches = parts.components(g2, 0.99)['touches_border']
    assert _np(touches).tolist() == ((want['bbox'][:, :3] == 0) | (want['bbox'][:, 3:] == hi)).any(1).tolist()
    k = parts.keep(p, seeds=[SMALL[1][0], (7, 6, 8), (0, 0, 0)])
    assert _np(k).tolist() == [c in (ref['comp'][SMALL[1][0]], ref['comp'][7, 6, 8]) for c in range(8)]
    msk = parts.mask(p, parts.keep(p, min_points=10))
    assert msk.dtype == U8 and (_np(msk) == ((ref['comp'] >= 0) & (ref['size'][np.maximum(ref['comp'], 0)] >= 10))).all()


def test_every_triangle_lies_in_one_component(cuda):
    s = _blobs(cuda)
    m, vc = s['m'], _np(s['vc'])
    tri = _np(m['triangles'])
    assert tri.shape[0] > 1000 and vc.shape[0] == m['vertices'].shape[0]
    assert (vc == P.vertex_component(s['ref']['comp'], _np(m['vertex_edge']), P.in_points(s['d'], None, 0.5))).all() and (vc >= 0).all()
    assert (vc[tri[:, 0]] == vc[tri[:, 1]]).all() and (vc[tri[:, 0]] == vc[tri[:, 2]]).all()
    assert sorted(np.unique(vc).tolist()) == list(range(8))


def _bits(t):
    return t.contiguous().view(I32) if t.dtype == torch.float32 else t


def test_select_is_a_compaction_that_keeps_order_and_bits(cuda):
    s = _blobs(cuda)
    m, p, vc = s['m'], s['p'], s['vc']
    k = parts.keep(p, min_points=10)
    assert _np(k).tolist() == (s['ref']['size'] >= 10).tolist() and int(k.sum()) == 3
    vmap, vsrc, tout, (nv, nt) = P.select_mesh(_np(vc), _np(m['triangles']), _np(k))
    got = ops.parts_select_mesh(m['counts'], vc, m['triangles'], k.to(U8))
    assert tuple(int(x) for x in got[3].cpu()) == (nv, nt) and 0 < nv < vc.shape[0] and 0 < nt < m['triangles'].shape[0]
    assert (_np(got[0]) == vmap).all() and (_np(got[1])[:nv] == vsrc).all() and (_np(got[2])[:nt] == tout).all()
    o = parts.select(m, s['g'], p, k)
    assert set(o) == set(m) | {'component'}
    assert tuple(int(x) for x in o['counts'].cpu()) == (nv, nt)
    assert o['triangles'].dtype == I32 and (_np(o['triangles']) == tout).all()
    src = torch.as_tensor(vsrc.astype(np.int64), device=cuda)
    for key in ('vertices', 'normals', 'vertex_t', 'vertex_edge'):
        assert o[key].shape[0] == nv and torch.equal(_bits(o[key]), _bits(m[key][src])), key
    assert (_np(o['component']) == _np(vc)[vsrc]).all() and o['component'].dtype == I32
    assert o['frame'] == m['frame'] and o['iso'] == m['iso'] and o['shape'] == m['shape']
    assert M.is_closed(_np(o['triangles'])), 'the margin makes every kept shell closed'
    assert M.is_closed(_np(m['triangles']))
    # a component of -1 (a hole next to an unusable point) is dropped, whatever keep says
    vc2 = vc.clone()
    vc2[::3] = -1
    got2 = ops.parts_select_mesh(m['counts'], vc2, m['triangles'], torch.ones(8, dtype=U8, device=cuda))
    want2 = P.select_mesh(_np(vc2), _np(m['triangles']), np.ones(8, bool))
    assert tuple(int(x) for x in got2[3].cpu()) == want2[3] and (_np(got2[0]) == want2[0]).all()
    # capacities smaller than the counts: V and T are the capacities
    mv, mt = vc.shape[0] - 5, m['triangles'].shape[0] - 7
    got3 = ops.parts_select_mesh(m['counts'], vc[:mv].contiguous(), m['triangles'][:mt].contiguous(), k.to(U8))
    tri3 = _np(m['triangles'])[:mt]
    inside = (tri3 < mv).all(1)
    want3 = P.select_mesh(_np(vc)[:mv], np.where(inside[:, None], tri3, 0), _np(k))
    assert int(got3[3][0].cpu()) == want3[3][0] and (_np(got3[0]) == want3[0]).all()


def test_split_gives_every_kept_component_its_own_mesh(cuda):
    s = _blobs(cuda)
    m, p = s['m'], s['p']
    everything = torch.ones(8, dtype=torch.bool, device=cuda)
    whole = parts.select(m, s['g'], p, everything)
    assert torch.equal(whole['triangles'], m['triangles']) and torch.equal(_bits(whole['vertices']), _bits(m['vertices']))
    pieces = parts.split(m, s['g'], p, everything)
    assert len(pieces) == 8 and sum(int(q['triangles'].shape[0]) for q in pieces) == int(whole['triangles'].shape[0])
    for c, q in enumerate(pieces):
        assert bool((q['component'] == c).all()) and q['vertices'].shape[0] > 0 and M.is_closed(_np(q['triangles']))
    two = parts.split(m, s['g'], p, parts.keep(p, largest=2))
    assert len(two) == 2 and sorted(int(q['component'][0]) for q in two) == sorted(np.argsort(-s['ref']['size'], kind='stable')[:2].tolist())


# ---- 3. with the model ---------------------------------------------------------------------------------------------------------------
GRID = dict(origin=(-0.2, -0.8, -0.5), shape=(24, 24, 12), step=0.06)


def test_extract_with_the_keywords_at_their_defaults_is_todays_extract(cuda):
    from durf_amd import field
    from tests import test_gpu_field as TF
    s = TF._scene(cuda)
    kw = dict(ext=s['ext'], box_enable=s['en'], colour='grid')
    g = field.grid(s['model'], s['variables'], GRID['origin'], GRID['shape'], step=GRID['step'], ext=s['ext'], box_enable=s['en'])
    iso = float(g['density'][g['valid'] != 0].median())
    a = mesh.extract(s['model'], s['variables'], GRID['origin'], GRID['shape'], step=GRID['step'], iso=iso, **kw)
    b = mesh.extract(s['model'], s['variables'], GRID['origin'], GRID['shape'], step=GRID['step'], iso=iso, min_points=0, largest=None, **kw)
    assert set(a) == set(b) == {'vertices', 'normals', 'vertex_edge', 'vertex_t', 'triangles', 'counts', 'frame', 'iso', 'shape', 'rgb', 'owner'}
    for key in a:
        if torch.is_tensor(a[key]):
            assert a[key].dtype == b[key].dtype and torch.equal(_bits(a[key]), _bits(b[key])), key
        else:
            assert a[key] == b[key], key
    # opted in: the oracle's components of the same grid, the big ones kept
    c = mesh.extract(s['model'], s['variables'], GRID['origin'], GRID['shape'], step=GRID['step'], iso=iso, min_points=3, **kw)
    ref = P.components(_np(g['density']), _np(g['valid']), iso)
    kept = ref['size'] >= 3
    assert c['cleaning'] == dict(components=ref['count'], kept=int(kept.sum()), dropped_points=int(ref['size'][~kept].sum()),
                                 sizes=ref['size'][kept].tolist())
    vc = P.vertex_component(ref['comp'], _np(a['vertex_edge']), P.in_points(_np(g['density']), _np(g['valid']), iso))
    vmap, vsrc, tout, (nv, nt) = P.select_mesh(vc, _np(a['triangles']), kept)
    assert set(c) == set(a) | {'component', 'cleaning'} and (_np(c['triangles']) == tout).all() and (_np(c['component']) == vc[vsrc]).all()
    src = torch.as_tensor(vsrc.astype(np.int64), device=cuda)
    for key in ('vertices', 'normals', 'rgb', 'owner', 'vertex_edge', 'vertex_t'):
        assert torch.equal(_bits(c[key]), _bits(a[key][src])), key


def test_extract_mesh_command_with_and_without_the_flags(cuda, tmp_path):
    docs = []
    for extra in (['--min_component', '4'], []):
        out = str(tmp_path / ('mesh%d' % len(docs)))
        cmd = [sys.executable, '-m', 'durf_amd.extract_mesh', '--synthetic', '--eval_dir', out, '--iso', '0.001', '--grid=-2,-2,-1;16,16,8;0.25',
               '--gin_param', 'MipNerfModel.num_samples = 32', '--gin_param', 'MipNerfModel.no_pose_opt = True',
               '--gin_param', 'MipNerfModel.no_yaw_opt = True', '--gin_param', 'MipNerfModel.mlp_precision = \'f32\''] + extra
        p = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)      # a fresh child process
        assert p.returncode == 0, p.stdout.decode()
        docs.append((json.load(open(os.path.join(out, 'mesh.json'))), mesh.read_ply(os.path.join(out, 'background.ply'))))
    (with_flag, ply_with), (without, ply_without) = docs
    assert set(without) == {'iso', 'ts', 'sigma', 'step', 'background', 'objects'}, 'exactly today\'s keys'
    assert set(without['background']) == {'vertices', 'triangles', 'frame'} and 'component' not in ply_without
    assert set(with_flag) == set(without) | {'components', 'kept', 'dropped_points', 'sizes'}
    assert with_flag['kept'] == len(with_flag['sizes']) <= with_flag['components'] and all(n >= 4 for n in with_flag['sizes'])
    assert with_flag['background']['vertices'] <= without['background']['vertices']
    assert ply_with['component'].shape[0] == with_flag['background']['vertices'] == ply_with['vertices'].shape[0]
    assert with_flag['background']['vertices'] == 0 or set(np.unique(ply_with['component']).tolist()) <= set(range(with_flag['components']))
