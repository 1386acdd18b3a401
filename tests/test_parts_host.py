"""The connected components without a device: the agreement of include/durf_parts.h, durf_amd/_parts_sigs.py and
libdurf_parts.so's symbol table, every refusal of the entry points (they come before any launch), tests/parts_ref.py against
scipy.ndimage.label under the 14-neighbour structure and on the four two-point cases that tell this connectivity from 6, 18 and
26 neighbours, parts.keep's three rules and its tie-breaking on hand-made sizes, parts.mask, the `component` property of the
PLY writer and the two flags of the commands."""
import os

import numpy as np
import pytest
import torch

from durf_amd import _lib, eval_geometry, extract_mesh, mesh, ops, parts
from tests import parts_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = {'durf_parts_workspace_bytes', 'durf_parts_label', 'durf_parts_number', 'durf_parts_stats', 'durf_parts_select_mesh'}
FAKE = 4096              # a non-null, 256-byte aligned address no refused call may touch


def _err():
    return _lib.lib().durf_last_error().decode()


# ---- the binding ----------------------------------------------------------------------------------------------------------------
def test_header_sigs_and_symbol_table_agree():
    hdr = open(os.path.join(ROOT, 'include', 'durf_parts.h')).read()
    assert ENTRY == set(_lib.parts_symbols())          # (header == table == symbol table: tests/test_satellites_host.py)
    assert 'parts' in _lib.SATELLITES and len(_lib.symbols()) == 118, 'libdurf_hip.so keeps its entry points'
    assert (ops.PARTS_TILE_I, ops.PARTS_TILE_J, ops.PARTS_TILE_K) == (4, 4, 16)
    assert ops.PARTS_TILE_POINTS == ops.PARTS_TILE_I * ops.PARTS_TILE_J * ops.PARTS_TILE_K == ops.PARTS_BLOCK
    for rule in ('14 neighbours', 'its LABEL is the smallest g in it', 'ascending order of their labels', 'old = atomicMin(&L[a], b)',
                 'Same inputs, same bits', 'relaxed atomic loads at agent scope', 'Every loop is bounded by construction',
                 'strictly decreasing indices', 'No workgroup waits for another', 'A stale read costs a retry, never a wrong union'):
        assert rule in hdr, rule


def test_every_refusal_comes_before_a_launch():
    L = _lib.parts_lib()
    big = 1 << 40
    need = L.durf_parts_workspace_bytes(4, 4, 4)
    assert need == 256 + 256 and L.durf_parts_workspace_bytes(1, 4, 4) == 0 and L.durf_parts_workspace_bytes(512, 512, 512) == 0
    assert L.durf_parts_workspace_bytes(3, 5, 70) == 4352 + 256 and L.durf_parts_workspace_bytes(511, 512, 512) > 4 * 511 * 512 * 512
    lab = lambda shape=(4, 4, 4), d=FAKE, iso=0.0, ws=FAKE, nb=big, out=FAKE: L.durf_parts_label(None, *shape, d, None, iso, ws, nb, out)
    for kw, text in ((dict(shape=(1, 4, 4)), 'nu = 1, nv = 4, nw = 4'), (dict(shape=(4, 4, 0)), 'nw = 0'),
                     (dict(shape=(512, 512, 512)), '512 x 512 x 512'), (dict(iso=float('nan')), 'iso = nan'),
                     (dict(d=None), 'density and labels'), (dict(out=None), 'density and labels'), (dict(ws=None), 'workspace aligned'),
                     (dict(ws=FAKE + 8), 'workspace aligned'),
                     (dict(nb=need - 1), 'workspace of %d bytes, durf_parts_workspace_bytes(4, 4, 4) = %d' % (need - 1, need))):
        assert lab(**kw) != 0 and text in _err() and 'durf_parts_label' in _err(), (kw, _err())
    num = lambda n=64, lb=FAKE, ws=FAKE, nb=big, comp=FAKE, count=FAKE: L.durf_parts_number(None, n, lb, ws, nb, comp, count)
    for kw, text in ((dict(n=0), 'n = 0'), (dict(n=1 << 27), 'n = %d' % (1 << 27)), (dict(lb=None), 'labels, comp and count'),
                     (dict(comp=None), 'labels, comp and count'), (dict(count=None), 'labels, comp and count'),
                     (dict(ws=None), 'workspace aligned'), (dict(ws=FAKE + 4), 'workspace aligned'),
                     (dict(nb=need - 1), 'workspace of %d bytes' % (need - 1))):
        assert num(**kw) != 0 and text in _err() and 'durf_parts_number' in _err(), (kw, _err())
    assert '= %d' % need in _err()
    st = lambda shape=(4, 4, 4), comp=FAKE, mc=8, size=FAKE, bbox=FAKE: L.durf_parts_stats(None, *shape, comp, mc, size, bbox)
    for kw, text in ((dict(shape=(4, 1, 4)), 'nv = 1'), (dict(shape=(1024, 1024, 128)), '1024 x 1024 x 128'),
                     (dict(mc=-1), 'max_components = -1'), (dict(comp=None), 'comp'), (dict(size=None), 'size and bbox for max_components = 8'),
                     (dict(bbox=None), 'size and bbox for max_components = 8')):
        assert st(**kw) != 0 and text in _err() and 'durf_parts_stats' in _err(), (kw, _err())
    assert st(mc=0, size=None, bbox=None) == 0                                           # nothing to write: no launch

    def sel(counts=FAKE, mv=8, mt=8, vc=FAKE, tri=FAKE, keep=FAKE, nc=3, ws=FAKE, nb=big, vmap=FAKE, vsrc=FAKE, tout=FAKE, cout=FAKE):
        return L.durf_parts_select_mesh(None, counts, mv, mt, vc, tri, keep, nc, ws, nb, vmap, vsrc, tout, cout)
    for kw, text in ((dict(mv=-1), 'max_vertices = -1'), (dict(mt=-2), 'max_triangles = -2'), (dict(nc=-1), 'n_components = -1'),
                     (dict(counts=None), 'counts and counts_out'), (dict(cout=None), 'counts and counts_out'),
                     (dict(vc=None), 'vertex_comp, vertex_map and vertex_src for max_vertices = 8'),
                     (dict(vmap=None), 'vertex_comp, vertex_map and vertex_src'), (dict(vsrc=None), 'vertex_comp, vertex_map and vertex_src'),
                     (dict(tri=None), 'triangles and triangles_out for max_triangles = 8'), (dict(tout=None), 'triangles and triangles_out'),
                     (dict(keep=None), 'keep for n_components = 3'), (dict(ws=None), 'workspace aligned'), (dict(ws=FAKE + 16), 'workspace aligned'),
                     (dict(mv=300, mt=700, nb=255), 'workspace of 255 bytes, the block sums of 300 vertices and 700 triangles = 256')):
        assert sel(**kw) != 0 and text in _err() and 'durf_parts_select_mesh' in _err(), (kw, _err())


# ---- the oracle -----------------------------------------------------------------------------------------------------------------
def _two(shape, a, b):
    inn = np.zeros(shape, bool)
    inn[a], inn[b] = True, True
    return P.number(P.labels_of(inn))[1]


def test_the_four_cases_that_tell_this_connectivity_from_6_18_and_26():
    s, p = (4, 4, 4), np.array((1, 1, 1))
    at = lambda *o: tuple(p + np.array(o))
    assert _two(s, at(0, 0, 0), at(1, 1, 0)) == 1, 'the (+,+) face diagonal connects (6 neighbours would not)'
    assert _two(s, at(1, 0, 0), at(0, 1, 0)) == 2, 'the (+,-) face diagonal does not (18 and 26 neighbours would)'
    assert _two(s, at(0, 0, 0), at(1, 1, 1)) == 1, 'the (+,+,+) body diagonal connects (6 and 18 neighbours would not)'
    assert _two(s, at(0, 0, 1), at(1, 1, 0)) == 2, 'the other body diagonals do not (26 neighbours would)'
    st = P.scipy_structure()
    assert int(st.sum()) == 15 and (st == st[::-1, ::-1, ::-1]).all()
    assert st[2, 2, 1] and st[0, 0, 1] and not st[2, 0, 1] and st[2, 2, 2] and not st[2, 2, 0] and not st[0, 2, 2]


def test_the_oracle_is_scipys_labelling_under_the_14_neighbour_structure():
    ndimage = pytest.importorskip('scipy.ndimage')
    rng = np.random.default_rng(0)
    for shape, p in (((17, 6, 33), 0.1), ((17, 6, 33), 0.2), ((17, 6, 33), 0.3), ((5, 9, 7), 0.5), ((2, 2, 2), 0.5), ((9, 9, 9), 0.25)):
        d = rng.random(shape).astype(np.float32)
        valid = (rng.random(shape) >= 0.1).astype(np.uint8)
        d[rng.random(shape) < 0.03] = np.nan
        for v in (None, valid):
            inn = P.in_points(1.0 - d, v, 1.0 - p)
            want, count = ndimage.label(inn, structure=P.scipy_structure())
            got = P.labels(1.0 - d, v, 1.0 - p)
            assert (got == P.min_index_labels(want)).all(), (shape, p)
            comp, c = P.number(got)
            assert c == count and ((comp >= 0) == inn).all()
            # scipy numbers in scan order of the first point met, which is ascending minimum index: the same numbering
            assert (comp == want.astype(np.int32) - 1).all()
            size, bbox = P.stats(comp, c)
            assert int(size.sum()) == int(inn.sum())
            for k, sl in enumerate(ndimage.find_objects(want)):
                assert bbox[k].tolist() == [s.start for s in sl] + [s.stop - 1 for s in sl]


def test_the_serpentine_is_one_component_and_a_cut_makes_two():
    T = (ops.PARTS_TILE_I, ops.PARTS_TILE_J, ops.PARTS_TILE_K)
    shape = tuple(2 * t + 1 for t in T)
    path = P.serpentine(shape)
    assert len(set(path)) == len(path) and path[0] == (0, 0, 0) and path[-1] == tuple(s - 1 for s in shape)
    inn = np.zeros(shape, bool)
    inn[tuple(np.array(path).T)] = True
    lab = P.labels_of(inn)
    assert P.number(lab)[1] == 1 and lab[path[-1]] == 0 and (lab[inn] == 0).all()
    mid = path[len(path) // 2]
    assert 2 < mid[2] < shape[2] - 3, 'the cut lies inside a run along k'
    inn[mid] = False
    lab = P.labels_of(inn)
    assert P.number(lab)[1] == 2 and lab[path[-1]] > 0 and lab[path[0]] == 0


def test_select_mesh_of_the_oracle_keeps_order():
    vc = np.array([0, 1, -1, 1, 2, 0], np.int32)
    tri = np.array([[0, 5, 5], [1, 3, 3], [4, 4, 4], [3, 1, 1], [5, 0, 0]], np.int32)
    vmap, vsrc, out, counts = P.select_mesh(vc, tri, [1, 0, 1])
    assert vmap.tolist() == [0, -1, -1, -1, 1, 2] and vsrc.tolist() == [0, 4, 5] and counts == (3, 3)
    assert out.tolist() == [[0, 2, 2], [1, 1, 1], [2, 0, 0]]


# ---- durf_amd/parts.py ----------------------------------------------------------------------------------------------------------
def _parts(size, comp=None, shape=(2, 2, 2)):
    size = torch.tensor(size, dtype=torch.int32)
    return dict(size=size, n=int(size.numel()), comp=comp, shape=shape)


def test_keeps_three_rules_and_its_tie_breaking():
    p = _parts([5, 9, 1, 9, 5, 9, 2])
    assert parts.keep(p).tolist() == [True] * 7
    assert parts.keep(p, min_points=5).tolist() == [True, True, False, True, True, True, False]
    assert parts.keep(p, min_points=10).tolist() == [False] * 7
    assert parts.keep(p, largest=0).tolist() == [False] * 7
    assert parts.keep(p, largest=2).tolist() == [False, True, False, True, False, False, False], 'of three 9s the two smaller numbers'
    assert parts.keep(p, largest=4).tolist() == [True, True, False, True, False, True, False], 'of two 5s the smaller number'
    assert parts.keep(p, largest=99).tolist() == [True] * 7
    assert parts.keep(p, largest=4, min_points=6).tolist() == [False, True, False, True, False, True, False], 'AND'
    comp = torch.tensor([[[0, -1], [1, 1]], [[-1, 2], [2, 3]]], dtype=torch.int32)
    q = _parts([1, 2, 2, 1], comp)
    assert parts.keep(q, seeds=[[0, 1, 0]]).tolist() == [False, True, False, False]
    assert parts.keep(q, seeds=[[0, 0, 1]]).tolist() == [False] * 4, 'a seed on a point that is not in selects nothing'
    assert parts.keep(q, seeds=torch.tensor([[1, 1, 1], [0, 0, 0], [1, 0, 0]])).tolist() == [True, False, False, True]
    assert parts.keep(q, seeds=[[0, 1, 1], [1, 1, 0]], min_points=2, largest=1).tolist() == [False, True, False, False]
    assert parts.keep(q, seeds=np.zeros((0, 3), np.int64)).tolist() == [False] * 4
    with pytest.raises(ValueError, match='outside the lattice'):
        parts.keep(q, seeds=[[0, 2, 0]])
    with pytest.raises(ValueError, match='largest'):
        parts.keep(q, largest=-1)
    m = parts.mask(q, torch.tensor([True, False, True, False]))
    assert m.dtype == torch.uint8 and m.tolist() == [[[1, 0], [0, 0]], [[0, 1], [1, 0]]]
    with pytest.raises(ValueError, match='on the device'):
        parts.components(dict(density=torch.zeros(3, 3, 3)), 0.5)
    with pytest.raises(ValueError, match='no default'):
        parts.components(dict(density=torch.zeros(3, 3, 3)), None)


def test_the_ply_carries_the_component_only_when_the_mesh_has_it(tmp_path):
    m = dict(vertices=np.arange(12, dtype=np.float32).reshape(4, 3), triangles=np.array([[0, 1, 2], [1, 2, 3]], np.int32))
    path = str(tmp_path / 'm.ply')
    mesh.write_ply(path, m)
    plain = open(path, 'rb').read()
    assert b'component' not in plain and 'component' not in mesh.read_ply(path)
    mesh.write_ply(path, dict(m, component=None))
    assert open(path, 'rb').read() == plain
    mesh.write_ply(path, dict(m, component=torch.tensor([3, 3, 0, 7], dtype=torch.int32)))
    blob = open(path, 'rb').read()
    assert b'property uchar blue\nproperty int component\nelement face 2\n' in blob and len(blob) == len(plain) + 4 * 4 + len('property int component\n')
    r = mesh.read_ply(path)
    assert r['component'].tolist() == [3, 3, 0, 7] and r['component'].dtype == np.int32
    assert (r['vertices'] == m['vertices']).all() and (r['triangles'] == m['triangles']).all()


def test_the_commands_take_the_two_flags():
    for mod in (extract_mesh, eval_geometry):
        ap = mod.build_parser()
        a = ap.parse_args(['--eval_dir', 'x', '--synthetic'])
        assert a.min_component == 0 and a.largest is None
        a = ap.parse_args(['--eval_dir', 'x', '--synthetic', '--min_component', '12', '--largest', '3'])
        assert a.min_component == 12 and a.largest == 3
        assert '--min_component' in ap.format_help() and '--largest' in ap.format_help()
