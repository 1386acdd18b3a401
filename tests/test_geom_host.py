"""Geometry metrics without a device: the three-way agreement of include/durf_geom.h, durf_amd/_geom_sigs.py and
libdurf_geom.so's symbol table, every refusal of the entry points (they come before any launch), the two brute-force
references of tests/geom_ref.py against each other, cloud_distance's host arithmetic from hand-made statistic rows, the grid
rule and its refusal, and the pure-host parts of durf_amd/geometry.py."""
import ctypes as C
import os

import numpy as np
import pytest

from durf_amd import _lib, eval_geometry, geometry, ops
from tests import geom_ref as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = {'durf_geom_workspace_bytes', 'durf_geom_keys', 'durf_geom_nearest', 'durf_geom_stats', 'durf_geom_sample_mesh'}
FAKE = 4096              # a non-null, 256-byte aligned address no refused call may touch


def _err():
    return _lib.lib().durf_last_error().decode()


# ---- the binding ----------------------------------------------------------------------------------------------------------------
def test_header_sigs_and_symbol_table_agree():
    hdr = open(os.path.join(ROOT, 'include', 'durf_geom.h')).read()
    assert ENTRY == set(_lib.geom_symbols())           # (header == table == symbol table: tests/test_satellites_host.py)
    # (the constants against the header: tests/test_headers_host.py)
    assert geometry.MAX_CELLS == ops.GEOM_MAX_CELLS == 2048 and geometry.SLACK == 1 + 2.0 ** -10
    assert ops.GEOM_STAT_DOUBLES == len(ops.GEOM_STAT_FIELDS) + ops.GEOM_MAX_THRESHOLDS
    for rule in ('d2 = (dx dx + dy dy) + dz dz', 'cell = max_dist (1 + 2^-10)', 'among equal d2 the smallest ref_index',
                 '0.7548776662466927', '0.5698402909980532', 'target = ((s + 0.5) * total) / n', 'a + (u (b - a) + v (c - a))'):
        assert rule in hdr, rule


def test_every_refusal_comes_before_a_launch():
    L = _lib.geom_lib()
    big = 1 << 40
    o3 = (C.c_float * 3)(0.0, 0.0, 0.0)
    ic = float(np.float32(1.0 / (0.5 * geometry.SLACK)))

    def keys(n=8, p=FAKE, org=o3, inv=ic, dims=(4, 4, 4), k=FAKE):
        return L.durf_geom_keys(None, n, p, org, inv, *dims, k)
    for kw, text in ((dict(n=-1), 'n = -1'), (dict(p=None), 'points and keys'), (dict(k=None), 'points and keys'), (dict(org=None), 'origin'),
                     (dict(dims=(0, 4, 4)), 'nx = 0'), (dict(dims=(4, 2049, 4)), 'ny = 2049'), (dict(inv=0.0), 'inv_cell = 0'),
                     (dict(inv=float('nan')), 'inv_cell = nan'), (dict(inv=float('inf')), 'inv_cell = inf')):
        assert keys(**kw) != 0 and text in _err() and 'durf_geom_keys' in _err(), (kw, _err())
    assert keys(n=0, p=None, k=None) == 0

    def near(q=8, qp=FAKE, m=8, rs=FAKE, rk=FAKE, ri=FAKE, org=o3, inv=ic, dims=(4, 4, 4), md=0.5, d=FAKE, i=FAKE):
        return L.durf_geom_nearest(None, q, qp, m, rs, rk, ri, org, inv, *dims, md, d, i)
    for kw, text in ((dict(q=-1), 'q = -1'), (dict(m=-2), 'm = -2'), (dict(qp=None), 'query, dist and index'), (dict(d=None), 'query, dist and index'),
                     (dict(i=None), 'query, dist and index'), (dict(rs=None), 'ref_sorted, ref_keys and ref_index'),
                     (dict(rk=None), 'ref_sorted, ref_keys and ref_index'), (dict(ri=None), 'ref_sorted, ref_keys and ref_index'),
                     (dict(org=None), 'origin'), (dict(dims=(4, 4, 2049)), 'at most 2048 cells per axis'), (dict(dims=(4, 4, 0)), 'nz = 0'),
                     (dict(md=float('nan')), 'max_dist = nan'), (dict(md=0.0), 'max_dist = 0'), (dict(md=-1.0), 'max_dist = -1'),
                     (dict(md=float('inf')), 'max_dist = inf'), (dict(md=1e19), 'max_dist = 1e+19'),
                     (dict(md=0.5001), 'grid rule'), (dict(inv=2.0), 'grid rule'), (dict(inv=float('nan')), 'inv_cell = nan')):
        assert near(**kw) != 0 and text in _err() and 'durf_geom_nearest' in _err(), (kw, _err())
    assert near(inv=2.0) != 0 and 'inv_cell = 2' in _err() and 'max_dist = 0.5' in _err(), 'both numbers are named'
    assert near(q=0, qp=None, d=None, i=None) == 0, 'nothing to ask: no launch'
    assert near(q=0, qp=None, d=None, i=None, md=0.25) == 0, 'cells wider than needed are within the rule'

    th = (C.c_float * 9)(*([0.1] * 9))
    need = L.durf_geom_workspace_bytes(2049, 0)
    assert need == 256 * 2 + 256 and L.durf_geom_workspace_bytes(-1, 0) == 0 and L.durf_geom_workspace_bytes(0, -1) == 0
    assert L.durf_geom_workspace_bytes(0, 0) == 256
    assert L.durf_geom_workspace_bytes(0, 257) == 2304 + 256 and L.durf_geom_workspace_bytes(1024, 256) == 256 + 2048 + 256

    def stats(q=2049, d=FAKE, i=FAKE, nt=2, t=th, ws=FAKE, nb=big, out=FAKE):
        return L.durf_geom_stats(None, q, d, i, nt, t, ws, nb, out)
    nan_th = (C.c_float * 2)(0.1, float('nan'))
    for kw, text in ((dict(q=-1), 'q = -1'), (dict(d=None), 'dist and index'), (dict(i=None), 'dist and index'), (dict(nt=9), 'n_thresholds = 9'),
                     (dict(nt=-1), 'n_thresholds = -1'), (dict(t=None), 'thresholds for n_thresholds = 2'), (dict(t=nan_th), 'thresholds[1] = nan'),
                     (dict(out=None), 'stats'), (dict(ws=None), 'workspace aligned'), (dict(ws=FAKE + 8), 'workspace aligned'),
                     (dict(nb=need - 1), 'durf_geom_workspace_bytes(2049, 0) = %d' % need)):
        assert stats(**kw) != 0 and text in _err() and 'durf_geom_stats' in _err(), (kw, _err())
    assert 'workspace of %d bytes' % (need - 1) in _err()

    need = L.durf_geom_workspace_bytes(0, 257)

    def samp(V=8, v=FAKE, T=257, t=FAKE, n=16, ws=FAKE, nb=big, p=FAKE, tri=FAKE, tot=FAKE):
        return L.durf_geom_sample_mesh(None, V, v, T, t, n, ws, nb, p, tri, tot)
    for kw, text in ((dict(n=-1), 'n = -1'), (dict(V=-1), 'n_vertices = -1'), (dict(T=-1), 'n_triangles = -1'), (dict(v=None), 'vertices for n_vertices = 8'),
                     (dict(t=None), 'triangles for n_triangles = 257'), (dict(p=None), 'points and tri'), (dict(tri=None), 'points and tri'),
                     (dict(tot=None), 'total_area'), (dict(ws=None), 'workspace aligned'), (dict(ws=FAKE + 16), 'workspace aligned'),
                     (dict(nb=need - 1), 'durf_geom_workspace_bytes(0, 257) = %d' % need)):
        assert samp(**kw) != 0 and text in _err() and 'durf_geom_sample_mesh' in _err(), (kw, _err())


# ---- the grid rule --------------------------------------------------------------------------------------------------------------
def test_the_grid_rule_and_its_refusal_message():
    g = geometry.grid_rule((0.0, -1.0, 2.0), (4.0, 1.0, 2.0), 0.25)
    assert g['cell'] == 0.25 * (1 + 2.0 ** -10) and g['inv_cell'] == float(np.float32(1.0 / g['cell']))
    assert g['dims'] == (16, 8, 1) and g['origin'].dtype == np.float32 and g['origin'].tolist() == [0.0, -1.0, 2.0]
    # what the entry point enforces, with the inv_cell the host computes, over the whole range of max_dist
    for md in (1e-18, 3e-7, 0.1, 1.0, 7.3, 1e18):
        gg = geometry.grid_rule((0, 0, 0), (0, 0, 0), md)
        assert gg['dims'] == (1, 1, 1) and gg['inv_cell'] * gg['max_dist'] * geometry.SLACK <= 1 + 2.0 ** -22
    # every reference point falls inside: the kernel's own t of the maximum, for awkward extents
    rng = np.random.default_rng(0)
    for _ in range(200):
        lo = rng.normal(size=3).astype(np.float32) * 50
        hi = lo + rng.uniform(0, 30, 3).astype(np.float32)
        md = float(rng.uniform(0.02, 1.0))
        gg = geometry.grid_rule(lo, hi, md)
        pts = np.concatenate([rng.uniform(lo, hi, (64, 3)).astype(np.float32).clip(lo, hi), lo[None], hi[None]])
        assert (G.keys(pts, gg) >= 0).all()
        assert (G.cells(hi[None], gg)[0] + 1 == gg['dims']).all()
    # an extent over the limit names the smallest max_dist that fits, and that one fits with exactly 2048 cells
    with pytest.raises(ValueError) as e:
        geometry.grid_rule((0, 0, 0), (100.0, 3.0, 1.0), 0.01)
    msg = str(e.value)
    assert 'the limit is 2048 per axis' in msg and 'smallest max_dist that fits is' in msg and 'geometry.nearest' in msg
    fits = float(msg.rsplit(' ', 1)[1])
    assert abs(fits - 100.0 / 2048 / geometry.SLACK) < 1e-6 * fits
    assert geometry.grid_rule((0, 0, 0), (100.0, 3.0, 1.0), fits)['dims'][0] == 2048
    with pytest.raises(ValueError, match='smallest max_dist'):
        geometry.grid_rule((0, 0, 0), (100.0, 3.0, 1.0), fits * (1 - 1e-3))
    for bad in (float('nan'), 0.0, -1.0, float('inf'), 1e-30):
        with pytest.raises(ValueError, match='max_dist'):
            geometry.grid_rule((0, 0, 0), (1, 1, 1), bad)
    with pytest.raises(ValueError, match='spans'):
        geometry.grid_rule((0, 0, 0), (1, float('nan'), 1), 0.5)


def test_neighbours_within_max_dist_share_the_27_cells_at_the_far_corner():
    """the header's invariant, checked in the reference's own fp32 at the place it is tightest: cell 2047 of 2048"""
    md = np.float32(0.37)
    ext = np.float32(2047.9) * np.float32(md * geometry.SLACK)
    g = geometry.grid_rule((0, 0, 0), (ext, 0, 0), md)
    assert g['dims'][0] == 2048
    k = np.arange(1900, 2048, dtype=np.float64)
    border = (k * g['cell']).astype(np.float32)                      # (near) the lower border of cell k
    a = np.nextafter(border, np.float32(-np.inf))
    for sep in (md, np.nextafter(md, np.float32(0))):
        b = (a + sep).astype(np.float32)
        ca = G.cells(np.stack([a, 0 * a, 0 * a], 1), g)[:, 0]
        cb = G.cells(np.stack([b, 0 * b, 0 * b], 1), g)[:, 0]
        assert (np.abs(cb - ca) <= 1).all() and (cb != ca).any()


# ---- the two references against each other ------------------------------------------------------------------------------------
def test_the_fp32_and_float64_references_agree():
    rng = np.random.default_rng(3)
    q, r = rng.uniform(0, 4, (700, 3)).astype(np.float32), rng.uniform(0, 4, (900, 3)).astype(np.float32)
    r[5] = r[4]                                                       # a duplicate: the lower index wins
    q[0] = r[5]
    md = 0.3
    d32, i32, b32 = G.nearest32(q, r, md)
    b64, i64, s64 = G.nearest64(q, r, md)
    found = i32 >= 0
    assert found.sum() > 400 and (~found).sum() > 5 and i32[0] == 4 and d32[0] == 0
    assert (b64[~found] > md * md * (1 - 1e-6)).all() and (d32[~found] == np.float32(md)).all()
    rel = np.abs(d32[found].astype(np.float64) - np.sqrt(b64[found])) / np.sqrt(b64[found]).clip(1e-30)
    assert rel[1:].max() <= 4 * 2.0 ** -24
    close = (s64 - b64) < 16 * 2.0 ** -24 * s64
    assert (i32[found & ~close] == i64[found & ~close]).all() and close.sum() <= 2
    # unusable queries and reference points
    q2, r2 = q.copy(), r.copy()
    q2[1, 2], q2[2, 0] = np.nan, np.inf
    j = int(np.flatnonzero(found)[3])
    r2[i32[j]] = np.nan
    d, i, _ = G.nearest32(q2, r2, md)
    assert i[1] == -2 and i[2] == -2 and np.isnan(d[1]) and np.isnan(d[2]) and j > 2 and i[j] != i32[j]
    same = (i32 != i32[j]) & (np.arange(700) > 2)
    assert (i[same] == i32[same]).all() and (d[same] == d32[same]).all() and not (i == i32[j]).any()
    # statistics
    row = G.stats(d32, i32, (0.1, float(d32[found][7])))
    assert row[0] == 700 and row[1] == found.sum() and abs(row[4] - (row[2] + (~found).sum() * np.float32(md))) < 1e-9
    assert row[6] == (d32[found] <= d32[found][7]).sum() >= 1 and (row[7:] == 0).all()


def test_the_reference_sampler():
    v = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [np.nan, 0, 0]], np.float32)
    t = np.array([[0, 1, 2], [0, 0, 1], [0, 2, 3], [0, 1, 4], [0, 1, 7]], np.int32)
    assert G.triangle_areas(v, t).tolist() == [0.5, 0.0, 0.5, 0.0, 0.0]
    p, g, uv, total = G.sample_mesh(v, t, 257)
    assert total == 1.0 and set(g.tolist()) == {0, 2} and abs((g == 0).sum() - 128.5) <= 1
    assert (uv >= 0).all() and (uv.sum(1) <= 1 + 1e-7).all() and (p[:, 2] == 0).all() and (p >= 0).all() and (p <= 1).all()
    p32 = G.sample_mesh(v, t, 257, np.float32)[0]
    assert p32.dtype == np.float32 and np.abs(p32 - p).max() < 4e-7
    z = G.sample_mesh(v, t[[1, 3]], 5)
    assert np.isnan(z[0]).all() and (z[1] == -1).all() and z[3] == 0.0


# ---- cloud_distance's host arithmetic -----------------------------------------------------------------------------------------
def test_summarise_from_hand_made_rows():
    rows = np.zeros((2, 13))
    rows[0, :7] = (10, 8, 4.0, 2.5, 5.0, 4, 8)                 # pred -> truth: 10 usable, 8 found, sums, within 0.1: 4, within 0.5: 8
    rows[1, :7] = (20, 10, 2.0, 0.9, 7.0, 10, 10)
    r = geometry.summarise(rows, (0.1, 0.5), 0.5)
    assert r['accuracy'] == 0.5 and r['completeness'] == 0.2 and r['chamfer'] == 0.7
    assert r['accuracy_truncated'] == 0.5 and r['completeness_truncated'] == 0.35 and r['chamfer_truncated'] == 0.85
    assert r['accuracy_rms'] == np.sqrt(2.5 / 8) and r['completeness_rms'] == np.sqrt(0.09)
    assert r['precision'] == [0.4, 0.8] and r['recall'] == [0.5, 0.5]
    assert r['fscore'] == [2 * 0.4 * 0.5 / 0.9, 2 * 0.8 * 0.5 / 1.3]
    assert (r['pred_usable'], r['pred_found'], r['truth_usable'], r['truth_found']) == (10, 8, 20, 10)
    assert r['thresholds'] == [0.1, 0.5] and r['max_dist'] == 0.5
    empty = np.zeros((2, 13))
    empty[0, :5] = (3, 0, 0, 0, 1.5)
    e = geometry.summarise(empty, (0.1,), 0.5)
    assert e['accuracy'] is None and e['chamfer'] is None and e['accuracy_truncated'] == 0.5 and e['completeness_truncated'] is None
    assert e['precision'] == [0.0] and e['recall'] == [None] and e['fscore'] == [None]
    both = np.zeros((2, 13))
    both[:, 0] = 4
    assert geometry.summarise(both, (0.1,), 0.5)['fscore'] == [0.0]
    with pytest.raises(ValueError, match='at most 8'):
        geometry._thresholds([0.1] * 9, 0.5, 'x')
    with pytest.raises(ValueError, match='nothing beyond max_dist'):
        geometry._thresholds([0.6], 0.5, 'x')


def test_error_colours_and_the_ply(tmp_path):
    lut = np.stack([np.linspace(0, 1, 256)] * 3, 1)
    c = geometry.error_colours([0.0, 0.25, 0.5, 9.0, np.nan], 0.5, lut)
    assert c.tolist() == [[0] * 3, [128] * 3, [255] * 3, [255] * 3, [128] * 3] and c.dtype == np.uint8
    path = str(tmp_path / 'e.ply')
    n = geometry.write_error_ply(path, np.arange(15, dtype=np.float32).reshape(5, 3), [0.0, 0.25, 0.5, 9.0, np.nan], 0.5, lut)
    blob = open(path, 'rb').read()
    end = blob.index(b'end_header\n') + len(b'end_header\n')
    assert n == 5 and b'element vertex 5' in blob[:end] and b'property float distance' in blob[:end] and len(blob) - end == 5 * 19
    rec = np.frombuffer(blob, geometry._ERROR_VERTEX, 5, end)
    assert rec['z'].tolist() == [2, 5, 8, 11, 14] and rec['red'].tolist() == [0, 128, 255, 255, 128]
    with pytest.raises(ValueError, match='5 points and 2 distances'):
        geometry.write_error_ply(path, np.zeros((5, 3)), [0, 1], 0.5, lut)


def test_the_commands_arguments():
    ap = eval_geometry.build_parser()
    a = ap.parse_args(['--eval_dir', 'x', '--synthetic'])
    assert a.source == 'mesh' and a.samples == 200000 and a.keep_objects is False and a.split == 'test'
    assert a.iso == eval_geometry.default_iso()
    for flag in ('--gin_file', '--grid', '--iso', '--eval_dir', '--synthetic', '--train_dir', '--data_dir', '--source', '--samples',
                 '--max_dist', '--thresholds', '--keep_objects', '--sweeps', '--split'):
        assert flag in ap.format_help(), flag
    assert ap.parse_args(['--eval_dir', 'x', '--thresholds', '0.1,0.2']).thresholds == '0.1,0.2'
    with pytest.raises(SystemExit):
        ap.parse_args(['--eval_dir', 'x', '--source', 'voxels'])
