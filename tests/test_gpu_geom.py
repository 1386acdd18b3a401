"""Nearest-point distances, their statistics and the mesh sampler on the device (include/durf_geom.h, csrc/geom.hip,
durf_amd/geometry.py) against tests/geom_ref.py.

The search is held to the brute-force np.float32 reference bit for bit: the header fixes the arithmetic (unfused fp32, d2 =
(dx dx + dy dy) + dz dz, the exact comparison with max_dist^2, ties to the lowest index) and its grid rule promises that the
27 cells hold every point that counts, so dist and index must be EQUAL, on every query, at every shape.  The float64 test
says what that fp32 answer is worth: dist within 4 * 2^-24 relative (each difference carries one rounding, so its square
2 * 2^-24; the two squares' roundings are dominated by the sums': three more; d2 is within 5 * 2^-24 and its root within half
of that plus the root's own rounding: 3.5 * 2^-24), and the same index wherever float64 itself separates the best from the
runner-up and from max_dist by more than 16 * 2^-24 relative.  Sizes are a few thousand points: more than one workgroup, odd
counts, and the grid's limit of 2048 cells on an axis, where the rule is tightest."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from durf_amd import geometry, mesh, ops, raygen
from tests import geom_ref as G
from tests import mesh_ref as M

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E = 2.0 ** -24
_R = {}


def _d(a, cuda, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a)).to(device=cuda, dtype=dtype).contiguous()


def _near(cuda, q, r, md, sort):
    q, r = np.asarray(q, np.float32).reshape(-1, 3), np.asarray(r, np.float32).reshape(-1, 3)
    d, i = geometry.nearest(_d(q, cuda), _d(r, cuda), md, sort_queries=sort)
    assert d.dtype == torch.float32 and i.dtype == torch.int32 and d.shape == (q.shape[0],) and i.shape == (q.shape[0],)
    return d.cpu().numpy(), i.cpu().numpy()


def _grid(r, md):
    lo, hi = G.bounds(r)
    return geometry.grid_rule(lo, hi, md)


def _same(got, want, what):
    (d, i), (wd, wi) = got, want[:2]
    bad = np.flatnonzero((i != wi) | (d.view(np.int32) != wd.view(np.int32)))
    assert bad.size == 0, '%s: %d of %d queries differ, first %d: got (%r, %d), want (%r, %d)' % (
        what, bad.size, i.size, bad[0], d[bad[0]], i[bad[0]], wd[bad[0]], wi[bad[0]])
    ok = wi != -2
    assert ((d[ok] * d[ok]) == (wd[ok] * wd[ok])).all()


def _both(cuda, q, r, md, what):
    """sorted and unsorted queries against the fp32 reference -> the reference's (dist, index, d2)"""
    want = G.nearest32(q, r, md, _grid(r, md))
    for sort in (False, True):
        _same(_near(cuda, q, r, md, sort), want, '%s (sort_queries=%s)' % (what, sort))
    return want


# ---- 1. exact lattice -------------------------------------------------------------------------------------------------------------
def test_an_exact_lattice_with_ties_and_the_radius_itself(cuda):
    rng = np.random.default_rng(11)
    step, md = 2.0 ** -6, 8 * 2.0 ** -6
    r = (rng.integers(0, 256, (2000, 3)) * step).astype(np.float32)
    q = (rng.integers(0, 256, (2000, 3)) * step).astype(np.float32)
    r[10], r[1500] = r[3], r[3]                                    # duplicates: the lowest index wins
    q[0] = r[3]
    q[1] = r[3] + np.float32([step, 0, 0])
    # an isolated reference point, a query at exactly max_dist (found) and one a lattice step beyond (not found)
    r[7], r[8] = (6.0, 6.0, 6.0), (6.5, 6.5, 6.5)                  # (the second keeps the queries below inside the grid)
    q[2], q[3], q[4] = (6.0 + md, 6.0, 6.0), (6.0 + md + step, 6.0, 6.0), (6.0, 6.0 - md, 6.0)
    # equidistant neighbours: +-step along an axis around a query far from everything else
    r[20], r[21], r[22] = (5.0, 0.0, 0.0), (5.0 + 2 * step, 0.0, 0.0), (5.0 + step, step, 0.0)
    q[5] = (5.0 + step, 0.0, 0.0)
    want = _both(cuda, q, r, md, 'lattice')
    d, i, d2 = want
    assert i[0] == 3 and d[0] == 0 and i[2] == 7 and d[2] == np.float32(md) and i[3] == -1 and d[3] == np.float32(md) and i[4] == 7
    assert i[5] == 20 and d[5] == np.float32(step), 'three points at the same distance: the lowest index'
    assert (i >= 0).sum() > 300 and (i == -1).sum() > 300
    exact = (q[i >= 0].astype(np.float64) - r[i[i >= 0]].astype(np.float64)) ** 2
    assert (d2[i >= 0].astype(np.float64) == exact.sum(1)).all(), 'on the lattice fp32 is exact'


# ---- 2. edges of the launch and of the grid --------------------------------------------------------------------------------------
@pytest.mark.parametrize('nq', (1, 255, 256, 257))
@pytest.mark.parametrize('kind', ('one', 'two', 'one cell', 'cloud'))
def test_edges_of_the_launch_and_the_grid(cuda, nq, kind):
    rng = np.random.default_rng(nq + len(kind))
    md = 0.1
    if kind == 'one':
        r = np.float32([[0.3, 0.2, 0.1]])
    elif kind == 'two':
        r = np.float32([[0.3, 0.2, 0.1], [0.35, 0.2, 0.1]])
    elif kind == 'one cell':
        r = rng.uniform(0, 0.09, (1000, 3)).astype(np.float32)
    else:
        r = rng.uniform(0, 1, (600, 3)).astype(np.float32)
        r[5], r[6, 1], r[7, 2] = np.nan, np.inf, -np.inf               # key -1: never returned
    lo, hi = G.bounds(r)
    q = rng.uniform(lo - 0.28, hi + 0.28, (nq, 3)).astype(np.float32)   # inside, one cell outside (searched), further out (-2)
    if nq > 200:
        q[3], q[4, 0], q[5, 2] = np.nan, np.inf, -np.inf
        q[6:14] = [[lo[0], lo[1], lo[2]], [hi[0], hi[1], hi[2]], [lo[0], hi[1], lo[2]], [hi[0], lo[1], hi[2]],                # corner cells
                   [lo[0] - 0.05, lo[1], lo[2]], [hi[0] + 0.05, hi[1], hi[2] + 0.05], [lo[0] - 0.25, lo[1], lo[2]], [hi[0], hi[1] + 0.35, hi[2]]]
    d, i, _ = _both(cuda, q, r, md, '%s, q = %d' % (kind, nq))
    if nq > 200:
        assert (i[3:6] == -2).all() and np.isnan(d[3:6]).all() and (i[12:14] == -2).all() and (kind == 'cloud' or (i[6:10] >= 0).all())
        assert (i == -2).sum() > 8 and (i == -1).sum() > 5, 'queries too far out, and empty neighbourhoods'
        g = _grid(r, md)
        c = G.cells(q, g)
        out1 = (((c == -1) | (c == np.asarray(g['dims']))).any(1)) & (i != -2)
        assert out1.sum() > 5, 'queries one cell outside are searched'
        if kind in ('one cell', 'cloud'):
            assert (i[out1] >= 0).any(), 'and find points'
    if kind == 'cloud':
        assert not np.isin(i, (5, 6, 7)).any()


def test_no_reference_point_at_all(cuda):
    q = np.float32([[0, 0, 0], [1, 2, 3], [np.nan, 0, 0], [0.05, 0, 0]])
    for r in (np.zeros((0, 3), np.float32), np.full((3, 3), np.nan, np.float32)):
        for sort in (False, True):
            d, i = _near(cuda, q, r, 0.1, sort)
            assert i.tolist() == [-1, -2, -2, -1] and d[0] == np.float32(0.1) and np.isnan(d[1:3]).all()
    d, i = _near(cuda, np.zeros((0, 3), np.float32), q[:2], 0.1, True)
    assert d.shape == (0,) and i.shape == (0,)


# ---- 3. the far corner of the largest grid -----------------------------------------------------------------------------------------
def test_pairs_across_a_cell_border_at_the_far_end_of_2048_cells(cuda):
    """max_dist = 0.375 and coordinates in [512, 1024) (one ulp = 2^-14) make b = a + max_dist exact: the pair's d2 is max_dist^2
    itself, or one ulp of the coordinate short of it.  a sits one ulp below a cell border, b a whole max_dist further: the two
    computed cell coordinates are as far apart as the rule allows, where their rounding is largest."""
    md = np.float32(0.375)
    cell = float(md) * geometry.SLACK
    ks = np.arange(1400, 2047, 2)
    a = np.nextafter((ks * cell).astype(np.float32), np.float32(-np.inf))
    assert a.min() >= 512 and a.max() + md < 1024
    anchors = np.float32([[0, 0, 0], [np.float32(2047.5 * cell), 3.0, 0.25]])      # (the grid's extent; far from every pair)
    for sep in (md, md - np.float32(2.0 ** -14)):
        b = a + sep
        assert ((b - a) == sep).all() and ((b.astype(np.float64) - a.astype(np.float64)) == float(sep)).all()
        A = np.concatenate([anchors, np.stack([a, 0 * a + 0.5, 0 * a + 0.25], 1)]).astype(np.float32)
        B = np.concatenate([anchors, np.stack([b, 0 * b + 0.5, 0 * b + 0.25], 1)]).astype(np.float32)
        for ref, qry, name in ((A, B[2:], 'b -> a'), (B, A[2:], 'a -> b')):
            g = _grid(ref, md)
            assert g['dims'][0] == 2048
            cq, cr = G.cells(qry, g)[:, 0], G.cells(ref[2:], g)[:, 0]
            assert (np.abs(cq - cr) == 1).sum() > 0.9 * ks.size, 'the pairs straddle a border'
            d, i, _ = _both(cuda, qry, ref, md, 'far corner %s, separation %r' % (name, sep))
            assert (i == np.arange(ks.size) + 2).all() and (d == sep).all(), 'every pair is found'


# ---- 4. random floats ---------------------------------------------------------------------------------------------------------------
def _random():
    if not _R:
        rng = np.random.default_rng(2024)
        _R['q'], _R['r'], _R['md'] = rng.uniform(0, 4, (3000, 3)).astype(np.float32), rng.uniform(0, 4, (3001, 3)).astype(np.float32), 0.2
        _R['want'] = G.nearest32(_R['q'], _R['r'], _R['md'], _grid(_R['r'], _R['md']))
        _R['f64'] = G.nearest64(_R['q'], _R['r'], _R['md'])
    return _R


def test_random_floats_bit_for_bit_sorted_and_unsorted(cuda):
    R = _random()
    a, b = _near(cuda, R['q'], R['r'], R['md'], False), _near(cuda, R['q'], R['r'], R['md'], True)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes(), 'sorted and unsorted queries: identical outputs'
    _same(a, R['want'], 'random floats')
    assert 1500 < (a[1] >= 0).sum() < 3000 and (a[1] == -1).sum() > 100


def test_random_floats_against_float64(cuda):
    R = _random()
    d, i = _near(cuda, R['q'], R['r'], R['md'], None)
    b, j, s = R['f64']
    md2 = float(np.float32(R['md'])) ** 2
    excused = ((s - b) < 16 * E * s) | (np.abs(b - md2) < 16 * E * md2)
    print('excused: %d of %d queries' % (excused.sum(), excused.size))
    assert excused.sum() <= 0.01 * excused.size
    want_i = np.where(b <= md2, j, -1)
    assert (i[~excused] == want_i[~excused]).all()
    ok = (i >= 0) & (i == j)
    rel = np.abs(d[ok].astype(np.float64) - np.sqrt(b[ok])) / np.sqrt(b[ok])
    print('dist against float64: worst relative error %.3f * 2^-24 over %d queries' % (rel.max() / E, ok.sum()))
    assert ok.sum() > 1500 and rel.max() <= 4 * E


# ---- 5. statistics --------------------------------------------------------------------------------------------------------------------
def test_statistics_are_the_float64_sums_and_deterministic(cuda):
    R = _random()
    wd, wi, _ = R['want']
    wd, wi = wd.copy(), wi.copy()
    wd[:5], wi[:5] = np.nan, -2                                       # unusable queries do not count
    present = float(wd[wi >= 0][17])
    th = (0.05, present, 0.3, 0.0)
    dd, ii = _d(wd, cuda), _d(wi, cuda, torch.int32)
    rows = [ops.geom_stats(dd, ii, th).cpu().numpy() for _ in range(2)]
    assert rows[0].tobytes() == rows[1].tobytes(), 'two runs, the same bits'
    want = G.stats(wd, wi, th)
    got = rows[0]
    assert got.shape == (13,) and (got[[0, 1]] == want[[0, 1]]).all() and (got[5:] == want[5:]).all(), (got, want)
    assert got[0] == 2995 and got[6] == (wd[wi >= 0] <= np.float32(present)).sum() >= 1 and got[7] == got[1] and (got[9:] == 0).all()
    assert (wd[wi >= 0] == np.float32(present)).any(), 'a threshold equal to a distance in the data counts it'
    assert (np.abs(got[2:5] - want[2:5]) <= 1e-12 * np.abs(want[2:5])).all(), (got[2:5], want[2:5])
    for n in (0, 1, 1024, 1025):
        row = ops.geom_stats(dd[:n].contiguous(), ii[:n].contiguous(), th[:1]).cpu().numpy()
        w = G.stats(wd[:n], wi[:n], th[:1])
        assert (row[[0, 1, 5]] == w[[0, 1, 5]]).all() and np.allclose(row[2:5], w[2:5], rtol=1e-12, atol=0) and (row[6:] == 0).all(), n


def test_cloud_distance_is_the_two_directions(cuda):
    R = _random()
    th = (0.05, 0.1, 0.2)
    res = geometry.cloud_distance(_d(R['q'], cuda), _d(R['r'], cuda), R['md'], thresholds=th, keep=True)
    back = G.nearest32(R['r'], R['q'], R['md'], _grid(R['q'], R['md']))
    _same((res['pred_dist'].cpu().numpy(), res['pred_index'].cpu().numpy()), R['want'], 'pred -> truth')
    _same((res['truth_dist'].cpu().numpy(), res['truth_index'].cpu().numpy()), back, 'truth -> pred')
    want = geometry.summarise(np.stack([G.stats(R['want'][0], R['want'][1], th), G.stats(back[0], back[1], th)]), [float(np.float32(t)) for t in th],
                              float(np.float32(R['md'])))
    for k, v in want.items():
        if isinstance(v, list):
            assert np.allclose(res[k], v, rtol=1e-12, atol=0), k
        elif isinstance(v, float):
            assert abs(res[k] - v) <= 1e-12 * abs(v), k
        else:
            assert res[k] == v, k
    assert res['chamfer'] == res['accuracy'] + res['completeness'] and res['pred_usable'] == 3000 and res['truth_usable'] == 3001
    assert res['grids']['pred_to_truth']['dims'] == list(_grid(R['r'], R['md'])['dims'])
    with pytest.raises(ValueError, match='smallest max_dist that fits'):
        geometry.cloud_distance(_d(R['q'], cuda), _d(R['r'], cuda), 1e-3)


# ---- 6. the mesh sampler ------------------------------------------------------------------------------------------------------------
def _strip(m):
    """2 m right triangles with legs 1/128 and 1/2 in a row: area 2^-9 each, so every partial sum of the areas is exact in
    float64 in any association (x = k / 128 is exact in fp32 far beyond m = 2^17)"""
    x = np.arange(m + 1, dtype=np.float32) / 128
    sv = np.concatenate([np.stack([x, 0 * x, 0 * x], 1), np.stack([x, 0 * x + 0.5, 0 * x], 1)])
    k = np.arange(m, dtype=np.int32)
    st = np.stack([np.stack([k, k + 1, m + 1 + k], 1), np.stack([k + 1, m + 2 + k, m + 1 + k], 1)], 1).reshape(-1, 3)
    return sv, st


@functools.lru_cache(maxsize=None)
def _meshes():
    square = (np.float32([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]]), np.int32([[0, 1, 2], [0, 2, 3]]))
    v = np.float32([[0, 0, 0], [2, 0, 0], [2, 1, 0], [0, 1, 0], [np.nan, 0, 0], [0, 0, 3]])                 # areas 1, 1, 3/2: exact sums
    holes = (v, np.int32([[0, 1, 1], [0, 1, 2], [0, 1, 4], [0, 2, 3], [0, 1, 9], [0, -1, 2], [0, 3, 5]]))      # zero-area, NaN, out of range
    single = (np.float32([[1, 2, 3], [1.5, 2, 3.25], [0.75, 4, 2]]), np.int32([[0, 1, 2]]))
    # strip: 600 triangles, more than two block sums.  long_strip: the scan of the block sums (csrc/scan.h) takes 1024 of them
    # per round, so 1024 blocks of 256 triangles and one more block, of two triangles, is the first size with a second round;
    # the sums being exact, the triangle ids equal the float64 oracle's there too.
    return dict(square=square, holes=holes, single=single, strip=_strip(300), long_strip=_strip((1024 * 256 + 2) // 2))


@pytest.mark.parametrize('name,n', [(name, n) for name in ('square', 'holes', 'single', 'strip') for n in (1, 255, 257, 2000)] +
                         [('long_strip', 257), ('long_strip', 2000)])
def test_the_mesh_sampler(cuda, name, n):
    v, t = _meshes()[name]
    p, tri = geometry.sample_mesh(dict(vertices=v, triangles=t), n)
    p, tri = p.cpu().numpy(), tri.cpu().numpy()
    want, wtri, uv, total = G.sample_mesh(v, t, n)
    assert p.shape == (n, 3) and tri.shape == (n,) and tri.dtype == np.int32
    assert (tri == wtri).all(), 'triangle ids'
    scale = np.abs(v[np.isfinite(v)]).max()
    assert (np.abs(p.astype(np.float64) - want) <= 4 * M.ulp32(scale)).all(), 'points within fp32 rounding of the float64 reference'
    area = G.triangle_areas(v, t).astype(np.float64)
    assert area[tri].min() > 0, 'no sample on a triangle without area'
    counts = np.bincount(tri, minlength=t.shape[0])
    assert (np.abs(counts - area / total * n) <= 1).all(), 'counts within 1 of the area share'
    # in the plane of its triangle and inside it: barycentric coordinates in float64
    a, b, c = (v[t[tri, k]].astype(np.float64) for k in range(3))
    e1, e2, w = b - a, c - a, p.astype(np.float64) - a
    nrm = np.cross(e1, e2)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    assert (np.abs(np.einsum('ij,ij->i', w, nrm)) <= 1e-6 * max(scale, 1.0)).all()
    # inside: on the third vertex's side of every edge, to 1e-6 on the small meshes (coordinates <= 4, whose fp32 ulp is below
    # it).  A stored coordinate of size `scale` is off by up to half its fp32 ulp, 2^-14 on the long strip: one ulp there.
    slack = max(1e-6, float(M.ulp32(scale)))
    for p0, p1, p2 in ((a, b, c), (b, c, a), (c, a, b)):
        inward = np.cross(nrm, p1 - p0)
        inward /= np.linalg.norm(inward, axis=1, keepdims=True)
        inward *= np.sign(np.einsum('ij,ij->i', inward, p2 - p0))[:, None]
        assert (np.einsum('ij,ij->i', p.astype(np.float64) - p0, inward) >= -slack).all()


def test_a_mesh_without_area_gives_nan(cuda):
    v = np.float32([[0, 0, 0], [1, 0, 0], [2, 0, 0]])
    for t in (np.int32([[0, 1, 2], [0, 0, 1]]), np.zeros((0, 3), np.int32)):
        p, tri, total = ops.geom_sample_mesh(_d(v, cuda), _d(t, cuda, torch.int32), 5)
        assert bool(torch.isnan(p).all()) and tri.tolist() == [-1] * 5 and float(total) == 0.0
    p, tri = geometry.sample_mesh(dict(vertices=v, triangles=np.int32([[0, 1, 2]])), 0)
    assert p.shape == (0, 3) and tri.shape == (0,)


# ---- 7. end to end ----------------------------------------------------------------------------------------------------------------------
def test_a_sphere_mesh_against_the_analytic_sphere(cuda):
    h, Rs, centre = 0.125, 1.3, np.asarray((0.03, -0.02, 0.01))
    n = int(round(4.0 / h)) + 1
    fr = M.unit_frame(h, (-2.0, -2.0, -2.0))
    m = mesh.surface(dict(density=_d(M.sphere_field(fr, (n, n, n), centre, Rs), cuda), valid=None, frame=fr), 0.0)
    pred, tri = geometry.sample_mesh(m, 4000)
    assert bool(torch.isfinite(pred).all()) and int(tri.min()) >= 0 and int(tri.max()) < m['triangles'].shape[0]
    k = np.arange(3000) + 0.5                                       # a Fibonacci lattice on the analytic sphere
    z, phi = 1 - 2 * k / 3000, np.pi * (1 + 5 ** 0.5) * k
    truth = centre + Rs * np.stack([np.sqrt(1 - z * z) * np.cos(phi), np.sqrt(1 - z * z) * np.sin(phi), z], 1)
    res = geometry.cloud_distance(pred, _d(truth, cuda), 2 * h, thresholds=(h,))
    print('sphere: accuracy %.4f completeness %.4f precision %.3f recall %.3f' % (res['accuracy'], res['completeness'], res['precision'][0],
                                                                                  res['recall'][0]))
    assert res['pred_found'] == 4000 and res['truth_found'] == 3000
    assert res['accuracy'] < h and res['completeness'] < h and res['recall'][0] == 1.0 and res['fscore'][0] > 0.99
    radial = np.abs(np.linalg.norm(pred.cpu().numpy().astype(np.float64) - centre, axis=1) - Rs)
    assert radial.max() < 0.1 * h, 'the samples lie on the mesh, a chord below the sphere'


def test_depth_points_are_the_rays_of_generate_batch(cuda):
    h, w, near, far = 7, 9, 0.1, 50.0
    c2w = np.array([[0.8, 0.0, 0.6, 1.0], [0.0, 1.0, 0.0, -2.0], [-0.6, 0.0, 0.8, 0.5]])
    rng = np.random.default_rng(1)
    depth = np.where(rng.uniform(size=(h, w)) < 0.5, rng.uniform(1, 9, (h, w)), 0.0).astype(np.float32)
    depth[0, 0], depth[0, 1] = 3.0, -1.0
    td = raygen.TimestepData([c2w], [6.5], [(4.4, 3.6)], [h], [w], depth=[depth], device=cuda)
    rays, _, dp, _ = raygen.generate_batch(td, None, near, far)
    cam = raygen.camera_row(c2w, 6.5, (4.4, 3.6), h, w)
    got = geometry.depth_points(cam, _d(depth, cuda), near, far)
    keep = dp.reshape(-1) > 0
    want = rays.origins[keep] + rays.directions[keep] * dp.reshape(-1)[keep][:, None]
    assert got.shape == (int((depth > 0).sum()), 3) and torch.equal(got, want)
    mask = np.zeros((h, w), np.uint8)
    mask[:3] = 1
    part = geometry.depth_points(cam, _d(depth, cuda).reshape(h, w, 1), near, far, mask=_d(mask, cuda, torch.uint8))
    assert torch.equal(part, want[:int((depth[:3] > 0).sum())])
    with pytest.raises(ValueError, match='7 x 9'):
        geometry.depth_points(cam, _d(depth[:3], cuda), near, far)


def _read_error_ply(path):
    blob = open(path, 'rb').read()
    end = blob.index(b'end_header\n') + len(b'end_header\n')
    n = int([l for l in blob[:end].decode().split('\n') if l.startswith('element vertex')][0].split()[-1])
    return np.frombuffer(blob, geometry._ERROR_VERTEX, n, end)


@pytest.mark.parametrize('source', ('mesh', 'frames'))
def test_eval_geometry_command_on_the_synthetic_scene(cuda, tmp_path, source):
    out = str(tmp_path / 'geom')
    cmd = [sys.executable, '-m', 'durf_amd.eval_geometry', '--synthetic', '--eval_dir', out, '--source', source, '--samples', '3000',
           '--iso', '0.001', '--grid=-2,-2,-1;16,16,8;0.25', '--max_dist', '0.5', '--thresholds', '0.1,0.5', '--synthetic_size', '16', '24',
           '--gin_param', 'MipNerfModel.num_samples = 32', '--gin_param', 'MipNerfModel.no_pose_opt = True',
           '--gin_param', 'MipNerfModel.no_yaw_opt = True']
    if source == 'mesh':                                                    # (extract_mesh's own test queries the fp32 field)
        cmd += ['--gin_param', 'MipNerfModel.mlp_precision = \'f32\'']
    p = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)      # a fresh child process
    assert p.returncode == 0, p.stdout.decode()
    print(p.stdout.decode()[-400:])
    assert sorted(os.listdir(out)) == ['accuracy.ply', 'completeness.ply', 'geometry.json']
    doc = json.load(open(os.path.join(out, 'geometry.json')))
    acc, com = _read_error_ply(os.path.join(out, 'accuracy.ply')), _read_error_ply(os.path.join(out, 'completeness.ply'))
    assert acc.shape[0] == doc['pred_points'] and com.shape[0] == doc['truth_points'] > 0 and doc['source']['kind'] == source
    if source == 'mesh':
        assert doc['pred_points'] == 3000
    else:
        assert doc['pred_points'] == doc['truth_points'], 'back-projected at the truth\'s pixels'
    xyz = lambda rec: _d(np.stack([rec['x'], rec['y'], rec['z']], 1), cuda)
    res = geometry.cloud_distance(xyz(acc), xyz(com), 0.5, thresholds=(0.1, 0.5), keep=True)
    for k, v in res.items():
        if k.endswith('_dist') or k.endswith('_index'):
            continue
        assert doc[k] == json.loads(json.dumps(v)), k
    assert np.array_equal(res['pred_dist'].cpu().numpy(), acc['distance'], equal_nan=True)
    assert np.array_equal(res['truth_dist'].cpu().numpy(), com['distance'], equal_nan=True)
    assert doc['truth_usable'] == doc['truth_points'] and doc['thresholds'] == [float(np.float32(0.1)), 0.5]
