"""libdurf_closest.so on the device against tests/closest_ref.py: closest32 (the header's definition by brute force) in every bit
of tri, dist, bary and point on the smallest shapes at which the walk can go wrong, whatever permutation the tree is built over;
the lattice entry against the point entry; and what the feature is for -- attributes at the closest points, exact completeness,
mesh-to-mesh distance, the offset surface of a mesh."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from durf_amd import _lib, cast, closest, geometry, mesh, ops
from tests import cast_ref as C, closest_ref as R, lattice_ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24
F32 = np.float32


def _d(a, cuda, dtype=torch.float32):
    return torch.as_tensor(np.array(a)).to(device=cuda, dtype=dtype).contiguous()


def _query(cuda, b, p, max_dist=np.inf):
    p = _d(p, cuda).reshape(-1, 3)
    return tuple(a.cpu().numpy() for a in ops.closest_points(b['ws'], b['T'], p, float(max_dist)))


def _same(got, want, what):
    for k, a, b in zip(('tri', 'dist', 'bary', 'point'), got, want):
        a, b = R.bits(a), R.bits(b)
        assert a.shape == b.shape and np.array_equal(a, b), (what, k, np.argwhere(a != b)[:5])


@pytest.mark.parametrize('name', sorted(R.scenes()))
def test_every_bit_of_the_definition_whatever_the_tree(cuda, name):
    s, want = R.scenes()[name], R.expected(name)
    m = dict(vertices=s['v'], triangles=s['t'])
    _same(_query(cuda, cast.build(m), s['p'], s['max_dist']), want, name)
    # a different valid permutation in place of the Morton sort: the tree cannot change an answer
    order = np.random.default_rng(7).permutation(s['t'].shape[0]).astype(np.int32)
    _same(_query(cuda, cast.build(m, order=order), s['p'], s['max_dist']), want, name + ' (random order)')


def test_counting_flips_exactly_at_max_dist(cuda):
    v, t, p, d0, caps = R.cap_cases()
    b = cast.build(dict(vertices=v, triangles=t))
    for i in range(len(p)):                                                 # max_dist is a scalar of the call: one point a call
        for k in ('below', 'at', 'above'):
            md = float(caps[k][i])
            _same(_query(cuda, b, p[i:i + 1], md), R.closest32(v, t, p[i:i + 1], md), (i, k))
    tri, dist, _, _ = _query(cuda, b, p, np.inf)
    assert (tri >= 0).all() and np.array_equal(R.bits(dist), R.bits(d0))


def test_sorted_queries_give_the_same_bits(cuda):
    s, want = R.scenes()['random_T5000_capped'], R.expected('random_T5000_capped')
    b = cast.build(dict(vertices=s['v'], triangles=s['t']))
    for sort in (True, False, None):
        r = closest.points(b, s['p'], s['max_dist'], sort_queries=sort)
        _same(tuple(r[k].cpu().numpy() for k in ('tri', 'dist', 'bary', 'point')), want, sort)
        assert np.array_equal(r['mask'].cpu().numpy(), want[0] >= 0)
    r = closest.points(b, s['p'].reshape(25, 20, 3), s['max_dist'])         # leading dimensions are kept
    assert tuple(r['tri'].shape) == (25, 20) and tuple(r['point'].shape) == (25, 20, 3)
    assert np.array_equal(r['tri'].cpu().numpy().reshape(-1), want[0])
    tri, dist, bary, point = ops.closest_points(b['ws'], b['T'], _d(s['p'], cuda), s['max_dist'], want_bary=False, want_point=False)
    assert bary is None and point is None and np.array_equal(tri.cpu().numpy(), want[0])


SKEW = dict(origin=(-1.45, -1.4, -1.5), du=(0.19, 0.01, 0.0), dv=(-0.008, 0.2, 0.012), dw=(0.004, -0.006, 0.2))


@pytest.mark.parametrize('shape', [(5, 9, 17), (16, 16, 16)])
def test_the_lattice_equals_the_points(cuda, shape):
    v, t = C.icosphere(2)
    b = cast.build(dict(vertices=v, triangles=t))
    P = lattice_ref.points(SKEW, shape, F32)
    for md in (np.inf, 0.6):
        dist, tri = ops.closest_grid(b['ws'], b['T'], shape, SKEW['origin'], SKEW['du'], SKEW['dv'], SKEW['dw'], md)
        assert tuple(dist.shape) == shape and tuple(tri.shape) == shape
        tri_p, dist_p, _, _ = _query(cuda, b, P, md)
        assert np.array_equal(R.bits(dist.cpu().numpy().reshape(-1)), R.bits(dist_p)) and np.array_equal(tri.cpu().numpy().reshape(-1), tri_p)
        want = R.closest32(v, t, P, md)
        assert np.array_equal(R.bits(dist_p), R.bits(want[1])) and np.array_equal(tri_p, want[0])
    only, none = ops.closest_grid(b['ws'], b['T'], shape, SKEW['origin'], SKEW['du'], SKEW['dv'], SKEW['dw'], want_tri=False)
    assert none is None and np.array_equal(R.bits(only.cpu().numpy().reshape(-1)), R.bits(R.closest32(v, t, P)[1]))


def test_the_offset_surface_of_a_sphere_through_mesh_surface(cuda):
    v, t = C.icosphere(2)
    b = cast.build(dict(vertices=v, triangles=t))
    r, step = 0.3, 0.2
    axes = np.stack([np.asarray(SKEW[k], np.float64) / step for k in ('du', 'dv', 'dw')])
    g = closest.grid(b, SKEW['origin'], (16, 16, 16), step, axes=axes)
    assert np.array_equal(R.bits(g['density'].cpu().numpy().reshape(-1)), R.bits(R.closest32(v, t, lattice_ref.points(SKEW, (16, 16, 16), F32))[1]))
    s = mesh.surface(g, r, normals=False)
    X = s['vertices'].cpu().numpy()
    assert X.shape[0] > 500 and s['triangles'].shape[0] > 1000
    # a vertex lies on a lattice edge a b of length l, at a + x (b - a) where the interpolated distance is r.  The distance is
    # 1-Lipschitz: d(X) <= d_a + x l and d(X) <= d_b + (1 - x) l, so d(X) - r <= 2 x (1 - x) l <= l / 2, and likewise from
    # below.  The longest edge of the tetrahedra is a cell diagonal, here below twice the step: every vertex within the step.
    diag = max(float(np.linalg.norm(a * np.asarray(SKEW['du']) + c * np.asarray(SKEW['dv']) + np.asarray(SKEW['dw']))) for a in (-1, 1) for c in (-1, 1))
    assert diag / 2 <= step
    d = R.closest64(v, t, X)['dist']
    assert np.abs(d - r).max() <= step, (np.abs(d - r).max(), step)


def test_attributes_at_the_closest_points_of_a_coloured_sphere(cuda):
    v, t = C.icosphere(2)
    rgb = ((v.astype(np.float64) + 1) / 2).astype(F32)
    owner = (np.arange(v.shape[0]) % 5).astype(np.int32)
    b = cast.build(dict(vertices=v, triangles=t, rgb=rgb, owner=owner))
    rng = np.random.default_rng(9)
    p = (rng.normal(size=(500, 3)) * 0.8).astype(F32)
    r = closest.points(b, p)
    a = closest.attributes(b, r)
    assert set(a) == {'rgb', 'owner'} and tuple(a['rgb'].shape) == (500, 3)
    tri, bary = r['tri'].cpu().numpy(), r['bary'].cpu().numpy().astype(np.float64)
    want = (bary[:, :, None] * rgb[t[tri]].astype(np.float64)).sum(1)      # float64 interpolation with the device's weights
    assert np.abs(a['rgb'].cpu().numpy() - want).max() <= 4 * U
    c = R.closest64(v, t, p)
    clear = c['gap'] > 1e-4 * c['dist']
    assert clear.sum() > 300 and np.array_equal(tri[clear], c['tri'][clear])
    # against the float64 weights: the weights' error is closest64's dC (5 U kappa (|s| + 1.5 L) <= 7e-6 here) over the shortest
    # edge (0.27), times the colour's range over a triangle (0.16): 4e-6, plus the interpolation's 4 U
    want64 = (c['bary'][:, :, None] * rgb[t[c['tri']]].astype(np.float64)).sum(1)
    assert np.abs(a['rgb'].cpu().numpy() - want64)[clear].max() <= 1e-5
    assert np.array_equal(a['owner'].cpu().numpy(), owner[t[tri, 0]])
    # the closest point is where the weights say
    assert np.abs((bary[:, :, None] * v[t[tri]].astype(np.float64)).sum(1) - r['point'].cpu().numpy()).max() <= 8 * U


def test_completeness_against_the_surface_has_no_sample_spacing(cuda):
    h = 0.05
    plane = dict(vertices=np.asarray([(0, 0, 0), (4, 0, 0), (4, 4, 0), (0, 4, 0)], F32), triangles=np.asarray([(0, 1, 2), (0, 2, 3)], np.int32))
    rng = np.random.default_rng(3)
    truth = _d(np.concatenate([rng.uniform(0.2, 3.8, (2000, 2)), np.full((2000, 1), h)], 1).astype(F32), cuda)
    exact = geometry.surface_distance(plane, truth, 0.5, thresholds=(0.1,), samples=400, keep=True)
    assert abs(exact['completeness'] - h) <= 4 * U and exact['truth_found'] == 2000 and exact['recall'] == [1.0]
    assert float((exact['truth_dist'] - h).abs().max()) <= 4 * U * 4
    pred = geometry.sample_mesh(plane, 400)[0]
    sampled = geometry.cloud_distance(pred, truth, 0.5, thresholds=(0.1,))
    assert sampled['completeness'] > 1.5 * h                                 # 400 samples of 16 square units: a spacing of 0.2
    assert set(sampled) == set(geometry.surface_distance(plane, truth, 0.5, thresholds=(0.1,), samples=400))
    assert abs(exact['accuracy'] - sampled['accuracy']) < 1e-6               # the accuracy side is cloud_distance's


def _error_ply(path):
    """geometry.write_error_ply's records"""
    raw = open(path, 'rb').read()
    head, body = raw.split(b'end_header\n', 1)
    n = int(head.split(b'element vertex ')[1].split(b'\n')[0])
    return np.frombuffer(body, geometry._ERROR_VERTEX, count=n)


def test_eval_geometry_exact_on_the_synthetic_scene(cuda, tmp_path):
    """the command end to end, with and without --exact, each in a fresh child process: the same truth, the same samples, and
    the completeness side measured against the mesh itself"""
    docs, plys = {}, {}
    for flag in ('exact', 'plain'):
        out = str(tmp_path / flag)
        cmd = [sys.executable, '-m', 'durf_amd.eval_geometry', '--synthetic', '--eval_dir', out, '--source', 'mesh', '--samples', '3000',
               '--iso', '0.001', '--grid=-2,-2,-1;16,16,8;0.25', '--max_dist', '0.5', '--thresholds', '0.1,0.5', '--synthetic_size', '16', '24',
               '--gin_param', 'MipNerfModel.num_samples = 32', '--gin_param', 'MipNerfModel.no_pose_opt = True',
               '--gin_param', 'MipNerfModel.no_yaw_opt = True', '--gin_param', 'MipNerfModel.mlp_precision = \'f32\''] + (['--exact'] if flag == 'exact' else [])
        p = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
        assert p.returncode == 0, p.stdout.decode()
        assert sorted(os.listdir(out)) == ['accuracy.ply', 'completeness.ply', 'geometry.json']
        docs[flag] = json.load(open(os.path.join(out, 'geometry.json')))
        plys[flag] = (_error_ply(os.path.join(out, 'accuracy.ply')), _error_ply(os.path.join(out, 'completeness.ply')))
    ex, pl = docs['exact'], docs['plain']
    assert ex['exact'] is True and 'exact' not in pl and set(ex) == set(pl) | {'exact'}
    assert set(ex['grids']) == {'pred_to_truth'} and set(pl['grids']) == {'pred_to_truth', 'truth_to_pred'}
    # (the freshly initialised synthetic field has no surface at any iso, as in the command's own test in test_gpu_geom.py: the
    # mesh is empty, the samples are NaN rows, every truth point reports max_dist -- the flag's whole path runs all the same;
    # a mesh with triangles goes through the same functions and files below)
    assert ex['source'] == pl['source'] and ex['pred_points'] == 3000 and ex['truth_points'] == pl['truth_points'] > 0
    # the accuracy side is cloud_distance's: the same samples against the same truth, the same file and figures
    assert plys['exact'][0].tobytes() == plys['plain'][0].tobytes()
    for k in ('accuracy', 'accuracy_truncated', 'accuracy_rms', 'precision', 'pred_usable', 'pred_found', 'truth_usable'):
        assert ex[k] == pl[k], k
    # completeness.ply holds the exact distances: the same points, never farther than the nearest SAMPLE of the mesh (to the
    # rounding of either distance: 64 U of the scene's extent of 4), with max_dist where nothing is within it, and they are
    # the figures of the json
    ce, cp = plys['exact'][1], plys['plain'][1]
    assert all(np.array_equal(ce[k], cp[k]) for k in 'xyz') and ce.shape[0] == ex['truth_points']
    de, dp = ce['distance'].astype(np.float64), cp['distance'].astype(np.float64)
    assert not np.isnan(de).any() and (de <= 0.5).all() and (de <= dp + 64 * U * 4).all()
    found = de < 0.5
    print('exact: %d of %d truth points within max_dist (sampled: %d); completeness %r against %r' % (found.sum(), len(de), (dp < 0.5).sum(), ex['completeness'], pl['completeness']))
    assert ex['truth_found'] >= pl['truth_found'] and ex['truth_found'] >= found.sum()
    assert abs(ex['completeness_truncated'] - de.mean()) <= 1e-9 and ex['completeness_truncated'] <= pl['completeness_truncated'] + 64 * U * 4
    if ex['truth_found'] == found.sum() > 0:                                 # (no point at exactly max_dist: found is what the json counts)
        assert abs(ex['completeness'] - de[found].mean()) <= 1e-9
    # what main() does with surface_distance's result, on a mesh that has triangles: the json takes it, the ply holds the exact distances
    from durf_amd import eval_geometry
    v, t = C.icosphere(2)
    truth = _d((np.random.default_rng(4).normal(size=(700, 3)) * 0.7).astype(F32), cuda)
    res = geometry.surface_distance(dict(vertices=v, triangles=t), truth, 0.5, thresholds=(0.1, 0.5), samples=500, keep=True)
    doc = {k: x for k, x in res.items() if k not in ('pred', 'pred_dist', 'pred_index', 'truth_dist', 'truth_index', 'truth_bary')}
    assert set(doc) == set(pl) - {'source', 'pred_points', 'truth_points', 'frames', 'split', 'keep_objects'} and json.loads(json.dumps(eval_geometry._json(doc)))
    assert tuple(res['pred'].shape) == (500, 3) and doc['truth_found'] > 100
    path = str(tmp_path / 'completeness.ply')
    assert geometry.write_error_ply(path, truth, res['truth_dist'], 0.5) == 700
    want = R.closest32(v, t, truth.cpu().numpy(), 0.5)
    assert np.array_equal(R.bits(_error_ply(path)['distance']), R.bits(want[1])) and np.array_equal(res['truth_index'].cpu().numpy(), want[0])


def test_mesh_to_mesh(cuda):
    v, t = C.icosphere(2)
    a = dict(vertices=v, triangles=t)
    same = closest.mesh_to_mesh(a, a, 3000, 0.5)
    # zero to rounding: a sample is built from its weights (5 U of a coordinate), and at dist = 0 the closest point's own
    # in-plane error counts in full (closest64: dC = 5 U kappa (|s| + 1.5 L), about 30 U here) beside dq (6 U): 64 U
    assert same['hausdorff'] <= 64 * U and same['accuracy'] <= 64 * U and same['completeness'] <= 64 * U and same['pred_found'] == 3000
    big = dict(vertices=v * F32(1.1), triangles=t)
    d = closest.mesh_to_mesh(a, big, 3000, 0.5)
    # between the two spheres' meshes: at least the gap between the inner's vertices and the outer's faces, at most 0.1 plus a sagitta
    assert 0.08 < d['accuracy'] < 0.12 and 0.08 < d['completeness'] < 0.12 and 0.08 < d['hausdorff_ab'] <= 0.115 and d['hausdorff'] >= d['hausdorff_ba']
    none = closest.mesh_to_mesh(a, dict(vertices=v + F32(5), triangles=t), 100, 0.5)
    assert none['hausdorff'] is None and none['pred_found'] == 0 and none['accuracy_truncated'] == 0.5


def test_an_empty_tree_and_no_points(cuda):
    b = cast.build(dict(vertices=np.zeros((0, 3), F32), triangles=np.zeros((0, 3), np.int32)))
    r = closest.points(b, np.asarray([(0, 0, 0), (np.nan, 0, 0)], F32), 0.25)
    assert r['tri'].tolist() == [-1, -2] and float(r['dist'][0]) == 0.25 and bool(torch.isnan(r['dist'][1]))
    r = closest.points(b, np.zeros((0, 3), F32))
    assert tuple(r['tri'].shape) == (0,) and tuple(r['bary'].shape) == (0, 3)
    g = closest.grid(b, (0, 0, 0), (3, 2, 5), 0.5, max_dist=2.0)
    assert bool((g['density'] == 2.0).all()) and bool((g['tri'] == -1).all())


def test_refusals_reach_python_with_their_text(cuda):
    v, t = C.quad_grid(2)
    b = cast.build(dict(vertices=v, triangles=t))
    p = _d(np.zeros((4, 3), F32), cuda)
    for call, text in ((lambda: ops.closest_points(b['ws'], b['T'], p, 0.0), 'max_dist is +inf or in [1e-18, 1e18]'),
                       (lambda: ops.closest_points(b['ws'], 100, p), 'durf_cast_workspace_bytes(100)'),
                       (lambda: ops.closest_points(b['ws'], -1, p), 'T = -1'),
                       (lambda: ops.closest_grid(b['ws'], b['T'], (0, 4, 4), (0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1)), 'nu = 0'),
                       (lambda: ops.closest_grid(b['ws'], b['T'], (4, 4, 4), (0, 0, 0), (np.inf, 0, 0), (0, 1, 0), (0, 0, 1)), 'are finite')):
        with pytest.raises(_lib.DurfError) as e:
            call()
        assert text in str(e.value) and text in _lib.lib().durf_last_error().decode()
