"""libdurf_cast.so on the device against tests/cast_ref.py: cast32 (the header's definition by brute force) in every bit of
tri, t and bary on the smallest shapes at which a cast can go wrong, whatever permutation the tree is built over; the keys;
cameras against rays; the rasteriser beside it; and what the feature is for -- a camera inside the mesh, a LIDAR sweep of a
mesh, visibility."""
import math

import numpy as np
import pytest
import torch

from durf_amd import camera, cast, lidar, ops, raster, raygen
from tests import camera_ref, cast_ref as R, raster_ref

pytestmark = pytest.mark.gpu
I32 = torch.int32
U = 2.0 ** -24


def _d(a, cuda, dtype=torch.float32):
    return torch.as_tensor(np.array(a)).to(device=cuda, dtype=dtype).contiguous()


def _mesh(s):
    return dict(vertices=s['v'], triangles=s['t'])


def _bound(b, n, cuda):
    return _d(np.array(np.broadcast_to(np.asarray(b, np.float32), (n,))), cuda) if isinstance(b, np.ndarray) else float(b)


def _cast(cuda, s, order=None):
    b = cast.build(_mesh(s), order=order)
    n = s['o'].shape[0]
    o, d = _d(s['o'], cuda).reshape(n, 3), _d(s['d'], cuda).reshape(n, 3)
    tmin, tmax = _bound(s['tmin'], n, cuda), _bound(s['tmax'], n, cuda)
    tri, t, bary = ops.cast_rays(b['ws'], b['T'], o, d, tmin, tmax, s['cull'])
    hit = ops.cast_any(b['ws'], b['T'], o, d, tmin, tmax, s['cull'])
    return tri.cpu().numpy(), t.cpu().numpy(), bary.cpu().numpy(), hit.cpu().numpy()


def _same(got, want, what):
    for k, a, b in zip(('tri', 't', 'bary'), got, want):
        a, b = R.bits(a), R.bits(b)
        assert a.shape == b.shape and np.array_equal(a, b), (what, k, np.argwhere(a != b)[:5])


@pytest.mark.parametrize('name', sorted(R.scenes()))
def test_every_bit_of_the_definition_whatever_the_tree(cuda, name):
    s, want = R.scenes()[name], R.expected(name)
    tri, t, bary, hit = _cast(cuda, s)
    _same((tri, t, bary), want, name)
    assert np.array_equal(hit, np.where(want[0] >= 0, 1, np.where(want[0] == -2, -2, 0))), name
    # a different valid permutation in place of the Morton sort: the tree cannot change an answer
    T = s['t'].shape[0]
    tri2, t2, bary2, hit2 = _cast(cuda, s, order=np.random.default_rng(7).permutation(T).astype(np.int32))
    _same((tri2, t2, bary2), want, name + ' (random order)')
    assert np.array_equal(hit2, hit)


def test_keys_follow_the_headers_rule(cuda):
    for v, t in (R.dirty_mesh(), R.random_soup(1025, 3), R.quad_grid(16)):
        bounds = np.concatenate([np.nanmin(np.where(np.isfinite(v), v, np.nan), 0), np.nanmax(np.where(np.isfinite(v), v, np.nan), 0)]).astype(np.float32)
        got = ops.cast_keys(_d(v, cuda), _d(t, cuda, I32), _d(bounds, cuda)).cpu().numpy()
        assert np.array_equal(got, R.keys(v, t, bounds))
    flat = np.asarray([0, 0, 0, 1, 1, 0], np.float32)                       # a zero-extent axis gives 0
    v, t = R.quad_grid(4)
    got = ops.cast_keys(_d(v * np.float32(0.25), cuda), _d(t, cuda, I32), _d(flat, cuda)).cpu().numpy()
    assert np.array_equal(got, R.keys(v * np.float32(0.25), t, flat)) and not (got & 0x1249249249249249).any()
    # build's own route sorts by them: the same order as the oracle's
    b = cast.build(dict(vertices=v, triangles=t))
    assert np.array_equal(b['order'].cpu().numpy(), R.morton_order(v, t))


@pytest.mark.parametrize('size', [(5, 51), (16, 16)])
def test_cameras_equal_rays_on_the_generators_rays(cuda, size):
    h, w = size
    v, t = R.icosphere(2)
    b = cast.build(dict(vertices=v, triangles=t))
    cams = camera.rows([camera_ref.look_at((0.3, 0.2, 3.0), (0.0, 0.0, 0.0)), camera_ref.look_at((0.1, 0.2, 0.3), (1.0, 0.5, 0.0))],
                       0.9 * w, (w / 2.0 - 0.25, h / 2.0), h, w)                # one outside, one inside the sphere
    for cull in (0, 1):
        tri, depth, bary = ops.cast_cameras(b['ws'], b['T'], _d(cams, cuda), h, w, 0.0, float('inf'), cull)
        assert tuple(tri.shape) == (2, h, w) and tuple(bary.shape) == (2, h, w, 3)
        for f in range(2):
            r = raygen.camera_rays(cams[f], 0.0, 1.0, device=cuda)
            tri_r, t_r, bary_r = ops.cast_rays(b['ws'], b['T'], r.origins.contiguous(), r.directions.contiguous(), 0.0, float('inf'), cull)
            _same((tri[f].cpu().numpy(), depth[f].cpu().numpy(), bary[f].cpu().numpy()),
                  (tri_r.cpu().numpy(), t_r.cpu().numpy(), bary_r.cpu().numpy()), (size, cull, f))
            o, d = R.pinhole32(cams[f], h, w)
            _same((tri[f].cpu().numpy().reshape(-1), depth[f].cpu().numpy().reshape(-1), bary[f].cpu().numpy().reshape(-1, 3)),
                  R.cast32(v, t, o, d, cull=cull), (size, cull, f, 'oracle'))
        if cull == 0:
            assert (tri[1] >= 0).all()                                       # from inside a closed surface every pixel sees it
    bad = cams.copy()
    bad[1, camera.CAM_W] = w + 1                                            # a row of another size: its frame is unusable
    tri, depth, _ = ops.cast_cameras(b['ws'], b['T'], _d(bad, cuda), h, w)
    assert (tri[1] == -2).all() and torch.isnan(depth[1]).all() and (tri[0] >= -1).all()


@pytest.mark.parametrize('cull', [0, 1])
def test_beside_the_rasteriser(cuda, cull):
    h = w = 64
    v, t = R.icosphere(2)
    cams = camera.rows([camera_ref.look_at((0.4, 0.3, 3.0), (0.0, 0.0, 0.0))], 80.0, (w / 2.0 - 0.5, h / 2.0 - 0.5), h, w)
    m = dict(vertices=v, triangles=t)
    rast = raster.render_mesh(m, cams, znear=0.1, attrs=(), label=None, cull=cull)
    cst = cast.cameras(cast.build(m), cams, attrs=(), label=None, cull=cull)
    host = lambda r: dict(tri=r['tri'].cpu().numpy(), depth=r['depth'].cpu().numpy())
    o, d = R.pinhole32(cams[0], h, w)
    c64 = R.cast64(v, t, o, d, cull=cull)
    c64 = dict(tri=c64['tri'].reshape(1, h, w), depth=c64['t'].reshape(1, h, w))
    res = R.rasteriser_comparison(host(rast), host(cst), raster_ref.draw64(cams, h, w, v, t, 0.1, cull), c64, t)
    print('cull %d: %s' % (cull, res))
    assert res['same'] > 1500                                                # the sphere fills a good part of the frame


def test_a_camera_inside_the_mesh_has_no_holes(cuda):
    """what the feature is for: the floor under a street-level camera crosses znear; the rasteriser drops it, a ray does not"""
    v, t = R.box_mesh((-6.0, 0.0, -6.0), (6.0, 3.0, 6.0))
    owner = np.zeros(v.shape[0], np.int32)
    m = dict(vertices=v, triangles=t, owner=owner, rgb=(v - v.min(0)) / (v.max(0) - v.min(0)))
    h, w = 24, 40
    cams = camera.rows([camera_ref.look_at((0.5, 1.5, 0.25), (4.0, 1.0, -3.0)), camera_ref.look_at((-2.0, 0.5, 1.0), (0.0, 0.0, 5.0))],
                       20.0, (w / 2.0, h / 2.0), h, w)
    rast = raster.render_mesh(m, cams, znear=0.1)
    crossing = int(rast['counts'][:, raster.COUNT_FIELDS.index('crossing')].sum())
    assert crossing > 0 and int((rast['tri'] < 0).sum()) > 0                 # the holes
    c = cast.cameras(cast.build(m), cams)
    assert int((c['tri'] < 0).sum()) == 0 and bool(c['mask'].all())
    assert tuple(c['rgb'].shape) == (2, h, w, 3) and tuple(c['owner'].shape) == (2, h, w) and int(c['owner'].abs().sum()) == 0
    # where the rasteriser did draw, the two agree on the triangle (flat faces: no silhouette inside the box) and on the colour
    both = rast['tri'] >= 0
    assert bool((rast['tri'][both] == c['tri'][both]).float().mean() > 0.98)
    same = both & (rast['tri'] == c['tri'])
    assert float((rast['rgb'][same] - c['rgb'][same]).abs().max()) < 2e-3
    assert float(c['depth'].min()) > 0.0


def test_a_lidar_sweep_of_a_sphere_around_the_sensor(cuda):
    radius = 10.0
    v, t = R.icosphere(3, radius=radius, centre=(1.0, -2.0, 0.5))
    sensor = lidar.LidarSensor.uniform(8, -0.4, 0.3, 96, max_range=75.0)
    pose = np.concatenate([np.eye(3), [[1.0], [-2.0], [0.5]]], 1)
    b = cast.build(dict(vertices=v, triangles=t))
    s = cast.lidar(b, sensor, [pose, pose], near=0.1, far=50.0)
    assert tuple(s['range'].shape) == (2, 8, 96) and tuple(s['xyz'].shape) == (2, 8, 96, 3)
    assert bool((s['valid'] == 1).all()) and bool((s['tri'] >= 0).all())     # every return is valid
    # the range is within the mesh's own chord error of the radius: the faces lie between their planes' distance and the radius
    P = v[t].astype(np.float64) - np.asarray([1.0, -2.0, 0.5])
    nrm = np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0])
    inner = float(np.abs((nrm * P[:, 0]).sum(1) / np.linalg.norm(nrm, axis=1)).min())
    rng = s['range'].cpu().numpy().astype(np.float64)
    assert inner < radius and rng.min() >= inner * (1 - 64 * U) and rng.max() <= radius * (1 + 64 * U), (inner, rng.min(), rng.max())
    # xyz lies on the named triangle: it is the barycentric combination of its vertices
    tri, bary, xyz = s['tri'].cpu().numpy(), s['bary'].cpu().numpy().astype(np.float64), s['xyz'].cpu().numpy().astype(np.float64)
    on = (bary[..., None] * v[t][tri].astype(np.float64)).sum(-2)
    assert np.abs(on - xyz).max() <= 64 * U * (radius + 3.0), np.abs(on - xyz).max()
    assert np.array_equal(s['range'][0].cpu().numpy(), s['range'][1].cpu().numpy())
    points, count = cast.point_cloud(s, 0)
    assert int(count) == 8 * 96 and np.allclose(points[:, :3].cpu().numpy(), xyz[0].reshape(-1, 3), atol=1e-5)
    assert np.array_equal(points[:, 3].cpu().numpy(), s['range'][0].reshape(-1).cpu().numpy())


def test_visible_across_a_wall_and_past_its_edge(cuda):
    v = np.asarray([(0, -1, -1), (0, 1, -1), (0, 1, 1), (0, -1, 1)], np.float32)
    b = cast.build(dict(vertices=v, triangles=np.asarray([(0, 1, 2), (0, 2, 3)], np.int32)))
    a = np.asarray([(-1, 0, 0), (-1, 0, 0), (-1, 0, 0), (-1, 0, 0), (1, 0.5, 0.5), (-1, 0, 0), (-1, 0.25, 0.5)], np.float32)
    p = np.asarray([(1, 0, 0), (1, 0, 3), (-0.5, 0.9, 0.9), (-0.001, 0, 0), (-1, -0.5, -0.5), (-1, 0, 0), (0, 0.25, 0.5)], np.float32)
    #             through it   past its edge  same side     stops short    back through  no length  ends on it
    got = cast.visible(b, a, p).cpu().numpy()
    assert got.tolist() == [False, True, True, True, False, False, False]
    want = R.cast32(v, [(0, 1, 2), (0, 2, 3)], a, p - a, 0.0, 1.0)[0]
    assert np.array_equal(got, want == -1)
    hit = cast.occluded(b, a, p - a, 0.0, 1.0).cpu().numpy()
    assert hit.tolist() == [1, 0, 0, 0, 1, -2, 1]
    assert math.isnan(float(cast.rays(b, a[5], (p - a)[5])['t']))


def test_cast_mesh_command_end_to_end(cuda, tmp_path):
    import json
    from durf_amd import cast_mesh
    out = tmp_path / 'out'
    assert cast_mesh.main(['--synthetic', '--frames', '2', '--eval_dir', str(out)]) == 0
    meta = json.loads((out / 'cast.json').read_text())
    assert len(meta['frames']) == 2 and meta['triangles'] > 1000
    assert all(f['rays'] == meta['h'] * meta['w'] and f['unusable'] == 0 and 0 < f['hits'] < f['rays'] for f in meta['frames'])
    for f in range(2):
        d = np.load(out / ('depth_%04d.npy' % f))
        assert d.shape == (meta['h'], meta['w']) and int((d > 0).sum()) == meta['frames'][f]['hits']
        assert (out / ('depth_%04d.ppm' % f)).exists() and (out / ('ids_%04d.ppm' % f)).exists()
    assert not (out / 'depth_0002.npy').exists()
    assert meta['sweeps'] == [dict(rays=16 * 180, hits=16 * 180, unusable=0)] and (meta['beams'], meta['columns']) == (16, 180)
    rng = np.load(out / 'range_0000.npy')
    assert rng.shape == (16, 180) and abs(rng - 1.0).max() < 0.02           # the unit sphere from its centre
    assert (out / 'sweep_0000.ply').read_bytes().startswith(b'ply\nformat binary_little_endian 1.0\nelement vertex %d\n' % (16 * 180))
