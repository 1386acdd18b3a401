"""One mesh through every consumer of csrc/triangles.h, bit for bit against the oracles the consumers already have:
dirty_mesh() as it is -- out-of-range and negative indices, vertices that are not finite, triangles without area -- merged with a
level-1 icosphere around it, so that something is hit and one camera stands inside.  Integers and written-out fp32 everywhere:
exact equality, no tolerance."""
import functools

import numpy as np
import pytest
import torch

from durf_amd import camera, cast, closest, geometry, ops, raster, shade
from durf_amd._cast_sigs import DURF_CAST_BLOCK
from tests import camera_ref, cast_ref as R, closest_ref, geom_ref as G, raster_ref, shade_ref as S, trimesh_ref as M

pytestmark = pytest.mark.gpu
I32, F32 = torch.int32, np.float32
H, W, N = 13, 21, DURF_CAST_BLOCK + 1           # a partial raster tile and partial 8 x 8 shade tiles; one live thread in the last block
BAD = 11                                        # dirty_mesh's triangle with the index -1


def _d(a, cuda, dtype=torch.float32):
    return torch.as_tensor(np.array(a)).to(device=cuda, dtype=dtype).contiguous()


def _same(got, want, what):
    got = got.cpu().numpy() if torch.is_tensor(got) else got
    a, b = (x if x.dtype == np.uint8 else R.bits(x) for x in (np.ascontiguousarray(got), np.ascontiguousarray(want)))
    assert a.shape == b.shape and np.array_equal(a, b), (what, np.argwhere(a != b)[:5])


@functools.lru_cache(maxsize=None)
def scene():
    """-> dict v, t, rgb [V,3], owner [V], cams [2,CAM_FLOATS], o, d [2 H W,3] (the pixels' rays); computed once, not to be written to"""
    v, t = M.merge(M.dirty_mesh(), M.icosphere(1, 2.0, (0.5, 0.5, 0.5)))   # (dirty first: its bad indices stay what they are)
    rng = np.random.default_rng(7)
    rgb, owner = rng.random((v.shape[0], 3)).astype(F32), rng.integers(0, 9, v.shape[0]).astype(np.int32)
    c2w = [camera_ref.look_at((0.5, 0.5, 0.5), (3.0, 1.0, 0.7), up=(0.0, 0.0, 1.0)), camera_ref.look_at((4.5, -3.0, 2.5), (0.5, 0.5, 0.5), up=(0.0, 0.0, 1.0))]
    cams = camera.rows(c2w, 11.0, (W / 2.0 - 0.25, H / 2.0), H, W)          # camera 0 stands inside the sphere, among the soup
    o, d = (np.concatenate(x) for x in zip(*(R.pinhole32(c, H, W) for c in cams)))
    return dict(v=v, t=t, rgb=rgb, owner=owner, cams=cams, o=o, d=d)


@functools.lru_cache(maxsize=None)
def primary():
    """cast32 of the pixels' rays: (tri, t, bary), shared"""
    s = scene()
    return R.cast32(s['v'], s['t'], s['o'], s['d'])


@pytest.fixture(scope='module')
def built(cuda):
    s = scene()
    return cast.build(dict(vertices=s['v'], triangles=s['t'], rgb=s['rgb'], owner=s['owner']))      # once


def _samples():
    """N samples on the mesh, some on no triangle, on an unusable ray, past the last triangle and on a triangle with a bad index"""
    s = scene()
    T = s['t'].shape[0]
    rng = np.random.default_rng(3)
    tri = rng.integers(0, T, N).astype(np.int32)
    tri[:8] = (-1, -2, T, BAD, 12, 13, 2 ** 31 - 1, T - 1)
    tri[-1] = BAD
    bary = rng.dirichlet((1, 1, 1), N).astype(F32)
    bary[1] = np.nan
    return tri, bary, rng.normal(size=(N, 3)).astype(F32)


def _label(s, tri):
    t, tri = s['t'].astype(np.int64), np.asarray(tri, np.int64).reshape(-1)
    ok = (tri >= 0) & (tri < t.shape[0])
    ok[ok] = ((t[tri[ok]] >= 0) & (t[tri[ok]] < s['v'].shape[0])).all(1)
    return np.where(ok, s['owner'][np.where(ok, t[np.where(ok, tri, 0), 0], 0)], -1).astype(np.int32)


def test_the_scene_reaches_what_it_is_for():
    s, (tri, _, _) = scene(), primary()
    valid = M.valid_triangles(s['v'], s['t'])[0]
    assert not valid[[11, 13, 20, 21, 22]].any() and valid.sum() > 250 and (tri >= 0).sum() > H * W and (tri[:H * W] >= 0).all()
    assert (tri[H * W:] == -1).any() and (tri[tri >= 0] < 200).any() and (tri >= 200).any() and H % 8 and W % 8 and W % 16


def test_cast_cameras_and_its_attribute_planes(cuda, built):
    s, (tri, t, bary) = scene(), primary()
    r = cast.cameras(built, s['cams'])
    _same(r['tri'].reshape(-1), tri, 'tri'), _same(r['depth'].reshape(-1), t, 'depth'), _same(r['bary'].reshape(-1, 3), bary, 'bary')
    _same(r['rgb'].reshape(-1, 3), M.interp32(s['t'], tri, bary, s['rgb']), 'rgb'), _same(r['owner'].reshape(-1), _label(s, tri), 'owner')
    # the same planes by hand: the attribute planes of a view are durf_raster_interp on its tri and bary
    by_hand = ops.raster_interp(built['triangles'], r['tri'], r['bary'], built['V'], attr_f=_d(s['rgb'], cuda), attr_i=_d(s['owner'], cuda, I32), fill=-1)
    assert torch.equal(by_hand[0].view(I32), r['rgb'].view(I32)) and torch.equal(by_hand[1], r['owner'])


def test_shade_cameras(cuda, built):
    s, (tri, t, bary) = scene(), primary()
    dirs, reach, ambient, bg = S.fibonacci(8), 0.5, 0.4, (0.25, 0.5, 1.0)
    r = shade.cameras(built, s['cams'], dirs=dirs, reach=reach, light=(0.3, -0.2, 0.9), ambient=ambient, background=bg)
    _same(r['tri'].reshape(-1), tri, 'tri'), _same(r['depth'].reshape(-1), t, 'depth')
    p, nr = S.surface32(s['v'], s['t'], tri, bary, s['d'])
    _same(r['normal'].reshape(-1, 3), nr, 'normal')
    used, blocked = S.occlusion32(s['v'], s['t'], p, nr, dirs, r['bias'], reach)
    sun = S.occlusion32(s['v'], s['t'], p, nr, np.asarray([r['light']], F32), r['bias'], np.inf)[1]
    _same(r['ao_used'].reshape(-1), used, 'used'), _same(r['ao_blocked'].reshape(-1), blocked, 'blocked')
    out_f, out_8 = S.compose32(tri, nr, used, blocked, r['light'], ambient, bg, sun, M.interp32(s['t'], tri, bary, s['rgb']))
    _same(r['shaded'].reshape(-1, 3), out_f, 'shaded'), _same(r['shaded8'].reshape(-1, 3), out_8, 'shaded8')
    _same(r['shaded8'].reshape(-1, 3), M.u8(r['shaded'].reshape(-1, 3).cpu().numpy()), 'the bytes of the floats')
    assert blocked.sum() > 0 and sun.sum() > 0


def test_render_mesh(cuda):
    s = scene()
    want = raster_ref.draw32(s['cams'], H, W, s['v'], s['t'], 0.05)
    r = raster.render_mesh(dict(vertices=s['v'], triangles=s['t'], rgb=s['rgb'], owner=s['owner']), s['cams'], znear=0.05)
    for k in ('tri', 'depth', 'bary'):
        _same(r[k], want[k], k)
    assert np.array_equal(r['counts'].sum(0)[1:], want['counts'].astype(np.int64)[1:]) and want['counts'][2] >= 5 and (want['tri'] >= 0).sum() > H * W
    _same(r['rgb'].reshape(-1, 3), M.interp32(s['t'], want['tri'], want['bary'], s['rgb']), 'rgb')
    _same(r['owner'].reshape(-1), _label(s, want['tri']), 'owner')


def test_rays_and_closest_points_with_one_thread_in_the_last_block(cuda, built):
    s = scene()
    o, d = R.random_rays(N, 17, centre=0.5, spread=2.5)
    r = cast.rays(built, o, d)
    for k, want in zip(('tri', 't', 'bary'), R.cast32(s['v'], s['t'], o, d)):
        _same(r[k], want, k)
    r = closest.points(built, o, max_dist=1.5)
    for k, want in zip(('tri', 'dist', 'bary', 'point'), closest_ref.closest32(s['v'], s['t'], o, 1.5)):
        _same(r[k], want, k)
    assert int(r['mask'].sum()) > N // 4 and not bool(r['mask'].all())


def test_surface_compose_and_interp_on_samples_that_name_no_readable_triangle(cuda, built):
    s, (tri, bary, toward) = scene(), _samples()
    p, nr = shade.surface(built, tri, bary, toward)
    wp, wn = S.surface32(s['v'], s['t'], tri, bary, toward)
    _same(p, wp, 'point'), _same(nr, wn, 'normal')
    assert not wp[[0, 1, 2, 3, 5, 6, -1]].any() and wp[4].any() and wp[7].any()      # (12 names vertex 600: the sphere's first, in this mesh)
    rng = np.random.default_rng(5)
    used = rng.integers(0, 9, N).astype(np.int32)
    blocked = (used * rng.random(N)).astype(np.int32)
    albedo = M.interp32(s['t'], tri, bary, s['rgb'])
    f, u8 = shade.compose(_d(tri, cuda, I32), wn, used, blocked, light=(0.0, 0.6, 0.8), ambient=0.3, background=(0.1, 0.2, 0.3), albedo=albedo)
    wf, w8 = S.compose32(tri, wn, used, blocked, (0.0, 0.6, 0.8), 0.3, (0.1, 0.2, 0.3), None, albedo)
    _same(f, wf, 'shaded'), _same(u8, w8, 'shaded8'), _same(u8, M.u8(f.cpu().numpy()), 'the bytes of the floats')
    for C in (1, 4):
        attr = rng.normal(size=(s['v'].shape[0], C)).astype(F32)
        got = ops.raster_interp(built['triangles'], _d(tri, cuda, I32), _d(bary, cuda), built['V'], attr_f=_d(attr, cuda), attr_i=_d(s['owner'], cuda, I32), fill=-1)
        _same(got[0], M.interp32(s['t'], tri, bary, attr), ('interp', C)), _same(got[1], _label(s, tri), ('label', C))
    assert not albedo[[0, 1, 2, 3, 5, 6, -1]].any() and albedo[4].any() and albedo[7].any()


def test_sample_mesh(cuda, built):
    s = scene()
    p, tri = geometry.sample_mesh(built, 257)
    want, wtri, _, total = G.sample_mesh(s['v'], s['t'], 257, dtype=np.float32)
    _same(tri, wtri, 'tri'), _same(p, want, 'points')
    assert total > 0 and np.isfinite(want).all() and M.valid_triangles(s['v'], s['t'])[0][wtri].all()


def test_the_8_bit_rule_is_one(cuda):
    """One float plane -- a rendered frame, packed by k_frame_pack -- gives the same bytes through the pack, through k_shade_compose
    and through trimesh_ref.u8.  The vis kernels take no plane (they colour a depth or a hue): their bytes are held to u8 of their
    own floats, and compose once more on values that cross every rounding case."""
    from tests import test_gpu_trajectory as TJ
    model, variables, _, ext, cams = TJ._scene(cuda, (9, 7))               # 63 pixels in chunks of 25: aligned groups and partial ones
    r = model.render_trajectory(variables, cams[:2], TJ.TIMES[:2], ext, True, TJ.ALPHA, near=TJ.NEAR, far=TJ.FAR, chunk=25, outputs=('rgb8', 'rgb'))
    frame = r['rgb'].reshape(-1, 3).contiguous()
    want = M.u8(frame.cpu().numpy())
    assert len(np.unique(want)) > 16, 'a picture, not a constant'
    _same(r['rgb8'].reshape(-1, 3), want, 'frame pack')

    def composed(plane3):
        # ambient 1, nothing blocked: shade = 1 exactly, so the colour is the albedo itself
        n = plane3.shape[0]
        one, zero = np.ones(n, np.int32), np.zeros(n, np.int32)
        return shade.compose(_d(zero, cuda, I32), np.zeros((n, 3), F32), one, zero, light=(0, 0, 1), ambient=1.0, albedo=plane3)
    f, u8 = composed(frame)
    assert torch.equal(f.view(I32), frame.view(I32)) and torch.equal(u8, r['rgb8'].reshape(-1, 3))      # the same plane, the same bytes
    x = np.concatenate([(np.arange(0, 512) + 0.5) / 510.0, [0.0, 1.0, 0.999, 0.5 / 255, 1.5 / 255, 2.5 / 255]]).astype(F32)
    rgb, rgb8 = ops.vis_sinebow(_d(x, cuda), want_u8=True)
    _same(rgb8, M.u8(rgb.cpu().numpy()), 'sinebow')
    plane = np.concatenate([x, [np.nan, -1.0, 2.0, np.inf, -np.inf, 1.5]]).astype(F32)
    f, u8 = composed(np.repeat(plane[:, None], 3, 1))
    _same(f[:, 0], plane, 'the plane itself'), _same(u8, np.repeat(M.u8(plane)[:, None], 3, 1), 'compose')
