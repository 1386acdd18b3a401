"""libdurf_raster.so against tests/raster_ref.draw32 on the device: tri, depth and bary EQUAL, compared as int32 bits, and the
counts equal -- exact pictures, launch and tile edges, every cull with its tally, a tile list longer than one LDS batch,
overflow of the pair list, the one-call route, interpolation, a real surface, and every refusal by its message."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from durf_amd import _lib, geometry, mesh, ops, raster, render_mesh, trajectory
from tests import raster_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I32 = torch.int32
U = 2.0 ** -24
CANARY = 0x5a5a5a5a


def _d(a, cuda, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a)).to(device=cuda, dtype=dtype).contiguous()


def _device(cuda, cams, h, w, v, t, znear, cull=0):
    """the three-call route: setup, the one read of counts, draw at the exact size -> host arrays"""
    cams = np.asarray(cams, np.float32).reshape(-1, 17)
    cd, vd, td = _d(cams, cuda), _d(v, cuda).reshape(-1, 3), _d(t, cuda, I32).reshape(-1, 3)
    counts, ws = ops.raster_setup(cd, h, w, vd, td, znear, cull)
    c = counts.cpu().numpy()
    tri, depth, bary = ops.raster_draw(cams.shape[0], td.shape[0], h, w, ws, int(c[0]))
    return dict(tri=tri.cpu().numpy(), depth=depth.cpu().numpy(), bary=bary.cpu().numpy(), counts=c)


def _same(got, want, what=''):
    assert np.array_equal(got['counts'], want['counts']), (what, got['counts'], want['counts'])
    assert np.array_equal(got['tri'], want['tri']), (what, np.argwhere(got['tri'] != want['tri'])[:5])
    for k in ('depth', 'bary'):
        a, b = got[k].view(np.int32), np.ascontiguousarray(want[k]).view(np.int32)
        assert np.array_equal(a, b), (what, k, np.argwhere(a != b)[:5])


def _both(cuda, cams, h, w, v, t, znear=0.5, cull=0, what=''):
    want = R.draw32(np.asarray(cams).reshape(-1, 17), h, w, v, t, znear, cull)
    got = _device(cuda, cams, h, w, v, t, znear, cull)
    _same(got, want, what)
    return got, want


# ---- 1 ---------------------------------------------------------------------------------------------------------------------------
def test_exact_pictures(cuda):
    """identity pose, focal and depths powers of two, vertices on pixel centres: the projection is exact, so the shared
    diagonal runs through pixel centres exactly"""
    h, w = 24, 28
    cam = R.camera(h, w, 64.0, pp=(0.0, 0.0))
    quad = np.array([(2, 2), (18, 2), (18, 18), (2, 18)], np.float64)
    v = R.to_world(cam, quad, 4.0)
    got, want = _both(cuda, cam, h, w, v, np.array([[0, 1, 2], [0, 2, 3]], np.int32), what='diagonal')
    diag = np.arange(3, 19)
    assert (want['cover'][0, diag, diag] == 1).all() and (got['tri'][0, diag, diag] >= 0).all()
    assert set(got['tri'][0, diag, diag].tolist()) <= {0, 1} and (got['depth'][0, diag, diag] == 4.0).all()
    assert got['counts'].tolist() == [2 * 4, 2, 0, 0, 0, 0, 0, 0]
    # two coincident triangles: the lower id wins, whichever comes first in memory order of evaluation
    got, _ = _both(cuda, cam, h, w, v, np.array([[0, 2, 3], [0, 1, 2], [2, 1, 0], [0, 1, 2]], np.int32), what='coincident')
    assert set(np.unique(got['tri']).tolist()) == {-1, 0, 1}
    # two interpenetrating triangles: the owner switches along the line where they meet
    a = R.to_world(cam, np.array([(2, 2), (20, 3), (4, 20)], np.float64), np.array([2.0, 8.0, 4.0]))
    b = R.to_world(cam, np.array([(3, 1), (21, 4), (3, 21)], np.float64), np.array([8.0, 2.0, 4.0]))
    got, want = _both(cuda, cam, h, w, np.concatenate([a, b]), np.array([[0, 1, 2], [3, 4, 5]], np.int32), what='interpenetrating')
    both = want['cover'][0] == 2
    assert both.sum() > 50 and (got['tri'][0][both] == 0).sum() > 10 and (got['tri'][0][both] == 1).sum() > 10


@pytest.mark.parametrize('rect', [(2.0, 3.0, 20.0, 17.0), (2.5, 3.5, 20.5, 16.5)])
def test_tilings_have_one_owner_per_pixel(cuda, rect):
    h, w = 24, 26
    cam = R.camera(h, w, 64.0, pp=(0.0, 0.0))
    for pts, tris in (R.fan(*rect, 11.0, 10.0, 6), R.grid(*rect, 6, 4)):
        pts = np.round(pts * 256.0) / 256.0
        got, want = _both(cuda, cam, h, w, R.to_world(cam, pts, 4.0), tris)
        assert want['cover'].max() == 1 and np.array_equal(got['tri'] >= 0, want['cover'] == 1)


# ---- 2 ---------------------------------------------------------------------------------------------------------------------------
def _edge_scene(h, w, T, seed):
    """triangle 0 covers the whole frame from behind everything; 1 has bounds ending exactly on the first tile border (or the
    frame's); the rest are random, many partly and some wholly off the frame -> three different cameras, vertices, triangles"""
    rng = np.random.default_rng(seed)
    focal = 32.0
    cams = np.stack([R.camera(h, w, focal, pp=(0.0, 0.0)),
                     R.camera(h, w, focal, R.look_at((0.3, 0.1, 0.2), (0.0, 0.0, -4.0)), pp=(1.0, 0.5)),
                     R.camera(h, w, 24.0, R.look_at((-0.4, 0.2, 0.0), (0.1, 0.0, -4.0)), pp=(w / 2.0, h / 2.0))])
    pts = [np.array([(-3.0 * w - 8, -8.0), (4.0 * w + 8, -8.0), (-8.0, 4.0 * h + 8)]), np.array([(0.0, 0.0), (min(15, w - 1), 0.0), (0.0, min(15, h - 1))])]
    zs = [np.full(3, 8.0), np.full(3, 4.0)]
    for _ in range(max(T - 2, 0)):
        c = rng.uniform((-6.0, -6.0), (w + 6.0, h + 6.0))
        pts.append(c + rng.normal(size=(3, 2)) * rng.choice([1.0, 4.0, 12.0]))
        zs.append(rng.uniform(2.0, 7.0, 3))
    pts, zs = np.concatenate(pts[:T]), np.concatenate(zs[:T])
    return cams, R.to_world(cams[0], pts, zs), np.arange(3 * T, dtype=np.int32).reshape(T, 3)


@pytest.mark.parametrize('size', [(1, 1), (15, 17), (16, 16), (17, 33)])
def test_launch_and_tile_edges(cuda, size):
    h, w = size
    for T in (1, 255, 256, 257):
        cams, v, t = _edge_scene(h, w, T, seed=T)
        got, _ = _both(cuda, cams, h, w, v, t, what='F = 3, T = %d' % T)
        assert (got['tri'][0] >= 0).all()                                     # triangle 0 is behind every pixel of the first camera
    _both(cuda, cams[1:2], h, w, v, t, what='F = 1, T = 257')


# ---- 3 ---------------------------------------------------------------------------------------------------------------------------
def test_every_cull_with_its_tally(cuda):
    h, w, znear = 16, 20, 0.5
    cam = R.camera(h, w, 64.0, pp=(0.0, 0.0))
    P = lambda pts, z: R.to_world(cam, np.array(pts, np.float64), np.array(z, np.float64))
    nan, inf = float('nan'), float('inf')
    blocks = [('drawn', P([(2, 2), (10, 2), (2, 10)], [4.0, 4.0, 4.0])),
              ('behind', P([(2, 2), (10, 2), (2, 10)], [-1.0, 0.25, 0.4999])),
              ('crossing', P([(2, 2), (10, 2), (2, 10)], [4.0, 4.0, 0.25])),
              ('drawn', P([(3, 3), (11, 3), (3, 11)], [znear, 1.0, 1.0])),      # a vertex at exactly znear is kept
              ('invalid', np.array([(0, 0, -4), (1, nan, -4), (0, 1, -4)], np.float32)),
              ('invalid', np.array([(0, 0, -4), (1, 0, -4), (inf, 1, -4)], np.float32)),
              ('degenerate', P([(5, 5), (5 + 1 / 1024, 5), (5, 5 + 1 / 1024)], [4.0, 4.0, 4.0])),   # one point after the snap
              ('degenerate', P([(1, 1), (5, 5), (9, 9)], [4.0, 2.0, 4.0])),                         # collinear in the picture
              ('range', P([(-40, 8), (10, 2), (3.0e6, 9)], [4.0, 4.0, 4.0])),   # 256 x 3e6 > 2^29: it would cross the frame
              ('drawn', P([(4, 4), (12, 4), (4, 12)], [2.0, 2.0, 2.0])),          # A2 > 0: a back face
              ('drawn', P([(4, 4), (4, 12), (12, 4)], [2.0, 2.0, 2.0]))]          # A2 < 0: a front face
    v = np.concatenate([b for _, b in blocks])
    V = v.shape[0]
    t = np.arange(V, dtype=np.int32).reshape(-1, 3)
    t = np.concatenate([t, np.array([[0, 1, V], [-1, 1, 2]], np.int32)])          # an id of V and of -1
    names = [n for n, _ in blocks] + ['invalid', 'invalid']
    removed_by = {0: 1, 3: 1, 9: 1, 10: 2}                # the drawn ones: right then down in the picture is a back face (A2 > 0)
    for cull in (0, 1, 2):
        want_names = ['culled' if removed_by.get(i) == cull else n for i, n in enumerate(names)]
        got, want = _both(cuda, cam, h, w, v, t, znear=znear, cull=cull, what='cull = %d' % cull)
        tally = dict(zip(R.COUNT_FIELDS, got['counts'].tolist()))
        for k in R.COUNT_FIELDS[1:]:
            assert tally[k] == want_names.count(k), (cull, k, tally)
        # 9 and 10 are one triangle wound both ways: the lower id wins while both are drawn; 3 has a vertex at exactly znear
        in_sight = {0: {0, 3, 9}, 1: {10}, 2: {0, 3, 9}}[cull]
        assert set(np.unique(got['tri']).tolist()) - {-1} == in_sight, cull
        assert got['tri'][0, 5, 5] == (10 if cull == 1 else 3)


# ---- 4, 5, 6 ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def random_scene():
    cams, v, t = R.random_scene(0)
    return cams, v, t, R.draw32(cams, 48, 64, v, t, 0.5)


def test_a_list_longer_than_one_lds_batch(cuda, random_scene):
    cams, v, t, want = random_scene
    assert (want['cover'][0, 16:32, 16:32] > 0).all()
    got = _device(cuda, cams, 48, 64, v, t, 0.5)
    _same(got, want)
    ws = ops.raster_setup(_d(cams, cuda), 48, 64, _d(v, cuda), _d(t, cuda, I32), 0.5)[1]
    F, tiles = 3, 3 * 4
    tile_count = ws[256 * ((40 * F * 2000 + 255) // 256):][:4 * F * tiles].view(I32).cpu().numpy()      # the layout the header states
    assert tile_count[1 * 4 + 1] >= 600 > ops.RASTER_BATCH and tile_count.sum() == got['counts'][0]
    again = _device(cuda, cams, 48, 64, v, t, 0.5)
    _same(again, got, 'a second run')


def test_overflow_draws_nothing_and_writes_nothing(cuda, random_scene):
    cams, v, t, want = random_scene
    cd, vd, td = _d(cams, cuda), _d(v, cuda), _d(t, cuda, I32)
    counts, ws = ops.raster_setup(cd, 48, 64, vd, td, 0.5)
    n, guard = int(counts.cpu()[0]), 1024
    assert n == want['counts'][0] and n > 2000
    pairs = torch.full((n + guard,), CANARY, dtype=I32, device=cuda)
    tri, depth, bary = ops.raster_draw(3, 2000, 48, 64, ws, n - 1, pairs=pairs)
    assert (tri == -2).all() and torch.isnan(depth).all() and torch.isnan(bary).all()
    assert (pairs == CANARY).all()
    tri, depth, bary = ops.raster_draw(3, 2000, 48, 64, ws, n, pairs=pairs)         # the same workspace, the exact size
    _same(dict(tri=tri.cpu().numpy(), depth=depth.cpu().numpy(), bary=bary.cpu().numpy(), counts=counts.cpu().numpy()), want)
    assert (pairs[n:] == CANARY).all()
    filled = pairs[:n].cpu().numpy()
    assert filled.min() >= 0 and filled.max() < 3 * 2000


def test_one_call_equals_three_and_chunks_do_not_matter(cuda, random_scene):
    cams, v, t, want = random_scene
    rng = np.random.default_rng(5)
    rgb, owner = rng.random((v.shape[0], 3)).astype(np.float32), rng.integers(-1, 5, v.shape[0]).astype(np.int32)
    cd, vd, td, ad, od = _d(cams, cuda), _d(v, cuda), _d(t, cuda, I32), _d(rgb, cuda), _d(owner, cuda, I32)
    counts, ws = ops.raster_setup(cd, 48, 64, vd, td, 0.5)
    n = int(counts.cpu()[0])
    tri, depth, bary = ops.raster_draw(3, 2000, 48, 64, ws, n)
    out_f = ops.raster_interp(td, tri, bary, v.shape[0], attr_f=ad)[0]
    out_i = ops.raster_interp(td, tri, None, v.shape[0], attr_i=od, fill=-7)[1]
    one = ops.raster_render_mesh(cd, 48, 64, vd, td, 0.5, n, attr_f=ad, attr_i=od, fill=-7)
    for k, x in (('counts', counts), ('tri', tri), ('depth', depth), ('bary', bary), ('out_f', out_f), ('out_i', out_i)):
        assert torch.equal(one[k].view(I32) if one[k].dtype == torch.float32 else one[k], x.view(I32) if x.dtype == torch.float32 else x), k
    short = ops.raster_render_mesh(cd, 48, 64, vd, td, 0.5, n - 1, attr_i=od, fill=-7)
    assert (short['tri'] == -2).all() and (short['out_i'] == -7).all() and int(short['counts'].cpu()[0]) == n
    m = dict(vertices=v, triangles=t, rgb=rgb, owner=owner)
    a, b = raster.render_mesh(m, cams, znear=0.5, frames_per_call=1), raster.render_mesh(m, cams, znear=0.5, frames_per_call=3)
    assert a['counts'].shape == (3, 8) and b['counts'].shape == (1, 8) and np.array_equal(a['counts'].sum(0), b['counts'][0])
    assert a['frames'] == [(0, 1), (1, 2), (2, 3)] and 'normals' not in a
    for k in ('tri', 'depth', 'bary', 'rgb', 'owner', 'mask'):
        assert torch.equal(a[k], b[k]), k
    assert torch.equal(b['tri'], tri) and torch.equal(b['rgb'].view(I32), out_f.view(I32))
    assert torch.equal(b['owner'], torch.where(tri >= 0, out_i, torch.full_like(out_i, -1)))


# ---- 7 ---------------------------------------------------------------------------------------------------------------------------
def test_interpolation(cuda, random_scene):
    """out = fl(fl(fl(q0 a0) + fl(q1 a1)) + fl(q2 a2)) with a_i = fl(a(P_i)) for a(P) = c0 + g . P.  Against a(P*) at the world
    point P* = sum q_i P_i in float64: three products and two additions, each at most u of a partial result no larger than
    A = max |a_i| (the q_i are positive and sum to 1 within 4 u): 5 u A; a_i itself is rounded: u A; and sum q_i a(P_i) =
    a(P*) + c0 (sum q_i - 1): 4 u |c0|.  Bound: 10 u max(A, |c0|).  P* is the point of the triangle the pixel sees: its
    projection sum w_i x_i differs from the pixel centre sum w_i X_i / 256 by the snap alone, at most 1/512 of a pixel per
    axis (plus the float32 error of x, below 1e-4 here).
    A constant attribute comes back within 4 u relative (q0 + q1 + q2 is 1 only to rounding)."""
    cams, v, t, want = random_scene
    c0, g = 0.75, np.array([0.5, -0.25, 0.125])
    affine = (c0 + v.astype(np.float64) @ g).astype(np.float32)
    const = np.array([1.0, 0.75, -3.0], np.float32)
    attr = np.concatenate([affine[:, None], np.broadcast_to(const, (v.shape[0], 3))], 1)
    first = np.arange(v.shape[0], dtype=np.int32) * 3 + 1
    tri, bary = _d(want['tri'], cuda, I32), _d(want['bary'], cuda)
    out_f, out_i = ops.raster_interp(_d(t, cuda, I32), tri, bary, v.shape[0], attr_f=_d(attr, cuda), attr_i=_d(first, cuda, I32), fill=-9)
    out_f, out_i = out_f.cpu().numpy(), out_i.cpu().numpy()
    cov = want['tri'] >= 0
    assert (out_f[~cov] == 0).all() and (out_i[~cov] == -9).all()
    assert np.array_equal(out_i[cov], first[t[want['tri'][cov], 0]])
    q = want['bary'][cov].astype(np.float64)
    Pi = v[t[want['tri'][cov]]].astype(np.float64)                             # [n,3,3]
    Pstar = (q[:, :, None] * Pi).sum(1)
    A = max(np.abs(affine).max(), abs(c0))
    err = np.abs(out_f[cov][:, 0] - (c0 + Pstar @ g))
    print('affine: max error %.3e, bound %.3e' % (err.max(), 10 * U * A))
    assert err.max() <= 10 * U * A
    f_idx, py, px = np.nonzero(cov)
    for f in range(3):
        c = cams[f].astype(np.float64)
        Rc, o = c[:12].reshape(3, 4)[:, :3], c[:12].reshape(3, 4)[:, 3]
        pc = (Pstar[f_idx == f] - o) @ Rc
        x, y = c[13] + c[12] * pc[:, 0] / -pc[:, 2], c[14] - c[12] * pc[:, 1] / -pc[:, 2]
        off = max(np.abs(x - px[f_idx == f]).max(), np.abs(y - py[f_idx == f]).max())
        print('frame %d: P* projects within %.5f px of the pixel centre' % (f, off))
        assert off <= 1.0 / 512.0 + 1e-4
    rel = np.abs(out_f[cov][:, 1:] - const) / np.abs(const)
    print('constant: max relative error %.3e, bound %.3e' % (rel.max(), 4 * U))
    assert rel.max() <= 4 * U
    # the same from the picture the device drew itself
    got = ops.raster_render_mesh(_d(cams, cuda), 48, 64, _d(v, cuda), _d(t, cuda, I32), 0.5, int(want['counts'][0]), attr_f=_d(attr, cuda))
    assert np.array_equal(got['out_f'].cpu().numpy().view(np.int32), out_f.view(np.int32))


# ---- 8 ---------------------------------------------------------------------------------------------------------------------------
def test_a_real_surface(cuda):
    """A sphere of radius 1 as the iso-surface of density = 1 - r on a 24^3 lattice of step 3 / 23, from outside.
    Watertight: a pixel whose ray passes the centre closer than R - 2 steps is covered, and so are its four neighbours.
    Depth: within one lattice step of the ray-sphere depth there (the surface lies within step^2 / (8 R) of the sphere
    radially; the ray meets it at more than 41 degrees off grazing).
    Cloud: against n samples of sample_mesh, the sampler's spacing is its GAP G, the largest distance from any point of the
    mesh to its nearest sample -- what a point that lies on the mesh cannot exceed.  (The nominal s = sqrt(area / n) is not a
    bound: the sampler's own gap is larger, which the test shows from the mesh and the samples alone, before the picture is
    looked at.)  G is certified from above without the rasteriser: every triangle is covered by the (M + 1)(M + 2) / 2 points
    of its barycentric grid of order M; a point x of the triangle lies in a sub-triangle similar to it at scale 1 / M, so
    within h_t = (longest edge of t) / M of a grid point y, and d(x, samples) <= d(y, samples) + h_t.  Hence
    G <= G_up = max over grid points of d(y, samples) + h_t, and max d(y, samples) <= G: G is known to within max h_t.
    A depth point is o + depth d_pixel.  The pixel's weights q are >= 0 and sum to 1 within 4 u, so P* = sum q_i P_i lies on
    the owning triangle, has exactly this camera depth, and projects within 1/512 px per axis of the pixel centre
    (test_interpolation): |point - P*| <= depth sqrt(2) / (512 focal) = delta.  So every depth point lies within
    G_up + delta + 1e-5 of a sample (1e-5: the float32 roundings of points of magnitude 5)."""
    cells, Rad = 24, 1.0
    step = 3.0 / (cells - 1)
    ax = torch.arange(cells, device=cuda, dtype=torch.float32) * step - 1.5
    r = torch.sqrt(ax[:, None, None] ** 2 + ax[None, :, None] ** 2 + ax[None, None, :] ** 2)
    frame = dict(origin=[-1.5, -1.5, -1.5], du=[step, 0.0, 0.0], dv=[0.0, step, 0.0], dw=[0.0, 0.0, step])
    m = mesh.surface(dict(density=(Rad - r).contiguous(), valid=None, frame=frame), 0.0)
    h, w, focal = 72, 88, 128.0
    eye = np.array([1.5, 1.0, 3.5])
    cam = R.camera(h, w, focal, R.look_at(eye, (0.0, 0.0, 0.0)))
    out = raster.render_mesh(m, cam, znear=0.1, attrs=('normals',), label=None, cull=1)
    depth, mask = out['depth'][0].cpu().numpy().astype(np.float64), out['mask'][0].cpu().numpy()
    c = cam.astype(np.float64)
    Rc = c[:12].reshape(3, 4)[:, :3]
    py, px = np.mgrid[0:h, 0:w]
    d = np.stack([(px - c[13]) / c[12], -(py - c[14]) / c[12], -np.ones((h, w))], -1) @ Rc.T          # world directions, z_cam = -1
    dd, od = (d * d).sum(-1), d @ eye
    tc = -od / dd
    b = np.sqrt(np.maximum(((eye + tc[..., None] * d) ** 2).sum(-1), 0.0))                            # closest approach to the centre
    inner = b < Rad - 2 * step
    assert inner.sum() > 1500 and mask[inner].all() and not mask[b > Rad + step].any()
    for dy, dx in ((0, 1), (0, -1), (1, 0), (-1, 0)):
        assert np.roll(mask, (dy, dx), (0, 1))[inner].all()
    analytic = tc - np.sqrt(np.maximum(Rad * Rad - b * b, 0.0) / dd)
    err = np.abs(depth - analytic)[inner]
    print('depth against the sphere: max %.4f, one step %.4f' % (err.max(), step))
    assert err.max() <= step
    # culling back faces changes nothing seen from outside a closed surface; the normals point at the camera
    both = raster.render_mesh(m, cam, znear=0.1, attrs=(), label=None, cull=0)
    assert torch.equal(both['depth'], out['depth']) and out['counts'][0, 7] > 0 and both['counts'][0, 7] == 0
    n_cam = out['normals'][0].cpu().numpy().astype(np.float64)[inner] @ Rc
    assert (n_cam[:, 2] > 0).all()
    points = geometry.depth_points(cam, out['depth'][0], 0.1, 10.0)
    assert points.shape[0] == mask.sum()
    v, t = m['vertices'].cpu().numpy().astype(np.float64), m['triangles'].cpu().numpy()
    area = 0.5 * np.linalg.norm(np.cross(v[t[:, 1]] - v[t[:, 0]], v[t[:, 2]] - v[t[:, 0]]), axis=1).sum()
    n, M = 40000, 48
    s = float(np.sqrt(area / n))
    samples, _ = geometry.sample_mesh(m, n)
    i, j = np.meshgrid(np.arange(M + 1), np.arange(M + 1), indexing='ij')
    keep = (i + j) <= M
    bw = np.stack([M - i[keep] - j[keep], i[keep], j[keep]], 1) / float(M)                              # [g,3] barycentric grid
    corners = m['vertices'].to(torch.float64)[m['triangles'].long()]                                   # [T,3,3]
    grid_pts = torch.einsum('gc,tcx->tgx', _d(bw, cuda, torch.float64), corners).to(torch.float32).reshape(-1, 3).contiguous()
    edges = torch.stack([(corners[:, a] - corners[:, b]).norm(dim=1) for a, b in ((0, 1), (1, 2), (2, 0))], 1)
    h_t = (edges.max(1).values / M).to(torch.float32)
    cap = 8 * s
    prepared_grid = geometry.make_grid(samples, cap)
    prepared = geometry.sort_reference(samples, prepared_grid)
    gd, gi = geometry.nearest(grid_pts, samples, cap, grid=prepared_grid, prepared=prepared)
    assert (gi >= 0).all()
    gap_low = float(gd.max())
    gap_up = float((gd.reshape(t.shape[0], -1) + h_t[:, None]).max())
    delta = float(out['depth'].max()) * np.sqrt(2.0) / (512.0 * focal)
    dist, index = geometry.nearest(points, samples, cap, grid=prepared_grid, prepared=prepared)
    print('sampler: s = sqrt(area / n) = %.4f; its gap lies in [%.4f, %.4f] (%d grid points, max h_t %.4f); delta %.1e'
          % (s, gap_low, gap_up, grid_pts.shape[0], float(h_t.max()), delta))
    print('depth points against %d samples: max %.4f' % (n, float(dist.max())))
    assert (index >= 0).all() and float(dist.max()) <= gap_up + delta + 1e-5


# ---- 9 ---------------------------------------------------------------------------------------------------------------------------
def test_every_refusal_by_its_message(cuda):
    L, s = _lib.raster_lib(), torch.cuda.current_stream().cuda_stream
    F, T, V, h, w = 2, 4, 12, 16, 16
    cams = _d(np.stack([R.camera(h, w, 16.0)] * F), cuda)
    v, t = torch.zeros(V, 3, device=cuda), torch.zeros(T, 3, dtype=I32, device=cuda)
    need = ops.raster_workspace_bytes(F, T, h, w)
    ws = torch.zeros(need + 256, dtype=torch.uint8, device=cuda)
    counts = torch.full((8,), CANARY, dtype=I32, device=cuda)
    pairs, tri, depth = torch.zeros(64, dtype=I32, device=cuda), torch.zeros(F, h, w, dtype=I32, device=cuda), torch.zeros(F, h, w, device=cuda)
    bary, attr, out_f = torch.zeros(F, h, w, 3, device=cuda), torch.zeros(V, 2, device=cuda), torch.zeros(F, h, w, 2, device=cuda)
    p = lambda x: x.data_ptr()

    def setup(**kw):
        a = dict(F=F, h=h, w=w, cams=p(cams), V=V, T=T, v=p(v), t=p(t), znear=0.5, cull=0, ws=p(ws), wsb=need, counts=p(counts))
        a.update(kw)
        return L.durf_raster_setup(s, a['F'], a['h'], a['w'], a['cams'], a['V'], a['T'], a['v'], a['t'], a['znear'], a['cull'], a['ws'], a['wsb'],
                                   a['counts'])

    def draw(**kw):
        a = dict(F=F, T=T, h=h, w=w, ws=p(ws), wsb=need, pairs=p(pairs), mp=64, tri=p(tri), depth=p(depth), bary=None)
        a.update(kw)
        return L.durf_raster_draw(s, a['F'], a['T'], a['h'], a['w'], a['ws'], a['wsb'], a['pairs'], a['mp'], a['tri'], a['depth'], a['bary'])

    def interp(**kw):
        a = dict(n=F * h * w, V=V, T=T, t=p(t), tri=p(tri), bary=p(bary), C=2, af=p(attr), of=p(out_f), ai=None, oi=None)
        a.update(kw)
        return L.durf_raster_interp(s, a['n'], a['V'], a['T'], a['t'], a['tri'], a['bary'], a['C'], a['af'], a['of'], a['ai'], 0, a['oi'])

    def whole(**kw):
        a = dict(F=F, znear=0.5, cull=0, wsb=need, mp=64, C=2, bary=p(bary))
        a.update(kw)
        return L.durf_render_mesh(s, a['F'], h, w, p(cams), V, T, p(v), p(t), a['znear'], a['cull'], p(ws), a['wsb'], p(pairs), a['mp'], p(counts),
                                  p(tri), p(depth), a['bary'], a['C'], p(attr), p(out_f), None, 0, None)

    small = 'workspace of %d bytes, durf_raster_workspace_bytes(%d, %d, %d, %d) = %d' % (need - 256, F, T, h, w, need)
    cases = [(setup, dict(F=-1), 'F >= 0 and T >= 0, F = -1, T = 4'), (setup, dict(T=-2), 'F = 2, T = -2'),
             (setup, dict(h=0), '1 <= h, w <= 4096, h = 0, w = 16'), (setup, dict(w=4097), 'h = 16, w = 4097'),
             (setup, dict(F=1 << 16, T=1 << 15), 'F T < 2^31 pairs, F = 65536, T = 32768'),
             (setup, dict(F=1 << 20, T=1, h=64, w=64), 'F h w < 2^31 pixels, F = 1048576, h = 64, w = 64'),
             (setup, dict(V=-1), 'V >= 0, V = -1'), (setup, dict(znear=0.0), 'znear > 0 (a normal float), znear = 0'),
             (setup, dict(znear=float('nan')), 'znear = nan'), (setup, dict(znear=-1.0), 'znear = -1'),
             (setup, dict(cull=3), 'cull in 0 .. 2, cull = 3'), (setup, dict(cull=-1), 'cull = -1'),
             (setup, dict(cams=None), 'cams_dev for F = 2'), (setup, dict(v=None), 'vertices for V = 12'),
             (setup, dict(t=None), 'triangles for T = 4'), (setup, dict(counts=None), 'requirement failed: counts'),
             (setup, dict(ws=None), 'workspace aligned to 256 bytes'), (setup, dict(ws=p(ws) + 4), 'workspace aligned to 256 bytes'),
             (setup, dict(wsb=need - 256), small),
             (draw, dict(w=0), 'h = 16, w = 0'), (draw, dict(mp=-1), '0 <= max_pairs < 2^31, max_pairs = -1'),
             (draw, dict(pairs=None), 'pairs for max_pairs = 64'), (draw, dict(tri=None), 'tri and depth for F = 2'),
             (draw, dict(depth=None), 'tri and depth for F = 2'), (draw, dict(ws=p(ws) + 128), 'workspace aligned to 256 bytes'),
             (draw, dict(wsb=need - 256), small),
             (interp, dict(n=-1), 'n_pixels = -1'), (interp, dict(af=None), 'attr_f or attr_i'), (interp, dict(of=None), 'out_f and bary with attr_f'),
             (interp, dict(bary=None), 'out_f and bary with attr_f'), (interp, dict(C=0), 'C >= 1, C = 0'),
             (interp, dict(ai=p(t)), 'out_i with attr_i'), (interp, dict(tri=None), 'tri for n_pixels = 512'),
             (interp, dict(t=None), 'triangles for T = 4'),
             (whole, dict(F=-1), 'F = -1'), (whole, dict(znear=0.0), 'znear = 0'), (whole, dict(cull=5), 'cull = 5'), (whole, dict(mp=-3), 'max_pairs = -3'),
             (whole, dict(C=0), 'C >= 1, C = 0'), (whole, dict(bary=None), 'out_f and bary with attr_f'), (whole, dict(wsb=need - 256), small)]
    for fn, kw, msg in cases:
        assert fn(**kw) != 0, (fn.__name__, kw)
        text = _lib.lib().durf_last_error().decode()
        assert msg in text and 'durf_r' in text, (fn.__name__, kw, text)
    torch.cuda.synchronize()
    assert (counts == CANARY).all() and not tri.any() and not depth.any()        # a refused call launches nothing
    assert ops.raster_workspace_bytes(1 << 16, 1 << 15, 16, 16) == 0 and ops.raster_workspace_bytes(1, 1, 0, 16) == 0 and need % 256 == 0
    # F T == 0 succeeds: counts 0, tri -1
    c0, ws0 = ops.raster_setup(cams, h, w, v, torch.zeros(0, 3, dtype=I32, device=cuda), 0.5)
    tri0, depth0, _ = ops.raster_draw(F, 0, h, w, ws0, 0)
    assert not c0.any() and (tri0 == -1).all() and not depth0.any()
    assert setup(F=0, cams=None) == 0 and draw(F=0, tri=None, depth=None) == 0


# ---- the command -----------------------------------------------------------------------------------------------------------------
def _ppm(path):
    blob = open(path, 'rb').read()
    magic, size, maxval, data = blob.split(b'\n', 3)
    w, h = (int(x) for x in size.split())
    assert magic == b'P6' and maxval == b'255' and len(data) == 3 * h * w, path
    return np.frombuffer(data, np.uint8).reshape(h, w, 3)


def _check_output(out, r, F, T, ids):
    meta = json.load(open(os.path.join(out, 'raster.json')))
    assert sorted(os.listdir(out)) == sorted(['raster.json'] + [n % f for f in range(F) for n in ('depth_%04d.npy', 'depth_%04d.ppm', 'ids_%04d.ppm')])
    assert meta['triangles'] == T and len(meta['frames']) == F and meta['ids'] == ids
    h, w = r['depth'].shape[1:]
    for f, rec in enumerate(meta['frames']):
        d = np.load(os.path.join(out, 'depth_%04d.npy' % f))
        assert d.dtype == np.float32 and np.array_equal(d.view(np.int32), r['depth'][f].cpu().numpy().view(np.int32)), f
        mask = r['mask'][f].cpu().numpy()
        pic = _ppm(os.path.join(out, 'depth_%04d.ppm' % f))
        assert pic.shape == (h, w, 3) and not pic[~mask].any() and pic[mask].any(1).all()         # black exactly where nothing covers
        want_ids = raster.id_colours(r['tri'][f] if ids == 'tri' else r[ids][f]).cpu().numpy()
        assert np.array_equal(_ppm(os.path.join(out, 'ids_%04d.ppm' % f)), want_ids)
        assert sum(rec[k] for k in R.COUNT_FIELDS[1:]) == T and rec['covered'] == mask.sum() > 0, rec
    assert sum(rec['pairs'] for rec in meta['frames']) == int(r['counts'][:, 0].sum())
    return meta


def test_render_mesh_command_end_to_end(cuda, tmp_path):
    out = str(tmp_path / 'synthetic')
    cmd = [sys.executable, '-m', 'durf_amd.render_mesh', '--synthetic', '--frames', '2', '--eval_dir', out]
    p = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)       # a fresh child process
    assert p.returncode == 0, p.stdout.decode()
    print(p.stdout.decode()[-300:])
    m, c2w, focal, h, w = render_mesh.synthetic_scene(2)
    T = int(m['triangles'].shape[0])
    cams = trajectory.camera_rows(c2w, focal, ((w - 1) / 2.0, (h - 1) / 2.0), h, w)
    r = raster.render_mesh(m, cams, attrs=(), label=None)
    _check_output(out, r, 2, T, 'tri')
    # the same mesh from files: once in the world, once as a box in its own frame at its pose of timestep 1
    a, b, poses, traj = (str(tmp_path / n) for n in ('background.ply', 'object_00.ply', 'poses.npy', 'traj.npz'))
    mesh.write_ply(a, m), mesh.write_ply(b, m)
    table = np.zeros((2, 1, 6))
    table[1, 0] = (1.6, 0.2, 0.0, 0.0, 0.3, 0.0)
    np.save(poses, table)
    trajectory.save_trajectory(traj, c2w, [0.0, 1.0])
    out2 = str(tmp_path / 'files')
    assert render_mesh.main(['--ply', a, '--ply', b, '--poses', poses, '--ts', '1', '--traj', traj, '--focal', str(focal), '--size', str(h), str(w),
                             '--cull', 'back', '--eval_dir', out2]) == 0
    merged = raster.merge([mesh.read_ply(a), mesh.read_ply(b)], [None, table[1, 0]])
    r2 = raster.render_mesh(merged, cams, attrs=(), label='part', cull=1)
    meta = _check_output(out2, r2, 2, 2 * T, 'part')
    assert meta['cull'] == 'back' and all(rec['culled'] > 0 for rec in meta['frames'])
    assert set(np.unique(r2['part'].cpu().numpy()).tolist()) == {-1, 0, 1}
