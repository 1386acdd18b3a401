"""libdurf_shade.so on the device against tests/shade_ref.py: surface32, occlusion32 and compose32 (the header's definitions) in
every bit of every output, on the smallest shapes at which they can go wrong and whatever permutation the tree is built over;
durf_shade_cameras against the six separate calls it is defined as; every refusal with its text; and the rasteriser's primaries
shaded by the cast's secondaries."""
import ctypes as C

import numpy as np
import pytest
import torch

from durf_amd import _lib, camera, cast, ops, raster, shade
from tests import camera_ref, cast_ref as R, shade_ref as S

pytestmark = pytest.mark.gpu
I32 = torch.int32
F32 = np.float32


def _d(a, cuda, dtype=torch.float32):
    return torch.as_tensor(np.array(a)).to(device=cuda, dtype=dtype).contiguous()


def _same(got, want, what):
    got = got.cpu().numpy() if torch.is_tensor(got) else got
    a, b = (x if x.dtype == np.uint8 else R.bits(x) for x in (np.ascontiguousarray(got), np.ascontiguousarray(want)))
    assert a.shape == b.shape and np.array_equal(a, b), (what, np.argwhere(a != b)[:5])


def _build(v, t, order=None):
    return cast.build(dict(vertices=v, triangles=t), order=order)


# ---- surface ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['soup_T300_n0', 'soup_T300_n1', 'soup_T300_n255', 'soup_T300_n256', 'soup_T300_n257', 'grid_cull0', 'dirty',
                                  'bad_rays', 'random_T5000_n3000'])
def test_surface_equals_the_definition_on_the_casts_hits(cuda, name):
    s, (tri, _, bary) = R.scenes()[name], R.expected(name)
    b = _build(s['v'], s['t'])
    for toward in (s['d'], None):
        p, nr = ops.shade_surface(b['vertices'], b['triangles'], _d(tri, cuda, I32), _d(bary, cuda), None if toward is None else _d(toward, cuda))
        wp, wn = S.surface32(s['v'], s['t'], tri, bary, toward)
        _same(p, wp, (name, 'point', toward is None)), _same(nr, wn, (name, 'normal', toward is None))
    if len(tri):
        assert (tri >= 0).any() or name == 'soup_T300_n1'


def test_surface_on_flat_and_sliver_triangles_and_on_no_triangle(cuda):
    v, t = S.flat_and_sliver()
    tri = np.asarray([0, 1, 2, 3, 4, 5, 6, -1, -2, 7, 2 ** 31 - 1] * 30, np.int32)
    rng = np.random.default_rng(1)
    bary = rng.dirichlet((1, 1, 1), len(tri)).astype(F32)
    bary[8::11] = np.nan
    toward = rng.normal(size=(len(tri), 3)).astype(F32)
    b = _build(v, t)
    for tw in (toward, None):
        p, nr = ops.shade_surface(b['vertices'], b['triangles'], _d(tri, cuda, I32), _d(bary, cuda), None if tw is None else _d(tw, cuda))
        wp, wn = S.surface32(v, t, tri, bary, tw)
        _same(p, wp, 'point'), _same(nr, wn, 'normal')
    assert not wn[1::11].any() and wn[3::11].any()


# ---- occlusion ----------------------------------------------------------------------------------------------------------------------
def _occlusion(cuda, c, order=None):
    b = _build(c['v'], c['t'], order)
    n = c['points'].shape[0]
    used, blocked = ops.shade_occlusion(b['ws'], b['T'], _d(c['points'], cuda).reshape(n, 3), _d(c['normals'], cuda).reshape(n, 3),
                                        _d(c['dirs'], cuda), c['bias'], c['reach'], c['cull'])
    return used.cpu().numpy(), blocked.cpu().numpy()


@pytest.mark.parametrize('name', sorted(S.cases()))
def test_occlusion_equals_the_definition_in_both_integers_whatever_the_tree(cuda, name):
    c, (used, blocked) = S.cases()[name], S.expected(name)
    u, b = _occlusion(cuda, c)
    assert np.array_equal(u, used) and np.array_equal(b, blocked), (name, np.argwhere((u != used) | (b != blocked))[:5])
    T = c['t'].shape[0]
    u2, b2 = _occlusion(cuda, c, order=np.random.default_rng(7).permutation(T).astype(np.int32))
    assert np.array_equal(u2, used) and np.array_equal(b2, blocked), (name, 'random order')


def test_what_the_header_says_of_odd_directions(cuda):
    c, (used, blocked) = S.cases()['odd_directions'], S.expected('odd_directions')
    # of the 14 directions: six have c > 0 against the normal (0, 0, 1) -- (0, 0, inf) among them, used and unusable, so never
    # blocked; the tangent ones, the zero one and every one with a NaN in c (0 * inf too) are not used
    assert (used == 6).all() and (blocked <= 5).all() and blocked.max() == 5
    one = dict(c, dirs=np.asarray([[0.0, 0.0, np.inf]], F32))
    u, b = _occlusion(cuda, one)
    assert (u == 1).all() and (b == 0).all()
    for d in ((0, 0, 0), (np.nan, 0, 1), (1, 0, 0), (0, 0, -1)):
        u, b = _occlusion(cuda, dict(c, dirs=np.asarray([d], F32)))
        assert not u.any() and not b.any(), d


def test_occlusion_of_1500_samples_64_directions_5000_triangles(cuda):
    c, (used, blocked) = S.big_case()
    u, b = _occlusion(cuda, c)
    assert np.array_equal(u, used) and np.array_equal(b, blocked)


# ---- compose ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('ambient', [0.0, 0.4, 1.0])
@pytest.mark.parametrize('given', ['none', 'albedo', 'sun', 'both'])
def test_compose_equals_the_definition_in_float_and_8_bit(cuda, ambient, given):
    rng = np.random.default_rng(3)
    n = 1027
    nr = S.random_samples(n, 4)[1]
    nr[::50] = 0
    used = rng.integers(0, 65, n).astype(np.int32)
    used[::7] = 0
    blocked = (used * rng.random(n)).astype(np.int32)
    tri = rng.integers(-2, 50, n).astype(np.int32)
    albedo = rng.uniform(-0.2, 1.4, (n, 3)).astype(F32) if given in ('albedo', 'both') else None
    if albedo is not None:
        albedo[::97, 1] = np.nan
    sun = rng.integers(0, 2, n).astype(np.int32) if given in ('sun', 'both') else None
    light, bg = (0.0, 0.6, 0.8), (1.0, 0.5, 0.25)
    want_f, want_8 = S.compose32(tri, nr, used, blocked, light, ambient, bg, sun, albedo)
    dev = lambda a, dt=torch.float32: None if a is None else _d(a, cuda, dt)
    out_f, out_8 = ops.shade_compose(dev(tri, I32), dev(nr), dev(used, I32), dev(blocked, I32), light, ambient, bg, dev(sun, I32), dev(albedo))
    _same(out_f, want_f, 'float'), _same(out_8, want_8, '8-bit')
    only8 = ops.shade_compose(dev(tri, I32), dev(nr), dev(used, I32), dev(blocked, I32), light, ambient, bg, dev(sun, I32), dev(albedo), want_f=False)
    assert only8[0] is None
    _same(only8[1], want_8, '8-bit alone')


# ---- cameras ------------------------------------------------------------------------------------------------------------------------
def _scene_with_colours():
    v, t = S.sphere_on_ground()
    rgb = ((v - v.min(0)) / (v.max(0) - v.min(0))).astype(F32)
    return v, t, rgb


def _sequence(cuda, b, cams, h, w, dirs, bias, reach, light, sun, ambient, rgb, bg, cull):
    """the six steps of durf_shade.h, each its own call"""
    F = cams.shape[0]
    tri, depth, bary = ops.cast_cameras(b['ws'], b['T'], _d(cams, cuda), h, w, 0.0, float('inf'), cull)
    toward = np.stack([R.pinhole32(cams[f], h, w)[1] for f in range(F)]).reshape(F, h, w, 3)
    point, normal = ops.shade_surface(b['vertices'], b['triangles'], tri, bary, _d(toward, cuda))
    used, blocked = ops.shade_occlusion(b['ws'], b['T'], point, normal, dirs, bias, reach, cull)
    sun_blocked = ops.shade_occlusion(b['ws'], b['T'], point, normal, _d(np.asarray([light], F32), cuda), bias, float('inf'), cull)[1] if sun else None
    albedo = ops.raster_interp(b['triangles'], tri, bary, b['V'], attr_f=rgb)[0] if rgb is not None else None
    out_f, out_8 = ops.shade_compose(tri, normal, used, blocked, light, ambient, bg, sun_blocked, albedo)
    return dict(tri=tri, depth=depth, normal=normal, ao_used=used, ao_blocked=blocked, out_f=out_f, out_u8=out_8)


@pytest.mark.parametrize('size', [(1, 1), (7, 9), (8, 8), (17, 33)])
@pytest.mark.parametrize('sun', [0, 1])
def test_cameras_equal_the_six_separate_calls(cuda, size, sun):
    h, w = size
    v, t, rgb = _scene_with_colours()
    b = _build(v, t)
    cams = camera.rows([camera_ref.look_at((7.5, 1.0, 3.5), (3.0, 3.0, 0.6), up=(0.0, 0.0, 1.0)), camera_ref.look_at((3.2, 2.9, 6.0), (3.0, 3.0, 0.0))],
                       0.9 * max(w, 4), (w / 2.0 - 0.25, h / 2.0), h, w)
    dirs, light, bg = _d(S.fibonacci(24), cuda), [0.3, -0.2, 0.933], (0.25, 0.5, 1.0)
    rgb_d = _d(rgb, cuda)
    for albedo in (rgb_d, None):
        got = ops.shade_cameras(b['ws'], b['vertices'], b['triangles'], _d(cams, cuda), h, w, dirs, 0.6 / 1024, 0.6, light, sun, 0.45, bg, albedo_vertex=albedo)
        want = _sequence(cuda, b, cams, h, w, dirs, 0.6 / 1024, 0.6, light, sun, 0.45, rgb_d if albedo is not None else None, bg, 0)
        for k in want:
            _same(got[k], want[k].cpu().numpy(), (size, sun, k))
    if h * w > 60:
        assert int((got['tri'] >= 0).sum()) > h * w // 2 and int(got['ao_blocked'].sum()) > 0
    # the oracle itself on frame 0: the device sequence is the definition
    o, d = R.pinhole32(cams[0], h, w)
    tri, _, bary = R.cast32(v, t, o, d)
    p, nr = S.surface32(v, t, tri, bary, d)
    _same(got['normal'][0].reshape(-1, 3), nr, 'normal against the oracle')
    used, blocked = S.occlusion32(v, t, p, nr, S.fibonacci(24), 0.6 / 1024, 0.6)
    assert np.array_equal(got['ao_used'][0].reshape(-1).cpu().numpy(), used) and np.array_equal(got['ao_blocked'][0].reshape(-1).cpu().numpy(), blocked)


def test_a_camera_row_of_another_size_shows_the_background(cuda):
    h, w = 7, 9
    v, t, _ = _scene_with_colours()
    b = _build(v, t)
    cams = camera.rows([camera_ref.look_at((3.2, 2.9, 6.0), (3.0, 3.0, 0.0))] * 2, 8.0, (4.5, 3.5), h, w)
    cams[1, camera.CAM_W] = w + 1
    r = ops.shade_cameras(b['ws'], b['vertices'], b['triangles'], _d(cams, cuda), h, w, _d(S.fibonacci(8), cuda), 1e-3, 1.0, [0, 0, 1], 1, 0.5, (0.25, 0.5, 1.0))
    assert (r['tri'][1] == -2).all() and torch.isnan(r['depth'][1]).all() and not r['normal'][1].any() and not r['ao_used'][1].any()
    assert (r['out_u8'][1].reshape(-1, 3) == torch.tensor([64, 128, 255], dtype=torch.uint8, device=cuda)).all()
    assert (r['tri'][0] >= -1).all() and int((r['tri'][0] >= 0).sum()) > h * w // 2      # the other frame is as it would be alone
    hi = shade.cameras(b, cams[:1], dirs=8, reach=1.0)                       # the Python entry: the same call
    assert tuple(hi['ao'].shape) == (1, h, w) and float(hi['ao'].min()) >= 0.0 and hi['shaded8'].dtype == torch.uint8


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def test_every_refusal_with_its_text_and_nothing_written(cuda):
    L, base = _lib.shade_lib(), _lib.lib()
    v, t, _ = _scene_with_colours()
    b = _build(v, t)
    V, T, ws = b['V'], b['T'], b['ws']
    n = 16
    f3 = torch.full((n, 3), 7.0, device=cuda)
    i1 = torch.full((n,), 7, dtype=I32, device=cuda)
    u8 = torch.full((n, 3), 7, dtype=torch.uint8, device=cuda)
    tri = torch.zeros(n, dtype=I32, device=cuda)
    dirs = _d(S.fibonacci(4), cuda)
    three = lambda *x: (C.c_float * 3)(*x)
    light, bg, inf, nan = three(0, 0, 1), three(1, 1, 1), float('inf'), float('nan')
    P = lambda x: None if x is None else x.data_ptr()

    def refused(rc, text):
        assert rc != 0 and text in base.durf_last_error().decode(), (text, base.durf_last_error().decode())
        torch.cuda.synchronize()
        assert (f3 == 7).all() and (i1 == 7).all() and (u8 == 7).all(), text

    def surface(n_=n, V_=V, T_=T, vert=b['vertices'], tris=b['triangles'], tri_=tri, bary=f3, point=f3, normal=f3):
        return L.durf_shade_surface(None, n_, V_, T_, P(vert), P(tris), P(tri_), P(bary), None, P(point), P(normal))
    refused(surface(n_=-1), 'durf_shade_surface: requirement failed: n >= 0, n = -1')
    refused(surface(V_=-1), 'durf_shade_surface: requirement failed: V >= 0')
    refused(surface(T_=-1), 'durf_shade_surface: requirement failed: 0 <= T <')
    refused(surface(T_=1 << 30), 'durf_shade_surface: requirement failed: 0 <= T <')
    refused(surface(vert=None), 'durf_shade_surface: requirement failed: vertices for V')
    refused(surface(tris=None), 'durf_shade_surface: requirement failed: triangles for T')
    refused(surface(tri_=None), 'durf_shade_surface: requirement failed: tri and bary for n = 16')
    refused(surface(normal=None), 'durf_shade_surface: requirement failed: point and normal for n = 16')
    assert surface(n_=0, tri_=None, bary=None, point=None, normal=None) == 0

    def occlusion(n_=n, points=f3, normals=f3, S_=4, dirs_=dirs, bias=0.0, reach=1.0, cull=0, T_=T, ws_=ws.data_ptr(), bytes_=ws.numel(), used=i1, blocked=i1):
        return L.durf_shade_occlusion(None, n_, P(points), P(normals), S_, P(dirs_), bias, reach, cull, T_, ws_, bytes_, P(used), P(blocked))
    who = 'durf_shade_occlusion: requirement failed: '
    refused(occlusion(n_=-1), who + 'n >= 0, n = -1')
    refused(occlusion(S_=0), who + 'S in 1 .. 256, S = 0')
    refused(occlusion(S_=257), who + 'S in 1 .. 256, S = 257')
    refused(occlusion(dirs_=None), who + 'dirs for S = 4')
    refused(occlusion(bias=-1.0), who + 'bias >= 0, bias = -1')
    refused(occlusion(bias=nan), who + 'bias >= 0, bias = nan')
    refused(occlusion(reach=0.0), who + 'reach is +inf or > 0, reach = 0')
    refused(occlusion(reach=-inf), who + 'reach is +inf or > 0, reach = -inf')
    refused(occlusion(reach=nan), who + 'reach is +inf or > 0, reach = nan')
    refused(occlusion(cull=3), who + 'cull in 0 .. 2, cull = 3')
    refused(occlusion(T_=-1), who + '0 <= T <')
    refused(occlusion(points=None), who + 'points and normals for n = 16')
    refused(occlusion(blocked=None), who + 'used and blocked for n = 16')
    refused(occlusion(ws_=None), who + 'workspace aligned to 256 bytes')
    refused(occlusion(ws_=ws.data_ptr() + 4), who + 'workspace aligned to 256 bytes')
    refused(occlusion(bytes_=ws.numel() - 1), 'durf_shade_occlusion: workspace of %d bytes, durf_cast_workspace_bytes(%d) = %d' % (ws.numel() - 1, T, ws.numel()))
    refused(occlusion(T_=T + 4000), 'durf_cast_workspace_bytes(%d)' % (T + 4000))
    assert occlusion(n_=0, points=None, normals=None, used=None, blocked=None) == 0
    assert occlusion(reach=inf, used=torch.empty_like(i1), blocked=torch.empty_like(i1)) == 0

    def compose(n_=n, tri_=tri, normals=f3, used=i1, blocked=i1, light_=light, ambient=0.5, bg_=bg, out_f=f3, out_8=u8):
        return L.durf_shade_compose(None, n_, P(tri_), P(normals), P(used), P(blocked), None, None, light_, ambient, bg_, P(out_f), P(out_8))
    who = 'durf_shade_compose: requirement failed: '
    refused(compose(n_=-1), who + 'n >= 0, n = -1')
    refused(compose(ambient=-0.1), who + 'ambient in [0, 1], ambient = -0.1')
    refused(compose(ambient=1.5), who + 'ambient in [0, 1], ambient = 1.5')
    refused(compose(ambient=nan), who + 'ambient in [0, 1], ambient = nan')
    refused(compose(light_=None), who + 'light and background (host floats)')
    refused(compose(bg_=None), who + 'light and background (host floats)')
    refused(compose(light_=three(0, inf, 0)), who + 'light and background are finite')
    refused(compose(bg_=three(nan, 0, 0)), who + 'light and background are finite')
    refused(compose(used=None), who + 'tri, normals, used and blocked for n = 16')
    refused(compose(out_f=None, out_8=None), who + 'out_f or out_u8 for n = 16')
    assert compose(n_=0, tri_=None, normals=None, used=None, blocked=None, out_f=None, out_8=None) == 0

    F, h, w = 1, 4, 4
    cams = _d(camera.rows([camera_ref.look_at((3.2, 2.9, 6.0), (3.0, 3.0, 0.0))], 4.0, (2.0, 2.0), h, w), cuda)
    sw = torch.empty(ops.shade_workspace_bytes(F, h, w), dtype=torch.uint8, device=cuda)
    assert ops.shade_workspace_bytes(-1, 4, 4) == 0 and ops.shade_workspace_bytes(1, 0, 4) == 0 and ops.shade_workspace_bytes(1 << 15, 1 << 8, 1 << 8) == 0
    assert ops.shade_workspace_bytes(0, 4, 4) == 256 and sw.numel() % 256 == 0

    def cameras(F_=F, h_=h, w_=w, cams_=cams, tmin=0.0, tmax=inf, cull=0, V_=V, T_=T, S_=4, bias=0.0, reach=1.0, light_=light, sun=1, ambient=0.5, bg_=bg,
                sw_=sw.data_ptr(), sw_bytes=sw.numel(), tri_=i1, depth=f3, used=i1, out_f=f3, out_8=u8, cast_bytes=ws.numel()):
        return L.durf_shade_cameras(None, F_, h_, w_, P(cams_), tmin, tmax, cull, V_, T_, P(b['vertices']), P(b['triangles']), ws.data_ptr(), cast_bytes, S_,
                                    P(dirs), bias, reach, light_, sun, ambient, None, bg_, sw_, sw_bytes, P(tri_), P(depth), P(f3), P(used), P(i1), P(out_f), P(out_8))
    who = 'durf_shade_cameras: requirement failed: '
    refused(cameras(F_=-1), who + 'F >= 0, h >= 1, w >= 1, F = -1')
    refused(cameras(h_=0), who + 'F >= 0, h >= 1, w >= 1')
    refused(cameras(F_=1 << 15, h_=1 << 8, w_=1 << 8), who + 'F h w < 2^31 pixels')
    refused(cameras(V_=-1), who + 'V >= 0')
    refused(cameras(T_=-1), who + '0 <= T <')
    refused(cameras(tmin=-1.0), who + 'tmin >= 0, tmin = -1')
    refused(cameras(tmin=nan), who + 'tmin >= 0, tmin = nan')
    refused(cameras(tmax=nan), who + 'tmax is a number')
    refused(cameras(sun=2), who + 'sun in 0 .. 1, sun = 2')
    refused(cameras(S_=0), who + 'S in 1 .. 256, S = 0')
    refused(cameras(bias=-1.0), who + 'bias >= 0')
    refused(cameras(reach=0.0), who + 'reach is +inf or > 0')
    refused(cameras(cull=-1), who + 'cull in 0 .. 2')
    refused(cameras(cast_bytes=ws.numel() - 1), 'durf_cast_workspace_bytes(%d)' % T)
    refused(cameras(ambient=2.0), who + 'ambient in [0, 1]')
    refused(cameras(light_=three(nan, 0, 0)), who + 'light and background are finite')
    refused(cameras(bg_=None), who + 'light and background (host floats)')
    refused(cameras(cams_=None), who + 'cams_dev, tri, depth, ao_used and ao_blocked for F = 1')
    refused(cameras(used=None), who + 'cams_dev, tri, depth, ao_used and ao_blocked for F = 1')
    refused(cameras(out_f=None, out_8=None), who + 'out_f or out_u8 for F = 1')
    refused(cameras(sw_=None), who + 'workspace aligned to 256 bytes')
    refused(cameras(sw_=sw.data_ptr() + 8), who + 'workspace aligned to 256 bytes')
    refused(cameras(sw_bytes=sw.numel() - 1), 'durf_shade_cameras: workspace of %d bytes, durf_shade_workspace_bytes(1, 4, 4) = %d' % (sw.numel() - 1, sw.numel()))
    assert cameras(F_=0, cams_=None, tri_=None, depth=None, used=None, out_f=None, out_8=None) == 0


# ---- the rasteriser's primaries, the cast's secondaries -------------------------------------------------------------------------------
def test_the_rasterisers_hits_shaded_equal_the_oracle_on_those_hits(cuda):
    h = w = 40
    v, t = R.icosphere(2)
    g, gt = R.quad_grid(6)
    v, t = S.merge((v, t), (g - F32([3.0, 3.0, 1.0]), gt))
    m = dict(vertices=v, triangles=t)
    cams = camera.rows([camera_ref.look_at((2.5, -2.0, 1.5), (0.0, 0.0, -0.5), up=(0.0, 0.0, 1.0))], 40.0, (w / 2.0 - 0.5, h / 2.0 - 0.5), h, w)
    rast = raster.render_mesh(m, cams, znear=0.1, attrs=(), label=None)
    b = cast.build(m)
    toward = R.pinhole32(cams[0], h, w)[1].reshape(1, h, w, 3)
    p, nr = shade.surface(b, rast['tri'], rast['bary'], toward=toward)
    used, blocked = shade.occlusion(b, p, nr, 32, reach=0.5)
    tri, bary = rast['tri'].cpu().numpy().reshape(-1), rast['bary'].cpu().numpy().reshape(-1, 3)
    wp, wn = S.surface32(v, t, tri, bary, toward.reshape(-1, 3))
    _same(p.reshape(-1, 3), wp, 'point'), _same(nr.reshape(-1, 3), wn, 'normal')
    wu, wb = S.occlusion32(v, t, wp, wn, S.fibonacci(32), 0.5 / 1024.0, 0.5)
    assert np.array_equal(used.cpu().numpy().reshape(-1), wu) and np.array_equal(blocked.cpu().numpy().reshape(-1), wb)
    ao = shade.ao_plane(used, blocked).cpu().numpy().reshape(-1)
    with np.errstate(all='ignore'):
        want = np.where(wu > 0, (wu - wb).astype(F32) / np.maximum(wu, 1).astype(F32), F32(1))
    _same(ao, want.astype(F32), 'ao')
    assert (tri >= 0).sum() > 800 and wb.sum() > 500 and want.min() < 0.8    # the contact shadow under the sphere


def test_the_commands_write_the_shaded_pictures_twice_alike(cuda, tmp_path):
    import json
    from durf_amd import cast_mesh, render_mesh
    for cmd, meta_name in ((cast_mesh, 'cast.json'), (render_mesh, 'raster.json')):
        outs = [tmp_path / ('%s_%d' % (meta_name, k)) for k in (0, 1)]
        for out in outs:
            assert cmd.main(['--synthetic', '--frames', '2', '--shade', '--ao_dirs', '16', '--eval_dir', str(out)]) == 0
        meta = json.loads((outs[0] / meta_name).read_text())
        assert meta['ao_dirs'] == 16 and meta['ao_reach'] > 0 and meta['bias'] > 0 and len(meta['light']) == 3
        for f in range(2):
            for kind in ('shade', 'ao', 'normals'):
                a, c = ((o / ('%s_%04d.ppm' % (kind, f))).read_bytes() for o in outs)
                assert a == c and a.startswith(b'P6\n64 48\n255\n') and len(a) == 13 + 3 * 48 * 64 and len(set(a[13:])) > 1, (kind, f)   # the same bytes, and a picture
        plain = tmp_path / ('plain_' + meta_name)
        assert cmd.main(['--synthetic', '--frames', '1', '--eval_dir', str(plain)]) == 0
        assert not (plain / 'shade_0000.ppm').exists() and 'ao_dirs' not in json.loads((plain / meta_name).read_text())
        assert (plain / 'depth_0000.npy').read_bytes() == (outs[0] / 'depth_0000.npy').read_bytes()
