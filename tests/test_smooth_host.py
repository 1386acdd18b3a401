"""include/durf_smooth.h on the host: the oracle's CSR against a construction by sets, the census on meshes whose answer is known
(and on the marching-tetrahedra oracle's sphere: the first check of "closed wherever the lattice is usable"), float32 against the
float64 twin, the properties smoothing rests on as inequalities between oracle runs, and the refusals of durf_amd/smooth.py and
of the library, none of which needs a device."""
import numpy as np
import pytest

from durf_amd import _lib, _smooth_sigs, smooth
from tests import mesh_ref as M, smooth_ref as S

F32 = np.float32


# ---- the oracle against brute force ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('V,T,seed', [(1, 1, 0), (5, 40, 1), (12, 100, 2), (40, 60, 3), (7, 300, 4)])
def test_the_csr_by_keys_equals_the_one_by_sets(V, T, seed):
    v, t = S.soup(V, T, seed)
    a = S.adjacency(v, t)
    rows, corners = S.brute_adjacency(t, V)
    assert a['offsets'][0] == 0 and a['offsets'][V] == a['neighbours'].size == a['multiplicity'].size <= 6 * T
    assert a['corner_offsets'][V] == a['corner_tri'].size == 3 * int(S.contributing(t, V).sum())
    for p in range(V):
        lo, hi = a['offsets'][p], a['offsets'][p + 1]
        assert list(zip(a['neighbours'][lo:hi].tolist(), a['multiplicity'][lo:hi].tolist())) == rows[p], p
        assert a['corner_tri'][a['corner_offsets'][p]:a['corner_offsets'][p + 1]].tolist() == corners[p], p
    ek, ck = S.keys(t, V)
    assert ek.size == 6 * T and ck.size == 3 * T
    assert ((ek == S.NO_KEY).reshape(T, 6).all(1) == ~S.contributing(t, V)).all()


def test_the_sentinel_and_the_limit_are_the_headers():
    assert int(S.NO_KEY) == _smooth_sigs.DURF_SMOOTH_NO_KEY == 2 ** 63 - 1
    assert smooth.MAX_TRIANGLES == _smooth_sigs.DURF_SMOOTH_MAX_TRIANGLES and 6 * (smooth.MAX_TRIANGLES - 1) < 2 ** 31 <= 6 * smooth.MAX_TRIANGLES
    assert (S.ISOLATED, S.INTERIOR, S.BOUNDARY, S.NONMANIFOLD) == tuple(getattr(_smooth_sigs, 'DURF_SMOOTH_' + k) for k in ('ISOLATED', 'INTERIOR', 'BOUNDARY', 'NONMANIFOLD'))
    assert smooth.BOUNDARY == dict(pin=_smooth_sigs.DURF_SMOOTH_PIN, slide=_smooth_sigs.DURF_SMOOTH_SLIDE) == dict(pin=S.PIN, slide=S.SLIDE)
    assert len(smooth.CENSUS_FIELDS) == _smooth_sigs.DURF_SMOOTH_CENSUS_INTS


# ---- census on known meshes -----------------------------------------------------------------------------------------------------
def _census(v, t):
    a = S.adjacency(v, t)
    c = S.census(a)
    return dict(zip(smooth.CENSUS_FIELDS, c.tolist())), S.derive(c, a['V'])


def test_census_on_known_meshes():
    c, (closed, euler) = _census(*S.tetrahedron())
    assert (c['interior'], c['triangles'], c['edges'], c['boundary_edges'], c['nonmanifold_edges']) == (4, 4, 6, 0, 0) and closed and euler == 2
    v, t = S.icosphere(2)
    c, (closed, euler) = _census(v, t)
    assert (c['interior'], c['triangles'], c['edges']) == (v.shape[0], 320, 480) and closed and euler == 2
    c, (closed, euler) = _census(*S.quad())
    assert (c['boundary'], c['interior'], c['triangles'], c['edges'], c['boundary_edges'], c['nonmanifold_edges']) == (4, 0, 2, 5, 4, 0)
    assert not closed and euler == 1
    c, (closed, euler) = _census(*S.book())
    assert (c['nonmanifold'], c['boundary'], c['triangles'], c['edges'], c['boundary_edges'], c['nonmanifold_edges']) == (2, 3, 3, 7, 6, 1) and not closed
    c, (closed, euler) = _census(*S.duplicate())
    assert (c['nonmanifold'], c['interior'], c['triangles'], c['edges'], c['boundary_edges'], c['nonmanifold_edges']) == (3, 1, 5, 6, 0, 3) and not closed
    c, (closed, euler) = _census(*S.bad_indices())
    v, t = S.quad_grid(3)
    assert c['triangles'] == t.shape[0] and c['isolated'] == 0 and c['edges'] == 33 and c['boundary_edges'] == 12 and euler == 1
    c, (closed, euler) = _census(np.zeros((3, 3), F32), np.zeros((0, 3), np.int32))
    assert c['isolated'] == 3 and c['triangles'] == 0 and closed and euler == 0


def test_marching_tetrahedra_of_a_sphere_inside_the_lattice_is_closed_and_manifold():
    fr = M.unit_frame(0.25, (-2.0, -2.0, -2.0))
    m = M.surface(M.sphere_field(fr, (17, 17, 17), (0.03, -0.02, 0.01), 1.3), None, 0.0, fr)
    c, (closed, euler) = _census(m['vertices'], m['triangles'])
    assert c['triangles'] == m['triangles'].shape[0] > 1000 and c['isolated'] == 0
    assert c['interior'] == m['vertices'].shape[0] and c['boundary'] == 0 and c['nonmanifold'] == 0
    assert closed and euler == 2
    assert M.is_closed(m['triangles']) and M.euler(m['triangles']) == 2      # the older census agrees


# ---- float32 against the float64 twin -------------------------------------------------------------------------------------------
# One step in float32 is n - 1 additions, a division, a subtraction, a product and a sum, each rounded once.  The bound is the
# issue's: 4 ulp of the largest operand of the vertex and axis (the vertex, every partial sum, the mean, the displacement), per step,
# both twins starting from the same float32 input.
@pytest.mark.parametrize('seed', [0, 1, 2])
def test_float32_is_within_4_ulp_of_the_float64_twin_per_step(seed):
    v, t = S.noisy_icosphere(3, seed)
    a = S.adjacency(v, t)
    x = v
    for factor in (0.5, -0.53, 1.0, -1.0):
        got, (want, largest) = S.step(a, x, factor), S.step(a, x, factor, dt=np.float64, operands=True)
        ulps = np.abs(got.astype(np.float64) - want) / M.ulp32(largest)      # per vertex and axis, in ulps of ITS largest operand
        print('seed %d factor %+.2f: at most %.3f ulp of the largest operand' % (seed, factor, ulps.max()))
        assert ulps.max() <= 4
        x = got
    n32, n64 = S.normals(a, x), S.normals(a, x, dt=np.float64)
    assert np.abs(n32 - n64).max() < 1e-5 and np.abs(np.linalg.norm(n32, axis=1) - 1).max() < 1e-6


# ---- what smoothing is for ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('seed', [0, 1, 2])
def test_taubin_smooths_and_keeps_the_volume_better_than_laplacian(seed):
    """Inequalities between oracle runs on the level-3 icosphere with 3 % radial noise (DESIGN.md 19 records the printed values)."""
    v, t = S.noisy_icosphere(3, seed)
    a = S.adjacency(v, t)
    tb = S.taubin(a, v, 10, 0.5, -0.53)
    lp = S.taubin(a, v, 20, 0.5, 0.0)
    r0, r1, r2 = S.rms_radial(v), S.rms_radial(tb), S.rms_radial(lp)
    v0, v1, v2 = S.volume(v, t), S.volume(tb, t), S.volume(lp, t)
    print('seed %d: rms radial deviation %.5f -> taubin %.5f, laplacian %.5f; volume %.5f -> taubin %.5f (%+.3f %%), laplacian %.5f (%+.3f %%)' % (
        seed, r0, r1, r2, v0, v1, 100 * (v1 / v0 - 1), v2, 100 * (v2 / v0 - 1)))
    assert r1 < r0
    assert abs(v1 - v0) < abs(v2 - v0)


def test_pinned_vertices_keep_their_bits_and_zero_iterations_copy():
    v, t = S.not_finite()
    a = S.adjacency(v, t)
    fixed = np.zeros(v.shape[0], np.uint8)
    fixed[[0, 3, 9]] = 1
    out = S.step(a, v, 0.5, fixed=fixed)
    for i in (0, 3, 9, 5, 17, 30):
        assert np.array_equal(S.bits(out[i]), S.bits(v[i])), i
    moved = np.isfinite(v).all(1) & (fixed == 0)
    assert (S.bits(out[moved]) != S.bits(v[moved])).any(1).all(), 'every free finite vertex of a noisy closed mesh moves'
    assert np.isfinite(out[moved]).all(), 'a neighbour that is not finite is left out of the mean'
    assert np.array_equal(S.bits(S.taubin(a, v, 0, 0.5, -0.53)), S.bits(v))
    # an open patch: the boundary is pinned, or slides along itself
    gv, gt = S.quad_grid(4)
    gv = gv + np.random.default_rng(0).uniform(-0.2, 0.2, gv.shape).astype(F32)
    ga = S.adjacency(gv, gt)
    edge = ga['vertex_class'] == S.BOUNDARY
    assert edge.sum() == 16 and (ga['vertex_class'] == S.INTERIOR).sum() == 9
    pin, slide = S.step(ga, gv, 0.5, S.PIN), S.step(ga, gv, 0.5, S.SLIDE)
    assert np.array_equal(S.bits(pin[edge]), S.bits(gv[edge])) and (S.bits(slide[edge]) != S.bits(gv[edge])).any(1).all()
    assert np.array_equal(S.bits(pin[~edge]), S.bits(slide[~edge]))
    corner = 0                                                              # its two boundary neighbours: 1 and 5
    want = gv[corner] + F32(0.5) * ((gv[1] + gv[5]) / F32(2.0) - gv[corner])
    assert np.array_equal(S.bits(slide[corner]), S.bits(want))
    # the normals of a closed outward mesh point outwards; a vertex without a triangle has none
    n = S.normals(S.adjacency(*S.icosphere(2)), S.icosphere(2)[0])
    assert ((n * S.icosphere(2)[0]).sum(1) > 0.99).all()
    assert np.array_equal(S.normals(S.adjacency(np.ones((2, 3), F32), np.zeros((0, 3), np.int32)), np.ones((2, 3), F32)), np.zeros((2, 3), F32))


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def test_smooth_py_refuses_before_anything_touches_the_device():
    v, t = S.tetrahedron()
    m = dict(vertices=v, triangles=t)
    for call, text in ((lambda: smooth.adjacency(dict(vertices=v)), 'smooth.adjacency: m is a dict with vertices [V,3] and triangles [T,3]'),
                       (lambda: smooth.adjacency(dict(vertices=v[:, :2], triangles=t)), 'smooth.adjacency: vertices of shape (4, 2)'),
                       (lambda: smooth.adjacency(dict(vertices=v, triangles=type('A', (), dict(shape=(smooth.MAX_TRIANGLES, 3)))())), 'the limit is 6 T < 2^31'),
                       (lambda: smooth.taubin(m, iters=-1), 'smooth.taubin: iters = -1'),
                       (lambda: smooth.taubin(m, iters=1.5), 'smooth.taubin: iters = 1.5'),
                       (lambda: smooth.taubin(m, lam=0.0), 'smooth.taubin: lam = 0.0, expected a number in (0, 1]'),
                       (lambda: smooth.taubin(m, lam=1.5), 'smooth.taubin: lam = 1.5'),
                       (lambda: smooth.taubin(m, mu=0.1), 'smooth.taubin: mu = 0.1, expected a number in [-1, 0]'),
                       (lambda: smooth.taubin(m, mu=float('nan')), 'smooth.taubin: mu = nan'),
                       (lambda: smooth.taubin(m, boundary='free'), "smooth.taubin: boundary = 'free', expected 'pin' or 'slide'"),
                       (lambda: smooth.taubin(dict(vertices=v), 3), 'smooth.taubin: m is a dict'),
                       (lambda: smooth.laplacian(m, 3, factor=-0.5), 'smooth.laplacian: factor = -0.5'),
                       (lambda: smooth.laplacian(m, None), 'smooth.laplacian: iters = None'),
                       (lambda: smooth.step(m, 2.0), 'smooth.step: factor = 2.0, expected a number in [-1, 1]'),
                       (lambda: smooth.step(m, 0.5, adj=dict(V=4)), "smooth.step: adj is smooth.adjacency's dict"),
                       (lambda: smooth.normals(m, adj=dict(dict.fromkeys(smooth.ADJ_KEYS, 0), V=5, T=4)), 'smooth.normals: adj of 5 vertices and 4 triangles for a mesh of 4 and 4'),
                       (lambda: smooth.census(None), "smooth.census: adj is smooth.adjacency's dict"),
                       (lambda: smooth.options(dict(iterations=3), 'mesh.extract'), "mesh.extract: smooth has no 'iterations'"),
                       (lambda: smooth.options(-2, 'mesh.extract'), 'mesh.extract: iters = -2')):
        with pytest.raises(ValueError) as e:
            call()
        assert text in str(e.value), (text, str(e.value))
    assert smooth.options(0, 'x') is None and smooth.options(None, 'x') is None and smooth.options(4, 'x') == dict(iters=4)
    assert smooth.options(dict(iters=3, mu=0.0), 'x') == dict(iters=3, mu=0.0)


FAKE = 0x1000                                                               # a pointer that is never followed: 256-aligned, not NULL


def _err():
    return _lib.lib().durf_last_error().decode()


def test_the_library_refuses_every_bad_argument_before_any_launch():
    L = _lib.smooth_lib()
    big = _smooth_sigs.DURF_SMOOTH_MAX_TRIANGLES
    assert L.durf_smooth_workspace_bytes(-1) == 0 and L.durf_smooth_workspace_bytes(big) == 0
    need = L.durf_smooth_workspace_bytes(100)
    assert need >= 4 * 601 and need % 256 == 0 and L.durf_smooth_workspace_bytes(0) >= 256
    nan, inf = float('nan'), float('inf')
    keys = lambda V=4, T=4, tr=FAKE, ek=FAKE, ck=FAKE: L.durf_smooth_keys(None, V, T, tr, ek, ck)
    adj = lambda V=4, T=100, ek=FAKE, ck=FAKE, cap=600, ws=FAKE, wb=need, off=FAKE, nb=FAKE, mu=FAKE, coff=FAKE, ct=FAKE: \
        L.durf_smooth_adjacency(None, V, T, ek, ck, cap, ws, wb, off, nb, mu, coff, ct)
    cls = lambda V=4, off=FAKE, mu=FAKE, out=FAKE: L.durf_smooth_classify(None, V, off, mu, out)
    cen = lambda V=4, off=FAKE, coff=FAKE, vc=FAKE, out=FAKE: L.durf_smooth_census(None, V, off, FAKE, FAKE, coff, vc, out)
    step = lambda V=4, x=FAKE, off=FAKE, vc=FAKE, f=0.5, b=0, out=2 * FAKE: L.durf_smooth_step(None, V, x, off, FAKE, FAKE, vc, f, b, None, out)
    tb = lambda V=4, x=FAKE, off=FAKE, vc=FAKE, it=2, la=0.5, mu=-0.53, b=0, tmp=3 * FAKE, out=2 * FAKE: \
        L.durf_smooth_taubin(None, V, x, off, FAKE, FAKE, vc, it, la, mu, b, None, tmp, out)
    nrm = lambda V=4, T=4, v=FAKE, t=FAKE, coff=FAKE, ct=FAKE, out=FAKE: L.durf_smooth_normals(None, V, T, v, t, coff, ct, out)
    for call, who, text in (
            (lambda: keys(V=-1), 'durf_smooth_keys', 'V >= 0, V = -1'), (lambda: keys(T=-1), 'durf_smooth_keys', 'T = -1'),
            (lambda: keys(T=big), 'durf_smooth_keys', 'T in 0 .. DURF_SMOOTH_MAX_TRIANGLES - 1 = %d, T = %d' % (big - 1, big)),
            (lambda: keys(tr=None), 'durf_smooth_keys', 'triangles for T = 4'), (lambda: keys(ck=None), 'durf_smooth_keys', 'edge_keys and corner_keys for T = 4'),
            (lambda: adj(V=-2), 'durf_smooth_adjacency', 'V >= 0, V = -2'), (lambda: adj(T=big), 'durf_smooth_adjacency', 'T = %d' % big),
            (lambda: adj(cap=599), 'durf_smooth_adjacency', 'cap >= 6 T, cap = 599, T = 100'),
            (lambda: adj(ek=None), 'durf_smooth_adjacency', 'edge_keys, corner_keys and corner_tri for T = 100'),
            (lambda: adj(ct=None), 'durf_smooth_adjacency', 'edge_keys, corner_keys and corner_tri for T = 100'),
            (lambda: adj(mu=None), 'durf_smooth_adjacency', 'neighbours and multiplicity for T = 100'),
            (lambda: adj(coff=None), 'durf_smooth_adjacency', 'offsets and corner_offsets [V+1]'),
            (lambda: adj(ws=None), 'durf_smooth_adjacency', 'workspace aligned to 256 bytes'),
            (lambda: adj(ws=FAKE + 4), 'durf_smooth_adjacency', 'workspace aligned to 256 bytes'),
            (lambda: adj(wb=need - 1), 'durf_smooth_adjacency', 'workspace of %d bytes, durf_smooth_workspace_bytes(100) = %d' % (need - 1, need)),
            (lambda: cls(V=-1), 'durf_smooth_classify', 'V >= 0, V = -1'), (lambda: cls(off=None), 'durf_smooth_classify', 'offsets [V+1]'),
            (lambda: cls(out=None), 'durf_smooth_classify', 'vertex_class for V = 4'),
            (lambda: cen(V=-1), 'durf_smooth_census', 'V >= 0, V = -1'), (lambda: cen(out=None), 'durf_smooth_census', 'offsets, corner_offsets and census'),
            (lambda: cen(coff=None), 'durf_smooth_census', 'offsets, corner_offsets and census'), (lambda: cen(vc=None), 'durf_smooth_census', 'vertex_class for V = 4'),
            (lambda: step(V=-1), 'durf_smooth_step', 'V >= 0, V = -1'), (lambda: step(f=nan), 'durf_smooth_step', 'factor finite and in [-1, 1], factor = nan'),
            (lambda: step(f=inf), 'durf_smooth_step', 'factor = inf'), (lambda: step(f=1.0001), 'durf_smooth_step', 'factor = 1.0001'),
            (lambda: step(f=-1.5), 'durf_smooth_step', 'factor = -1.5'), (lambda: step(b=2), 'durf_smooth_step', 'boundary = 2'),
            (lambda: step(out=FAKE), 'durf_smooth_step', 'in != out'), (lambda: step(off=None), 'durf_smooth_step', 'offsets [V+1]'),
            (lambda: step(x=None), 'durf_smooth_step', 'in, out and vertex_class for V = 4'), (lambda: step(vc=None), 'durf_smooth_step', 'in, out and vertex_class for V = 4'),
            (lambda: tb(it=-1), 'durf_smooth_taubin', 'iters = -1'), (lambda: tb(it=2 ** 30), 'durf_smooth_taubin', 'iters = %d' % 2 ** 30),
            (lambda: tb(la=nan), 'durf_smooth_taubin', 'lambda finite and in [-1, 1], lambda = nan'), (lambda: tb(mu=-2.0), 'durf_smooth_taubin', 'mu = -2'),
            (lambda: tb(b=-1), 'durf_smooth_taubin', 'boundary = -1'), (lambda: tb(out=FAKE), 'durf_smooth_taubin', 'in != out'),
            (lambda: tb(tmp=None), 'durf_smooth_taubin', 'tmp [V,3] that is neither in nor out, for 4 steps'),
            (lambda: tb(tmp=FAKE), 'durf_smooth_taubin', 'tmp [V,3] that is neither in nor out'),
            (lambda: tb(tmp=2 * FAKE, mu=0.0), 'durf_smooth_taubin', 'neither in nor out, for 2 steps'),
            (lambda: nrm(V=-1), 'durf_smooth_normals', 'V >= 0, V = -1'), (lambda: nrm(T=big), 'durf_smooth_normals', 'T = %d' % big),
            (lambda: nrm(v=None), 'durf_smooth_normals', 'vertices for V = 4'), (lambda: nrm(t=None), 'durf_smooth_normals', 'triangles for T = 4'),
            (lambda: nrm(ct=None), 'durf_smooth_normals', 'corner_tri for T = 4'), (lambda: nrm(coff=None), 'durf_smooth_normals', 'corner_offsets [V+1]'),
            (lambda: nrm(out=None), 'durf_smooth_normals', 'normals for V = 4')):
        assert call() != 0 and who in _err() and text in _err(), (who, text, _err())
    # the empty shapes that need no launch succeed without a device
    assert keys(V=0, T=0, tr=None, ek=None, ck=None) == 0 and cls(V=0, out=None) == 0
    assert step(V=0, x=None, vc=None, out=None) == 0 and tb(V=0, x=None, vc=None, tmp=None, out=None) == 0
    assert nrm(V=0, T=0, v=None, t=None, ct=None, out=None) == 0


def test_the_commands_take_the_four_flags_and_refuse_bad_values_under_their_own_name():
    from durf_amd import extract_mesh, fuse_tsdf
    for mod, prog in ((extract_mesh, 'extract_mesh'), (fuse_tsdf, 'fuse_tsdf')):
        ap = mod.build_parser()
        a = ap.parse_args(['--eval_dir', 'o', '--synthetic'])
        assert (a.smooth, a.smooth_lambda, a.smooth_mu, a.smooth_boundary) == (0, 0.5, -0.53, 'pin') and smooth.from_args(a, prog) is None
        a = ap.parse_args(['--eval_dir', 'o', '--synthetic', '--smooth', '3', '--smooth_mu', '0', '--smooth_boundary', 'slide'])
        assert smooth.from_args(a, prog) == dict(iters=3, lam=0.5, mu=0.0, boundary='slide')
        assert smooth.options(smooth.from_args(a, prog), prog) == smooth.from_args(a, prog)
        for argv, text in ((['--smooth', '-1'], prog + ': iters = -1'), (['--smooth', '2', '--smooth_lambda', '0'], prog + ': --smooth_lambda = 0.0'),
                           (['--smooth', '2', '--smooth_mu', '0.5'], prog + ': --smooth_mu = 0.5, expected a number in [-1, 0]')):
            with pytest.raises(SystemExit) as e:
                smooth.from_args(ap.parse_args(['--eval_dir', 'o', '--synthetic'] + argv), prog)
            assert text in str(e.value), str(e.value)
        with pytest.raises(SystemExit):
            ap.parse_args(['--eval_dir', 'o', '--smooth_boundary', 'free'])
