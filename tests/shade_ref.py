"""The oracle of include/durf_shade.h in numpy.  surface32, occlusion32 and compose32: float32, every operation in the header's
order (numpy's float32 ufuncs round each operation once and fuse nothing).  occlusion32 forms the origins and the c > 0 mask
itself and asks tests/cast_ref.py whether a ray is blocked: cast32 (brute force over all triangles: the definition) or, with an
`order`, bvh32's any-hit walk of the implicit tree -- equal in every integer by durf_cast.h's proof, which
tests/test_shade_host.py exercises.  occlusion64: the float64 twin without box rule or clamp, with the margin by which each
(sample, direction) pair is decided.  Scenes shared by the tests."""
import functools

import numpy as np

from tests import cast_ref as R
from tests.trimesh_ref import interp32, merge, u8  # noqa: F401  (the interpolation, the 8-bit pack and the merge are trimesh_ref's)

F32 = np.float32
INF = F32(np.inf)


def _f(a):
    return np.ascontiguousarray(a, dtype=F32)


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def surface32(vertices, triangles, tri, bary, toward=None):
    """-> (point, normal) float32 [n,3]"""
    valid, P = R.valid_triangles(vertices, triangles)
    tri = np.asarray(tri, np.int64).reshape(-1)
    n, T = tri.shape[0], P.shape[0]
    bary = _f(bary).reshape(n, 3)
    ok = (tri >= 0) & (tri < T)
    ok[ok] = valid[tri[ok]]
    Pt = P[np.where(ok, tri, 0)] if T else np.zeros((n, 3, 3), F32)
    u, v = np.where(ok, bary[:, 1], F32(0))[:, None], np.where(ok, bary[:, 2], F32(0))[:, None]
    with np.errstate(all='ignore'):
        A = Pt[:, 0]
        e1, e2 = Pt[:, 1] - A, Pt[:, 2] - A
        point = (A + u * e1) + v * e2
        N = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2], e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], 1)
        len2 = _dot(N, N)
        flat = ~(len2 > 0) | ~np.isfinite(len2)
        inv = F32(1.0) / np.sqrt(len2)
        nrm = N * inv[:, None]
        if toward is not None:
            flip = _dot(nrm, _f(toward).reshape(n, 3)) > 0
            nrm = np.where(flip[:, None], -nrm, nrm)
    point = np.where(ok[:, None], point, F32(0)).astype(F32)
    normal = np.where((ok & ~flat)[:, None], nrm, F32(0)).astype(F32)
    return point, normal


def _pairs32(points, normals, dirs, bias):
    """-> (live [n], origins [n,3], used [n,S] bool)"""
    p, nr, d = _f(points).reshape(-1, 3), _f(normals).reshape(-1, 3), _f(dirs).reshape(-1, 3)
    live = np.isfinite(p).all(1) & np.isfinite(nr).all(1) & ~(nr == 0).all(1)
    with np.errstate(all='ignore'):
        o = p + F32(bias) * nr
        c = _dot(nr[:, None, :], d[None, :, :])
        used = (c > 0) & live[:, None]
    return live, o.astype(F32), used


def occlusion32(vertices, triangles, points, normals, dirs, bias, reach, cull=0, order=None, chunk=1 << 15, stats=None):
    """-> (used, blocked) int32 [n].  order: None for the definition (cast32 over all triangles), else a permutation of the
    triangles: bvh32's any-hit walk of the implicit tree over it.  The used rays go through in chunks, so that rays x triangles
    fits memory.  stats: a dict that receives tree_walk32's nodes and leaves per used ray (with an order)."""
    _, o, used = _pairs32(points, normals, dirs, bias)
    d = _f(dirs).reshape(-1, 3)
    i, s = np.nonzero(used)
    hit = np.zeros(len(i), bool)
    nodes, leaves = [], []
    for a in range(0, len(i), chunk):
        sl = slice(a, a + chunk)
        if order is None:
            hit[sl] = R.cast32(vertices, triangles, o[i[sl]], d[s[sl]], 0.0, reach, cull)[0] >= 0
        else:
            st = {}
            hit[sl] = R.bvh32(vertices, triangles, order, o[i[sl]], d[s[sl]], 0.0, reach, cull, any_hit=True, stats=st) == 1
            nodes.append(st['nodes']), leaves.append(st['leaves'])
    if stats is not None and order is not None:
        stats.update(nodes=np.concatenate(nodes) if nodes else np.zeros(0, np.int64), leaves=np.concatenate(leaves) if leaves else np.zeros(0, np.int64))
    blocked = np.zeros(used.shape, bool)
    blocked[i, s] = hit
    return used.sum(1).astype(np.int32), blocked.sum(1).astype(np.int32)


def occlusion64(vertices, triangles, points, normals, dirs, bias, reach, cull=0, chunk=1 << 12):
    """the float64 twin, no box rule and no clamp -> dict used, blocked bool [n,S] and margin float64 [n,S]: the least of |c|, the
    nearest hit's (any t >= 0) least barycentric weight, and |t - reach| / reach for that hit: how far the pair is from being
    decided the other way"""
    valid, P = R.valid_triangles(vertices, triangles)
    P = P[valid].astype(np.float64)
    p, nr, d = (np.asarray(a, np.float64).reshape(-1, 3) for a in (_f(points), _f(normals), _f(dirs)))
    n, S = p.shape[0], d.shape[0]
    live = np.isfinite(p).all(1) & np.isfinite(nr).all(1) & ~(nr == 0).all(1)
    with np.errstate(all='ignore'):
        o = p + float(F32(bias)) * nr
        c = (nr[:, None, :] * d[None]).sum(-1)
    used = (c > 0) & live[:, None]
    blocked = np.zeros((n, S), bool)
    margin = np.where(live[:, None], np.abs(c), np.inf)
    i, s = np.nonzero(used)
    A = P[None, :, 0]
    e1, e2 = P[None, :, 1] - A, P[None, :, 2] - A
    for a in range(0, len(i), chunk):
        ii, ss = i[a:a + chunk], s[a:a + chunk]
        oo, dd = o[ii][:, None], d[ss][:, None]
        with np.errstate(all='ignore'):
            pv = np.cross(dd, e2)
            det = (e1 * pv).sum(-1)
            sv = oo - A
            u = (sv * pv).sum(-1) / det
            q = np.cross(sv, e1)
            v = (dd * q).sum(-1) / det
            w = 1.0 - u - v
            t = (e2 * q).sum(-1) / det
            ok = (det != 0) & np.isfinite(1.0 / det) & (u >= 0) & (v >= 0) & (w >= 0) & (t >= 0)
            if cull:
                ok &= ~(det < 0) if cull == 1 else ~(det > 0)
            tt = np.where(ok, t, np.inf)
            if tt.shape[1]:
                j = tt.argmin(1)
                rows = np.arange(len(ii))
                hit = ok[rows, j]
                tn = tt[rows, j]
                edge = np.minimum(np.minimum(u[rows, j], v[rows, j]), w[rows, j])
                m = np.where(hit, np.minimum(edge, np.abs(tn - reach) / reach if np.isfinite(reach) else np.inf), np.inf)
                blocked[ii, ss] = hit & (tn <= reach)
                margin[ii, ss] = np.minimum(margin[ii, ss], m)
    return dict(used=used, blocked=blocked, margin=margin)


def compose32(tri, normals, used, blocked, light, ambient, background, sun_blocked=None, albedo=None):
    """-> (out_f float32 [n,3], out_u8 uint8 [n,3])"""
    tri = np.asarray(tri, np.int64).reshape(-1)
    n = tri.shape[0]
    nr, used, blocked = _f(normals).reshape(n, 3), np.asarray(used, np.int64).reshape(n), np.asarray(blocked, np.int64).reshape(n)
    light, background, ambient = _f(light).reshape(3), _f(background).reshape(3), F32(ambient)
    with np.errstate(all='ignore'):
        ao = np.where(used > 0, (used - blocked).astype(F32) / np.maximum(used, 1).astype(F32), F32(1)).astype(F32)
        lam = np.fmax(_dot(nr, light[None]), F32(0))
        sun = np.ones(n, F32) if sun_blocked is None else np.where(np.asarray(sun_blocked).reshape(n) > 0, F32(0), F32(1)).astype(F32)
        shade = ambient * ao + (F32(1.0) - ambient) * (lam * sun)
        c = np.repeat(shade[:, None], 3, 1) if albedo is None else _f(albedo).reshape(n, 3) * shade[:, None]
    out = np.where((tri >= 0)[:, None], c, background[None]).astype(F32)
    return out, u8(out)


# ---- scenes -----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def sphere_on_ground(grid=6):
    """the unit icosphere resting on a grid x grid ground of unit quads: the contact shadow -> (v, t); triangles 0 .. 319 are the
    sphere's"""
    return merge(R.icosphere(2, 1.0, (grid / 2.0, grid / 2.0, 1.0)), R.quad_grid(grid))


def face_samples(vertices, triangles, n, seed, min_weight=0.0, faces=None):
    """n samples on the faces (chosen by area among `faces`, default all) -> (tri int32 [n], bary float32 [n,3] = (w, u, v)); every
    weight at least min_weight"""
    rng = np.random.default_rng(seed)
    v, t = _f(vertices).reshape(-1, 3).astype(np.float64), np.asarray(triangles, np.int64).reshape(-1, 3)
    faces = np.arange(t.shape[0]) if faces is None else np.asarray(faces)
    P = v[t[faces]]
    area = np.linalg.norm(np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]), axis=1)
    tri = faces[rng.choice(len(faces), n, p=area / area.sum())]
    w = rng.dirichlet((1.0, 1.0, 1.0), n)
    w = min_weight + (1.0 - 3.0 * min_weight) * w
    return tri.astype(np.int32), w.astype(F32)


def flat_and_sliver():
    """a mesh of a good triangle, a zero-area one (three collinear points), a repeated vertex, a sliver, one with a NaN vertex
    and one with an index out of range -> (v, t)"""
    v = np.asarray([(0, 0, 0), (1, 0, 0), (0, 1, 0), (2, 0, 0), (0.5, 1e-15, 0), (np.nan, 0, 0), (0, 0, 1), (3, 1e-7, 1)], F32)
    t = np.asarray([(0, 1, 2), (0, 1, 3), (0, 0, 1), (0, 1, 4), (0, 1, 5), (0, 1, 99), (6, 0, 7)], np.int32)
    return v, t


def random_samples(n, seed, lo=0.0, hi=1.0):
    """n points in the cube [lo, hi]^3 with random unit normals (rounded to float32: unit to an ulp)"""
    rng = np.random.default_rng(seed)
    nr = rng.normal(size=(n, 3))
    return (lo + (hi - lo) * rng.random((n, 3))).astype(F32), (nr / np.linalg.norm(nr, axis=1, keepdims=True)).astype(F32)


def fibonacci(S):
    """durf_amd.shade.directions(S), restated: the oracle does not import what it checks"""
    k = np.arange(S, dtype=np.float64)
    z = 1.0 - (2.0 * k + 1.0) / S
    rho = np.sqrt(np.maximum(1.0 - z * z, 0.0))
    phi = k * (np.pi * (3.0 - np.sqrt(5.0)))
    d = np.stack([rho * np.cos(phi), rho * np.sin(phi), z], 1)
    return (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F32)


SAMPLE_COUNTS = (0, 1, 63, 64, 65, 255, 256, 257)
DIR_COUNTS = (1, 2, 3, 63, 64, 65, 256)
TRIANGLE_COUNTS = (0, 1, 4, 5, 9, 1025, 4097)      # the tree's leaf, level and top edges


def surface_samples(v, t, n, seed, min_weight=0.0, faces=None, inward=False):
    """n samples on the mesh with their point and flat normal (the right-hand one; inward: negated) by surface32"""
    tri, bary = face_samples(v, t, n, seed, min_weight, faces)
    p, nr = surface32(v, t, tri, bary)
    return p, (-nr if inward else nr)


@functools.lru_cache(maxsize=None)
def cases():
    """the smallest shapes at which the occlusion can go wrong -> {name: dict v, t, points, normals, dirs, bias, reach, cull};
    computed once, not to be written to"""
    C = {}

    def add(name, v, t, points, normals, dirs, reach, bias=None, cull=0):
        C[name] = dict(v=_f(v).reshape(-1, 3), t=np.asarray(t, np.int32).reshape(-1, 3), points=_f(points).reshape(-1, 3), normals=_f(normals).reshape(-1, 3),
                       dirs=_f(dirs).reshape(-1, 3), reach=float(reach), bias=float(reach) / 1024.0 if bias is None else float(bias), cull=cull)
    v, t = sphere_on_ground()
    for n in SAMPLE_COUNTS:                                                  # every sample count against one scene
        add('ground_n%d' % n, v, t, *surface_samples(v, t, n, 10 + n), fibonacci(16), 0.75)
    for S in DIR_COUNTS:                                                     # every direction count
        add('ground_S%d' % S, v, t, *surface_samples(v, t, 65, 20 + S), fibonacci(S), 0.75)
    for i, T in enumerate(TRIANGLE_COUNTS):
        add('soup_T%d' % T, *R.random_soup(T, 300 + i, scale=0.6 if T < 16 else 0.15), *random_samples(96, 310 + i), fibonacci(8), 0.5)
    add('ground_contact', v, t, *surface_samples(v, t, 300, 31), fibonacci(64), 0.5)
    add('ground_inf', v, t, *surface_samples(v, t, 100, 32), fibonacci(64), np.inf, bias=1.0 / 1024.0)
    add('ground_bias0', v, t, *surface_samples(v, t, 100, 33), fibonacci(32), 0.5, bias=0.0)
    for cull in (1, 2):
        add('ground_cull%d' % cull, v, t, *surface_samples(v, t, 100, 34), fibonacci(32), 0.75, cull=cull)
    d = R.scenes()['duplicates_300']
    add('duplicates_300', d['v'], d['t'], *random_samples(80, 41, -0.2, 1.0), fibonacci(32), 2.0)
    s = R.scenes()['sheets_one_ulp']                                        # samples on the lower sheet itself, nothing lifts them off it
    rng = np.random.default_rng(42)
    p = np.concatenate([rng.uniform(-1.0, 1.0, (60, 2)), np.ones((60, 1))], 1)
    add('sheets_one_ulp_bias0', s['v'], s['t'], p, np.tile(np.asarray([[0.0, 0.0, 1.0]]), (60, 1)), fibonacci(32), 4.0, bias=0.0)
    add('dirty', *R.dirty_mesh(), *random_samples(257, 43), fibonacci(16), 0.6)
    # directions: zero and subnormal components, one exactly in the tangent plane (c == 0: not used), all zero and NaN (c > 0
    # cannot hold: not used), an infinite component (used when c > 0, unusable: not blocked), not unit length
    gp = np.asarray([(x + 0.25, y + 0.5, 0.0) for x in range(6) for y in range(6)], F32)
    odd = np.asarray([(0, 0, 1), (1e-42, -1e-41, 1), (0, 1e-39, 3), (1, 0, 0), (0.5, 0.5, 0), (0, 0, 0), (np.nan, 0, 1), (0, np.nan, 0),
                      (np.inf, 0, 1), (0, 0, np.inf), (-np.inf, 0, 1), (0.3, -0.2, 1e-3), (0, 0, -1), (3, 4, 12)], F32)
    add('odd_directions', v, t, gp, np.tile(np.asarray([[0.0, 0.0, 1.0]]), (36, 1)), odd, np.inf, bias=0.0)
    # reach at a blocker's t and one ulp either side: straight up from under the sphere alone (no ground: it would block at t = 0)
    up = np.asarray([[0.0, 0.0, 1.0]], F32)
    under = np.asarray([(3.0 + 0.11 * i, 3.0 - 0.07 * i, -0.5) for i in range(-6, 7)], F32)
    sv, st = R.icosphere(2, 1.0, (3.0, 3.0, 1.0))
    t0 = R.cast32(sv, st, under, np.tile(up, (13, 1)))[1]
    assert (t0 > 0).all()
    for name, reach in (('reach_below_t', np.nextafter(t0[6], F32(0))), ('reach_at_t', t0[6]), ('reach_above_t', np.nextafter(t0[6], INF))):
        add(name, sv, st, under, np.tile(up, (13, 1)), up, reach, bias=0.0)
    return C


@functools.lru_cache(maxsize=None)
def expected(name):
    """occlusion32 of a case by the definition (brute force), computed once and shared: (used, blocked), not to be written to"""
    c = cases()[name]
    return occlusion32(c['v'], c['t'], c['points'], c['normals'], c['dirs'], c['bias'], c['reach'], c['cull'])


@functools.lru_cache(maxsize=None)
def big_case():
    """1500 samples x 64 directions x 5000 triangles, with its expectation by the any-hit walk over the Morton order (the host
    tests hold the walk to the definition; brute force here would take a minute)"""
    v, t = R.random_soup(5000, 81, scale=0.08)
    p, nr = random_samples(1500, 82)
    c = dict(v=v, t=t, points=p, normals=nr, dirs=fibonacci(64), bias=0.2 / 1024.0, reach=0.2, cull=0)
    return c, occlusion32(v, t, p, nr, c['dirs'], c['bias'], c['reach'], 0, order=R.morton_order(v, t))
