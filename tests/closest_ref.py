"""The oracle of include/durf_closest.h in numpy.  closest32: brute force over points x triangles in float32, every operation
in the header's order (numpy's float32 ufuncs round each operation once and fuse nothing).  closest64: the float64 twin without
box bound or clamp, with the first-order error bound of the float32 formula.  walk32: csrc/closest.hip's box bound and
triangle rule on cast_ref.tree_walk32's walk -- by the header's proof it equals closest32 in every bit, which
tests/test_closest_host.py exercises.  Scenes shared by the tests."""
import functools

import numpy as np

from tests import cast_ref as C

F32 = np.float32
INF = C.INF
U = 2.0 ** -24


def _f(a):
    return np.ascontiguousarray(a, dtype=F32)


def _dot(x, y):
    return (x[..., 0] * y[..., 0] + x[..., 1] * y[..., 1]) + x[..., 2] * y[..., 2]


def box_bound(lo, hi, P):
    """the box bound, broadcasting: lo, hi, P [...,3] -> lb [...]; +inf for the empty box by the formula itself"""
    with np.errstate(all='ignore'):
        e = np.fmax(np.fmax(lo - P, P - hi), F32(0))
        return _dot(e, e).astype(F32)


def _clamped(num, den):
    with np.errstate(all='ignore'):
        return np.where(den > 0, np.fmin(np.fmax(num / den, F32(0)), F32(1)), F32(0)).astype(F32)


def tri_rule(V, P):
    """the triangle rule and the clamp on valid triangles, broadcasting: V [...,3,3], P [...,3] ->
    (d2 [...], wuv [...,3], point [...,3], lb [...]: the bound of the triangle's own box, d2_0 [...]: d2 before the clamp)"""
    V, P = np.broadcast_arrays(V, P[..., None, :])
    P = P[..., 0, :]
    one, zero = F32(1), F32(0)
    with np.errstate(all='ignore'):
        A, B, Cv = V[..., 0, :], V[..., 1, :], V[..., 2, :]
        e1, e2, s, f, r = B - A, Cv - A, P - A, Cv - B, P - B
        a, b, c, d, e, l, g = _dot(e1, e1), _dot(e1, e2), _dot(e2, e2), _dot(e1, s), _dot(e2, s), _dot(f, f), _dot(f, r)
        shape = a.shape
        best_d2 = np.full(shape, INF)
        best_w = np.stack([np.full(shape, one), np.full(shape, zero), np.full(shape, zero)], -1)
        best_c = np.array(A, F32)

        def candidate(w, u, v, allowed):
            nonlocal best_d2, best_w, best_c
            c_ = (A + u[..., None] * e1) + v[..., None] * e2
            q = P - c_
            d2 = _dot(q, q)
            take = allowed & (d2 < best_d2)
            best_d2 = np.where(take, d2, best_d2)
            best_w = np.where(take[..., None], np.stack([w, u, v], -1), best_w)
            best_c = np.where(take[..., None], c_, best_c)
        det = a * c - b * b
        u, v = (c * d - b * e) / det, (a * e - b * d) / det
        w = (one - u) - v
        candidate(w, u, v, (det > 0) & (u >= 0) & (v >= 0) & (w >= 0))
        yes, nul = np.ones(shape, bool), np.zeros(shape, F32)
        x = _clamped(d, a)
        candidate(one - x, x, nul, yes)
        x = _clamped(e, c)
        candidate(one - x, nul, x, yes)
        x = _clamped(g, l)
        candidate(nul, one - x, x, yes)
        lb = box_bound(*C.tri_box(V), P)
        d2 = np.fmax(best_d2, lb) + zero
    return d2.astype(F32), best_w.astype(F32), best_c.astype(F32), lb, best_d2.astype(F32)


def cap2_of(max_dist):
    with np.errstate(over='ignore'):
        return F32(max_dist) * F32(max_dist)


def _finish(P, usable, max_dist, best_id, best_d2, best_w, best_c):
    tri = np.where(usable, best_id, -2).astype(np.int32)
    found = tri >= 0
    with np.errstate(all='ignore'):
        dist = np.where(found, np.sqrt(np.where(found, best_d2, F32(0)).astype(F32)), F32(max_dist)).astype(F32)
    dist[~usable] = np.nan
    bary, point = np.where(found[:, None], best_w, F32(0)).astype(F32), np.where(found[:, None], best_c, F32(0)).astype(F32)
    bary[~usable], point[~usable] = np.nan, np.nan
    return tri, dist, bary, point


def closest32(vertices, triangles, points, max_dist=np.inf, chunk=None):
    """-> (tri int32 [n], dist float32 [n], bary float32 [n,3] = (w, u, v), point float32 [n,3]): the definition, by brute force"""
    valid, V = C.valid_triangles(vertices, triangles)
    P = _f(points).reshape(-1, 3)
    n = P.shape[0]
    usable = np.isfinite(P).all(1)
    cap2 = cap2_of(max_dist)
    ids = np.nonzero(valid)[0]
    Vv = V[ids]
    best_id, best_d2, best_w, best_c = np.full(n, -1, np.int64), np.zeros(n, F32), np.zeros((n, 3), F32), np.zeros((n, 3), F32)
    chunk = chunk or max(1, (1 << 19) // max(len(ids), 1))
    for a in range(0, n, chunk):
        if not len(ids):
            break
        sl = slice(a, a + chunk)
        d2, w, c, _, _ = tri_rule(Vv[None], np.where(usable[sl, None], P[sl], F32(0))[:, None])
        ok = d2 <= cap2
        dd = np.where(ok, d2, INF)
        dmin = dd.min(1)
        j = np.argmax(ok & (dd == dmin[:, None]), axis=1)                    # the smallest id among the counting triangles at the minimum
        hit = ok.any(1)
        rows = np.arange(dd.shape[0])
        best_id[sl] = np.where(hit, ids[j], -1)
        best_d2[sl], best_w[sl], best_c[sl] = d2[rows, j], w[rows, j], c[rows, j]
    return _finish(P, usable, max_dist, best_id, best_d2, best_w, best_c)


def point_segment64(P, A, B):
    """float64 distance from P [...,3] to the segment A B"""
    ab = B - A
    with np.errstate(all='ignore'):
        t = np.clip(np.nan_to_num(((P - A) * ab).sum(-1) / (ab * ab).sum(-1)), 0.0, 1.0)
    return np.linalg.norm(P - (A + t[..., None] * ab), axis=-1)


def closest64(vertices, triangles, points, max_dist=np.inf):
    """the float64 twin without box bound or clamp -> dict tri, dist, bary (w, u, v), point, gap (the second smallest distance
    over the triangles minus the smallest, inf with fewer than two), err32: a first-order bound of the float32 formula's
    rounding error in dist, derived as follows (U = 2^-24, everything per winning triangle):
      the point.  C_k = fl(fl(A_k + fl(u e1_k)) + fl(v e2_k)) with e1_k = fl(B_k - A_k): the roundings of e1_k and of the product
        give 2 U |e1_k|, likewise 2 U |e2_k|, the two sums U M_k each (M_k the largest |coordinate| of the three vertices: both
        partial sums are convex combinations), and q_k = fl(P_k - C_k) adds U |q_k|: |dq| <= U |2 |e1| + 2 |e2| + 2 M + |q||_2;
      the sum.  three squares, two additions and the square root: 3 U dist (the clamp's lb: a rounded difference, squares, sums:
        the same 3 U);
      the weights.  (u, v) solves the 2 x 2 normal equations G (u, v) = (d, e), G the Gram matrix of (e1, e2).  Its entries and
        right-hand sides carry about 5 U of their magnitudes (two rounded differences, three products, two sums), and 1 /
        lambda_min(G) <= L^2 / det for L^2 = a + c, so |d(u, v)| <= 5 U (L^2 / det) (|s| L + 1.5 L^2) and the point moves IN THE
        PLANE by dC <= 5 U kappa (|s| + 1.5 L), kappa = L^4 / det (>= 4; it grows as the triangle degenerates).  On a segment x
        = d / a gives dC <= 5 U |s| + 3 U L: kappa = 1.  The true closest point is the foot of a perpendicular, so moving it by
        dC in the plane lengthens the distance by sqrt(dist^2 + dC^2) - dist <= min(dC, dC^2 / (2 dist)); a clamped end point
        does not move.
    kappa is returned too."""
    valid, V = C.valid_triangles(vertices, triangles)
    V = V.astype(np.float64)[None]
    P = np.asarray(points, np.float64).reshape(-1, 3)
    n, T = P.shape[0], V.shape[1]
    Pb = P[:, None]
    A, B, Cv = V[:, :, 0], V[:, :, 1], V[:, :, 2]
    e1, e2, s = B - A, Cv - A, Pb - A
    with np.errstate(all='ignore'):
        a, b, c, d, e = (e1 * e1).sum(-1), (e1 * e2).sum(-1), (e2 * e2).sum(-1), (e1 * s).sum(-1), (e2 * s).sum(-1)
        det = a * c - b * b
        u, v = (c * d - b * e) / det, (a * e - b * d) / det
        inside = (det > 1e-30 * (a + c) ** 2) & (u >= 0) & (v >= 0) & (u + v <= 1)
        cand_uv = [np.stack([np.where(inside, u, 0.0), np.where(inside, v, 0.0)], -1)]
        for (X, Y, uv) in ((A, B, lambda t: (t, 0 * t)), (A, Cv, lambda t: (0 * t, t)), (B, Cv, lambda t: (1 - t, t))):
            xy = Y - X
            t = np.clip(np.nan_to_num(((Pb - X) * xy).sum(-1) / (xy * xy).sum(-1)), 0.0, 1.0)
            cand_uv.append(np.stack(uv(t), -1))
        cand_uv = np.stack(cand_uv, 2)                                       # [n,T,4,2]
        pts = A[:, :, None] + cand_uv[..., :1] * e1[:, :, None] + cand_uv[..., 1:] * e2[:, :, None]
        dd = np.linalg.norm(Pb[:, :, None] - pts, axis=-1)
        dd[..., 0] = np.where(inside, dd[..., 0], np.inf)
        which = dd.argmin(-1)
        rows, cols = np.arange(n)[:, None], np.arange(T)[None]
        dist_t = np.where(valid[None], dd[rows, cols, which], np.inf)
    if T == 0:
        z = np.zeros(n)
        return dict(tri=np.full(n, -1), dist=np.full(n, float(max_dist)), bary=np.zeros((n, 3)), point=np.zeros((n, 3)), gap=np.full(n, np.inf),
                    err32=z, kappa=z)
    order = np.argsort(dist_t, axis=1, kind='stable')[:, :2]
    r1 = np.arange(n)
    j = order[:, 0]
    dist = dist_t[r1, j]
    hit = dist <= max_dist
    second = dist_t[r1, order[:, 1]] if T > 1 else np.full(n, np.inf)
    wj = which[r1, j]
    uv = cand_uv[r1, j, wj]
    point = pts[r1, j, wj]
    with np.errstate(all='ignore'):
        L = np.sqrt((a + c)[0, j])
        kappa = np.where(wj == 0, L ** 4 / det[0, j], 1.0)
        M = np.abs(V[0, j]).max(1)
        dq = U * np.linalg.norm(2 * np.abs(e1[0, j]) + 2 * np.abs(e2[0, j]) + 2 * M + np.abs(P - point), axis=1)
        dC = 5 * U * kappa * (np.linalg.norm(s[r1, j], axis=1) + 1.5 * L)
        err = dq + 3 * U * dist + np.minimum(dC, dC * dC / np.maximum(2 * dist, 1e-300))
    bary = np.stack([1.0 - uv[:, 0] - uv[:, 1], uv[:, 0], uv[:, 1]], 1)
    return dict(tri=np.where(hit, j, -1), dist=np.where(hit, dist, float(max_dist)), bary=np.where(hit[:, None], bary, 0.0),
                point=np.where(hit[:, None], point, 0.0), gap=np.where(hit, second - dist, np.inf), err32=np.where(hit, err, 0.0),
                kappa=np.where(hit, kappa, 1.0))


def walk32(vertices, triangles, order, points, max_dist=np.inf, stats=None):
    """csrc/closest.hip's query of the implicit tree over `order` -> closest32's outputs.  stats: cast_ref.tree_walk32's."""
    tree = C.build_tree(vertices, triangles, order)
    P = _f(points).reshape(-1, 3)
    n = P.shape[0]
    usable = np.isfinite(P).all(1)
    Pz = np.where(usable[:, None], P, F32(0))
    cap2 = cap2_of(max_dist)
    best_id, best_d2, best_w, best_c = np.full(n, -1, np.int64), np.full(n, INF), np.zeros((n, 3), F32), np.zeros((n, 3), F32)

    def node_test(q, node):
        lb = box_bound(tree['lo'][node], tree['hi'][node], Pz[q])
        with np.errstate(invalid='ignore'):
            return ~(lb > cap2) & ~(lb > best_d2[q]), lb

    def leaf_test(q, slot):
        ids = tree['rec_id'][slot]
        d2, w, c, _, _ = tri_rule(tree['rec_P'][slot], Pz[q])
        better = (ids >= 0) & (d2 <= cap2) & ((d2 < best_d2[q]) | ((d2 == best_d2[q]) & (ids < best_id[q])) | (best_id[q] < 0))
        qb = q[better]
        best_id[qb], best_d2[qb], best_w[qb], best_c[qb] = ids[better], d2[better], w[better], c[better]
        return best_id[q] >= 0

    C.tree_walk32(tree, usable, node_test, leaf_test, stats=stats)
    return _finish(P, usable, max_dist, best_id, best_d2, best_w, best_c)


# ---- scenes -----------------------------------------------------------------------------------------------------------------------
def near_points(vertices, triangles, n, seed, spread=0.2):
    """n points: three in four near a point of a triangle of the mesh (within `spread`), the others anywhere around the unit cube"""
    rng = np.random.default_rng(seed)
    P = (0.5 + 1.5 * (rng.random((n, 3)) - 0.5) * 2)
    T = np.asarray(triangles).reshape(-1, 3).shape[0]
    if T and n:
        V = _f(vertices).reshape(-1, 3)[np.asarray(triangles).reshape(-1, 3)[rng.integers(0, T, n)]].astype(np.float64)
        w = rng.dirichlet((1.0, 1.0, 1.0), n)
        near = (w[:, :, None] * V).sum(1) + spread * rng.normal(size=(n, 3)) * rng.random((n, 1))
        P = np.where((np.arange(n) % 4 != 3)[:, None], near, P)
    return P.astype(F32)


POINT_COUNTS = (0, 1, 255, 256, 257)
TRIANGLE_COUNTS = C.TRIANGLE_COUNTS + C.BUILD_EDGES      # 0, 1, 3, 4, 5, 7, 8, 9, 1023, 1024, 1025, 4097, 1028, 2048, 2049


@functools.lru_cache(maxsize=None)
def scenes():
    """the smallest shapes at which a query can go wrong -> {name: dict v, t, p, max_dist}; computed once, not to be written to"""
    S = {}

    def add(name, v, t, p, max_dist=np.inf):
        S[name] = dict(v=_f(v).reshape(-1, 3), t=np.asarray(t, np.int32).reshape(-1, 3), p=_f(p).reshape(-1, 3), max_dist=max_dist)
    for i, T in enumerate(TRIANGLE_COUNTS):
        v, t = C.random_soup(T, 100 + i, scale=0.6 if T < 16 else 0.15)
        add('soup_T%d' % T, v, t, near_points(v, t, 160 if T else 5, 300 + i), max_dist=np.inf if i % 2 else 0.25)
    v, t = C.random_soup(300, 31)
    for n in POINT_COUNTS:
        add('soup_T300_n%d' % n, v, t, near_points(v, t, n, 33))
    # 33 leaves: 33, 17, 9, 5, 3, 2, 1 nodes per level -- a missing sibling on five levels
    v, t = C.random_soup(131, 41, scale=0.4)
    add('siblings_T131', v, t, near_points(v, t, 200, 43))
    tri = np.asarray([(0, 0, 0), (1, 0, 0.25), (0, 1, 0.5)], F32)
    add('duplicates_300', tri, np.tile(np.asarray([[0, 1, 2]], np.int32), (300, 1)), near_points(tri, [[0, 1, 2]], 64, 51, spread=0.5))
    z1 = np.nextafter(F32(1), F32(2))
    zm = F32((np.float64(1) + np.float64(z1)) / 2)                           # rounds to one of the two: exactly between does not exist in fp32,
    sheet = lambda z: [(-4, -4, z), (4, -4, z), (0, 4, z)]                   # so "between" is each sheet's own height, where the other is one ulp off
    xy = np.random.default_rng(53).uniform(-1, 1, (30, 2))
    p = np.concatenate([np.concatenate([xy, np.full((30, 1), z)], 1) for z in (3.0, 0.5, 1.0, float(z1), float(zm), 1.0 + 3 * 2.0 ** -23, -3.0)])
    add('sheets_one_ulp', np.asarray(sheet(F32(1)) + sheet(z1), F32), [[3, 4, 5], [0, 1, 2]], p)
    # exactly on a vertex, on an edge, inside a triangle of the flat grid: dist 0 and the smallest incident id
    gv, gt = C.quad_grid(16)
    on = [(x, y, 0.0) for x in (0.0, 3.0, 8.0, 16.0) for y in (0.0, 4.0, 7.5, 16.0)] + [(2.5, 2.5, 0.0), (2.25, 2.5, 0.0), (9.75, 3.5, 0.0), (5.5, 5.0, 0.0)]
    off = [(x, y, z) for x, y, _ in on for z in (0.5, -2.0)] + [(-3.0, -3.0, 0.0), (20.0, 8.0, 1.0), (8.0, -1.0, 0.0)]
    add('grid_on_and_off', gv, gt, np.asarray(on + off, F32))
    # the medial plane of two triangles: x = 0 between mirror images
    left = np.asarray([(-1, 0, 0), (-1, 1, 0), (-1, 0, 1)], F32)
    right = left * F32([-1, 1, 1])
    rng = np.random.default_rng(57)
    medial = np.concatenate([np.zeros((40, 1)), rng.uniform(-1, 2, (40, 2))], 1)
    add('medial_plane', np.concatenate([right, left]), [[0, 1, 2], [3, 4, 5]], medial)
    dv_, dt_ = C.dirty_mesh()
    add('dirty', dv_, dt_, near_points(*C.random_soup(200, 5), 257, 61))
    nan, inf = np.nan, np.inf
    add('unusable_points', *C.quad_grid(2), [(nan, 0, 0), (0, inf, 0), (0, 0, -inf), (nan, nan, nan), (0.5, 0.5, 1.0)])
    sv, st = C.random_soup(60, 71, scale=0.5)
    far = np.random.default_rng(72).normal(size=(48, 3))
    add('far_away', sv, st, (far / np.linalg.norm(far, axis=1, keepdims=True) * 1.7e6 + 0.5).astype(F32))
    add('random_T5000_n3000', *C.random_soup(5000, 81, scale=0.08), near_points(*C.random_soup(5000, 81, scale=0.08), 3000, 82, spread=0.1))
    add('random_T5000_capped', *C.random_soup(5000, 81, scale=0.08), near_points(*C.random_soup(5000, 81, scale=0.08), 500, 83, spread=0.1), max_dist=0.02)
    return S


@functools.lru_cache(maxsize=None)
def expected(name):
    """closest32 of a scene, computed once and shared: (tri, dist, bary, point), not to be written to"""
    s = scenes()[name]
    return closest32(s['v'], s['t'], s['p'], s['max_dist'])


@functools.lru_cache(maxsize=None)
def cap_cases():
    """max_dist at a point's own dist and one ulp either side -> (v, t, p [48,3], dist0 [48], {name: max_dist [48]}): one query
    per point and bound, since max_dist is a scalar of the call"""
    v, t = C.random_soup(60, 71, scale=0.5)
    p = near_points(v, t, 48, 73, spread=0.4)
    d0 = closest32(v, t, p)[1]
    return v, t, p, d0, dict(below=np.nextafter(d0, F32(0)), at=d0.copy(), above=np.nextafter(d0, INF))


bits = C.bits
