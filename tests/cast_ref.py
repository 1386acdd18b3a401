"""The oracle of include/durf_cast.h in numpy.  cast32: brute force over rays x triangles in float32, every operation in the
header's order (numpy's float32 ufuncs round each operation once and fuse nothing).  cast64: the float64 twin without box rule
or clamp.  tree_walk32: csrc/cast_tree.h's implicit tree and its one walk, vectorised over queries; bvh32: the rays' box and
triangle rules on it -- by the header's proof it equals cast32 in every bit, which tests/test_cast_host.py exercises.  keys: the
Morton key rule.  Scenes shared by the tests."""
import functools

import numpy as np

from tests.trimesh_ref import box_mesh, dirty_mesh, icosphere, quad_grid, random_soup, valid_triangles  # noqa: F401  (the mesh and its scenes are trimesh_ref's)

F32 = np.float32
LEAF, STACK, KEY_BITS = 4, 32, 21
INF = F32(np.inf)


def _f(a):
    return np.ascontiguousarray(a, dtype=F32)


def tri_box(P):
    """P [...,3,3] -> (lo, hi) [...,3]: one ulp outward"""
    return np.nextafter(P.min(-2), -INF).astype(F32), np.nextafter(P.max(-2), INF).astype(F32)


def ray_setup(o, d, tmin, tmax):
    """-> dict o, d, inv, zero [n,3], tmin, tmax [n], usable [n]"""
    o, d = _f(o).reshape(-1, 3), _f(d).reshape(-1, 3)
    n = o.shape[0]
    tmin, tmax = np.broadcast_to(_f(tmin), (n,)).copy(), np.broadcast_to(_f(tmax), (n,)).copy()
    with np.errstate(all='ignore'):
        inv = F32(1.0) / d
        usable = np.isfinite(o).all(1) & np.isfinite(d).all(1) & ~(d == 0).all(1) & (tmin >= 0) & ~np.isnan(tmax)
    return dict(o=o, d=d, inv=inv, zero=(d == 0) | ~np.isfinite(inv), tmin=tmin, tmax=tmax, usable=usable)


def box_rule(lo, hi, o, inv, zero, tmin, tmax):
    """the box rule, broadcasting: lo, hi, o, inv, zero [...,3]; tmin, tmax [...] -> (passes, bn, bf)"""
    with np.errstate(all='ignore'):
        x1, x2 = (lo - o) * inv, (hi - o) * inv
        n, f = np.fmin(x1, x2), np.fmax(x1, x2)
        bn = np.where(zero, -INF, n).max(-1)
        bf = np.where(zero, INF, f).min(-1)
        zero_ok = (~zero | ((lo <= o) & (o <= hi))).all(-1)
        ok = ~(lo > hi).any(-1) & zero_ok & (bn <= bf) & (bf >= tmin) & (bn <= tmax)
    return ok, bn.astype(F32), bf.astype(F32)


def tri_rule(P, o, d, inv, zero, tmin, tmax, cull):
    """the triangle rule on valid triangles, broadcasting: P [...,3,3], the ray fields [...,3] and [...] ->
    (counts, t, u, v, w, det)"""
    ok, bn, bf = box_rule(*tri_box(P), o, inv, zero, tmin, tmax)
    with np.errstate(all='ignore'):
        A, B, C = P[..., 0, :], P[..., 1, :], P[..., 2, :]
        e1, e2 = B - A, C - A
        x = lambda a, i: a[..., i]
        cross = lambda a, b: (x(a, 1) * x(b, 2) - x(a, 2) * x(b, 1), x(a, 2) * x(b, 0) - x(a, 0) * x(b, 2), x(a, 0) * x(b, 1) - x(a, 1) * x(b, 0))
        dot = lambda a, c: (x(a, 0) * c[0] + x(a, 1) * c[1]) + x(a, 2) * c[2]
        p = cross(d, e2)
        det = dot(e1, p)
        invd = F32(1.0) / det
        ok = ok & (det != 0) & np.isfinite(invd)
        if cull == 1:
            ok = ok & ~(det < 0)
        elif cull == 2:
            ok = ok & ~(det > 0)
        s = o - A
        u = dot(s, p) * invd
        q = cross(s, e1)
        v = dot(d, q) * invd
        w = (F32(1.0) - u) - v
        t0 = dot(e2, q) * invd
        t = np.fmin(np.fmax(t0, bn), bf) + F32(0.0)
        ok = ok & (u >= 0) & (v >= 0) & (w >= 0) & ~np.isnan(t0) & (tmin <= t) & (t <= tmax)
    return ok, t, u, v, w, det


def _finish(R, best_id, best_t, best_b):
    n = R['usable'].shape[0]
    tri = np.where(R['usable'], best_id, -2).astype(np.int32)
    found = tri >= 0
    t = np.where(found, best_t, F32(0)).astype(F32)
    t[~R['usable']] = np.nan
    bary = np.where(found[:, None], best_b, F32(0)).astype(F32)
    bary[~R['usable']] = np.nan
    return tri, t, bary


def cast32(vertices, triangles, o, d, tmin=0.0, tmax=np.inf, cull=0, chunk=None):
    """-> (tri int32 [n], t float32 [n], bary float32 [n,3] = (w, u, v)): the definition, by brute force"""
    valid, P = valid_triangles(vertices, triangles)
    R = ray_setup(o, d, tmin, tmax)
    n, T = R['o'].shape[0], P.shape[0]
    ids = np.nonzero(valid)[0]
    Pv = P[ids]
    best_id, best_t, best_b = np.full(n, -1, np.int64), np.zeros(n, F32), np.zeros((n, 3), F32)
    chunk = chunk or max(1, (1 << 22) // max(len(ids), 1))
    for a in range(0, n, chunk):
        if not len(ids):
            break
        sl = slice(a, a + chunk)
        r = {k: R[k][sl] for k in R}
        ok, t, u, v, w, _ = tri_rule(Pv[None], r['o'][:, None], r['d'][:, None], r['inv'][:, None], r['zero'][:, None],
                                     r['tmin'][:, None], r['tmax'][:, None], cull)
        tt = np.where(ok, t, INF)
        tbest = tt.min(1)
        # the smallest id among the counting triangles whose t equals the minimum (ids ascend along the axis)
        j = np.argmax(ok & (tt == tbest[:, None]), axis=1)
        hit = ok.any(1)
        rows = np.arange(tt.shape[0])
        best_id[sl] = np.where(hit, ids[j], -1)
        best_t[sl] = np.where(hit, t[rows, j], 0)
        best_b[sl] = np.where(hit[:, None], np.stack([w[rows, j], u[rows, j], v[rows, j]], 1), 0)
    return _finish(R, best_id, best_t, best_b)


def cast64(vertices, triangles, o, d, tmin=0.0, tmax=np.inf, cull=0):
    """the float64 twin without box rule or clamp -> dict tri, t, bary (w, u, v), gap (the second smallest t minus the smallest,
    inf with fewer than two candidates), edge (the winner's smallest barycentric weight), cancel (|det| over the sum of the
    magnitudes of its six products: small when det is cancelled away), err32 (a first-order bound of the float32 formula's
    rounding error in t, in units of t) -- float64 [n]"""
    valid, P = valid_triangles(vertices, triangles)
    P = P.astype(np.float64)
    o, d = np.asarray(o, np.float64).reshape(-1, 3)[:, None], np.asarray(d, np.float64).reshape(-1, 3)[:, None]
    n = o.shape[0]
    tmin, tmax = (np.broadcast_to(np.asarray(b, np.float64), (n,))[:, None] for b in (tmin, tmax))
    with np.errstate(all='ignore'):
        A = P[None, :, 0]
        e1, e2 = P[None, :, 1] - A, P[None, :, 2] - A
        p = np.cross(d, e2)
        det = (e1 * p).sum(-1)
        s = o - A
        u = (s * p).sum(-1) / det
        q = np.cross(s, e1)
        v = (d * q).sum(-1) / det
        w = 1.0 - u - v
        t = (e2 * q).sum(-1) / det
        ok = valid[None] & (det != 0) & np.isfinite(1.0 / det) & (u >= 0) & (v >= 0) & (w >= 0) & (tmin <= t) & (t <= tmax)
        if cull:
            ok &= ~(det < 0) if cull == 1 else ~(det > 0)
        tt = np.where(ok, t, np.inf)
        order = np.argsort(tt, axis=1, kind='stable')[:, :2]
        rows = np.arange(n)
        j = order[:, 0]
        hit = ok[rows, j]
        second = tt[rows, order[:, 1]] if tt.shape[1] > 1 else np.full(n, np.inf)
        a3 = np.abs
        roll = lambda a, k: np.roll(a, k, -1)
        mag_det = (a3(e1) * (a3(roll(d, -1) * roll(e2, -2)) + a3(roll(d, -2) * roll(e2, -1)))).sum(-1)
        mag_num = (a3(e2) * (a3(roll(s, -1) * roll(e1, -2)) + a3(roll(s, -2) * roll(e1, -1)))).sum(-1)
        U = 2.0 ** -24
        err = (8 * U * mag_num + a3(t) * 8 * U * mag_det) / a3(det) + U * a3(t)
    pick = lambda a: a[rows, j]
    with np.errstate(all='ignore'):
        return dict(tri=np.where(hit, j, -1), t=np.where(hit, pick(t), 0.0), bary=np.where(hit[:, None], np.stack([pick(w), pick(u), pick(v)], 1), 0.0),
                gap=np.where(hit, second - pick(tt), np.inf), edge=np.where(hit, np.minimum(np.minimum(pick(u), pick(v)), pick(w)), np.inf),
                cancel=np.where(hit, a3(pick(det)) / np.maximum(pick(mag_det), 1e-300), np.inf), err32=np.where(hit, pick(err), 0.0))


# ---- the implicit tree ------------------------------------------------------------------------------------------------------------
def keys(vertices, triangles, bounds):
    """the Morton key rule -> int64 [T]"""
    valid, P = valid_triangles(vertices, triangles)
    b = _f(bounds).reshape(6)
    key = np.zeros(P.shape[0], np.uint64)
    with np.errstate(all='ignore'):
        for a in range(3):
            lo, ext = b[a], b[3 + a] - b[a]
            c = ((P[:, 0, a] + P[:, 1, a]) + P[:, 2, a]) / F32(3.0)
            x = ((c - lo) / ext) * F32(2097152.0)
            g = np.where(~(ext > 0) | ~(x >= 0), 0, np.where(x >= F32(2097151.0), 2097151, np.trunc(np.where(np.isfinite(x), x, 0)))).astype(np.uint64)
            for bit in range(KEY_BITS):
                key |= ((g >> np.uint64(bit)) & np.uint64(1)) << np.uint64(3 * bit + (2 - a))
    key = key.astype(np.int64)
    key[~valid] = np.iinfo(np.int64).max
    return key


def morton_order(vertices, triangles):
    """what cast.build does: bounds of all vertices, keys, a stable sort -> order int32 [T]"""
    v = _f(vertices).reshape(-1, 3)
    if v.shape[0] == 0:
        return np.zeros(np.asarray(triangles).reshape(-1, 3).shape[0], np.int32)
    with np.errstate(all='ignore'):
        b = np.concatenate([v.min(0), v.max(0)])
    return np.argsort(keys(vertices, triangles, b), kind='stable').astype(np.int32)


def build_tree(vertices, triangles, order):
    """-> dict T, K, n [K+1], off [K+1], lo, hi [nodes,3], rec_P [n0 LEAF,3,3], rec_id [n0 LEAF]; None-like (K = -1) for T = 0"""
    valid, P = valid_triangles(vertices, triangles)
    T = P.shape[0]
    if T == 0:
        return dict(T=0, K=-1)
    order = np.asarray(order, np.int64).reshape(T)
    n0 = (T + LEAF - 1) // LEAF
    ids = np.full(n0 * LEAF, -1, np.int64)
    ids[:T] = np.where((order >= 0) & (order < T), order, -1)
    ids[ids >= 0] = np.where(valid[ids[ids >= 0]], ids[ids >= 0], -1)
    rec_P = np.where((ids >= 0)[:, None, None], P[np.maximum(ids, 0)], F32(0))
    lo, hi = tri_box(rec_P)
    lo[ids < 0], hi[ids < 0] = INF, -INF
    los, his = [lo.reshape(n0, LEAF, 3).min(1)], [hi.reshape(n0, LEAF, 3).max(1)]
    while los[-1].shape[0] > 1:
        a, b = los[-1], his[-1]
        if a.shape[0] % 2:
            a, b = np.concatenate([a, np.full((1, 3), INF)]), np.concatenate([b, np.full((1, 3), -INF)])
        los.append(a.reshape(-1, 2, 3).min(1))
        his.append(b.reshape(-1, 2, 3).max(1))
    n = np.array([x.shape[0] for x in los])
    return dict(T=T, K=len(los) - 1, n=n, off=np.concatenate([[0], np.cumsum(n)[:-1]]), lo=np.concatenate(los).astype(F32),
                hi=np.concatenate(his).astype(F32), rec_P=rec_P.astype(F32), rec_id=ids)


def _depth(h):
    return np.frexp(h.astype(np.float64))[1].astype(np.int64) - 1


def tree_walk32(tree, usable, node_test, leaf_test, any_hit=False, stats=None):
    """csrc/cast_tree.h's walk of build_tree's tree, every usable query at its own pace; the caller keeps each query's best.
    node_test(q, node) -> (enter bool [m], key [m]): the box rule with the prune against the best of queries q at their nodes;
    leaf_test(q, slot) -> found bool [m]: the triangle rule on the records `slot`, after which it says which of q hold a winner.
    any_hit: a query that has found something is done with the leaf.  stats: a dict that receives nodes and leaves [n], the node
    boxes tested and the leaves entered per query."""
    n = usable.shape[0]
    n_nodes, n_leaves = np.zeros(n, np.int64), np.zeros(n, np.int64)

    def enter(q, node):
        n_nodes[q] += 1
        return node_test(q, node)

    if tree['T'] > 0:
        K, nk, off = tree['K'], tree['n'], tree['off']
        cur, sp, stack = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros((n, STACK), np.int64)
        us = np.nonzero(usable)[0]
        ok, _ = enter(us, np.full(len(us), off[K]))
        cur[us[ok]] = 1
        while (cur != 0).any():
            act = np.nonzero(cur != 0)[0]
            h = cur[act]
            depth = _depth(h)
            k = K - depth
            leaf = k == 0
            if leaf.any():
                q, l = act[leaf], h[leaf] - (1 << depth[leaf])
                n_leaves[q] += 1
                for j in range(LEAF):
                    found = leaf_test(q, l * LEAF + j)
                cur[q] = 0
                if any_hit:
                    sp[q[found]] = 0
            inner = ~leaf
            if inner.any():
                q, hh, dd, kk = act[inner], h[inner], depth[inner], k[inner]
                c0 = 2 * hh
                j0 = c0 - (2 << dd)
                nb, base = nk[kk - 1], off[kk - 1]
                p, key = [np.zeros(len(q), bool), np.zeros(len(q), bool)], [np.zeros(len(q), F32), np.zeros(len(q), F32)]
                for c in (0, 1):
                    ex = j0 + c < nb
                    p[c][ex], key[c][ex] = enter(q[ex], (base + j0 + c)[ex])
                both = p[0] & p[1]
                swap = key[1] < key[0]
                qb = q[both]
                stack[qb, sp[qb]] = np.where(swap, c0, c0 + 1)[both]
                sp[qb] += 1
                assert (sp <= STACK).all()
                cur[q] = np.where(both, np.where(swap, c0 + 1, c0), np.where(p[0], c0, np.where(p[1], c0 + 1, 0)))
            while True:
                pop = np.nonzero((cur == 0) & (sp > 0))[0]
                if not len(pop):
                    break
                sp[pop] -= 1
                hp = stack[pop, sp[pop]]
                dp = _depth(hp)
                ok, _ = enter(pop, off[K - dp] + hp - (1 << dp))
                cur[pop[ok]] = hp[ok]
    if stats is not None:
        stats.update(nodes=n_nodes, leaves=n_leaves)


def bvh32(vertices, triangles, order, o, d, tmin=0.0, tmax=np.inf, cull=0, any_hit=False, stats=None):
    """csrc/cast.hip's queries of the implicit tree over `order` -> cast32's outputs (any_hit: hit int32 [n]).  stats: tree_walk32's."""
    tree = build_tree(vertices, triangles, order)
    R = ray_setup(o, d, tmin, tmax)
    n = R['o'].shape[0]
    best_id, best_t, best_b = np.full(n, -1, np.int64), np.full(n, INF), np.zeros((n, 3), F32)
    ray = lambda rays: (R['o'][rays], R['inv'][rays], R['zero'][rays], R['tmin'][rays], R['tmax'][rays])

    def node_test(rays, node):
        ok, bn, _ = box_rule(tree['lo'][node], tree['hi'][node], *ray(rays))
        return (ok if any_hit else ok & ~(bn > best_t[rays])), bn

    def leaf_test(rays, slot):
        ids = tree['rec_id'][slot]
        o_, *rest = ray(rays)
        okt, t, u, v, w, _ = tri_rule(tree['rec_P'][slot], o_, R['d'][rays], *rest, cull)
        better = okt & (ids >= 0) & ((t < best_t[rays]) | ((t == best_t[rays]) & (ids < best_id[rays])) | (best_id[rays] < 0))
        rb = rays[better]
        best_id[rb], best_t[rb], best_b[rb] = ids[better], t[better], np.stack([w, u, v], 1)[better]
        return best_id[rays] >= 0

    tree_walk32(tree, R['usable'], node_test, leaf_test, any_hit, stats)
    best_t = np.where(best_id >= 0, best_t, F32(0))
    tri, t, bary = _finish(R, best_id, best_t, best_b)
    if any_hit:
        return np.where(tri >= 0, 1, np.where(tri == -2, -2, 0)).astype(np.int32)
    return tri, t, bary


# ---- scenes (the meshes themselves: trimesh_ref) --------------------------------------------------------------------------------
def random_rays(n, seed, centre=0.5, spread=1.5):
    """origins around the unit cube, directions towards points inside it: not unit length"""
    rng = np.random.default_rng(seed)
    o = centre + spread * (rng.random((n, 3)) - 0.5) * 2
    d = rng.random((n, 3)) - o
    return o.astype(F32), d.astype(F32)


def aimed_rays(vertices, triangles, n, seed):
    """n rays from around the unit cube, three in four of them through a point inside a triangle of the mesh (the others at
    random: some find nothing); random_rays when there is no triangle"""
    o, d = random_rays(n, seed)
    T = np.asarray(triangles).reshape(-1, 3).shape[0]
    if T and n:
        rng = np.random.default_rng(seed + 1000)
        P = _f(vertices).reshape(-1, 3)[np.asarray(triangles).reshape(-1, 3)[rng.integers(0, T, n)]].astype(np.float64)
        w = rng.dirichlet((2.0, 2.0, 2.0), n)
        aim = ((w[:, :, None] * P).sum(1) - o) * rng.uniform(0.3, 1.7, (n, 1))   # the hit is not at t = 1
        d = np.where((np.arange(n) % 4 != 3)[:, None], aim, d).astype(F32)
    return o, d


def grid_rays():
    """rays against quad_grid(16): through vertices, along edges, grazing, origins on the plane and on box faces, one and two
    zero components, subnormal components"""
    o, d = [], []
    for x in (0.0, 3.0, 7.5, 16.0):
        for y in (0.0, 4.0, 8.25, 16.0):
            o.append((x, y, 2.0)), d.append((0.0, 0.0, -1.0))               # straight down: two zero components, vertices and edges
            o.append((x, y, 0.0)), d.append((0.0, 0.0, -1.0))               # the origin on the plane
            o.append((x, y, -1.0)), d.append((0.0, 0.0, 0.5))               # from below
            o.append((x - 1.0, y, 1.0)), d.append((1.0, 0.0, -1.0))         # one zero component, onto a vertex or an edge
            o.append((x, y - 2.0, 1e-3)), d.append((0.25, 4.0, -1e-3))      # grazing
            o.append((x, y, 1.0)), d.append((1e-42, -1e-41, -1.0))          # subnormal components
            o.append((x, y, 1.0)), d.append((0.0, 1e-39, -3.0))
    o.append((-1.0, 3.0, 0.0)), d.append((1.0, 0.0, 0.0))                   # in the plane, along an edge
    o.append((-1.0, 3.5, 0.0)), d.append((1.0, 0.25, 0.0))                  # in the plane, across
    o.append((2.0, 2.0, np.nextafter(F32(0), F32(1)))), d.append((0.5, 0.5, 0.0))
    return np.asarray(o, F32), np.asarray(d, F32)


def bad_rays():
    """NaN and infinite rays, a zero direction, a negative tmin, a NaN tmax -> (o, d, tmin, tmax)"""
    nan, inf = np.nan, np.inf
    o = [(nan, 0, 0), (0, 0, 2), (inf, 0, 0), (0, 0, 2), (0, 0, 2), (0, 0, 2), (0, 0, 2), (0.2, 0.2, 2)]
    d = [(0, 0, -1), (0, nan, -1), (0, 0, -1), (0, -inf, -1), (0, 0, 0), (0, 0, -1), (0, 0, -1), (0, 0, -1)]
    return np.asarray(o, F32), np.asarray(d, F32), np.asarray([0, 0, 0, 0, 0, -1, 0, 0], F32), np.asarray([inf, inf, inf, inf, inf, inf, nan, inf], F32)


RAY_COUNTS = (0, 1, 63, 64, 65, 255, 256, 257)
TRIANGLE_COUNTS = (0, 1, 3, 4, 5, 7, 8, 9, 1023, 1024, 1025, 4097)       # the leaf, level and workgroup edges of the build
BUILD_EDGES = (1028, 2048, 2049)     # 257 leaves: the first level k_cast_level builds; 512 leaves: the fullest level k_cast_top reads; 513


@functools.lru_cache(maxsize=None)
def scenes():
    """the smallest shapes at which a cast can go wrong -> {name: dict v, t, o, d, tmin, tmax, cull}; computed once, not to be
    written to"""
    S = {}

    def add(name, v, t, o, d, tmin=0.0, tmax=np.inf, cull=0):
        S[name] = dict(v=_f(v).reshape(-1, 3), t=np.asarray(t, np.int32).reshape(-1, 3), o=_f(o), d=_f(d), tmin=tmin, tmax=tmax, cull=cull)
    for i, T in enumerate(TRIANGLE_COUNTS + BUILD_EDGES):                   # every count with rays that hit it (T = 0: that find nothing)
        v, t = random_soup(T, 100 + i, scale=0.6 if T < 16 else 0.15)
        add('soup_T%d' % T, v, t, *aimed_rays(v, t, 192 if T else 5, 200 + i))
    v, t = random_soup(300, 31)
    for n in RAY_COUNTS:                                                     # every ray count against one fixed mesh
        add('soup_T300_n%d' % n, v, t, *aimed_rays(v, t, n, 32))
    # 33 leaves: 33, 17, 9, 5, 3, 2, 1 nodes per level -- a missing sibling on five levels
    add('siblings_T131', *random_soup(131, 41, scale=0.4), *random_rays(200, 42))
    go, gd = grid_rays()
    for cull in (0, 1, 2):
        add('grid_cull%d' % cull, *quad_grid(16), go, gd, cull=cull)
    tri = np.asarray([(0, 0, 0), (1, 0, 0.25), (0, 1, 0.5)], F32)
    o, d = random_rays(64, 51, centre=0.3, spread=0.8)
    add('duplicates_300', tri, np.tile(np.asarray([[0, 1, 2]], np.int32), (300, 1)), o, np.asarray([0.3, 0.3, 0.2], F32) - o + 0.2 * (random_rays(64, 52)[1]))
    z1 = np.nextafter(F32(1), F32(2))
    sheet = lambda z: [(-4, -4, z), (4, -4, z), (0, 4, z)]
    o = np.concatenate([random_rays(40, 53)[0] * F32(0.5) + F32([0, 0, 3]), random_rays(40, 54)[0] * F32(0.5) - F32([0, 0, 3])])
    add('sheets_one_ulp', np.asarray(sheet(F32(1)) + sheet(z1), F32), [[3, 4, 5], [0, 1, 2]], o, random_rays(80, 55)[1] * F32(0.3) - o)
    add('dirty', *dirty_mesh(), *random_rays(257, 61))
    v, t = random_soup(60, 71, scale=0.5)
    o, d = random_rays(48, 72)
    _, t0, _ = cast32(v, t, o, d)
    t0 = np.where(t0 > 0, t0, F32(0.5))
    lo, hi = np.nextafter(t0, F32(0)), np.nextafter(t0, INF)
    zero, inf = np.zeros_like(t0), np.full_like(t0, INF)
    add('bounds_at_t', v, t, np.tile(o, (6, 1)), np.tile(d, (6, 1)), np.concatenate([lo, t0, hi, zero, zero, zero]),
        np.concatenate([inf, inf, inf, lo, t0, hi]))
    bo, bd, btmin, btmax = bad_rays()
    add('bad_rays', *quad_grid(2), bo, bd, btmin, btmax)
    add('random_T5000_n3000', *random_soup(5000, 81, scale=0.08), *random_rays(3000, 82))
    return S


@functools.lru_cache(maxsize=None)
def expected(name):
    """cast32 of a scene, computed once and shared: (tri, t, bary), not to be written to"""
    s = scenes()[name]
    return cast32(s['v'], s['t'], s['o'], s['d'], s['tmin'], s['tmax'], s['cull'])


def bits(a):
    """the int32 bits of a float32 array (an int32 array as it is): equality of these is equality in every bit, NaN included"""
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a.astype(np.int32)


def pinhole32(cam, h, w):
    """csrc/camera.h's pinhole_ray in float32 for every pixel of one camera row -> (origins, directions) [h w, 3], row-major"""
    cam = _f(cam).reshape(-1)
    y, x = (a.reshape(-1).astype(F32) for a in np.meshgrid(np.arange(h), np.arange(w), indexing='ij'))
    cd = ((x - cam[13]) / cam[12], -(y - cam[14]) / cam[12], np.full(h * w, F32(-1.0)))
    d = np.stack([(cd[0] * cam[4 * a] + cd[1] * cam[4 * a + 1]) + cd[2] * cam[4 * a + 2] for a in range(3)], 1)
    return np.tile(cam[[3, 7, 11]], (h * w, 1)).astype(F32), d.astype(F32)


def rasteriser_comparison(rast, cst, rast64, c64, tris, judged=None, edge=None):
    """the rule under which a cast picture and a raster picture of the same cameras agree (tests/test_gpu_cast.py; tools/time_cast.py applies it to windows of its pictures).
    rast, cst: dict tri, depth (float32); rast64: raster_ref.draw64's; c64: cast_ref.cast64's, reshaped.
    -> dict same (pixels naming one triangle), differ, twin_differ, worst (the largest depth difference beyond the float64
    twins' own, in units of 2^-24 depth) or an AssertionError.  judged: a bool mask of the pixels the rule is applied to (default: all).  edge: the float64 cast's smallest barycentric weight
    per pixel, for scenes where a surface hides another: rule 2 then also admits a pixel whose ray passes within a hundredth of
    the winner's outline (a silhouette against whatever lies behind it, not against nothing)"""
    U = 2.0 ** -24
    judged = np.ones(cst['tri'].shape, bool) if judged is None else judged
    same = (rast['tri'] == cst['tri']) & (cst['tri'] >= 0) & judged
    differ = (rast['tri'] != cst['tri']) & judged
    twin_same = same & (rast64['tri'] == rast['tri']) & (c64['tri'] == cst['tri'])
    twin_differ = (rast64['tri'] != c64['tri']) & judged
    # 1 where all four name one triangle, the two float32 depths differ by no more than their float64 twins do (the
    #   rasteriser snaps vertices to 1/256 pixel and interpolates 1/z, the cast intersects the unsnapped triangle: a
    #   difference of geometry, the same in either precision) plus 64 roundings of 2^-24 depth for the two float32 formulas
    dr, dc = rast['depth'].astype(np.float64), cst['depth'].astype(np.float64)
    excess = (np.abs(dr - dc) - np.abs(rast64['depth'] - c64['depth'])) / (U * np.maximum(dc, 1e-30))
    worst = float(excess[twin_same].max()) if twin_same.any() else 0.0
    assert worst <= 64.0, worst
    # 2 the pixels where the two name different triangles are silhouette pixels (one of the two sees nothing) or shared-edge
    #   pixels (the two triangles share two vertices)
    for f, y, x in np.argwhere(differ):
        a, c = int(rast['tri'][f, y, x]), int(cst['tri'][f, y, x])
        assert a < 0 or c < 0 or len(set(tris[a].tolist()) & set(tris[c].tolist())) >= 2 or (edge is not None and edge[f, y, x] < 1e-2), (f, y, x, a, c)
    # 3 and they are no more than twice those of the float64 twins (the snap moves an edge by up to 1/512 pixel in either
    #   precision; float32 adds pixels whose centre lies within rounding of an edge), plus four
    assert int(differ.sum()) <= 2 * int(twin_differ.sum()) + 4, (int(differ.sum()), int(twin_differ.sum()))
    return dict(same=int(same.sum()), differ=int(differ.sum()), twin_differ=int(twin_differ.sum()), worst=worst)
