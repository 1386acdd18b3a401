"""The definitions of include/durf_smooth.h restated in numpy: the keys, the two CSR structures (np.unique on the keys), the
vertex class, the census, one smoothing step (a float32 sequential sum written as a loop over the degree with masked adds, and a
float64 twin), Taubin as a sequence of steps, and the area-weighted vertex normals (float32 and float64).  Every float32 result
is what the device must give bit for bit.  Meshes for the tests stand at the end."""
import numpy as np

from tests.trimesh_ref import icosphere, quad_grid  # noqa: F401

NO_KEY = np.int64(0x7fffffffffffffff)
ISOLATED, INTERIOR, BOUNDARY, NONMANIFOLD = 0, 1, 2, 3
PIN, SLIDE = 0, 1


def contributing(triangles, V):
    t = np.asarray(triangles, np.int64).reshape(-1, 3)
    ok = ((t >= 0) & (t < V)).all(1)
    return ok & (t[:, 0] != t[:, 1]) & (t[:, 1] != t[:, 2]) & (t[:, 2] != t[:, 0])


def keys(triangles, V):
    """-> (edge_keys int64 [6T], corner_keys int64 [3T]) in the header's order, unsorted"""
    t = np.asarray(triangles, np.int64).reshape(-1, 3)
    T, ok = t.shape[0], contributing(triangles, V)
    ek, ck = np.full((T, 6), NO_KEY, np.int64), np.full((T, 3), NO_KEY, np.int64)
    tt = np.arange(T, dtype=np.int64)
    for c in range(3):
        p, q = t[:, c], t[:, (c + 1) % 3]
        ek[ok, 2 * c] = ((p << 32) | q)[ok]
        ek[ok, 2 * c + 1] = ((q << 32) | p)[ok]
        ck[ok, c] = ((p << 32) | tt)[ok]
    return ek.reshape(-1), ck.reshape(-1)


def csr(sorted_or_not_keys, V):
    """the unique keys below the sentinel, split by their high word -> (offsets int32 [V+1], low int32 [U], multiplicity int32 [U])"""
    k = np.asarray(sorted_or_not_keys, np.int64)
    u, m = np.unique(k[k != NO_KEY], return_counts=True)
    offsets = np.searchsorted(u, np.arange(V + 1, dtype=np.int64) << 32, side='left').astype(np.int32)
    return offsets, (u & 0xffffffff).astype(np.int32), m.astype(np.int32)


def classes(offsets, multiplicity):
    V = offsets.size - 1
    cls = np.zeros(V, np.uint8)
    rows = np.flatnonzero(np.diff(offsets) > 0)
    if rows.size:
        at = offsets[rows].astype(np.int64)
        many = np.add.reduceat((multiplicity > 2).astype(np.int64), at) > 0
        one = np.add.reduceat((multiplicity == 1).astype(np.int64), at) > 0
        cls[rows] = np.where(many, NONMANIFOLD, np.where(one, BOUNDARY, INTERIOR))
    return cls


def adjacency(vertices, triangles):
    """-> the dict durf_amd.smooth.adjacency returns, as host arrays (neighbours, multiplicity and corner_tri cut to what is written)"""
    v = np.asarray(vertices, np.float32).reshape(-1, 3)
    t = np.asarray(triangles, np.int32).reshape(-1, 3)
    V = v.shape[0]
    ek, ck = keys(t, V)
    offsets, nb, mult = csr(ek, V)
    coff, ctri, _ = csr(ck, V)
    return dict(vertices=v, triangles=t, V=V, T=t.shape[0], edge_keys=ek, corner_keys=ck, offsets=offsets, neighbours=nb, multiplicity=mult,
                corner_offsets=coff, corner_tri=ctri, vertex_class=classes(offsets, mult))


def census(adj):
    """-> int32 [8] in the header's order"""
    off, nb, mult, cls = adj['offsets'], adj['neighbours'], adj['multiplicity'], adj['vertex_class']
    V = off.size - 1
    row = np.repeat(np.arange(V), np.diff(off))
    once = nb > row
    return np.array([(cls == c).sum() for c in range(4)] + [adj['corner_offsets'][V] // 3, off[V] // 2, (once & (mult == 1)).sum(),
                                                           (once & (mult > 2)).sum()], np.int32)


def derive(c, V):
    """what the host derives from the census -> (closed, euler)"""
    return bool(c[6] == 0 and c[7] == 0), int(V - c[0]) - int(c[5]) + int(c[4])


def _padded_rows(adj, x, boundary):
    """the rows as [V,D] with a mask: neighbour ids, whether each entry counts"""
    off, nb, mult, cls = adj['offsets'], adj['neighbours'], adj['multiplicity'], adj['vertex_class']
    V = off.size - 1
    deg = np.diff(off).astype(np.int64)
    D = int(deg.max()) if V and deg.size and deg.max() > 0 else 0
    col = np.arange(D)[None, :]
    inside = col < deg[:, None]
    idx = np.where(inside, off[:-1, None].astype(np.int64) + col, 0)
    j = np.where(inside, nb[idx] if nb.size else 0, 0)
    m = np.where(inside, mult[idx] if mult.size else 0, 0)
    finite = np.isfinite(x).all(1)
    interior = (cls == INTERIOR)[:, None]
    slide = ((cls == BOUNDARY) & (boundary == SLIDE))[:, None]
    counts = inside & finite[j] & (interior | (slide & (m == 1)))
    return j, counts


def step(adj, x, factor, boundary=PIN, fixed=None, dt=np.float32, operands=False):
    """one step in dt (float32: the device's bits; float64: the twin), the sum a loop over the degree with masked adds.
    operands: also return, per vertex and axis, the largest magnitude among the step's operands (the vertex, every partial sum,
    the mean and the displacement)"""
    x32 = np.asarray(x, np.float32).reshape(-1, 3)
    V = x32.shape[0]
    xin = x32.astype(dt)
    j, counts = _padded_rows(adj, x32, boundary)
    free = np.isfinite(x32).all(1)
    if fixed is not None:
        free &= np.asarray(fixed).reshape(V) == 0
    counts = counts & free[:, None]
    n = np.zeros(V, np.int64)
    s = np.zeros((V, 3), dt)
    with np.errstate(all='ignore'):
        big = np.where(np.isfinite(xin), np.abs(xin), 0)
        for k in range(j.shape[1]):
            c = counts[:, k]
            y = xin[j[:, k]]
            first = (c & (n == 0))[:, None]
            s = np.where(first, y, np.where(c[:, None], s + y, s))
            big = np.maximum(big, np.abs(s))
            n += c
        moved = n > 0
        m = s / np.maximum(n, 1).astype(dt)[:, None]
        out = xin + dt(factor) * (m - xin)
        big = np.maximum(big, np.where(moved[:, None], np.abs(m - xin), 0))
    if operands:
        return (np.where(moved[:, None], out, xin), big) if dt != np.float32 else (None, big)
    if dt == np.float32:
        res = x32.copy()                                                     # pinned: the bits as they are
        res[moved] = out[moved]
        return res
    return np.where(moved[:, None], out, xin)


def taubin(adj, x, iters, lam, mu, boundary=PIN, fixed=None, dt=np.float32):
    """the sequence of steps: lam, mu, lam, mu ...; mu == 0: lam alone.  (float64: the state stays float64 between steps)"""
    y = np.asarray(x, np.float32).reshape(-1, 3)
    if dt != np.float32:
        raise ValueError('the float64 twin is per step: use step(..., dt=np.float64)')
    for _ in range(iters):
        y = step(adj, y, lam, boundary, fixed)
        if np.float32(mu) != 0:
            y = step(adj, y, mu, boundary, fixed)
    return y.copy()


def normals(adj, x, dt=np.float32):
    """area-weighted vertex normals over the corner rows in ascending triangle id"""
    x32 = np.asarray(x, np.float32).reshape(-1, 3)
    V = x32.shape[0]
    if V == 0:
        return np.zeros((0, 3), dt)
    xx = x32.astype(dt)
    t = np.asarray(adj['triangles'], np.int64).reshape(-1, 3)
    coff, ctri = adj['corner_offsets'], adj['corner_tri']
    with np.errstate(all='ignore'):
        if t.shape[0]:
            tc = np.clip(t, 0, max(V - 1, 0))
            A, B, C = xx[tc[:, 0]], xx[tc[:, 1]], xx[tc[:, 2]]
            e1, e2 = B - A, C - A
            N = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                          e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], 1).astype(dt)
            good = np.isfinite(x32[tc]).all((1, 2)) & ((t >= 0) & (t < V)).all(1)
        else:
            N, good = np.zeros((0, 3), dt), np.zeros(0, bool)
        deg = np.diff(coff).astype(np.int64)
        D = int(deg.max()) if V and deg.max() > 0 else 0
        S, n = np.zeros((V, 3), dt), np.zeros(V, np.int64)
        for k in range(D):
            inside = k < deg
            tk = np.where(inside, ctri[np.where(inside, coff[:-1].astype(np.int64) + k, 0)] if ctri.size else 0, 0)
            c = inside & (good[tk] if good.size else False)
            y = N[tk] if N.shape[0] else np.zeros((V, 3), dt)
            first = (c & (n == 0))[:, None]
            S = np.where(first, y, np.where(c[:, None], S + y, S))
            n += c
        len2 = (S[:, 0] * S[:, 0] + S[:, 1] * S[:, 1]) + S[:, 2] * S[:, 2]
        flat = (n == 0) | ~(len2 > 0) | ~np.isfinite(len2)
        inv = dt(1.0) / np.sqrt(np.where(flat, dt(1.0), len2)).astype(dt)
        out = np.where(flat[:, None], dt(0.0), S * inv[:, None]).astype(dt)
    return out


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- brute force, for the oracle's own test ---------------------------------------------------------------------------------------
def brute_adjacency(triangles, V):
    """sets and dicts, no keys -> (rows: per vertex a sorted list of (neighbour, multiplicity); corner rows: sorted triangle ids)"""
    count, corners = {}, [set() for _ in range(V)]
    for ti, (a, b, c) in enumerate(np.asarray(triangles, np.int64).reshape(-1, 3).tolist()):
        if min(a, b, c) < 0 or max(a, b, c) >= V or a == b or b == c or c == a:
            continue
        for p, q in ((a, b), (b, c), (c, a)):
            count[(p, q)] = count.get((p, q), 0) + 1
            count[(q, p)] = count.get((q, p), 0) + 1
        for p in (a, b, c):
            corners[p].add(ti)
    rows = [[] for _ in range(V)]
    for (p, q), m in sorted(count.items()):
        rows[p].append((q, m))
    return rows, [sorted(s) for s in corners]


# ---- meshes -------------------------------------------------------------------------------------------------------------------------
def _mesh(v, t):
    return np.asarray(v, np.float32).reshape(-1, 3), np.asarray(t, np.int32).reshape(-1, 3)


def tetrahedron():
    return _mesh([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], [[0, 2, 1], [0, 1, 3], [1, 2, 3], [0, 3, 2]])


def quad():
    return _mesh([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]], [[0, 1, 2], [0, 2, 3]])


def book():
    """three triangles on the edge {0,1}: one non-manifold edge"""
    return _mesh([[0, 0, 0], [0, 0, 1], [1, 0, 0], [-1, 1, 0], [-1, -1, 0]], [[0, 1, 2], [0, 1, 3], [0, 1, 4]])


def duplicate():
    """a tetrahedron with one triangle twice: its three edges have multiplicity 3"""
    v, t = tetrahedron()
    return v, np.concatenate([t, t[:1]])


def bad_indices():
    """a quad grid plus triangles with a repeated index, an index of -1 and an index of V: none of the three contributes"""
    v, t = quad_grid(3)
    V = v.shape[0]
    return _mesh(v, np.concatenate([t[:5], [[1, 1, 2]], t[5:9], [[-1, 0, 1]], t[9:], [[0, 1, V]], [[2, 3, 2]]]))


def not_finite():
    """an icosphere with a NaN vertex and an infinite vertex: pinned as vertices, skipped as neighbours"""
    v, t = icosphere(1)
    v = v.copy()
    v[5, 1] = np.nan
    v[17, 0] = np.inf
    v[30] = [-np.inf, np.nan, 0.0]
    return v, t


def fan(n=300):
    """a closed fan of n triangles round vertex 0: degree n, above a wave and above a workgroup's share"""
    a = np.arange(n) * (2 * np.pi / n)
    v = np.concatenate([[[0.0, 0.0, 0.3]], np.stack([np.cos(a), np.sin(a), 0 * a], 1)])
    i = np.arange(n)
    return _mesh(v, np.stack([0 * i, 1 + i, 1 + (i + 1) % n], 1))


def soup(V, T, seed):
    """random vertices and a random index soup (indices in -1 .. V: some bad, some repeated)"""
    rng = np.random.default_rng(seed)
    return _mesh(rng.uniform(-1, 1, (V, 3)), rng.integers(-1, V + 1, (T, 3)))


def strip(T, seed):
    """a triangle strip of T triangles with jittered vertices, its triangles in a random order"""
    rng = np.random.default_rng(seed)
    V = T + 2
    i = np.arange(V)
    v = np.stack([i // 2 * 0.5, (i % 2) * 1.0, 0 * i], 1) + rng.uniform(-0.1, 0.1, (V, 3))
    k = np.arange(T)
    t = np.where((k % 2 == 0)[:, None], np.stack([k, k + 1, k + 2], 1), np.stack([k + 1, k, k + 2], 1))
    return _mesh(v, t[rng.permutation(T)])


def noisy_icosphere(level, seed, amp=0.03):
    """the unit icosphere with radial noise -> (v, t)"""
    v, t = icosphere(level)
    r = 1.0 + amp * np.random.default_rng(seed).standard_normal(v.shape[0])
    return (v.astype(np.float64) * r[:, None]).astype(np.float32), t


def rms_radial(v):
    r = np.linalg.norm(np.asarray(v, np.float64), axis=1)
    return float(np.sqrt(((r - r.mean()) ** 2).mean()))


def volume(v, t):
    X, tri = np.asarray(v, np.float64), np.asarray(t, np.int64)
    return float((X[tri[:, 0]] * np.cross(X[tri[:, 1]], X[tri[:, 2]])).sum() / 6.0)
