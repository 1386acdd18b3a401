"""The triangle mesh of the oracles in numpy (csrc/triangles.h and csrc/durf_common.h's rgb8 are the device side):
which triangle is readable, the attribute interpolation and the 8-bit pack, each stated once for cast_ref, closest_ref, shade_ref
and the raster tests, and the scene builders they share.  The modules that held these before re-export them."""
import numpy as np

F32 = np.float32


def _f(a):
    return np.ascontiguousarray(a, dtype=F32)


def valid_triangles(vertices, triangles):
    """-> (valid [T] bool, P [T,3,3] float32: the vertices of the valid triangles, 0 for the others)"""
    v, t = _f(vertices).reshape(-1, 3), np.asarray(triangles, np.int64).reshape(-1, 3)
    ok = ((t >= 0) & (t < v.shape[0])).all(1)
    P = np.zeros((t.shape[0], 3, 3), F32)
    if ok.any():
        P[ok] = v[t[ok]]
    ok &= np.isfinite(P).all((1, 2))
    P[~ok] = 0
    return ok, P


def interp32(triangles, tri, bary, attr):
    """durf_raster_interp's rule on a per-vertex attr [V,C]: (q0 a0 + q1 a1) + q2 a2, 0 where the sample names no triangle whose
    indices lie in 0 .. V-1"""
    t, tri, attr = np.asarray(triangles, np.int64).reshape(-1, 3), np.asarray(tri, np.int64).reshape(-1), _f(attr)
    n, V = tri.shape[0], attr.shape[0]
    hit = (tri >= 0) & (tri < t.shape[0])
    v = t[np.where(hit, tri, 0)] if t.shape[0] else np.zeros((n, 3), np.int64)
    hit &= ((v >= 0) & (v < V)).all(1)
    v = np.where(hit[:, None], v, 0)
    q = np.where(hit[:, None], _f(bary).reshape(n, 3), F32(0))
    with np.errstate(all='ignore'):
        a = (q[:, 0:1] * attr[v[:, 0]] + q[:, 1:2] * attr[v[:, 1]]) + q[:, 2:3] * attr[v[:, 2]]
    return np.where(hit[:, None], a, F32(0)).astype(F32)


def u8(x):
    """rgb8's rule: round-half-even of clamp(x, 0, 1) * 255, 0 for a NaN"""
    x = _f(x)
    with np.errstate(all='ignore'):
        c = np.where(np.isnan(x), F32(0), np.fmin(np.fmax(x, F32(0)), F32(1)))
        return np.rint(c * F32(255.0)).astype(np.uint8)


# ---- scenes -----------------------------------------------------------------------------------------------------------------------
def icosphere(level=2, radius=1.0, centre=(0.0, 0.0, 0.0)):
    """a closed, outward-facing (counter-clockwise from outside) icosphere -> (vertices float32 [V,3], triangles int32 [T,3])"""
    g = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g), (g, 0, -1), (g, 0, 1), (-g, 0, -1), (-g, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.asarray(x, np.float64) / np.linalg.norm(x) for x in v]
    for _ in range(level):
        mid, nf = {}, []

        def m(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                x = v[a] + v[b]
                v.append(x / np.linalg.norm(x))
                mid[key] = len(v) - 1
            return mid[key]
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return (np.asarray(v) * radius + np.asarray(centre)).astype(F32), np.asarray(f, np.int32)


def quad_grid(n=16, z=0.0):
    """n x n axis-aligned unit quads in the plane z (flat boxes), two triangles each, normals +z"""
    xs = np.arange(n + 1, dtype=F32)
    v = np.stack(list(np.meshgrid(xs, xs, indexing='ij')) + [np.full((n + 1, n + 1), z, F32)], -1).reshape(-1, 3)
    i, j = (a.reshape(-1) for a in np.meshgrid(np.arange(n), np.arange(n), indexing='ij'))
    a, b, c, d = i * (n + 1) + j, (i + 1) * (n + 1) + j, (i + 1) * (n + 1) + j + 1, i * (n + 1) + j + 1
    return v.astype(F32), np.concatenate([np.stack([a, b, c], 1), np.stack([a, c, d], 1)]).astype(np.int32)


def box_mesh(lo, hi):
    """the closed box [lo, hi] as 12 triangles, outward-facing"""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    v = np.asarray([[(lo, hi)[i >> a & 1][a] for a in range(3)] for i in range(8)], F32)      # bit a of i: the high side of axis a
    q = [(0, 2, 6, 4), (1, 5, 7, 3), (0, 4, 5, 1), (2, 3, 7, 6), (0, 1, 3, 2), (4, 6, 7, 5)]   # -x +x -y +y -z +z
    return v, np.asarray([t for a, b, c, d in q for t in ((a, c, b), (a, d, c))], np.int32)


def random_soup(T, seed, scale=0.15):
    """T small random triangles in the unit cube, no shared vertices"""
    rng = np.random.default_rng(seed)
    c = rng.random((T, 1, 3))
    return (c + scale * (rng.random((T, 3, 3)) - 0.5)).reshape(-1, 3).astype(F32), np.arange(3 * T, dtype=np.int32).reshape(T, 3)


def dirty_mesh(seed=5):
    """a valid soup with degenerate triangles, out-of-range indices and non-finite vertices mixed in"""
    v, t = random_soup(200, seed)
    v, t = v.copy(), t.copy()
    t[3] = (t[3, 0], t[3, 0], t[3, 1])                                      # degenerate: two equal vertices
    v[3 * 7 + 1] = v[3 * 7]                                                 # degenerate: two coincident vertices
    t[11, 2] = -1
    t[12, 0] = v.shape[0]
    t[13, 1] = 2 ** 31 - 1
    v[3 * 20, 1] = np.nan
    v[3 * 21 + 2, 0] = np.inf
    v[3 * 22 + 1, 2] = -np.inf
    return v, t


def merge(*meshes):
    """(v, t) pairs as one mesh, the triangle indices offset"""
    vs, ts, off = [], [], 0
    for v, t in meshes:
        vs.append(_f(v).reshape(-1, 3)), ts.append(np.asarray(t, np.int32).reshape(-1, 3) + off)
        off += vs[-1].shape[0]
    return np.concatenate(vs), np.concatenate(ts)
