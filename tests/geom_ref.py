"""Brute-force references of include/durf_geom.h in numpy, with no grid: every query against every reference point.

nearest32: the header's arithmetic in np.float32 (numpy does not fuse): dx = qx - rx, d2 = (dx dx + dy dy) + dz dz, a candidate
counts when d2 <= max_dist * max_dist (fp32), the smallest d2 wins and among equals the smallest index -- what the kernel must
give bit for bit.  nearest64: the same search in float64, with the runner-up, to say where fp32 may legitimately differ.
The mesh sampler as the header states it (areas fp32, prefix sum and the sample's (triangle, u, v) in float64), with the
point in float32 (sample_mesh(..., np.float32): the kernel's twin) or float64."""
import numpy as np

F32 = np.float32
G1, G2 = 0.7548776662466927, 0.5698402909980532


def bounds(ref):
    """per-axis minimum and maximum of the finite rows of ref, float32 (zeros when there is none)"""
    ref = np.asarray(ref, F32).reshape(-1, 3)
    ok = np.isfinite(ref).all(1)
    if not ok.any():
        return np.zeros(3, F32), np.zeros(3, F32)
    return ref[ok].min(0), ref[ok].max(0)


def cells(points, grid):
    """the header's cell coordinates (floorf of the fp32 t) as float64 [n,3]; NaN stays NaN"""
    p = np.asarray(points, F32).reshape(-1, 3)
    with np.errstate(invalid='ignore', over='ignore'):
        t = (p - np.asarray(grid['origin'], F32)[None]) * F32(grid['inv_cell'])
    assert t.dtype == F32
    return np.floor(t.astype(np.float64))


def keys(points, grid):
    c = cells(points, grid)
    n = np.asarray(grid['dims'], np.float64)
    with np.errstate(invalid='ignore'):
        ok = ((c >= 0) & (c < n[None])).all(1)
    c = np.where(ok[:, None], c, 0).astype(np.int64)
    return np.where(ok, (c[:, 0] * int(n[1]) + c[:, 1]) * int(n[2]) + c[:, 2], -1)


def usable_queries(query, grid):
    c = cells(query, grid)
    n = np.asarray(grid['dims'], np.float64)
    with np.errstate(invalid='ignore'):
        return ((c >= -1) & (c <= n[None])).all(1) & np.isfinite(np.asarray(query, F32).reshape(-1, 3)).all(1)


def nearest32(query, ref, max_dist, grid=None):
    """-> (dist float32 [q], index int32 [q], d2 float32 [q] (NaN where nothing was found)).  grid (optional): only to mark
    the queries the header calls unusable (-2, NaN); the search itself never uses it."""
    q, r = np.asarray(query, F32).reshape(-1, 3), np.asarray(ref, F32).reshape(-1, 3)
    md = F32(max_dist)
    md2 = md * md
    rok = np.isfinite(r).all(1)
    if grid is not None:
        rok &= keys(r, grid) >= 0
    dist, index, best = np.full(q.shape[0], md, F32), np.full(q.shape[0], -1, np.int32), np.full(q.shape[0], np.nan, F32)
    with np.errstate(invalid='ignore', over='ignore'):
        for lo in range(0, q.shape[0], 512):
            a = q[lo:lo + 512]
            dx, dy, dz = (a[:, None, c] - r[None, :, c] for c in range(3))
            d2 = (dx * dx + dy * dy) + dz * dz
            assert d2.dtype == F32
            d2 = np.where(rok[None] & (d2 <= md2), d2, np.inf)
            j = d2.argmin(1) if r.shape[0] else np.zeros(a.shape[0], np.int64)          # (argmin: the first of equal minima)
            m = d2[np.arange(a.shape[0]), j] if r.shape[0] else np.full(a.shape[0], np.inf)
            hit = np.isfinite(m)
            index[lo:lo + 512] = np.where(hit, j, -1)
            best[lo:lo + 512] = np.where(hit, m, np.nan)
            dist[lo:lo + 512] = np.where(hit, np.sqrt(np.where(hit, m, 0).astype(F32)), md)
    bad = ~np.isfinite(q).all(1) if grid is None else ~usable_queries(q, grid)
    dist[bad], index[bad], best[bad] = np.nan, -2, np.nan
    return dist, index, best


def nearest64(query, ref, max_dist):
    """float64, unbounded: -> (d2 of the nearest finite reference point [q], its index, d2 of the runner-up (inf: none))"""
    q, r = np.asarray(query, np.float64).reshape(-1, 3), np.asarray(ref, np.float64).reshape(-1, 3)
    rok = np.isfinite(r).all(1)
    b, i, s = np.full(q.shape[0], np.inf), np.full(q.shape[0], -1, np.int64), np.full(q.shape[0], np.inf)
    with np.errstate(invalid='ignore'):
        for lo in range(0, q.shape[0], 512):
            a = q[lo:lo + 512]
            d2 = ((a[:, None] - r[None]) ** 2).sum(-1)
            d2 = np.where(rok[None], d2, np.inf)
            if r.shape[0] == 0:
                continue
            j = d2.argmin(1)
            rows = np.arange(a.shape[0])
            b[lo:lo + 512], i[lo:lo + 512] = d2[rows, j], j
            if r.shape[0] > 1:
                d2[rows, j] = np.inf
                s[lo:lo + 512] = d2.min(1)
    return b, i, s


def stats(dist, index, thresholds):
    """the row of durf_geom_stats in float64 (a sequential numpy sum)"""
    d, i = np.asarray(dist, F32), np.asarray(index)
    usable, found = i != -2, i >= 0
    d64 = d.astype(np.float64)
    row = [usable.sum(), found.sum(), d64[found].sum(), (d64[found] * d64[found]).sum(), d64[usable].sum()]
    row += [(found & (d <= F32(t))).sum() for t in thresholds]
    return np.asarray(row + [0] * (13 - len(row)), np.float64)


# ---- mesh samples -----------------------------------------------------------------------------------------------------------------
def triangle_areas(vertices, triangles):
    """fp32, as the header states; 0 for an index out of range or an area that is not finite"""
    v, t = np.asarray(vertices, F32).reshape(-1, 3), np.asarray(triangles, np.int64).reshape(-1, 3)
    ok = ((t >= 0) & (t < v.shape[0])).all(1)
    ts = np.where(ok[:, None], t, 0)
    a, b, c = v[ts[:, 0]], v[ts[:, 1]], v[ts[:, 2]]
    with np.errstate(invalid='ignore', over='ignore'):
        e1, e2 = b - a, c - a
        cx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
        cy = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
        cz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
        area = F32(0.5) * np.sqrt((cx * cx + cy * cy) + cz * cz)
    assert area.dtype == F32
    return np.where(ok & np.isfinite(area), area, F32(0)).astype(F32)


def sample_mesh(vertices, triangles, n, dtype=np.float64):
    """-> (points [n,3] dtype, tri int32 [n], (u, v) float32 [n,2], total float64)"""
    v, t = np.asarray(vertices, F32).reshape(-1, 3), np.asarray(triangles, np.int64).reshape(-1, 3)
    cum = np.cumsum(triangle_areas(v, t).astype(np.float64))
    total = float(cum[-1]) if cum.size else 0.0
    if not total > 0:
        return np.full((n, 3), np.nan, dtype), np.full(n, -1, np.int32), np.full((n, 2), np.nan, F32), 0.0
    s = np.arange(n, dtype=np.float64)
    target = ((s + 0.5) * total) / float(n)
    g = np.minimum(np.searchsorted(cum, target, side='right'), t.shape[0] - 1)           # the first i with cum[i] > target
    u, w = 0.5 + s * G1, 0.5 + s * G2
    u, w = u - np.floor(u), w - np.floor(w)
    flip = u + w > 1.0
    u, w = np.where(flip, 1.0 - u, u), np.where(flip, 1.0 - w, w)
    uv = np.stack([u, w], 1).astype(F32)
    a, b, c = (v[t[g, k]].astype(dtype) for k in range(3))
    uu, ww = uv[:, :1].astype(dtype), uv[:, 1:].astype(dtype)
    p = a + (uu * (b - a) + ww * (c - a))
    assert p.dtype == dtype
    return p, g.astype(np.int32), uv, total
