"""The closest point of a triangle mesh to arbitrary points, on the device (include/durf_closest.h, csrc/closest.hip,
libdurf_closest.so): the exact distance from a point to the surface, the triangle it lands on and where on it.

    b = cast.build(m)                                              # the tree the rays are cast at: this module reads it too
    r = points(b, p, max_dist=0.5)                                 # tri, dist, bary, point, mask
    a = attributes(b, r)                                           # the mesh's rgb, normals, owner at the closest points
    g = grid(b, origin, dims, step)                                # the unsigned distance field over a lattice, for mesh.surface
    d = mesh_to_mesh(ma, mb, 200000, max_dist=0.5)                 # Metro-style distance between two meshes

The result of a query is defined in the header as a minimum over all triangles; the tree only finds it sooner.  Nothing beyond
max_dist is looked for: such a point reports tri = -1 and dist = max_dist (geometry.nearest's convention, so durf_geom_stats
takes the two arrays as they are); a point with a NaN or infinite coordinate reports -2 and NaN."""
import numpy as np

from . import lattice, trimesh

SORT_QUERIES = True                 # points()'s default: queries in the order of a Morton key of their own


def _tree(b, entry):
    if not isinstance(b, dict) or b.get('ws') is None or b.get('T') is None:
        raise ValueError('%s: b is what cast.build returns (a dict with ws and T)' % entry)
    return b


def _spread(x):
    """21 bits -> every third bit of an int64"""
    x = (x | (x << 32)) & 0x1f00000000ffff
    x = (x | (x << 16)) & 0x1f0000ff0000ff
    x = (x | (x << 8)) & 0x100f00f00f00f00f
    x = (x | (x << 4)) & 0x10c30c30c30c30c3
    return (x | (x << 2)) & 0x1249249249249249


def morton_keys(p):
    """durf_cast_keys' rule on points [n,3] on the device (21 bits per axis inside the bounds of the finite points) -> int64
    [n]; an unusable point sorts last.  Torch arithmetic, no read-back: the keys affect speed only, never a result."""
    import torch
    ok = torch.isfinite(p).all(1)
    inf = torch.tensor(float('inf'), device=p.device)
    lo, hi = torch.where(ok[:, None], p, inf).amin(0), torch.where(ok[:, None], p, -inf).amax(0)
    x = ((p - lo) / (hi - lo) * 2097152.0).nan_to_num(0.0, 0.0, 0.0).clamp(0.0, 2097151.0).to(torch.int64)
    key = (_spread(x[:, 0]) << 2) | (_spread(x[:, 1]) << 1) | _spread(x[:, 2])
    return torch.where(ok, key, torch.full_like(key, 2 ** 63 - 1))


def points(b, p, max_dist=float('inf'), sort_queries=None):
    """p [...,3] against cast.build()'s b -> dict tri int32 [...] (-1 nothing within max_dist, -2 an unusable point), dist [...]
    (max_dist and NaN there), bary [...,3] = (w, u, v) in the mesh's vertex order, point [...,3] (the closest point), mask [...]
    bool.  sort_queries (default SORT_QUERIES): hand the points over in the order of morton_keys, so that the lanes of a wave
    walk the same nodes, and scatter the results back -- the outputs are bit-identical either way."""
    entry = 'closest.points'
    md = lattice._max_dist(max_dist, entry, inf=True)
    _tree(b, entry)
    import torch
    from . import ops
    dev = b['ws'].device
    p = trimesh.upload(p, torch.float32, dev)
    if p.dim() < 1 or p.shape[-1] != 3:
        raise ValueError('%s: points of shape %s, expected [..., 3]' % (entry, tuple(p.shape)))
    if p.numel() // 3 >= 2 ** 31:
        raise ValueError('%s: %d points, the limit is 2^31 - 1' % (entry, p.numel() // 3))
    lead, flat = tuple(p.shape[:-1]), p.reshape(-1, 3)
    if (SORT_QUERIES if sort_queries is None else sort_queries) and flat.shape[0] > 1:
        perm = torch.sort(morton_keys(flat), stable=True)[1]
        got = ops.closest_points(b['ws'], b['T'], flat[perm].contiguous(), md)
        out = [torch.empty_like(a) for a in got]
        for o, a in zip(out, got):
            o[perm] = a
    else:
        out = ops.closest_points(b['ws'], b['T'], flat, md)
    tri, dist, bary, point = (a.reshape(lead + tuple(a.shape[1:])) for a in out)
    return dict(tri=tri, dist=dist, bary=bary, point=point, mask=tri >= 0)


def attributes(b, r, attrs=('rgb', 'normals'), label='owner'):
    """The mesh's per-vertex arrays at the closest points of points()'s result r -> dict: every key of `attrs` that b holds as
    [...,C] ((w a0 + u a1) + v a2: durf_raster_interp; uint8 colours as [0, 1] floats) and `label` as [...] int32 (the label of
    the triangle's first vertex, -1 where nothing was found)."""
    entry = 'closest.attributes'
    _tree(b, entry)
    trimesh.check_attrs(attrs, entry)
    if not isinstance(r, dict) or r.get('tri') is None or r.get('bary') is None:
        raise ValueError('%s: r is what closest.points returns (a dict with tri and bary)' % entry)
    from . import cast
    return cast.attributes_at(b, r['tri'].contiguous(), r['bary'].contiguous(), attrs, label, {})


def grid(b, origin, dims, step, max_dist=float('inf'), axes=None):
    """The unsigned distance to the mesh at the nu x nv x nw points origin + i du + j dv + k dw, (du, dv, dw) = step times the
    rows of `axes` (default: the world axes), generated in the kernel -> dict density [nu,nv,nw] (the distance; max_dist where
    the mesh is farther, NaN at a point that is not finite), tri int32 [nu,nv,nw], valid None, frame dict(origin, du, dv, dw):
    what mesh.surface(g, iso) accepts -- a point is `in` when its distance is >= iso, so the surface at iso = r is the offset
    surface at distance r with normals towards the mesh."""
    entry = 'closest.grid'
    md = lattice._max_dist(max_dist, entry, inf=True)
    _tree(b, entry)
    dims = tuple(int(d) for d in np.asarray(dims).reshape(-1))
    if len(dims) != 3 or min(dims) < 1 or dims[0] * dims[1] * dims[2] >= 2 ** 31:
        raise ValueError('%s: dims = %r, expected three counts >= 1 with fewer than 2^31 points' % (entry, dims))
    frame = lattice.frame(origin, step=step, axes=axes, entry=entry, scaled=True)
    from . import ops
    dist, tri = ops.closest_grid(b['ws'], b['T'], dims, frame['origin'], frame['du'], frame['dv'], frame['dw'], md)
    return dict(density=dist, tri=tri, valid=None, frame=frame)


def mesh_to_mesh(a, b, n, max_dist, thresholds=None):
    """Metro-style distance between meshes a and b (dicts vertices, triangles): n area-uniform samples of each
    (geometry.sample_mesh) against the OTHER mesh by points() -> geometry.summarise's dict (accuracy: a's samples to b,
    completeness: b's samples to a) plus hausdorff_ab, hausdorff_ba (the largest distance found on each side, None when nothing
    was) and hausdorff.  The statistic rows are summed on the device and read back in one copy with the two maxima."""
    entry = 'closest.mesh_to_mesh'
    import torch
    from . import cast, geometry, ops
    md = lattice._max_dist(max_dist, entry)
    if int(n) < 1:
        raise ValueError('%s: n = %r samples' % (entry, n))
    th = geometry._thresholds(tuple(t for t in geometry.DEFAULT_THRESHOLDS if t <= md) if thresholds is None else thresholds, md, entry)
    trees = [m if (isinstance(m, dict) and m.get('ws') is not None) else cast.build(m) for m in (a, b)]
    dev = trees[0]['ws'].device
    rows, worst = torch.empty(2, ops.GEOM_STAT_DOUBLES, dtype=torch.float64, device=dev), torch.zeros(2, dtype=torch.float64, device=dev)
    for i in (0, 1):
        samples = geometry.sample_mesh(trees[i], int(n))[0]
        r = points(trees[1 - i], samples, md)
        ops.geom_stats(r['dist'].contiguous(), r['tri'].contiguous(), th, out=rows[i])
        found = torch.where(r['mask'], r['dist'], torch.full_like(r['dist'], -1.0))
        worst[i] = found.max().to(torch.float64) if found.numel() else -1.0
    host = torch.cat([rows.reshape(-1), worst]).cpu().numpy()
    res = geometry.summarise(host[:-2].reshape(2, -1), th, md)
    hab, hba = (float(x) if x >= 0 else None for x in host[-2:])
    res.update(hausdorff_ab=hab, hausdorff_ba=hba, hausdorff=None if hab is None or hba is None else max(hab, hba), samples=int(n))
    return res
