"""How far a reconstructed surface lies from measured points, on the device (include/durf_geom.h, csrc/geom.hip,
libdurf_geom.so): nearest-point distances between two unordered clouds, and from them accuracy, completeness, Chamfer distance
and precision / recall / F-score at thresholds.

    dist, index = nearest(query, ref, max_dist)                    # per query: distance and index of the nearest ref point
    r = cloud_distance(pred, truth, max_dist=0.5, thresholds=(0.05, 0.1, 0.2))
    points, tri = sample_mesh(mesh.surface(g, iso), 1_000_000)     # a mesh as a cloud, area-uniform
    truth = depth_points(cam17, lidar_depth, near, far)            # a depth image as a cloud (Waymo.eval_set()['depth'])
    write_error_ply('accuracy.ply', pred, r['pred_dist'], 0.5)

The search is a uniform grid of cells a little wider than max_dist over the reference set, kept as a SORTED KEY ARRAY (one
torch.sort, the plumbing) that the kernel binary-searches: no dense cell table, no atomics, the same inputs give the same
bits.  Distances beyond max_dist are not looked for: such a query reports max_dist and index -1, which is what the truncated
means and the thresholds (<= max_dist) need.  The grid rule of include/durf_geom.h (cell = max_dist (1 + 2^-10), at most 2048
cells per axis) makes the result equal to a brute-force search in the same fp32 arithmetic, bit for bit."""
import numpy as np

from . import camera, trimesh
from .lattice import _max_dist
from ._geom_sigs import DURF_GEOM_MAX_CELLS as MAX_CELLS        # per axis (include/durf_geom.h)
SLACK = 1.0 + 2.0 ** -10            # a cell is max_dist * SLACK wide
SORT_QUERIES = True                 # nearest()'s default: queries in the order of their own cell keys (profiles/geometry_time.txt)
DEFAULT_THRESHOLDS = (0.05, 0.1, 0.2, 0.5)


def grid_rule(lo, hi, max_dist, entry='geometry.nearest'):
    """The grid include/durf_geom.h prescribes for reference points whose finite coordinates span [lo, hi] per axis (float32)
    -> dict(origin float32 [3], inv_cell (a float32 value), dims (nx, ny, nz), cell, max_dist).  An extent of more than 2048
    cells on an axis is refused with the smallest max_dist that fits."""
    md = _max_dist(max_dist, entry)
    lo, hi = np.asarray(lo, np.float32).reshape(3), np.asarray(hi, np.float32).reshape(3)
    if not (np.isfinite(lo).all() and np.isfinite(hi).all() and (hi >= lo).all()):
        raise ValueError('%s: the reference set spans %s .. %s' % (entry, lo.tolist(), hi.tolist()))
    cell = md * SLACK                                                   # float64; md is a float32 value: exact
    inv_cell = np.float32(1.0 / cell)
    with np.errstate(over='ignore'):
        t = (hi - lo) * inv_cell                                        # float32, two roundings: the kernel's own t of the maximum
    dims = np.floor(t.astype(np.float64)) + 1.0
    if not (dims <= MAX_CELLS).all():
        ext = float((hi.astype(np.float64) - lo.astype(np.float64)).max())
        fits = ext / (MAX_CELLS * SLACK) * (1.0 + 2.0 ** -20)
        raise ValueError('%s: max_dist = %g over an extent of %g needs %d cells on an axis, the limit is %d per axis; the smallest '
                         'max_dist that fits is %.9g' % (entry, md, ext, int(min(dims.max(), 2.0 ** 62)), MAX_CELLS, fits))
    return dict(origin=lo.copy(), inv_cell=float(inv_cell), dims=tuple(int(d) for d in dims), cell=cell, max_dist=md)


def make_grid(ref, max_dist, entry='geometry.nearest'):
    """grid_rule over the finite rows of ref [m,3] on the device: ONE read of six floats (the bounds; the library takes the
    origin on the host).  No finite point: a grid of one cell at 0."""
    import torch
    ok = torch.isfinite(ref).all(1, keepdim=True)
    inf = torch.tensor(float('inf'), device=ref.device)
    lo = torch.where(ok, ref, inf).amin(0) if ref.shape[0] else inf.expand(3)
    hi = torch.where(ok, ref, -inf).amax(0) if ref.shape[0] else (-inf).expand(3)
    b = torch.cat([lo, hi]).cpu().numpy()
    if not np.isfinite(b).all():
        _max_dist(max_dist, entry)
        b = np.zeros(6, np.float32)
    return grid_rule(b[:3], b[3:], max_dist, entry)


def _cloud(x, what, entry):
    import torch
    if not (torch.is_tensor(x) and x.is_cuda and x.dim() == 2 and x.shape[1] == 3):
        raise ValueError('%s: %s is a [n,3] tensor on the device' % (entry, what))
    if x.shape[0] >= 2 ** 31:
        raise ValueError('%s: %s has %d points, the limit is 2^31 - 1' % (entry, what, x.shape[0]))
    return x.to(torch.float32).contiguous()


def sort_reference(ref, grid):
    """the reference set as durf_geom_nearest takes it: keys (durf_geom_keys), one stable torch.sort, one gather
    -> (ref_sorted [m,3], keys [m] int64 ascending, index [m] int32: where each row was)"""
    import torch
    from . import ops
    keys = ops.geom_keys(ref, grid['origin'], grid['inv_cell'], grid['dims'])
    skeys, order = torch.sort(keys, stable=True)
    return ref[order].contiguous(), skeys.contiguous(), order.to(torch.int32).contiguous()


def nearest(query, ref, max_dist, sort_queries=None, grid=None, prepared=None):
    """Per query point the nearest reference point within max_dist -> (dist [q] float32, index [q] int32): index -1 and
    dist = max_dist when there is none, index -2 and dist = NaN for a query with a NaN / infinite coordinate or more than one
    cell outside the reference set's bounds (it cannot be within max_dist).  Reference points with a NaN or infinite coordinate
    are never returned.  sort_queries (default SORT_QUERIES): hand the queries over in the order of their own cell keys, so
    that the lanes of a wave walk the same cells, and scatter the results back -- the outputs are bit-identical either way.
    grid / prepared: make_grid's and sort_reference's results, to reuse them."""
    import torch
    from . import ops
    query, ref = _cloud(query, 'query', 'geometry.nearest'), _cloud(ref, 'ref', 'geometry.nearest')
    grid = make_grid(ref, max_dist) if grid is None else grid
    rs, rk, ri = sort_reference(ref, grid) if prepared is None else prepared
    args = (rs, rk, ri, grid['origin'], grid['inv_cell'], grid['dims'], grid['max_dist'])
    if not (SORT_QUERIES if sort_queries is None else sort_queries):
        return ops.geom_nearest(query, *args)
    perm = torch.sort(ops.geom_keys(query, grid['origin'], grid['inv_cell'], grid['dims']), stable=True)[1]
    d, i = ops.geom_nearest(query[perm].contiguous(), *args)
    dist, index = torch.empty_like(d), torch.empty_like(i)
    dist[perm] = d
    index[perm] = i
    return dist, index


def _thresholds(thresholds, max_dist, entry):
    th = [float(np.float32(t)) for t in thresholds]
    if len(th) > 8:
        raise ValueError('%s: %d thresholds, at most 8' % (entry, len(th)))
    if any(not (0.0 <= t <= max_dist) for t in th):
        raise ValueError('%s: thresholds %s must lie in [0, max_dist = %g]: nothing beyond max_dist is looked for' % (entry, th, max_dist))
    return th


def summarise(rows, thresholds, max_dist):
    """The metrics from the two statistic rows of durf_geom_stats (rows [2, 13] float64 on the host: pred -> truth, then
    truth -> pred) -- host arithmetic only.  accuracy / completeness: the mean distance over the queries that found a point
    (None when none did); *_truncated: over every usable query, one that found nothing counting max_dist; chamfer: their sums;
    rms: the root mean square over found; precision / recall / fscore per threshold: the share of usable pred (truth) points
    within the threshold of truth (pred), and their harmonic mean (0 when both are 0)."""
    rows = np.asarray(rows, np.float64).reshape(2, -1)
    th = list(thresholds)

    def side(r):
        usable, found = r[0], r[1]
        return dict(usable=int(usable), found=int(found), mean=r[2] / found if found > 0 else None,
                    rms=float(np.sqrt(r[3] / found)) if found > 0 else None, truncated=r[4] / usable if usable > 0 else None,
                    within=[r[5 + k] / usable if usable > 0 else None for k in range(len(th))])
    p, t = side(rows[0]), side(rows[1])
    add = lambda a, b: None if a is None or b is None else a + b
    f = []
    for a, b in zip(p['within'], t['within']):
        f.append(None if a is None or b is None else (2.0 * a * b / (a + b) if a + b > 0 else 0.0))
    return dict(max_dist=float(max_dist), thresholds=th, accuracy=p['mean'], completeness=t['mean'], chamfer=add(p['mean'], t['mean']),
                accuracy_truncated=p['truncated'], completeness_truncated=t['truncated'],
                chamfer_truncated=add(p['truncated'], t['truncated']), accuracy_rms=p['rms'], completeness_rms=t['rms'],
                precision=p['within'], recall=t['within'], fscore=f, pred_usable=p['usable'], pred_found=p['found'],
                truth_usable=t['usable'], truth_found=t['found'])


def cloud_distance(pred, truth, max_dist, thresholds=DEFAULT_THRESHOLDS, sort_queries=None, keep=False):
    """Both directions of nearest() and their statistics -> summarise()'s dict plus `grids` (the two grids: dims, cell,
    origin).  The statistic rows are summed on the device in float64 in a fixed order and read back in ONE copy at the end
    (beside the six bounds each grid needs on the host).  thresholds: at most 8, each <= max_dist (the default set is cut to
    those).  A finite point more than a cell beyond the other cloud's bounds (nearest()'s -2) counts as one that found nothing;
    usable excludes only points with a NaN or infinite coordinate.  keep=True adds pred_dist, pred_index, truth_dist, truth_index (device tensors) for write_error_ply."""
    import torch
    from . import ops
    md = _max_dist(max_dist, 'geometry.cloud_distance')
    if thresholds is DEFAULT_THRESHOLDS:
        thresholds = tuple(t for t in DEFAULT_THRESHOLDS if t <= md)
    th = _thresholds(thresholds, md, 'geometry.cloud_distance')
    pred, truth = _cloud(pred, 'pred', 'geometry.cloud_distance'), _cloud(truth, 'truth', 'geometry.cloud_distance')
    rows = torch.empty(2, ops.GEOM_STAT_DOUBLES, dtype=torch.float64, device=pred.device)
    out, grids = {}, {}
    for r, (name, q, ref) in enumerate((('pred', pred, truth), ('truth', truth, pred))):
        g = make_grid(ref, md, 'geometry.cloud_distance')
        d, i = nearest(q, ref, md, sort_queries=sort_queries, grid=g)
        # a finite point beyond the other cloud's grid has nothing within max_dist: for the metrics it found nothing (it is
        # not left out, which would flatter the truncated means); only a NaN / infinite point stays unusable
        far = (i == -2) & torch.isfinite(q).all(1)
        d, i = torch.where(far, torch.full_like(d, md), d), torch.where(far, torch.full_like(i, -1), i)
        ops.geom_stats(d, i, th, out=rows[r])
        grids[name + '_to_' + ('truth' if name == 'pred' else 'pred')] = dict(origin=g['origin'].tolist(), dims=list(g['dims']), cell=g['cell'])
        if keep:
            out[name + '_dist'], out[name + '_index'] = d, i
    res = summarise(rows.cpu().numpy(), th, md)
    res['grids'] = grids
    res.update(out)
    return res


def surface_distance(m, truth, max_dist, thresholds=DEFAULT_THRESHOLDS, samples=200000, sort_queries=None, keep=False):
    """cloud_distance for a MESH m (dict vertices, triangles) against the measured cloud truth, without a sample spacing on the
    completeness side: accuracy is `samples` area-uniform samples of m (sample_mesh) against the truth cloud by nearest(), as
    cloud_distance does; completeness is every truth point against the surface itself by closest.points (the exact
    point-to-triangle distance, include/durf_closest.h).  -> cloud_distance's keys (`grids` holds the one grid there is);
    keep=True adds pred (the samples), pred_dist, pred_index, truth_dist, truth_index (the triangle each truth point lands on)
    and truth_bary."""
    import torch
    from . import cast, closest, ops
    entry = 'geometry.surface_distance'
    md = _max_dist(max_dist, entry)
    if thresholds is DEFAULT_THRESHOLDS:
        thresholds = tuple(t for t in DEFAULT_THRESHOLDS if t <= md)
    th = _thresholds(thresholds, md, entry)
    if int(samples) < 1:
        raise ValueError('%s: samples = %r, expected at least one sample of the mesh (the accuracy side)' % (entry, samples))
    truth = _cloud(truth, 'truth', entry)
    b = m if (isinstance(m, dict) and m.get('ws') is not None) else cast.build(m)
    pred = sample_mesh(b, int(samples))[0]
    rows = torch.empty(2, ops.GEOM_STAT_DOUBLES, dtype=torch.float64, device=pred.device)
    g = make_grid(truth, md, entry)
    d, i = nearest(pred, truth, md, sort_queries=sort_queries, grid=g)
    far = (i == -2) & torch.isfinite(pred).all(1)                       # (as cloud_distance: beyond the grid is `found nothing`)
    d, i = torch.where(far, torch.full_like(d, md), d), torch.where(far, torch.full_like(i, -1), i)
    ops.geom_stats(d, i, th, out=rows[0])
    r = closest.points(b, truth, md, sort_queries=sort_queries)
    ops.geom_stats(r['dist'], r['tri'], th, out=rows[1])
    res = summarise(rows.cpu().numpy(), th, md)
    res['grids'] = dict(pred_to_truth=dict(origin=g['origin'].tolist(), dims=list(g['dims']), cell=g['cell']))
    if keep:
        res.update(pred=pred, pred_dist=d, pred_index=i, truth_dist=r['dist'], truth_index=r['tri'], truth_bary=r['bary'])
    return res


def sample_mesh(m, n):
    """n area-uniform samples of a triangle mesh: what mesh.surface / mesh.extract / mesh.read_ply return (dict vertices
    [V,3], triangles [T,3]; host arrays are uploaded) -> (points [n,3], tri [n] int32: the triangle each sample lies on, so the
    caller carries normals, colours or the owner label).  Stratified over the cumulative area, with the R2 low-discrepancy
    sequence inside each triangle: deterministic.  A mesh of total area 0: n rows of NaN with id -1."""
    import torch
    from . import ops
    v, t = m['vertices'], m['triangles']                              # (no refusal of its own: a mesh of any shape with 3 V and 3 T values)
    dev = trimesh.device_of(v)
    v, t = trimesh.upload(v, torch.float32, dev).reshape(-1, 3), trimesh.upload(t, torch.int32, dev).reshape(-1, 3)
    if int(n) < 0:
        raise ValueError('geometry.sample_mesh: n = %r samples' % (n,))
    points, tri, _ = ops.geom_sample_mesh(v, t, int(n))
    return points, tri


def depth_points(cam17, depth, near, far, mask=None):
    """The world points of a depth image's positive pixels: origin + direction * depth along the rays of raygen.camera_rays
    (the parametrisation of the renderer's `distance` and of the LIDAR depth planes of eval_set()).  depth [h,w] (or [h,w,1])
    on the device; mask [h,w] (optional): pixels to keep besides depth > 0 -> points [n,3] in pixel order.  Plumbing: torch
    arithmetic, one boolean gather."""
    import torch
    from . import raygen
    cam, h, w = camera.as_rows(cam17, 'geometry.depth_points', frames=1)
    depth = torch.as_tensor(depth)
    if depth.numel() != h * w:
        raise ValueError('geometry.depth_points: a depth image of %d values for a camera of %d x %d' % (depth.numel(), h, w))
    dev = depth.device if depth.is_cuda else torch.device('cuda', torch.cuda.current_device())
    rays = raygen.camera_rays(cam, near, far, device=dev)
    d = depth.to(device=dev, dtype=torch.float32).reshape(h * w)
    keep = d > 0
    if mask is not None:
        keep = keep & (torch.as_tensor(mask).to(dev).reshape(h * w) != 0)
    o, v = rays.origins.reshape(-1, 3)[keep], rays.directions.reshape(-1, 3)[keep]
    return (o + v * d[keep][:, None]).contiguous()


def outside_boxes(points, poses, ext, pad=0.0):
    """True for the points [n,3] that lie in none of the K boxes: poses [K,6] (centre, rotation vector: P = R (X - c)), ext
    [K,3] half extents, both host arrays; inside means |P_j| <= ext_j (1 + pad).  Torch arithmetic."""
    import torch
    from . import mesh
    poses, ext = np.asarray(poses, np.float64).reshape(-1, 6), np.asarray(ext, np.float64).reshape(-1, 3)
    out = torch.ones(points.shape[0], dtype=torch.bool, device=points.device)
    for k in range(poses.shape[0]):
        R = torch.tensor(mesh.aa2matrix(poses[k, 3:]), dtype=torch.float32, device=points.device)
        c = torch.tensor(poses[k, :3], dtype=torch.float32, device=points.device)
        e = torch.tensor(ext[k] * (1.0 + pad), dtype=torch.float32, device=points.device)
        out &= ~((((points - c) @ R.T).abs() <= e).all(1))
    return out


_ERROR_VERTEX = np.dtype([('x', '<f4'), ('y', '<f4'), ('z', '<f4'), ('red', 'u1'), ('green', 'u1'), ('blue', 'u1'), ('distance', '<f4')])


def error_colours(dist, max_dist, lut=None):
    """distances -> uint8 [n,3]: the library's turbo table (durf_vis_turbo_lut) at dist / max_dist, clipped to [0, 1]; a NaN
    (an unusable point) is grey"""
    if lut is None:
        from . import ops
        lut = ops.vis_turbo_lut()
    d = np.asarray(dist, np.float64).reshape(-1)
    x = np.clip(np.nan_to_num(d / float(max_dist), nan=0.0), 0.0, 1.0)
    rgb = np.rint(np.clip(np.asarray(lut, np.float64)[np.rint(x * 255.0).astype(np.int64)], 0.0, 1.0) * 255.0).astype(np.uint8)
    rgb[np.isnan(d)] = 128
    return rgb


def write_error_ply(path, points, dist, max_dist, lut=None):
    """The cloud coloured by its distance through the turbo table -> binary little-endian PLY: x y z (float), red green blue
    (uchar), distance (float).  Reads the points and distances back; returns the number of points."""
    host = lambda a: a.detach().cpu().numpy() if hasattr(a, 'detach') else np.asarray(a)
    X, d = host(points).astype('<f4').reshape(-1, 3), host(dist).astype('<f4').reshape(-1)
    if X.shape[0] != d.shape[0]:
        raise ValueError('write_error_ply: %d points and %d distances' % (X.shape[0], d.shape[0]))
    V = np.zeros(X.shape[0], _ERROR_VERTEX)
    V['x'], V['y'], V['z'], V['distance'] = X[:, 0], X[:, 1], X[:, 2], d
    rgb = error_colours(d, max_dist, lut)
    V['red'], V['green'], V['blue'] = rgb[:, 0], rgb[:, 1], rgb[:, 2]
    head = ('ply\nformat binary_little_endian 1.0\ncomment durf_amd.geometry: distance to the other cloud, turbo over [0, %g]\n'
            'element vertex %d\nproperty float x\nproperty float y\nproperty float z\nproperty uchar red\nproperty uchar green\n'
            'property uchar blue\nproperty float distance\nend_header\n' % (float(max_dist), X.shape[0]))
    with open(path, 'wb') as f:
        f.write(head.encode('ascii'))
        f.write(V.tobytes())
    return X.shape[0]
