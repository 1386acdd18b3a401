"""Rays against a triangle mesh, on the device (include/durf_cast.h, csrc/cast.hip, libdurf_cast.so): the nearest triangle along
arbitrary rays -- a LIDAR sweep of an extracted surface, depth from a camera that stands inside the mesh, visibility.

    b = build(m)                                                   # m: mesh.surface / extract / read_ply / raster.merge
    r = rays(b, origins, directions)                               # tri, t, bary, mask
    c = cameras(b, cams)                                           # the planes of raster.render_mesh, without a near plane
    s = lidar(b, sensor, poses, near=0.1, far=75.0)                # range, valid, xyz, tri as [F,H,W] range images
    free = visible(b, a, p)                                        # does the segment a -> p miss the mesh

The result of a cast is defined in the header as a minimum over all triangles; the tree only finds it sooner.  t is in units
of |direction|: camera depth for the ray generator's z = -1 directions (comparable with `distance` and with the rasteriser's
depth), range for the LIDAR's unit directions.  A ray has no near plane: nothing is dropped around a camera that stands on the
mesh.  Meshes of moving boxes: one raster.merge(meshes, poses, ts) and one build per timestep."""
import numpy as np

from . import trimesh


def _check_bounds(entry, tmin, tmax, cull):
    for name, b in (('tmin', tmin), ('tmax', tmax)):
        if not hasattr(b, 'shape') and (b != b or (name == 'tmin' and not b >= 0)):
            raise ValueError('%s: %s = %r, expected %s' % (entry, name, b, 'a number >= 0' if name == 'tmin' else 'a number'))
    if cull not in (0, 1, 2):
        raise ValueError('%s: cull = %r, expected 0 (both faces), 1 (drop back faces) or 2 (drop front faces)' % (entry, cull))


def build(m, order=None):
    """The tree of mesh m (host arrays are uploaded) -> dict: the mesh's arrays on the device (vertices, triangles, and every
    other per-vertex array of m as it was), V, T, order (the permutation the tree was built over) and ws (the workspace the
    casts read).  Bounds by torch.aminmax, durf_cast_keys, a stable torch.sort, durf_cast_build: no read-back.  order: a
    permutation of the triangles to build over instead (it changes the speed of a cast, never its result)."""
    from ._cast_sigs import DURF_CAST_MAX_TRIANGLES
    V, T = trimesh.arrays(m, 'cast.build', DURF_CAST_MAX_TRIANGLES, 'the limits are 2^31 - 1 and %d' % (DURF_CAST_MAX_TRIANGLES - 1))
    import torch
    from . import ops
    dev = trimesh.device_of(m['vertices'])
    vertices, triangles = trimesh.on_device(m, V, T, dev)
    if order is None:
        if V > 0 and T > 0:
            lo, hi = torch.aminmax(vertices, dim=0)
            keys = ops.cast_keys(vertices, triangles, torch.cat([lo, hi]).contiguous())
            order = torch.sort(keys, stable=True)[1].to(torch.int32)
        else:
            order = torch.arange(T, dtype=torch.int32, device=dev)
    else:
        order = trimesh.upload(order, torch.int32, dev).reshape(-1)
        if order.numel() != T:
            raise ValueError('cast.build: order has %d entries for %d triangles' % (order.numel(), T))
    b = {k: a for k, a in m.items() if k not in ('vertices', 'triangles')}
    b.update(vertices=vertices, triangles=triangles, V=V, T=T, order=order, ws=ops.cast_build(vertices, triangles, order))
    return b


def _rays_on(b, origins, directions, entry):
    import torch
    o, d = (trimesh.upload(a, torch.float32, b['ws'].device) for a in (origins, directions))
    if o.dim() < 1 or o.shape[-1] != 3 or tuple(o.shape) != tuple(d.shape):
        raise ValueError('%s: origins of shape %s and directions of shape %s, expected the same [..., 3]' % (entry, tuple(o.shape), tuple(d.shape)))
    return o, d


def _bound_on(b, x, lead, entry, name):
    import torch
    if torch.is_tensor(x) or isinstance(x, np.ndarray):
        x = torch.as_tensor(x).to(device=b['ws'].device, dtype=torch.float32).contiguous()
        if tuple(x.shape) != lead:
            raise ValueError('%s: %s of shape %s for rays of shape %s' % (entry, name, tuple(x.shape), lead))
        return x
    return float(x)


def rays(b, origins, directions, tmin=0.0, tmax=float('inf'), cull=0):
    """origins, directions [...,3] against build()'s b -> dict tri int32 [...] (-1 nothing, -2 an unusable ray), t [...] (0 and
    NaN there), bary [...,3] = (w, u, v) in the mesh's vertex order, mask [...] bool.  tmin, tmax: numbers or arrays [...]."""
    _check_bounds('cast.rays', tmin, tmax, cull)
    from . import ops
    o, d = _rays_on(b, origins, directions, 'cast.rays')
    lead = tuple(o.shape[:-1])
    tri, t, bary = ops.cast_rays(b['ws'], b['T'], o, d, _bound_on(b, tmin, lead, 'cast.rays', 'tmin'), _bound_on(b, tmax, lead, 'cast.rays', 'tmax'), cull)
    return dict(tri=tri, t=t, bary=bary, mask=tri >= 0)


def occluded(b, origins, directions, tmin=0.0, tmax=float('inf'), cull=0):
    """-> int32 [...]: 1 where some triangle counts on the ray, 0 where none does, -2 for an unusable ray (durf_cast_any)"""
    _check_bounds('cast.occluded', tmin, tmax, cull)
    from . import ops
    o, d = _rays_on(b, origins, directions, 'cast.occluded')
    lead = tuple(o.shape[:-1])
    return ops.cast_any(b['ws'], b['T'], o, d, _bound_on(b, tmin, lead, 'cast.occluded', 'tmin'), _bound_on(b, tmax, lead, 'cast.occluded', 'tmax'), cull)


def visible(b, a, p):
    """points a, p [...,3] -> bool [...]: the segment a -> p touches no triangle (the ray o = a, d = p - a with 0 <= t <= 1; a
    segment that is not finite, or of no length, is not visible)"""
    o, e = _rays_on(b, a, p, 'cast.visible')
    return occluded(b, o, e - o, 0.0, 1.0) == 0


def attributes_at(b, tri, bary, attrs, label, out):
    """The per-vertex arrays of build()'s b at (tri, bary), through durf_raster_interp, added to the dict `out`: every key of
    `attrs` that b holds as [...,C] (uint8 colours as [0, 1] floats) and `label` as [...] int32 (-1 where tri < 0).  cameras()
    and closest.attributes share it."""
    from . import ops
    V = b['V']
    fattrs, lab = trimesh.vertex_attributes(b, attrs, label, V, tri.device)
    for key, a in fattrs.items():
        out[key] = ops.raster_interp(b['triangles'], tri, bary, V, attr_f=a)[0]
    if lab is not None:
        out[label] = ops.raster_interp(b['triangles'], tri, None, V, attr_i=lab, fill=-1)[1]
    return out


def cameras(b, cams, tmin=0.0, tmax=float('inf'), attrs=('rgb', 'normals'), label='owner', cull=0):
    """build()'s b through the cameras cams [F,CAM_FLOATS] of one frame size -> the planes of raster.render_mesh: depth [F,h,w]
    (camera depth, 0 where nothing is hit), tri [F,h,w] int32, mask, bary [F,h,w,3], every key of `attrs` that b holds as
    [F,h,w,C] and `label` as [F,h,w] int32, through durf_raster_interp.  One launch for the cast: the rays are generated in
    the kernel.  There is no near plane: tmin is a bound on depth, 0 by default."""
    from . import camera
    entry = 'cast.cameras'
    cams, h, w = camera.as_rows(cams, entry)
    if not np.isfinite(cams).all():
        raise ValueError('%s: a camera row that is not finite' % entry)
    _check_bounds(entry, tmin, tmax, cull)
    trimesh.check_attrs(attrs, entry)
    if cams.shape[0] * h * w >= 2 ** 31:
        raise ValueError('%s: %d frames of %d x %d: frames x pixels must stay below 2^31' % (entry, cams.shape[0], h, w))
    import torch
    from . import ops
    tri, depth, bary = ops.cast_cameras(b['ws'], b['T'], torch.as_tensor(cams).to(b['ws'].device).contiguous(), h, w, tmin, tmax, cull)
    return attributes_at(b, tri, bary, attrs, label, dict(tri=tri, depth=depth, bary=bary, mask=tri >= 0))


def lidar(b, sensor, poses, near, far, pose_end=None):
    """F sweeps of lidar.LidarSensor `sensor` against build()'s b: poses [F,3,4] the sensor at the start of every sweep
    (pose_end: at its end) -> dict of [F,H,W] range images: range (0 where nothing is hit within near .. min(far,
    sensor.max_range)), valid int32, tri int32, xyz [F,H,W,3] (world), bary.  The rays are durf_lidar_rays' (unit directions: t
    is range), one launch per sweep for them and one for the cast."""
    import torch
    from . import lidar as L, ops
    _check_bounds('cast.lidar', near, far, 0)
    rows = L.sweep_rows(poses, pose_end)
    dev = b['ws'].device
    incl = torch.as_tensor(sensor.inclinations, device=dev)
    H, W = sensor.height, sensor.width
    out = dict(range=[], valid=[], tri=[], xyz=[], bary=[])
    for row in rows:
        o, d = ops.lidar_rays(sensor.row(), incl, row, near, far)[:2]
        tri, t, bary = ops.cast_rays(b['ws'], b['T'], o, d, float(near), min(float(far), float(sensor.max_range)))
        valid = (tri >= 0).to(torch.int32)
        out['range'].append(t.reshape(H, W)), out['valid'].append(valid.reshape(H, W)), out['tri'].append(tri.reshape(H, W))
        out['xyz'].append(torch.where(valid[:, None] > 0, o + t[:, None] * d, torch.zeros_like(o)).reshape(H, W, 3))
        out['bary'].append(bary.reshape(H, W, 3))
    return {k: torch.stack(x) if x else torch.empty((0, H, W) + ((3,) if k in ('xyz', 'bary') else ()), device=dev) for k, x in out.items()}


def point_cloud(result, sweep=0):
    """the valid returns of one sweep of lidar()'s result -> (points [n,8], count [1] int32 on the device), through
    durf_lidar_compact as lidar.point_cloud does: no read-back"""
    from . import ops
    g = lambda k: result[k][sweep].reshape(-1, *result[k].shape[3:]).contiguous()
    points, _, count = ops.lidar_compact(g('valid'), g('xyz'), g('range'))
    return points, count
