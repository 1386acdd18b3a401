"""A triangle mesh seen through the renderer's cameras, on the device (include/durf_raster.h, csrc/raster.hip,
libdurf_raster.so): per pixel the nearest triangle, its camera depth, and the vertex attributes there.

    s = mesh.extract_scene(model, variables, origin, shape, step=0.25, iso=5.0, ext=ext, obj_step=0.05)
    m = merge(s, ts=3)                                             # one mesh in the world, the boxes at their poses of time 3
    r = render_mesh(m, cams)                                       # cams: camera.rows / camera.row
    e = depth_error(r['depth'], frames['distance'], frames['acc'])  # against render_trajectory's frames of the same cameras
    write_depth('out/depth_0000', r['depth'][0], r['mask'][0]); write_ids('out/ids_0000.ppm', r['owner'][0])

The camera directions of the ray generator have z = -1, so the renderer's `distance` is camera depth and the z-buffer here is
comparable with it pixel by pixel, as it is with the LIDAR depth planes of eval_set().  The draw is a binned gather with exact
integer coverage: the same inputs give the same bits.  A triangle that crosses the camera's near plane is dropped, not clipped
(counts['crossing'] says how many)."""
import numpy as np

from . import camera, trimesh
from .lattice import _host
from ._raster_sigs import DURF_RASTER_MAX_SIZE as MAX_SIZE, DURF_RASTER_RECORD_INTS as RECORD_INTS, DURF_RASTER_TILE as TILE

COUNT_FIELDS = ('pairs', 'drawn', 'invalid', 'behind', 'crossing', 'range', 'degenerate', 'culled')
WORKSPACE_BOUND = 1 << 30           # bytes: render_mesh chunks over frames to keep the workspace of one call under this
ATTRIBUTES = ('rgb', 'normals', 'owner', 'component')              # what merge carries when every mesh has it


def workspace_estimate(F, T, h, w):
    """the bytes durf_raster_workspace_bytes will ask for, to within the alignment: 40 per (frame, triangle), 16 per tile"""
    tiles = F * ((h + TILE - 1) // TILE) * ((w + TILE - 1) // TILE)
    return 4 * RECORD_INTS * F * T + 16 * tiles + 8 * (tiles // 256 + 2) + 5 * 256


def default_frames_per_call(F, T, h, w, bound=WORKSPACE_BOUND):
    """the most frames whose workspace stays under `bound` bytes and whose pairs and pixels stay under 2^31 (at least 1)"""
    n = max(int(F), 1)
    while n > 1 and (workspace_estimate(n, T, h, w) > bound or n * T >= 2 ** 31 or n * h * w >= 2 ** 31):
        n = (n + 1) // 2
    return n


def _check(m, cams, znear, attrs, label, cull, per_call):
    """every refusal of render_mesh, on the host, before anything touches the device -> (cams float32 [F,CAM_FLOATS], h, w, V, T)"""
    entry = 'raster.render_mesh'
    V, T = trimesh.shapes(m, entry)
    cams, h, w = camera.as_rows(cams, entry)
    if not np.isfinite(cams).all():
        raise ValueError('%s: a camera row that is not finite' % entry)
    if not (1 <= h <= MAX_SIZE and 1 <= w <= MAX_SIZE):
        raise ValueError('%s: frames of %d x %d, expected 1 .. %d each way' % (entry, h, w, MAX_SIZE))
    trimesh.limits(V, T, entry)
    if not float(znear) > 0:
        raise ValueError('%s: znear = %r, expected a number > 0' % (entry, znear))
    if cull not in (0, 1, 2):
        raise ValueError('%s: cull = %r, expected 0 (both faces), 1 (drop back faces) or 2 (drop front faces)' % (entry, cull))
    trimesh.check_attrs(attrs, entry, of='m')
    trimesh.check_attribute_rows(m, attrs, label, V, entry)
    if per_call is not None and (int(per_call) != per_call or per_call < 1):
        raise ValueError('%s: frames_per_call = %r, expected an integer >= 1 or None' % (entry, per_call))
    return cams, h, w, V, T


def render_mesh(m, cams, znear=1e-2, attrs=('rgb', 'normals'), label='owner', cull=0, frames_per_call=None):
    """The mesh m (mesh.surface / extract / read_ply / merge: dict vertices [V,3], triangles [T,3], host arrays are uploaded)
    through the cameras cams [F,CAM_FLOATS] of one frame size -> dict depth [F,h,w] (camera depth, 0 where nothing covers), tri
    [F,h,w] int32 (-1 there), mask [F,h,w] bool, bary [F,h,w,3], every key of `attrs` that m holds as [F,h,w,C] (float vertex
    attributes, perspective-correct; a uint8 colour counts as / 255; 0 where nothing covers), `label` as [F,h,w] int32 (the
    int attribute of the owning triangle's first vertex, -1 where nothing covers), counts (int64 [calls, 8] on the host:
    COUNT_FIELDS per call) and frames (the frames of every call).  A key of attrs, or the label, that m lacks or holds as None
    is left out.  Per call: durf_raster_setup, ONE read of counts for the exact size of the pair list (as mesh.surface reads
    its two counts), durf_raster_draw, durf_raster_interp.  frames_per_call: None keeps the workspace of a call (40 bytes per
    frame and triangle) under WORKSPACE_BOUND; 1 gives counts per frame.  The pictures do not depend on it.
    cull: 0 both faces, 1 drop back faces, 2 drop front faces."""
    cams, h, w, V, T = _check(m, cams, znear, attrs, label, cull, frames_per_call)
    import torch
    from . import ops
    dev = trimesh.device_of(m['vertices'])
    vertices, triangles = trimesh.on_device(m, V, T, dev)
    fattrs, lab = trimesh.vertex_attributes(m, attrs, label, V, dev)
    F = cams.shape[0]
    per = int(frames_per_call) if frames_per_call is not None else default_frames_per_call(F, T, h, w)
    cams_dev = torch.as_tensor(cams).to(dev)
    out = {k: [] for k in ('tri', 'depth', 'bary') + tuple(fattrs) + ((label,) if lab is not None else ())}
    counts, frames = [], []
    for f0 in range(0, F, per):
        c = cams_dev[f0:f0 + per].contiguous()
        n = int(c.shape[0])
        if n * T >= 2 ** 31 or n * h * w >= 2 ** 31:
            raise ValueError('raster.render_mesh: %d frames of %d x %d and %d triangles in one call: frames x triangles and '
                             'frames x pixels must stay below 2^31; lower frames_per_call' % (n, h, w, T))
        cnt, ws = ops.raster_setup(c, h, w, vertices, triangles, znear, cull)
        row = cnt.cpu().numpy().astype(np.int64)                   # the one read-back of the call
        if row[0] >= 2 ** 31 - 1:
            raise ValueError('raster.render_mesh: the pair list of %d frames reaches 2^31 entries; lower frames_per_call' % n)
        tri, depth, bary = ops.raster_draw(n, T, h, w, ws, int(row[0]))
        out['tri'].append(tri), out['depth'].append(depth), out['bary'].append(bary)
        for key, a in fattrs.items():
            out[key].append(ops.raster_interp(triangles, tri, bary, V, attr_f=a)[0])
        if lab is not None:
            out[label].append(ops.raster_interp(triangles, tri, None, V, attr_i=lab, fill=-1)[1])
        counts.append(row)
        frames.append((f0, f0 + n))
    res = {k: torch.cat(x) for k, x in out.items()}
    res['mask'] = res['tri'] >= 0
    res['counts'], res['frames'] = np.stack(counts), frames
    return res


def _pose(p):
    """None, (c [3], R [3,3]) as mesh.extract_object returns it, or a 6-vector (centre, rotation vector) -> (c, R) float64"""
    from . import mesh
    if p is None:
        return None
    if len(p) == 2:
        c, R = np.asarray(p[0], np.float64).reshape(3), np.asarray(p[1], np.float64).reshape(3, 3)
        return c, R
    p = np.asarray(p, np.float64).reshape(6)
    return p[:3], mesh.aa2matrix(p[3:])


def merge(meshes, poses=None, ts=0):
    """Several meshes as one, on the host.  meshes: a list of mesh dicts -- or mesh.extract_scene's dict, whose background and
    object meshes are taken with the objects' poses of timestep `ts` (poses[ts, k]).  poses: per mesh None (already in the
    world) or the pose of its frame, (c, R) or (centre, rotation vector): X = c + R^T P, the object -> world map of
    mesh.extract_object; normals turn with it.  Triangle ids are offset; rgb, normals, owner and component are carried when
    every mesh has them; `part` [V] int32 says which mesh a vertex came from.  -> dict of host arrays."""
    if isinstance(meshes, dict):
        scene = meshes
        if poses is not None:
            raise ValueError('raster.merge: a scene brings its own poses')
        all_poses = np.asarray(scene['poses'], np.float64)
        objs = list(scene.get('objects', ()))
        if objs and not 0 <= int(ts) < all_poses.shape[0]:
            raise ValueError('raster.merge: ts = %r of %d timesteps' % (ts, all_poses.shape[0]))
        meshes = [scene['background']] + objs
        poses = [None] + [all_poses[int(ts), k, :6] for k in range(len(objs))]
    meshes = list(meshes)
    poses = [None] * len(meshes) if poses is None else list(poses)
    if not meshes or len(poses) != len(meshes):
        raise ValueError('raster.merge: %d meshes and %d poses' % (len(meshes), len(poses)))
    keep = [k for k in ATTRIBUTES if all(x.get(k) is not None for x in meshes)]
    V, T, A, part, off = [], [], {k: [] for k in keep}, [], 0
    for i, (x, p) in enumerate(zip(meshes, poses)):
        v = _host(x['vertices']).astype(np.float64).reshape(-1, 3)
        t = _host(x['triangles']).astype(np.int64).reshape(-1, 3)
        p = _pose(p)
        if p is not None:
            v = p[0] + v @ p[1]                                     # rows: c + R^T P
        if off + v.shape[0] >= 2 ** 31:
            raise ValueError('raster.merge: more than 2^31 - 1 vertices')
        V.append(v.astype(np.float32))
        T.append((t + off).astype(np.int32))
        for k in keep:
            a = _host(x[k])
            if k == 'normals' and p is not None:
                a = (a.astype(np.float64) @ p[1]).astype(np.float32)
            if k == 'rgb' and a.dtype == np.uint8:
                a = a.astype(np.float32) / np.float32(255.0)
            A[k].append(a)
        part.append(np.full(v.shape[0], i, np.int32))
        off += v.shape[0]
    out = dict(vertices=np.concatenate(V), triangles=np.concatenate(T), part=np.concatenate(part))
    for k in keep:
        out[k] = np.concatenate(A[k])
    return out


def depth_error(mesh_depth, distance, acc, min_acc=0.5):
    """The mesh's depth against the renderer's `distance` for the same cameras, where both see a surface: the mesh covers the
    pixel (depth > 0) and acc >= min_acc.  -> dict pixels, both, mesh_only, render_only, abs_mean, abs_median, abs_max, rms,
    rel_mean, rel_median (None where `both` is 0).  One copy of the three pictures to the host, float64 there."""
    d, r, a = (_host(x).astype(np.float64) for x in (mesh_depth, distance, acc))
    r, a = r.reshape(d.shape), a.reshape(d.shape)
    seen_m, seen_r = d > 0, (a >= float(min_acc)) & np.isfinite(r)
    both = seen_m & seen_r
    n = int(both.sum())
    out = dict(pixels=int(d.size), both=n, mesh_only=int((seen_m & ~seen_r).sum()), render_only=int((seen_r & ~seen_m).sum()),
               min_acc=float(min_acc))
    e = np.abs(d[both] - r[both])
    with np.errstate(all='ignore'):
        rel = e / np.abs(r[both])
    stat = lambda fn, x: float(fn(x)) if n else None
    out.update(abs_mean=stat(np.mean, e), abs_median=stat(np.median, e), abs_max=stat(np.max, e), rms=stat(lambda x: np.sqrt(np.mean(x * x)), e),
               rel_mean=stat(np.mean, rel), rel_median=stat(np.median, rel))
    return out


def write_depth(base, depth, mask=None):
    """depth [h,w] on the device -> base + '.npy' (the float32 depth itself) and base + '.ppm' (vis.visualize_depth under
    turbo over the covered pixels; an uncovered pixel is black)"""
    import torch
    from . import trajectory, vis
    mask = (depth > 0) if mask is None else mask.to(torch.bool)
    np.save(base + '.npy', depth.cpu().numpy().astype(np.float32))
    if bool(mask.any()):
        far = depth[mask].max()
        pic = vis.visualize_depth(torch.where(mask, depth, far), mask.to(torch.float32), out8=True)
        pic = torch.where(mask[..., None], pic, torch.zeros_like(pic))
    else:
        pic = torch.zeros(tuple(depth.shape) + (3,), dtype=torch.uint8, device=depth.device)
    trajectory.write_ppm(base + '.ppm', pic)


def id_colours(ids):
    """ids [...] int32 -> uint8 [...,3]: the sinebow at id x the golden ratio (neighbouring ids far apart), black below 0"""
    import torch
    from . import vis
    hue = torch.remainder(ids.to(torch.float32) * 0.6180339887, 1.0)
    rgb = torch.round(vis.sinebow(hue).clamp(0.0, 1.0) * 255.0).to(torch.uint8)
    return torch.where((ids >= 0)[..., None], rgb, torch.zeros_like(rgb))


def write_ids(path, ids):
    """ids [h,w] int32 on the device (the owner, component, part or triangle picture) -> a PPM of id_colours"""
    from . import trajectory
    trajectory.write_ppm(path, id_colours(ids))
