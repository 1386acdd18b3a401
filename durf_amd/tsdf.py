"""Depth frames fused into a truncated signed distance (TSDF) volume, on the device (include/durf_tsdf.h, csrc/tsdf.hip,
libdurf_tsdf.so): the surface the renderer SHOWS -- its `distance` from many cameras -- as a mesh, instead of an iso-surface of
raw density whose place moves with `iso`.

    vol = volume(origin, shape, step=0.25, trunc=0.75)
    integrate(vol, cams, frames['distance'], acc=frames['acc'], rgb=frames['rgb'])       # F frames, one launch
    m = surface(vol, min_points=64)                                                      # mesh.write_ply / raster.render_mesh take it
    d = sample(vol, lidar_points)['sdf']                                                 # signed distance to the fused surface
    s = fuse_scene(model, variables, cams, times, ext, white_bkgd, alpha, origin, shape, step, trunc, obj_step=0.05)

Every voxel looks its own depth up (the nearest pixel, never interpolated) and takes a running weighted mean: a gather with no
atomics, whose result is defined bit for bit and does not depend on how the frames are split into calls.  The street is fused
from the `background` layer, where the boxes are switched off; every vehicle in its own box frame over all the timesteps it
moves through, from the pixels the instance map gives it.  The known artefact is documented, not repaired: a
false surface at the back of the truncation band where another camera sees free space."""
import numpy as np

from . import camera, lattice as lat                  # (lattice() below is this module's own function)
from .lattice import _host


def volume(origin, shape, step=None, axes=None, trunc=None, colour=True, device=None):
    """A new volume over the lattice X(i, j, k) = origin + i du + j dv + k dw (field.grid's arguments: step, one spacing along
    x, y, z, or axes = (du, dv, dw)); trunc: the half width of the band, in scene units (a few voxel steps) -> dict tsdf, weight
    [nu,nv,nw] float32 and colour [nu,nv,nw,4] (None with colour=False) on the device, all zero, plus frame, shape and trunc."""
    import torch
    frame = lat.frame(origin, shape, step, axes, 'tsdf.volume')
    shape = lat.check_shape(shape, 'tsdf.volume')
    if trunc is None or not (float(trunc) > 0 and np.isfinite(float(trunc))):
        raise ValueError('tsdf.volume: trunc = %r, expected a finite number > 0 (the half width of the band, in scene units)' % (trunc,))
    lat.host(frame, 'tsdf.volume')                                       # a singular frame is refused here, not at sample()
    dev = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
    return dict(tsdf=torch.zeros(shape, device=dev), weight=torch.zeros(shape, device=dev),
                colour=torch.zeros(shape + (4,), device=dev) if colour else None, frame=frame, shape=shape, trunc=float(trunc))


def _check_volume(vol, entry):
    if not isinstance(vol, dict) or any(vol.get(k) is None for k in ('tsdf', 'weight', 'frame', 'shape', 'trunc')):
        raise ValueError('%s: vol is tsdf.volume\'s dict (tsdf, weight, colour, frame, shape, trunc)' % entry)
    shape = tuple(int(s) for s in vol['shape'])
    for k in ('tsdf', 'weight'):
        if tuple(vol[k].shape) != shape:
            raise ValueError('%s: vol[%r] of shape %s for a lattice of %s' % (entry, k, tuple(vol[k].shape), shape))
    if vol.get('colour') is not None and tuple(vol['colour'].shape) != shape + (4,):
        raise ValueError('%s: vol[\'colour\'] of shape %s for a lattice of %s' % (entry, tuple(vol['colour'].shape), shape))
    return shape


def check_frames(cams, depth, acc=None, rgb=None, label=None, select=None, carve=False, xform=None, frame_weight=None, min_acc=0.5,
                 max_weight=64.0, znear=1e-2, entry='tsdf.integrate'):
    """every refusal of integrate that needs no device, from shapes alone -> (F, h, w)"""
    cs, ds = tuple(cams.shape), tuple(depth.shape)
    camera.check_shape(cs, entry)
    if len(ds) != 3 or ds[0] != cs[0]:
        raise ValueError('%s: depth of shape %s for %d cameras, expected [F,h,w]' % (entry, ds, cs[0]))
    F, h, w = ds
    if not (1 <= h <= 4096 and 1 <= w <= 4096):
        raise ValueError('%s: frames of %d x %d, expected 1 .. 4096 each way' % (entry, h, w))
    if F * h * w >= 2 ** 31:
        raise ValueError('%s: %d frames of %d x %d in one call: frames x pixels must stay below 2^31' % (entry, F, h, w))
    for name, a, want in (('acc', acc, (F, h, w)), ('rgb', rgb, (F, h, w, 3)), ('label', label, (F, h, w)), ('xform', xform, (F, 3, 4)),
                          ('frame_weight', frame_weight, (F,))):
        if a is not None and tuple(a.shape) != want:
            raise ValueError('%s: %s of shape %s, expected %s' % (entry, name, tuple(a.shape), want))
    if label is None and (select is not None or carve):
        raise ValueError('%s: select = %r, carve = %r without label' % (entry, select, carve))
    if label is not None and (select is None or int(select) != select):
        raise ValueError('%s: select = %r, expected the integer label this volume takes' % (entry, select))
    if not float(max_weight) > 0:
        raise ValueError('%s: max_weight = %r, expected a number > 0' % (entry, max_weight))
    if not float(znear) > 0:
        raise ValueError('%s: znear = %r, expected a number > 0' % (entry, znear))
    if acc is not None and not float(min_acc) == float(min_acc):
        raise ValueError('%s: min_acc = %r' % (entry, min_acc))
    return F, h, w


def integrate(vol, cams, depth, acc=None, rgb=None, label=None, select=None, carve=False, xform=None, frame_weight=None, min_acc=0.5,
              max_weight=64.0, znear=1e-2):
    """F frames into vol, IN PLACE, one launch (durf_tsdf_integrate; the header states the rule).  cams [F,CAM_FLOATS] camera rows; depth
    [F,h,w] camera depth (the renderer's `distance`, raster's depth; 0, NaN, inf and negative values are holes); acc [F,h,w]: a
    pixel below min_acc is no observation; rgb [F,h,w,3]; label int32 [F,h,w] with select: only pixels of that label are
    observations of this volume's surface -- with carve=True a pixel of another label whose depth lies beyond the voxel by at
    least trunc still counts as free space; xform [F,3,4]: the volume's coordinates to frame f's world (box_xforms);
    frame_weight [F].  Host or device arrays.  -> vol."""
    shape = _check_volume(vol, 'tsdf.integrate')
    F, h, w = check_frames(cams, depth, acc, rgb, label, select, carve, xform, frame_weight, min_acc, max_weight, znear)
    import torch
    from . import ops
    o, du, dv, dw = lat.host(vol['frame'], 'tsdf.integrate')[:4]
    dev = vol['tsdf'].device
    up = lambda a, dt: None if a is None else \
        torch.as_tensor(np.ascontiguousarray(a) if not torch.is_tensor(a) else a).to(device=dev, dtype=dt).contiguous()
    if F == 0:
        return vol
    ops.tsdf_integrate(vol['tsdf'], vol['weight'], vol.get('colour'), shape, o, du, dv, dw, up(cams, torch.float32), up(depth, torch.float32),
                       vol['trunc'], acc=up(acc, torch.float32), min_acc=min_acc, rgb=up(rgb, torch.float32), label=up(label, torch.int32),
                       select=0 if select is None else int(select), other_mode=int(bool(carve)), xform=up(xform, torch.float32),
                       frame_weight=up(frame_weight, torch.float32), max_weight=max_weight, znear=znear)
    return vol


def lattice(vol, min_weight=1.0):
    """what mesh.surface and parts.components take as they are: dict density [nu,nv,nw] = -D (with iso = 0 a point is in when it
    is at or behind the surface), valid uint8 (W >= min_weight), rgb [nu,nv,nw,3] (None without colour), frame"""
    shape = _check_volume(vol, 'tsdf.lattice')
    if not float(min_weight) == float(min_weight):
        raise ValueError('tsdf.lattice: min_weight = %r' % (min_weight,))
    from . import ops
    density, valid, rgb = ops.tsdf_lattice(vol['tsdf'], vol['weight'], vol.get('colour'), shape, min_weight)
    return dict(density=density, valid=valid, rgb=rgb, frame=dict(vol['frame']))


def surface(vol, min_weight=1.0, min_points=0, largest=None):
    """The zero level of the volume as a mesh: mesh.surface(lattice(vol), iso=0, attrs=('rgb',)), normals towards the observer,
    then (opt-in) parts.clean: drop the connected regions of fewer than min_points lattice points, or all but the `largest`
    biggest -> the dict mesh.write_ply and raster.render_mesh take, plus `observed` (the count of valid voxels, a device tensor)."""
    from . import mesh
    g = lattice(vol, min_weight)
    m = mesh.surface(g, 0.0, attrs=('rgb',) if g['rgb'] is not None else ())
    if g['rgb'] is None:
        m['rgb'] = None
    if min_points or largest is not None:
        from . import parts
        m, m['cleaning'] = parts.clean(m, g, 0.0, min_points=min_points, largest=largest)
    m['observed'] = g['valid'].sum()
    return m


def sample(vol, points, min_weight=1.0):
    """The signed distance of points [m,3] (host or device) to the fused surface, in scene units, positive in front of it:
    trilinear over the eight voxels around -> dict sdf [m] (NaN outside the lattice or next to a voxel with W < min_weight), ok
    [m] bool, rgb [m,3] (None without colour; 0 where a corner has no colour)."""
    shape = _check_volume(vol, 'tsdf.sample')
    if not float(min_weight) == float(min_weight):
        raise ValueError('tsdf.sample: min_weight = %r' % (min_weight,))
    if len(tuple(points.shape)) != 2 or points.shape[1] != 3:
        raise ValueError('tsdf.sample: points of shape %s, expected [m,3]' % (tuple(points.shape),))
    import torch
    from . import ops
    o, du, dv, dw, A, _ = lat.host(vol['frame'], 'tsdf.sample')
    inv = np.ascontiguousarray(A.reshape(3, 3).T)                            # lattice.host's A is the inverse TRANSPOSE of [du dv dw]
    dev = vol['tsdf'].device
    p = torch.as_tensor(np.ascontiguousarray(points) if not torch.is_tensor(points) else points).to(device=dev, dtype=torch.float32).contiguous()
    sdf, ok, rgb = ops.tsdf_sample(vol['tsdf'], vol['weight'], vol.get('colour'), shape, o, inv, vol['trunc'], p, min_weight)
    return dict(sdf=sdf, ok=ok.to(torch.bool), rgb=rgb)


def box_xforms(poses_fk6, k):
    """poses [F,K,6] (render_trajectory's: centre, rotation vector) -> [F,3,4] float32, box k's frame to the world of every
    frame: [R_f^T | c_f], X = c_f + R_f^T P, with R = mesh.aa2matrix in float64.  One host read of the poses."""
    from . import mesh
    p = np.asarray(_host(poses_fk6), np.float64)
    if p.ndim != 3 or p.shape[2] < 6 or not 0 <= int(k) < p.shape[1]:
        raise ValueError('tsdf.box_xforms: poses of shape %s and box %r, expected [F,K,6] and 0 <= k < K' % (p.shape, k))
    out = np.zeros((p.shape[0], 3, 4), np.float32)
    for f in range(p.shape[0]):
        out[f, :, :3] = mesh.aa2matrix(p[f, int(k), 3:6]).T
        out[f, :, 3] = p[f, int(k), :3]
    return out


def fuse_scene(model, variables, cams, times, ext, white_bkgd, alpha, origin, shape, step, trunc, obj_step=None, obj_trunc=None, pad=0.05,
               carve=False, near=None, far=None, chunk=8192, batch=8, min_acc=0.5, max_weight=64.0, znear=1e-2, min_weight=1.0,
               min_points=0, largest=None, objects=True):
    """The whole scene fused from rendered depth: cams [F,CAM_FLOATS] host camera rows and times [F] (render_trajectory's).  The poses
    [F,K,6] come from render_trajectory(outputs=()); per frame ONE render_layers call with layers=('instance', 'background') at
    ts = floor(t_f) and pose = poses[f].  The background volume (origin, shape, step, trunc) integrates bg_distance, bg_acc and
    bg_rgb: the street with every box switched off.  Object k's volume is mesh.object_lattice's lattice in the box's own frame
    (spacing obj_step, band obj_trunc: default 3 obj_step) and integrates the composite distance, acc and rgb with
    label=instance, select=k and xform=box_xforms(poses, k): the box is followed through all the timesteps it moves through.
    The frames are staged `batch` at a time: memory is bounded by the batch, not by F.  near, far: the ray bounds.
    -> dict background, objects (meshes as surface() returns them, the objects in their canonical frames), poses [T,K,6] (the
    model's table, what raster.merge reads; the poses of the frames are under frame_poses [F,K,6]) and volumes (dict
    background=, objects=[...])."""
    import torch
    from . import mesh, raygen
    cams = camera.as_rows(cams, 'tsdf.fuse_scene', one_size=False)[0]
    times = [float(t) for t in np.asarray(_host(times), np.float64).reshape(-1)]
    F = cams.shape[0]
    if len(times) != F:
        raise ValueError('tsdf.fuse_scene: %d cameras and %d times' % (F, len(times)))
    if near is None or far is None:
        raise ValueError('tsdf.fuse_scene: near and far are the ray bounds of the render (config.near, config.far)')
    if int(batch) < 1:
        raise ValueError('tsdf.fuse_scene: batch = %r' % (batch,))
    K = variables.layout.K if objects else 0
    if K and (obj_step is None or ext is None):
        raise ValueError('tsdf.fuse_scene: obj_step and ext are needed for K = %d boxes' % K)
    dev = variables.flat.device
    if variables.layout.K:
        poses = model.render_trajectory(variables, None, times, ext, white_bkgd, alpha, near=near, far=far, chunk=chunk, outputs=())['poses']
    else:
        poses = torch.zeros(F, 0, 6, device=dev)
    poses_host = poses.detach().cpu().numpy()                                # the one read of the poses
    bg_vol = volume(origin, shape, step=step, trunc=trunc, device=dev)
    obj_vols, xforms = [], []
    if K:
        e = np.asarray(_host(torch.as_tensor(ext)), np.float64).reshape(-1, 3)
        for k in range(K):
            frame, _, oshape = mesh.object_lattice(np.zeros(3), np.eye(3), e[k], obj_step, pad)
            obj_vols.append(volume(frame['origin'], oshape, axes=(frame['du'], frame['dv'], frame['dw']),
                                   trunc=3.0 * float(obj_step) if obj_trunc is None else obj_trunc, device=dev))
            xforms.append(box_xforms(poses_host, k))
    layers = ('instance', 'background') if variables.layout.K else ()
    kw = dict(min_acc=min_acc, max_weight=max_weight, znear=znear)
    for f0 in range(0, F, int(batch)):
        f1 = min(f0 + int(batch), F)
        names = ('bg_distance', 'bg_acc', 'bg_rgb') + (('distance', 'acc', 'rgb', 'instance') if K else ())
        stage = {k: [] for k in names}
        for f in range(f0, f1):
            rays = raygen.camera_rays(cams[f], near, far, device=dev)
            out = model.render_layers(variables, rays, None, ext, int(np.floor(times[f])), white_bkgd, alpha, chunk=chunk,
                                      pose=poses[f] if layers else None, layers=layers)
            if not layers:                                                   # a scene without boxes: the composite IS the background
                out = dict(bg_distance=out['distance'], bg_acc=out['acc'], bg_rgb=out['rgb'])
            h, w = out['bg_rgb'].shape[:2]
            for name in names:
                stage[name].append(out[name].reshape((h, w, 3) if name.endswith('rgb') else (h, w)))
        st = {k: torch.stack(v).contiguous() for k, v in stage.items()}
        c = cams[f0:f1]
        integrate(bg_vol, c, st['bg_distance'], acc=st['bg_acc'], rgb=st['bg_rgb'], **kw)
        for k in range(K):
            integrate(obj_vols[k], c, st['distance'], acc=st['acc'], rgb=st['rgb'], label=st['instance'], select=k, carve=carve,
                      xform=xforms[k][f0:f1], **kw)
    clean = dict(min_weight=min_weight, min_points=min_points, largest=largest)
    table = variables['params']['box_centers'].detach().cpu().numpy() if variables.layout.K else poses_host
    return dict(background=surface(bg_vol, **clean), objects=[surface(v, **clean) for v in obj_vols], poses=table,
                frame_poses=poses_host, volumes=dict(background=bg_vol, objects=obj_vols))
