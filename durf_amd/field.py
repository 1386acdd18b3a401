"""The field itself at world points: density and colour at any position, over regular grids, and top-down maps of a grid's
columns (include/durf_field.h, csrc/field.hip, libdurf_field.so).  Everything else the package renders is a picture of the
field along rays; this asks the model what is AT a point -- the way to occupancy grids, top-down density maps of a street,
collision checks against the learned scene, and a look at what a BoxMLP has learned inside its box.

    f = query(model, variables, points, viewdirs, ext=ext, ts=3)          # density [n], rgb [n,3], owner, valid, raw [n,4]
    g = grid(model, variables, origin=(-20, -20, 0), shape=(128, 128, 32), step=0.25, ext=ext)
    m = columns(g, threshold=5.0)                                         # max, opacity, first along the grid's last axis
    write_density('out/density', g)

What "the field at X" means: a point inside exactly one enabled box k is evaluated by BoxMLP_k in the box's frame
plus the background MLP's constant term (what the renderer adds on a box-hit ray), owner = k; a point in no box by the
background MLP through the contraction, owner = -1; a point in several boxes is no geometry: owner = -2, NaN, valid = 0.  The
MLPs are the exact-fp32 kernels (a measuring instrument); a bf16 route is out of scope."""
import json

import numpy as np

from . import lattice


def _refuse(model, variables, entry):
    if model.use_viewdirs is False or not variables.layout.use_viewdirs:
        raise NotImplementedError('%s: use_viewdirs=False has no point-wise field here (the view layer is part of both MLPs the '
                                  'query evaluates)' % entry)
    if not model.dynamics and variables.layout.K > 0:
        raise NotImplementedError('%s: dynamics=False with K = %d boxes: its box-hit rays feed object-frame coordinates to the '
                                  'background network, there is no point-wise field' % (entry, variables.layout.K))
    if variables.flat.device.type != 'cuda':
        raise NotImplementedError('%s: the parameter tree is on %s; the query runs on the device only' % (entry, variables.flat.device))


def _args(model, variables, entry, ext, sigma, ts, alpha, pose, box_enable, inside_tol):
    """the checks, the scene edit and the parameter half of durf_field_args -> (FieldArgs, keep-alive)"""
    import torch
    from . import obbpose_model as om, ops
    _refuse(model, variables, entry)
    model._check()
    if not (float(sigma) >= 0.0):
        raise ValueError('%s: sigma = %r, expected >= 0' % (entry, sigma))
    if not (float(inside_tol) >= 0.0):
        raise ValueError('%s: inside_tol = %r, expected >= 0' % (entry, inside_tol))
    lay = variables.layout
    K, dev = lay.K, variables.flat.device
    if K > 0 and ext is None:
        raise ValueError('%s: ext [K,3] (the boxes\' half extents) is needed for K = %d boxes' % (entry, K))
    if pose is None and float(ts) != int(ts):
        pose = model.interpolate_pose(variables, float(ts))
    p, en = model._scene_edit(variables, int(ts), pose, box_enable)
    bk = variables.mlp_flat('MLP_0')
    bws = ops.mlp_f32_pack(om.W_BKGD, om.IN_BKGD, bk)
    obj = ows = trunk = e = None
    stride = lay.mlp_size[om.W_OBJ]
    if K:
        o0 = lay.mlp_off['BoxMLP_0']
        obj = variables.flat[o0:o0 + K * stride]
        ows = ops.mlp_f32_pack(om.W_OBJ, om.IN_OBJ, obj, K=K, param_stride=stride)
        trunk = ops.bkgd_const_trunk_f32(bk)
        e = torch.as_tensor(ext).detach().to(device=dev, dtype=torch.float32).reshape(-1, 3).contiguous()
        if tuple(e.shape) != (K, 3):
            raise ValueError('%s: ext of shape %s, expected (%d, 3)' % (entry, tuple(e.shape), K))
    return ops.field_args(K, bk, bws, obj, stride, ows, trunk, p if K else None, e, en, sigma, alpha, model.contraction, inside_tol,
                          model.density_bias)


def _points(x, name, dev, entry):
    import torch
    t = torch.as_tensor(x)
    if t.dim() != 2 or t.shape[1] != 3:
        raise ValueError('%s: %s of shape %s, expected [n,3]' % (entry, name, tuple(t.shape)))
    return t.detach().to(device=dev, dtype=torch.float32).contiguous()


def query(model, variables, points, viewdirs=None, sigma=0.0, ts=0, alpha=10.0, pose=None, box_enable=None, chunk=65536,
          inside_tol=0.0, ext=None):
    """The field at points [n,3] (world frame) as ONE library call (durf_field_query) -> dict: density [n], rgb [n,3] (None
    when viewdirs is None: a density-only query), owner [n] int32 (the box that owns the point, -1 background, -2 several
    boxes), valid [n] uint8, raw [n,4] (r, g, b, density before the activations).  viewdirs [n,3]: the world-frame view
    direction per point, for both networks.  sigma >= 0: the point is an isotropic Gaussian of that standard deviation (0: the
    plain positional encoding).  ts: the timestep whose box poses hold (a fractional ts interpolates them, interpolate_pose);
    pose [K,6] / box_enable [K]: the scene edits of render_layers; ext [K,3]: the boxes' half extents.  alpha: the BARF
    schedule value of the object encoding (10: all weights 1).  inside_tol: a point within ext (1 + inside_tol) is inside."""
    from . import ops
    a, keep = _args(model, variables, 'field.query', ext, sigma, ts, alpha, pose, box_enable, inside_tol)
    dev = variables.flat.device
    pts = _points(points, 'points', dev, 'field.query')
    vd = None if viewdirs is None else _points(viewdirs, 'viewdirs', dev, 'field.query')
    if vd is not None and vd.shape[0] != pts.shape[0]:
        raise ValueError('field.query: %d view directions for %d points' % (vd.shape[0], pts.shape[0]))
    if int(chunk) <= 0:
        raise ValueError('field.query: chunk = %r' % (chunk,))
    return ops.field_query(a, pts, vd, chunk)


def grid(model, variables, origin, shape, step=None, axes=None, view=None, sigma=0.0, ts=0, alpha=10.0, pose=None, box_enable=None,
         chunk=65536, inside_tol=0.0, ext=None, want_points=False):
    """The field over the regular grid X(i, j, k) = origin + i du + j dv + k dw, shape = (nu, nv, nw), k fastest, as ONE library
    call (durf_field_grid: the points are built chunk by chunk on the device).  step: one spacing along x, y, z; or axes =
    (du, dv, dw), three vectors.  view: one direction for the whole grid, or None (density only).  -> query's dict with
    [nu,nv,nw,.] tensors, plus `frame` (origin, du, dv, dw, shape: what write_density records) and, with want_points,
    points [nu,nv,nw,3]."""
    from . import ops
    frame = lattice.frame(origin, shape, step, axes, 'field.grid')
    shape = tuple(frame['shape'])
    if int(chunk) <= 0:
        raise ValueError('field.grid: chunk = %r' % (chunk,))
    a, keep = _args(model, variables, 'field.grid', ext, sigma, ts, alpha, pose, box_enable, inside_tol)
    res = ops.field_grid(a, frame['origin'], frame['du'], frame['dv'], frame['dw'], shape, view, chunk, variables.flat.device, want_points)
    out = {k: (None if v is None else v.reshape(shape + tuple(v.shape[1:]))) for k, v in res.items()}
    out['frame'] = frame
    return out


def columns(g, step=None, threshold=1.0):
    """The top-down map of a grid (durf_field_columns): along the grid's last axis, per column, `max` the largest valid density,
    `opacity` = 1 - exp(-step sum density) (step: the spacing along that axis; None: |dw| of the grid's frame) and `first` the
    first k whose density reaches `threshold` (-1: none) -> dict of [nu,nv] tensors.  g: grid()'s result, or any dict with
    density and valid [nu,nv,nw]."""
    from . import ops
    d, v = g['density'], g['valid']
    if step is None:
        step = float(np.linalg.norm(np.asarray(g['frame']['dw'], np.float64)))
    cmax, cop, cfirst = ops.field_columns(d.contiguous().reshape(-1), v.contiguous().reshape(-1), tuple(d.shape), step, threshold)
    return dict(max=cmax, opacity=cop, first=cfirst)


def write_density(path, g):
    """path.npy: the grid's density [nu,nv,nw] float32 (NaN where invalid); path.json: the grid's frame (origin, du, dv, dw,
    shape; cell (i, j, k) is at origin + i du + j dv + k dw)"""
    d = g['density']
    d = d.cpu().numpy() if hasattr(d, 'cpu') else np.asarray(d)
    np.save(path + '.npy', np.asarray(d, np.float32))
    with open(path + '.json', 'w') as f:
        json.dump(dict(g['frame'], file=path.split('/')[-1] + '.npy', order='k fastest'), f, indent=1)


def _plane8(plane):
    a = plane.cpu().numpy() if hasattr(plane, 'cpu') else np.asarray(plane)
    if a.dtype != np.uint8:
        a = np.rint(np.clip(np.nan_to_num(np.asarray(a, np.float64)), 0.0, 1.0) * 255.0).astype(np.uint8)
    return a


def write_ppm(path, rgb):
    """a colour map [h,w,3] (uint8, or float in [0, 1]) -> binary PPM, by trajectory's writer"""
    from . import trajectory
    trajectory.write_ppm(path, _plane8(rgb))


def write_pgm(path, plane):
    """a map [h,w] (uint8, or float in [0, 1]; NaN is black) -> binary PGM (P5, maxval 255)"""
    a = _plane8(plane)
    if a.ndim != 2:
        raise ValueError('write_pgm: [h,w], got %s' % (a.shape,))
    with open(path, 'wb') as f:
        f.write(b'P5\n%d %d\n255\n' % (a.shape[1], a.shape[0]))
        f.write(np.ascontiguousarray(a).tobytes())
