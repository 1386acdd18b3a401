"""The regular lattice on the host: X(i, j, k) = ((origin + i du) + j dv) + k dw, shape = (nu, nv, nw), k fastest, the object
field, mesh, parts, tsdf and closest share (csrc/lattice.h is the device side).  Every module that builds a frame,
refuses a shape, inverts a frame or takes a lattice dict apart does it here, under its own entry name.  numpy only at import."""
import numpy as np


# (two helpers with no lattice in them live here because this is the numpy-only module that mesh, tsdf, raster, closest and
# geometry can all import without a cycle: _host, an array on the host, and _max_dist, the distance cap of closest and geometry)
def _host(a):
    return a.detach().cpu().numpy() if hasattr(a, 'detach') else np.asarray(a)


def _max_dist(max_dist, entry, inf=False):
    md = float(np.float32(max_dist))
    if not ((inf and md == float('inf')) or 1e-18 <= md <= 1e18):
        raise ValueError('%s: max_dist = %r, expected %s number in [1e-18, 1e18]' % (entry, max_dist, '+inf or a' if inf else 'a'))
    return md


def frame(origin, shape=None, step=None, axes=None, entry='lattice.frame', scaled=False):
    """The frame dict(origin, du, dv, dw).  step: one spacing along x, y, z, XOR axes = (du, dv, dw): lists of Python floats, plus
    `shape` (a list) when one is given -- what field.grid and tsdf.volume record.  scaled=True is closest.grid's rule instead: step
    (one, or one per axis) times the rows of `axes` (default: the world axes), all finite, as float32 arrays."""
    if scaled:
        o = np.asarray(origin, np.float32).reshape(-1)
        A = np.eye(3, dtype=np.float64) if axes is None else np.asarray(axes, np.float64).reshape(3, 3)
        st = np.broadcast_to(np.asarray(step, np.float64).reshape(-1), (3,)) if np.size(step) in (1, 3) else None
        if o.size != 3 or st is None or not (np.isfinite(o).all() and np.isfinite(A).all() and np.isfinite(st).all()):
            raise ValueError('%s: origin = %r, step = %r: three finite floats and one or three finite steps' % (entry, origin, step))
        du, dv, dw = ((A[i] * st[i]).astype(np.float32) for i in range(3))
        return dict(origin=o, du=du, dv=dv, dw=dw)
    if (step is None) == (axes is None):
        raise ValueError('%s: give step or axes' % entry)
    if axes is None:
        s = float(step)
        axes = ((s, 0.0, 0.0), (0.0, s, 0.0), (0.0, 0.0, s))
    du, dv, dw = ([float(x) for x in v] for v in axes)
    f = dict(origin=[float(x) for x in origin], du=du, dv=dv, dw=dw)
    if shape is not None:
        f['shape'] = [int(s) for s in shape]
    if any(len(v) != 3 for v in f.values()):
        raise ValueError('%s: origin, the axes and shape have three components each' % entry)
    return f


def check_shape(shape, entry):
    """the lattices mesh, parts and tsdf take (include/durf_mesh.h) -> the shape as a tuple of ints"""
    shape = tuple(int(s) for s in shape)
    if min(shape) < 2 or shape[0] * shape[1] * shape[2] >= 2 ** 27:
        raise ValueError('%s: a lattice of %d x %d x %d points (each dimension >= 2, fewer than 2^27 points)' % ((entry,) + shape))
    return shape


def host(frame, entry):
    """frame dict -> (origin, du, dv, dw float32 [3], A float32 [9]: the inverse transpose of [du dv dw], computed in float64 from
    the float32 values the library receives, flip: the frame is left-handed).  A singular frame is refused."""
    o, du, dv, dw = (np.asarray(frame[k], np.float64).reshape(-1).astype(np.float32) for k in ('origin', 'du', 'dv', 'dw'))
    if any(v.size != 3 for v in (o, du, dv, dw)):
        raise ValueError('%s: origin, du, dv and dw have three components each' % entry)
    J = np.stack([du, dv, dw], 1).astype(np.float64)
    det = float(np.linalg.det(J))
    scale = float(np.linalg.norm(J[:, 0]) * np.linalg.norm(J[:, 1]) * np.linalg.norm(J[:, 2]))
    if not np.isfinite(J).all() or not np.isfinite(o).all() or not abs(det) > 1e-9 * scale:
        raise ValueError('%s: a singular frame (det [du dv dw] = %g): du = %s, dv = %s, dw = %s'
                         % (entry, det, du.tolist(), dv.tolist(), dw.tolist()))
    return o, du, dv, dw, np.linalg.inv(J).T.astype(np.float32).reshape(-1), det < 0


def device_lattice(g, entry, with_frame=False):
    """g: any dict(density= [nu,nv,nw] on the device, valid= uint8 or None) -> (density float32, valid, both contiguous, shape);
    with_frame: plus host(g['frame']), refused after the shape and before `valid`, as mesh.surface always did"""
    import torch
    d = g['density']
    if not (torch.is_tensor(d) and d.is_cuda and d.dim() == 3):
        raise ValueError('%s: density is a [nu,nv,nw] tensor on the device' % entry)
    shape = check_shape(d.shape, entry)
    frame = (host(g['frame'], entry),) if with_frame else ()
    d = d.to(torch.float32).contiguous()
    v = g.get('valid')
    if v is not None:
        v = v.to(device=d.device, dtype=torch.uint8).contiguous()
        if tuple(v.shape) != shape:
            raise ValueError('%s: valid of shape %s for a lattice of %s' % (entry, tuple(v.shape), shape))
    return (d, v, shape) + frame
