"""Depth visualisations of the reference's evaluation block (internal/vis.py; train_boxpose.py:558 vis.visualize_suite) on the
device: names, argument order and defaults are the reference's, torch device tensors go in and come out, and any leading
dimensions of `depth` are frames ([..., H, W] -> [..., H, W, 3]).  The pixels are csrc/vis.hip's (ops.vis_*): one statistics
call of three launches for the automatic near / far planes and the normal scale, then one launch per picture, none of which
waits for the device.  out8=True returns uint8 pictures (rintf(clamp(x, 0, 1) * 255), a NaN is 0) and no float picture is
ever written.

Where the reference's arithmetic has a quirk it is kept (far is NaN, and the whole picture the map's first colour, as soon
as one depth is NaN; near > far still normalises by |far - near|; with modulus > 0 a NaN depth stays NaN)."""
import torch

from . import ops

EPS = float(torch.finfo(torch.float32).eps)


def _frames(depth, acc):
    """[..., H, W] -> contiguous fp32 [F, H, W] views and the leading shape"""
    if depth.dim() < 2:
        raise ValueError('depth: [..., H, W], got %s' % (tuple(depth.shape),))
    lead = tuple(depth.shape[:-2])
    H, W = depth.shape[-2:]
    d = depth.to(torch.float32).reshape(-1, H, W).contiguous()
    a = None
    if acc is not None:
        if acc.shape != depth.shape:
            raise ValueError('acc %s against depth %s' % (tuple(acc.shape), tuple(depth.shape)))
        a = acc.to(torch.float32).reshape(-1, H, W).contiguous()
    return d, a, lead


def _picture(pair, lead, out8):
    t = pair[1] if out8 else pair[0]
    return t.reshape(lead + tuple(t.shape[1:]))


def sinebow(h):
    """A cyclic and uniform colormap, see http://basecase.org/env/on-rainbows: [...] -> [..., 3]"""
    return ops.vis_sinebow(h.to(torch.float32).contiguous())[0]


def depth_to_normals(depth):
    """Assuming `depth` is orthographic, linearize it to a set of normals: [..., H, W] -> [..., H, W, 3]"""
    d, _, lead = _frames(depth, None)
    return _picture(ops.vis_normals(d, None, None, raw=True), lead, False)


def _sorted_range(d, a, ignore_frac):
    """near / far of vis.py:77-91 for ignore_frac > 0: per frame, sort the depths (NaNs last), accumulate acc (0 where the
    depth is NaN) in that order and keep the depths whose running sum lies within [ignore_frac, 1 - ignore_frac] of the total;
    near / far are the first / last kept depth -/+ eps.  torch.sort + cumsum on the device, no read-back -- so a frame whose
    mask is empty (the reference raises there) silently takes its least depth for both.  The running sum is float64: which
    depth the threshold falls on must not depend on fp32 summation order."""
    F = d.shape[0]
    flat = d.reshape(F, -1)
    w = torch.ones_like(flat) if a is None else a.reshape(F, -1)
    w = torch.where(torch.isnan(flat), torch.zeros_like(w), w)
    ds, idx = torch.sort(flat, dim=1)
    cum = torch.cumsum(torch.gather(w, 1, idx).to(torch.float64), dim=1)
    total = cum[:, -1:]
    mask = (cum >= total * ignore_frac) & (cum <= total * (1 - ignore_frac))
    first = torch.argmax(mask.to(torch.uint8), dim=1, keepdim=True)
    last = flat.shape[1] - 1 - torch.argmax(mask.flip(1).to(torch.uint8), dim=1, keepdim=True)
    last = torch.where(mask.any(dim=1, keepdim=True), last, first)
    return torch.cat([torch.gather(ds, 1, first) - EPS, torch.gather(ds, 1, last) + EPS], dim=1)


def _range(d, a, near, far, ignore_frac, stats):
    """the [F, >= 2] device range visualize_depth hands the kernel: the statistics record itself when both planes are
    automatic, otherwise a [F,2] buffer with the caller's planes written over the automatic ones (`near or ...`: None and 0
    mean automatic; a tensor -- 0-d or [F] -- is always the caller's value, its truth is not read back)"""
    auto_near = near is None or (not torch.is_tensor(near) and not near)
    auto_far = far is None or (not torch.is_tensor(far) and not far)
    if ignore_frac:
        rng = _sorted_range(d, a, ignore_frac)
    elif auto_near or auto_far:
        rng = stats if stats is not None else ops.vis_stats(d)
    else:
        rng = torch.empty(d.shape[0], 2, device=d.device)
    if auto_near and auto_far:
        return rng
    rng = rng[:, :2].clone()
    for col, auto, val in ((0, auto_near, near), (1, auto_far, far)):
        if not auto:
            rng[:, col] = val.to(device=d.device, dtype=torch.float32) if torch.is_tensor(val) else float(val)
    return rng


def visualize_depth(depth, acc=None, near=None, far=None, ignore_frac=0, curve_fn='neglog', modulus=0, colormap=None,
                    out8=False, _stats=None):
    """Visualize a depth map (vis.visualize_depth).

    depth [..., H, W]; acc like depth, in [0, 1], or None; near / far: the planes, None or 0 = automatic (the least / greatest
    depth, a NaN far plane if any depth is NaN); ignore_frac: fraction of acc to ignore on either side when the planes are
    automatic; curve_fn: 'neglog' (-log(x + eps), the default: near is red, far is blue under turbo), 'identity' or 'inverse'
    (1 / (x + eps)), applied to depth, near and far; modulus > 0: the curved depth modulo `modulus` through the sinebow;
    colormap: None (turbo, or the sinebow with a modulus) or a [256,3] tensor of colours."""
    d, a, lead = _frames(depth, acc)
    lut = None if colormap is None else colormap.to(device=d.device, dtype=torch.float32).contiguous()
    rng = None if modulus > 0 else _range(d, a, near, far, ignore_frac, _stats)
    return _picture(ops.vis_depth(d, a, rng, curve_fn, modulus, lut, want_float=not out8, want_u8=bool(out8)), lead, out8)


def visualize_normals(depth, acc, scaling=None, out8=False, _stats=None):
    """Visualize fake normals of `depth` (optionally scaled to be isotropic): scaling None = sqrt(((var x + var y) / 2) /
    var depth) per frame over the non-NaN pixels; a number, or a tensor of one value per frame, otherwise."""
    d, a, lead = _frames(depth, acc)
    if scaling is None:
        scale = (_stats if _stats is not None else ops.vis_stats(d))[:, 2]
    elif torch.is_tensor(scaling):
        scale = scaling.to(device=d.device, dtype=torch.float32).reshape(-1).expand(d.shape[0]).contiguous()
    else:
        scale = torch.full((d.shape[0],), float(scaling), device=d.device)
    return _picture(ops.vis_normals(d, a, scale, want_float=not out8, want_u8=bool(out8)), lead, out8)


def visualize_suite(depth, acc, out8=False):
    """A wrapper around other visualizations for easy integration: {'depth', 'depth_mod', 'depth_normals'} -- six launches
    for any number of frames (the statistics are computed once and shared)."""
    d, _, _ = _frames(depth, None)
    stats = ops.vis_stats(d)
    return {
        'depth': visualize_depth(depth, acc, out8=out8, _stats=stats),
        'depth_mod': visualize_depth(depth, acc, modulus=0.1, out8=out8),
        'depth_normals': visualize_normals(depth, acc, out8=out8, _stats=stats),
    }
