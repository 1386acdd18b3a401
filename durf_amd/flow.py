"""How the scene moves between two rendered frames: optical flow, scene flow, the backward warp of one frame onto another
with its occlusion mask, a temporal-consistency number and the flow picture (include/durf_flow.h, csrc/flow.hip,
libdurf_flow.so).  The model knows the answer exactly -- a sample moves rigidly with the box that contains it, everything else
is static -- so nothing is learned or approximated and no MLP runs: the inputs are render_trajectory's own result.

    out = model.render_trajectory(variables, cams, times, ext, white_bkgd, alpha, near=near, far=far, outputs=('rgb', 'distance', 'acc'))
    fl = render_flow(out, cams, ext, near=near, far=far, outputs=('flow', 'valid', 'moving', 'target'))
    w = warp(fl, out['rgb'], frame_depth(out, cams, ext, near=near, far=far))      # frame f + 1 seen from frame f
    c = consistency(w, out['rgb'], fl['pairs'])                                    # count, mse, mae, psnr per pair
    write_flo('flow_0000.flo', fl['flow'][0], fl['valid'][0])

Conventions: flow[p] = (x' - x, y' - y) in pixels, x to the right and y down, of the point seen at pixel p of the source frame;
invalid pixels (too little accumulated weight, a ray through several boxes, a target behind the camera) hold NaN."""
import struct

import numpy as np

from . import camera

FLO_MAGIC = b'PIEH'
FLO_UNKNOWN = 1e10            # what an invalid pixel is written as; the format's threshold for "unknown" is 1e9
FLO_UNKNOWN_THRESH = 1e9


def default_pairs(F, backward=False):
    """f -> f + 1 for every consecutive pair, then (backward) f + 1 -> f: [P,2] int32"""
    fwd = [(f, f + 1) for f in range(F - 1)]
    return np.asarray(fwd + ([(b, a) for a, b in fwd] if backward else []), np.int32).reshape(-1, 2)


def render_flow(out, cams, ext, *, near, far, pairs=None, backward=False, normalise=True, min_acc=0.5, znear=1e-2, inside_tol=1e-3,
                box_enable=None, chunk=8192, outputs=('flow', 'valid', 'moving')):
    """Where every pixel of a source frame lands in a target frame, for P pairs of frames as ONE library call
    (durf_render_flow).  out: render_trajectory's own result -- it needs distance, acc [F,h,w] and poses [F,K,6]; cams [F,CAM_FLOATS]
    the camera rows it was rendered with, ext [K,3]; near / far as rendered (they only fill ray fields nothing here reads).
    pairs [P,2] (source, target); None: f -> f + 1 for every consecutive pair, backward = True adds f + 1 -> f.
    -> dict of [P,h,w,.] tensors for `outputs` (ops.FLOW_OUTPUTS: flow [.,2], scene_flow, xyz, target [.,3], zcam, moving --
    the box a pixel rides, -1 static, -2 invalid --, valid) plus pairs [P,2] (numpy).  normalise: divide distance by acc (the
    renderer's distance is not); min_acc: pixels with less accumulated weight are invalid; znear: a target nearer than that to
    the target camera's plane is invalid; inside_tol: a point within ext (1 + inside_tol) of its box rides it.
    box_enable: as rendered."""
    from . import ops
    missing = [k for k in ('distance', 'acc', 'poses') if k not in out]
    if missing:
        raise ValueError('render_flow needs the outputs %s of render_trajectory' % missing)
    cams, h, w = camera.as_rows(cams, 'flow.render_flow', one_size=False)
    F = int(cams.shape[0])
    pairs = default_pairs(F, backward) if pairs is None else np.asarray(pairs, np.int32).reshape(-1, 2)
    poses = out['poses']
    K, dev = int(poses.shape[1]), poses.device
    en = ops._enable(box_enable, K, dev) if K > 0 else None
    dist, acc = out['distance'].reshape(F, h * w), out['acc'].reshape(F, h * w)
    res = ops.render_flow(cams, poses, ext, dist, acc, pairs, near, far, chunk, box_enable=en, normalise=normalise, min_acc=min_acc,
                          znear=znear, inside_tol=inside_tol, outputs=outputs)
    res = {k: v.reshape((v.shape[0], h, w) + tuple(v.shape[2:])) for k, v in res.items()}
    res['pairs'] = pairs
    return res


def frame_depth(out, cams, ext, **kw):
    """every frame's own zcam [F,h,w] -- the depth along the camera's axis of what each pixel sees, NaN where invalid:
    render_flow with every frame as its own target.  What warp() tests occlusion against."""
    F = int(camera.as_rows(cams, 'flow.frame_depth', one_size=False)[0].shape[0])
    kw.pop('pairs', None)
    return render_flow(out, cams, ext, pairs=[(f, f) for f in range(F)], outputs=('zcam',), **kw)['zcam']


def warp(flows, images, zcam, *, occ_rel=0.02, occ_abs=0.0):
    """Every pair's target frame sampled where the source frame's pixels land (durf_flow_warp, one launch per pair): flows:
    render_flow's result with target, valid and pairs; images [F,h,w,C] float (C 1 or 3); zcam [F,h,w]: frame_depth().
    A pixel is visible when its target is valid, inside the picture, and not behind what the target frame sees there: z <=
    zcam (1 + occ_rel) + occ_abs.  -> dict: warped [P,h,w,C] (NaN where not visible), mask [P,h,w] int32."""
    import torch
    from . import ops
    missing = [k for k in ('target', 'valid', 'pairs') if k not in flows]
    if missing:
        raise ValueError('warp needs %s of render_flow\'s result' % missing)
    pairs = flows['pairs']
    P, h, w = (int(x) for x in flows['valid'].shape)
    C = int(images.shape[-1])
    warped = torch.empty(P, h, w, C, device=images.device)
    mask = torch.empty(P, h, w, dtype=torch.int32, device=images.device)
    for p in range(P):
        b = int(pairs[p][1])
        wp, mk = ops.flow_warp(flows['target'][p].reshape(-1, 3), flows['valid'][p].reshape(-1), images[b].contiguous(),
                               zcam[b].contiguous(), occ_rel, occ_abs)
        warped[p], mask[p] = wp.reshape(h, w, C), mk.reshape(h, w)
    return dict(warped=warped, mask=mask)


def consistency(warped, images, pairs):
    """How well every pair's warped target frame agrees with its source frame under the occlusion mask
    (durf_flow_consistency: deterministic, no atomics): warped: warp()'s result; images [F,h,w,C]; pairs [P,2].
    -> dict of [P] tensors on the device: count (visible pixels), mse and mae (over them and their channels), psnr
    (-10 log10 mse; NaN where nothing is visible, +inf where the frames agree exactly)."""
    import torch
    from . import ops
    wp, mask = warped['warped'], warped['mask']
    P, h, w, C = (int(x) for x in wp.shape)
    src = torch.as_tensor(np.asarray(pairs, np.int64).reshape(-1, 2)[:, 0], device=images.device)
    img_a = images.index_select(0, src).reshape(P, h * w, C).contiguous()
    r = ops.flow_consistency(wp.reshape(P, h * w, C), img_a, mask.reshape(P, h * w))
    terms = r[:, 0] * C
    return dict(count=r[:, 0], mse=r[:, 1] / terms, mae=r[:, 2] / terms, psnr=r[:, 3])


def flow_to_color(flow, max_mag=None, out8=False):
    """flow [...,2] -> the Middlebury flow picture [...,3] (float in [0, 1], or uint8 with out8): hue the direction, saturation
    the magnitude relative to max_mag; invalid (NaN) flow is black.  max_mag = None takes the largest finite magnitude of
    `flow`, found with torch on the device and READ BACK to become the kernel's argument -- the one place in this module where
    a value travels to the host; pass max_mag to stay asynchronous."""
    import torch
    from . import ops
    f = flow.reshape(-1, 2).contiguous()
    if max_mag is None:
        mag = torch.linalg.vector_norm(f, dim=1)
        mag = torch.where(torch.isfinite(mag), mag, torch.zeros_like(mag))
        max_mag = float(mag.max()) if mag.numel() else 0.0
        max_mag = max_mag if max_mag > 0.0 else 1.0
    rgb, rgb8 = ops.flow_color(f, max_mag, want_float=not out8, want_u8=out8)
    return (rgb8 if out8 else rgb).reshape(tuple(flow.shape[:-1]) + (3,))


def write_flo(path, flow, valid=None):
    """flow [h,w,2] (numpy or a tensor) -> the Middlebury .flo format: the 4 bytes PIEH, int32 width, int32 height, then float32
    u, v interleaved row-major, little-endian.  Pixels with valid == 0 or a non-finite component are written as 1e10 in both
    components (the format calls anything above 1e9 unknown)."""
    a = flow.cpu().numpy() if hasattr(flow, 'cpu') else np.asarray(flow)
    a = np.array(a, np.float32)
    if a.ndim != 3 or a.shape[2] != 2:
        raise ValueError('write_flo: flow of shape %s, expected [h,w,2]' % (a.shape,))
    bad = ~np.isfinite(a).all(-1)
    if valid is not None:
        v = valid.cpu().numpy() if hasattr(valid, 'cpu') else np.asarray(valid)
        bad |= v.reshape(a.shape[:2]) == 0
    a[bad] = FLO_UNKNOWN
    with open(path, 'wb') as f:
        f.write(FLO_MAGIC)
        f.write(struct.pack('<ii', a.shape[1], a.shape[0]))
        f.write(a.astype('<f4').tobytes())


def read_flo(path):
    """-> (flow [h,w,2] float32 with NaN where unknown, valid [h,w] int32): the inverse of write_flo"""
    blob = open(path, 'rb').read()
    if blob[:4] != FLO_MAGIC:
        raise ValueError('%s: not a .flo file (magic %r)' % (path, blob[:4]))
    w, h = struct.unpack('<ii', blob[4:12])
    if w < 1 or h < 1 or len(blob) != 12 + h * w * 8:
        raise ValueError('%s: %d bytes for a %d x %d flow field' % (path, len(blob), w, h))
    a = np.frombuffer(blob, '<f4', offset=12).reshape(h, w, 2).astype(np.float32)
    unknown = (np.abs(a) > FLO_UNKNOWN_THRESH).any(-1)
    a[unknown] = np.nan
    return a, (~unknown).astype(np.int32)
