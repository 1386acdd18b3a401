"""Evaluation metrics of the reference's test loop (train_boxpose.py:398,562-575):
PSNR (internal/math.py:49-51) and SSIM (internal/math.py:66-137) on device images."""
import numpy as np
import torch

from . import _lib
from .math import mse_to_psnr  # noqa: F401  (re-exported: psnr = mse_to_psnr(((pred - gt) ** 2).mean()))
from .ops import _p, _stream


def compute_ssim(img0, img1, max_val, filter_size=11, filter_sigma=1.5, k1=0.01, k2=0.03, return_map=False):
    """math.compute_ssim for [H,W,C] fp32 device images -> 0-d tensor (or the [H-fs+1, W-fs+1, C] map)."""
    assert img0.shape == img1.shape and img0.dim() == 3
    H, W, Cc = img0.shape
    dev = img0.device
    hw = filter_size // 2
    shift = (2 * hw - filter_size + 1) / 2
    f_i = ((np.arange(filter_size) - hw + shift) / filter_sigma) ** 2          # math.py:96-100
    filt = np.exp(-0.5 * f_i)
    filt = (filt / filt.sum()).astype(np.float32)
    fd = torch.tensor(filt, device=dev)
    L = _lib.lib()
    scratch = torch.empty(int(L.durf_ssim_scratch_floats(H, W, Cc, filter_size)), device=dev)
    smap = torch.empty(H - filter_size + 1, W - filter_size + 1, Cc, device=dev) if return_map else None
    out = torch.empty((), device=dev)
    # bind the converted images to locals: a temporary made inside the call expression is freed as soon as its
    # address has been taken, and the caching allocator would hand the second conversion the same block
    a = img0.to(torch.float32).contiguous()
    b = img1.to(torch.float32).contiguous()
    _lib.check(L.durf_ssim(_stream(), H, W, Cc, _p(a), _p(b),
                           float(max_val), filter_size, _p(fd), float(k1), float(k2), _p(smap), _p(scratch), _p(out)),
               'durf_ssim')
    return smap if return_map else out


def evaluate_frames(rgb, gt_rgb, distance=None, gt_depth=None, obj_mask=None):
    """The evaluation loop's numbers for F frames at once (ops.eval_frames; include/durf_hip.h durf_eval_frames): rgb, gt_rgb
    [F,H,W,3] or [H,W,3]; distance with gt_depth (the LIDAR plane, 0 = no return) and obj_mask [F,H,W] / [H,W] or None, any
    float dtype or layout -> dict of [F] device tensors keyed by ops.EVAL_FIELDS.  Nothing is read back."""
    single = rgb.dim() == 3

    def frames(t, tail):
        if t is None:
            return None
        if single:
            t = t[None]
        return t.reshape(t.shape[:3] + tail).to(torch.float32).contiguous()
    # bound to locals for the call, as in compute_ssim: a temporary's block could be handed to the next conversion
    a, b = frames(rgb, (3,)), frames(gt_rgb, (3,))
    d, g, m = frames(distance, ()), frames(gt_depth, ()), frames(obj_mask, ())
    from . import ops
    rec, fields = ops.eval_frames(a, b, d, g, m)
    return {name: rec[:, i] for i, name in enumerate(fields)}
