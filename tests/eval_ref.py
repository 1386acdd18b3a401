"""The evaluation record of durf_eval_frames (include/durf_hip.h) restated in float64 numpy: what the reference's evaluation
loop computes per image (train_boxpose.py:562-563; math.py:49-51,66-137), the training step's object loss as a metric (:192)
and the depth error against the LIDAR plane (:174-175 with the unit mask).  SSIM is oracle.durf_data_ref.compute_ssim, which
tests/test_reference_data_crosscheck.py holds to the reference's own math.py."""
import numpy as np

from oracle import durf_data_ref as D

FIELDS = ('mse', 'psnr', 'ssim', 'obj_count', 'obj_mse', 'obj_psnr', 'depth_count', 'depth_abs', 'depth_rmse', 'nonfinite')
# the fields the device sums in fp64 and rounds once, and the counts
SUMMED = ('mse', 'psnr', 'obj_mse', 'obj_psnr', 'depth_abs', 'depth_rmse')
COUNTS = ('obj_count', 'depth_count', 'nonfinite')


def mse_to_psnr(mse):
    with np.errstate(divide='ignore', invalid='ignore'):
        return -10.0 / np.log(10.0) * np.log(np.float64(mse))


def frame_metrics(rgb, gt, distance=None, gt_depth=None, obj_mask=None, swap_blur=False, obj_div3=False, depth_all=False):
    """one frame: rgb, gt [H,W,3]; distance with gt_depth [H,W] or neither; obj_mask [H,W] or None -> {field: float64}.
    swap_blur / obj_div3 / depth_all: deliberately WRONG variants (the blur along H first -- the images are transposed, which
    swaps the passes --, the object MSE over 3 * count, every pixel a LIDAR return) for the tests' negative controls."""
    a, b = np.asarray(rgb, np.float64), np.asarray(gt, np.float64)
    H, W = a.shape[:2]
    nan = np.float64('nan')
    out = dict.fromkeys(FIELDS, nan)
    with np.errstate(divide='ignore', invalid='ignore'):
        d2 = (a - b) ** 2
        out['mse'] = d2.mean()
        out['psnr'] = mse_to_psnr(out['mse'])
        if swap_blur:
            # the reference's order on the transposed images = H first on these; the Gaussian passes commute in exact
            # arithmetic, so this differs from the right order by float64 rounding only
            out['ssim'] = D.compute_ssim(a.transpose(1, 0, 2), b.transpose(1, 0, 2), 1.0)
        else:
            out['ssim'] = D.compute_ssim(a, b, 1.0)
        out['obj_count'] = out['depth_count'] = 0.0
        if obj_mask is not None:
            m = np.asarray(obj_mask, np.float64)
            out['obj_count'] = m.sum()
            out['obj_mse'] = (m[..., None] * d2).sum() / (out['obj_count'] * (3.0 if obj_div3 else 1.0))
            out['obj_psnr'] = mse_to_psnr(out['obj_mse'])
        if gt_depth is not None:
            g, d = np.asarray(gt_depth, np.float64), np.asarray(distance, np.float64)
            ret = np.ones_like(g, bool) if depth_all else (g > 0)
            n = float(ret.sum())
            out['depth_count'] = n
            out['depth_abs'] = np.abs(d - g)[ret].sum() / max(n, 1.0)
            out['depth_rmse'] = np.sqrt(((d - g) ** 2)[ret].sum() / max(n, 1.0))
        out['nonfinite'] = float((~np.isfinite(a)).sum())
    return {k: np.float64(v) for k, v in out.items()}


def frames_metrics(rgb, gt, distance=None, gt_depth=None, obj_mask=None, **kw):
    """[F,...] inputs -> [F, 10] float64 in FIELDS order"""
    pick = lambda t, f: None if t is None else t[f]
    return np.array([[frame_metrics(rgb[f], gt[f], pick(distance, f), pick(gt_depth, f), pick(obj_mask, f), **kw)[k]
                      for k in FIELDS] for f in range(len(rgb))])


def make_case(F, H, W, seed=0):
    """seeded frames in [0, 1] of different content: gt = clip(rgb + N(0, 0.1)) as the SSIM test makes its pair, a depth
    plane with ~30 % LIDAR returns, a blob mask -> float32 arrays rgb, gt [F,H,W,3], distance, gt_depth, obj_mask [F,H,W]"""
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    rgb = np.empty((F, H, W, 3), np.float32)
    for f in range(F):
        base = 0.5 + 0.3 * np.sin(0.31 * (f + 1) * xx + 0.17 * yy + f)[..., None] * np.array([1.0, 0.7, -0.8])
        rgb[f] = np.clip(base + rs.uniform(-0.2, 0.2, (H, W, 3)), 0, 1)
    gt = np.clip(rgb + rs.normal(0, 0.1, rgb.shape), 0, 1).astype(np.float32)
    distance = rs.uniform(0.5, 30.0, (F, H, W)).astype(np.float32)
    gt_depth = np.where(rs.uniform(0, 1, (F, H, W)) < 0.3, distance + rs.normal(0, 0.5, (F, H, W)), 0.0).astype(np.float32)
    gt_depth = np.maximum(gt_depth, 0.0).astype(np.float32)
    obj_mask = (((xx - W * 0.4) ** 2 + (yy - H * 0.5) ** 2)[None] < (0.1 + 0.05 * np.arange(F))[:, None, None] * H * W).astype(np.float32)
    return rgb, gt, distance, gt_depth, obj_mask
