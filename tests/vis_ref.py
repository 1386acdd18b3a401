"""The reference's internal/vis.py restated in numpy: sinebow, depth_to_normals, visualize_depth, visualize_normals,
visualize_suite, one 2-D plane at a time as the reference takes them.  `dt` is the arithmetic: np.float64 is the truth the
HIP kernels are held to (tests/test_gpu_vis.py), np.float32 its twin -- the same operations in the reference's own working
precision, whose distance from float64 says what fp32 can promise.  The float64 form is pinned to the reference's file,
imported unmodified, by tests/golden/ref_vis_cases.npz (tests/golden/make_vis_fixture.py, tests/test_vis_host.py).

Differences from the reference's signatures: `curve_fn` is a name ('neglog', 'identity', 'inverse'), the colour map is a
[256,3] table `lut` looked up as matplotlib looks up a 256-entry map (row min(int(value * 256), 255)), and the convolution is
written out (no scipy).  Also here: the inputs of the test cases (`case`), so that the fixture and the GPU tests draw the same."""
import warnings

import numpy as np

EPS = np.finfo(np.float32).eps


def _curve(name, x, dt):
    e = dt(EPS)
    if name == 'neglog':
        return -np.log(x + e)
    if name == 'identity':
        return x
    if name == 'inverse':
        return dt(1) / (x + e)
    raise ValueError(name)


def sinebow(h, dt=np.float64):
    h = np.asarray(h, dt)
    f = lambda x: np.sin(dt(np.pi) * x) ** 2           # noqa: E731
    return np.stack([f(dt(3) / dt(6) - h), f(dt(5) / dt(6) - h), f(dt(7) / dt(6) - h)], -1)


def convolve2d_same(z, k):
    """scipy.signal.convolve2d(z, k, mode='same') for a 3 x 3 k: a true convolution (k flipped), zeros outside.  Every
    tap is multiplied, the zero ones too, so NaN and inf spread as they do there."""
    H, W = z.shape
    p = np.zeros((H + 2, W + 2), z.dtype)
    p[1:-1, 1:-1] = z
    out = np.zeros_like(z)
    for a in range(3):
        for b in range(3):
            out = out + k[a, b] * p[2 - a:2 - a + H, 2 - b:2 - b + W]
    return out


def depth_to_normals(depth, dt=np.float64):
    depth = np.asarray(depth, dt)
    f_blur = np.array([1, 2, 1], dt) / dt(4)
    f_edge = np.array([-1, 0, 1], dt) / dt(2)
    with np.errstate(invalid='ignore'):
        dy = convolve2d_same(depth, f_blur[None, :] * f_edge[:, None])
        dx = convolve2d_same(depth, f_blur[:, None] * f_edge[None, :])
        inv_denom = dt(1) / np.sqrt(dt(1) + dx ** 2 + dy ** 2)
        return np.stack([dx * inv_denom, dy * inv_denom, inv_denom], -1)


def depth_range(depth, acc=None, ignore_frac=0, dt=np.float64):
    """the automatic near / far of visualize_depth (vis.py:73-91)"""
    depth = np.asarray(depth, dt)
    acc = np.ones_like(depth) if acc is None else np.asarray(acc, dt)
    acc = np.where(np.isnan(depth), np.zeros_like(acc), acc)
    sortidx = np.argsort(depth.reshape(-1), kind='stable')          # NaNs last
    depth_sorted = depth.reshape(-1)[sortidx]
    cum = np.cumsum(acc.reshape(-1)[sortidx])
    mask = (cum >= cum[-1] * dt(ignore_frac)) & (cum <= cum[-1] * dt(1 - ignore_frac))
    keep = depth_sorted[mask]
    return keep[0] - dt(EPS), keep[-1] + dt(EPS)


def visualize_depth(depth, acc=None, near=None, far=None, ignore_frac=0, curve_fn='neglog', modulus=0, lut=None,
                    dt=np.float64, parts=False):
    """-> vis [H,W,3]; parts=True: (vis, value, a) with `value` what the colour map is called with and `a` the blend weight.
    lut: the [256,3] table (required when modulus == 0; with modulus > 0 None means the sinebow)"""
    depth = np.asarray(depth, dt)
    acc = np.ones_like(depth) if acc is None else np.asarray(acc, dt)
    acc = np.where(np.isnan(depth), np.zeros_like(acc), acc)
    auto = depth_range(depth, acc, ignore_frac, dt) if not (near and far) else (None, None)
    near = dt(near) if near else auto[0]
    far = dt(far) if far else auto[1]
    with np.errstate(invalid='ignore', divide='ignore'):
        d, near, far = [_curve(curve_fn, x, dt) for x in (depth, near, far)]
        if modulus > 0:
            value = np.mod(d, dt(modulus)) / dt(modulus)
        else:
            value = np.nan_to_num(np.clip((d - np.minimum(near, far)) / np.abs(far - near), 0, 1))
        if modulus > 0 and lut is None:
            vis = sinebow(value, dt)
        else:
            row = np.minimum(np.nan_to_num(value * 256).astype(np.int64), 255)
            vis = np.where(np.isnan(value)[..., None], 0, np.asarray(lut, dt)[row])
        vis = vis * acc[:, :, None] + (dt(1) - acc)[:, :, None]
    return (vis, value, acc) if parts else vis


def normal_scaling(depth, dt=np.float64):
    depth = np.asarray(depth, dt)
    mask = ~np.isnan(depth)
    x, y = np.meshgrid(np.arange(depth.shape[1]), np.arange(depth.shape[0]), indexing='xy')
    with np.errstate(invalid='ignore', divide='ignore'), warnings.catch_warnings():
        warnings.simplefilter('ignore')     # (the mean of nothing)
        xy_var = (np.var(x[mask].astype(dt)) + np.var(y[mask].astype(dt))) / dt(2)
        z_var = np.var(depth[mask])
        return np.sqrt(xy_var / z_var)


def visualize_normals(depth, acc, scaling=None, dt=np.float64):
    depth = np.asarray(depth, dt)
    if scaling is None:
        scaling = normal_scaling(depth, dt)
    with np.errstate(invalid='ignore', over='ignore'):
        normals = depth_to_normals(dt(scaling) * depth, dt)
        vis = np.isnan(normals) + np.nan_to_num((normals + dt(1)) / dt(2))
        if acc is not None:
            acc = np.asarray(acc, dt)
            vis = vis * acc[:, :, None] + (dt(1) - acc)[:, :, None]
    return vis


def visualize_suite(depth, acc, lut, dt=np.float64):
    return {'depth': visualize_depth(depth, acc, lut=lut, dt=dt),
            'depth_mod': visualize_depth(depth, acc, modulus=0.1, dt=dt),
            'depth_normals': visualize_normals(depth, acc, dt=dt)}


def stats(depth):
    """the record durf_vis_stats writes for one plane, in float64: near_auto, far_auto, normal_scale, count, var_x, var_y,
    var_depth, mean_depth"""
    depth = np.asarray(depth, np.float64)
    mask = ~np.isnan(depth)
    x, y = np.meshgrid(np.arange(depth.shape[1]), np.arange(depth.shape[0]), indexing='xy')
    near, far = depth_range(depth)
    with np.errstate(invalid='ignore', divide='ignore'), warnings.catch_warnings():
        warnings.simplefilter('ignore')     # (the mean of nothing)
        vx, vy, vd = np.var(x[mask].astype(np.float64)), np.var(y[mask].astype(np.float64)), np.var(depth[mask])
        return np.array([near, far, np.sqrt(((vx + vy) / 2) / vd), mask.sum(), vx, vy, vd, np.mean(depth[mask])], np.float64)


# ---- the inputs of the test cases ---------------------------------------------------------------------------------------
def smooth_depth(seed, F, H, W):
    """[F,H,W] float32, smooth and random in [1, 40] (the scene's far bound): a few random plane waves per frame"""
    rs = np.random.default_rng(seed)
    y, x = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing='ij')
    out = np.zeros((F, H, W))
    for f in range(F):
        g = np.zeros((H, W))
        for _ in range(6):
            kx, ky = rs.uniform(-0.25, 0.25, 2)
            g += rs.uniform(0.3, 1.0) * np.sin(kx * x + ky * y + rs.uniform(0, 2 * np.pi))
        g += 0.05 * rs.standard_normal((H, W))
        g -= 0.5 * (g.max() + g.min())
        out[f] = 20.5 + rs.uniform(12.0, 19.0) * g / max(np.abs(g).max(), 1e-12)
    return out.astype(np.float32)


#           name: (seed, F, H, W, acc: None | 'rand' | 'zero', fraction of NaN depths, constant plane)
CASES = {
    'p1x1': (11, 1, 1, 1, 'rand', 0.0, False),
    'p1x7': (12, 1, 1, 7, 'rand', 0.0, False),
    'p7x1': (13, 1, 7, 1, 'rand', 0.0, False),
    'p3x3': (14, 1, 3, 3, 'rand', 0.0, False),
    'p37x53': (15, 1, 37, 53, 'rand', 0.0, False),
    'f3_37x53': (16, 3, 37, 53, 'rand', 0.0, False),
    'nan_acc0': (17, 1, 37, 53, 'zero', 0.03, False),
    'nan_noacc': (18, 2, 37, 53, None, 0.03, False),
    'const': (19, 1, 6, 5, 'rand', 0.0, True),
    'big': (20, 1, 320, 480, 'rand', 0.0, False),
}


def case(name):
    """-> (depth [F,H,W] float32, acc [F,H,W] float32 or None)"""
    seed, F, H, W, acc_mode, nan_frac, const = CASES[name]
    depth = smooth_depth(seed, F, H, W)
    rs = np.random.default_rng(seed + 1000)
    if const:
        depth[:] = np.float32(7.25)
    if nan_frac:
        depth[rs.uniform(size=depth.shape) < nan_frac] = np.nan
    if name == 'nan_noacc':
        depth[1, :5] = np.nan                      # a frame whose first rows are gone entirely
    acc = None
    if acc_mode == 'rand':
        acc = rs.uniform(0.0, 1.0, depth.shape).astype(np.float32)
    elif acc_mode == 'zero':
        acc = np.zeros(depth.shape, np.float32)
    return depth, acc
