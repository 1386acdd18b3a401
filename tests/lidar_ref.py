"""include/durf_lidar.h restated in numpy: the sensor's rays (float64, and a float32 twin that runs the same operations in
np.float32), the return model (quantile / mean / spread / valid, float64) and the compaction.  What tests/test_gpu_lidar.py
holds csrc/lidar.hip to, and tests/test_lidar_host.py checks on its own."""
import numpy as np

F64, F32 = np.float64, np.float32


# ---- rays -----------------------------------------------------------------------------------------------------------------
def rays(sensor_row, inclinations, sweep_row, near, far, dt=F64):
    """the six ray fields of the whole sweep, row-major r = h W + w, every operation in `dt` in the header's order (the
    inputs are the float32 rows the device gets) -> dict origins, directions, viewdirs [n,3], radii, near, far [n]"""
    row = np.asarray(sensor_row, F32)
    H, W = int(row[0]), int(row[1])
    az0, span = dt(row[2]), dt(row[3])
    sw = np.asarray(sweep_row, F32).astype(dt)
    R, p, om, dp = sw[:12].reshape(3, 4)[:, :3], sw[:12].reshape(3, 4)[:, 3], sw[12:15], sw[15:18]
    th = np.repeat(np.asarray(inclinations, F32).astype(dt), W)
    w = np.tile(np.arange(W), H)
    s = ((w.astype(dt) + dt(0.5)) / dt(W)).astype(dt)
    phi = az0 + s * span
    ct, st = np.cos(th), np.sin(th)
    d = np.stack([ct * np.cos(phi), ct * np.sin(phi), st], -1).astype(dt)
    v = (s[:, None] * om[None, :]).astype(dt)
    t2 = (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]
    small = t2 < dt(1e-12)
    t2s = np.where(small, dt(1.0), t2)
    t = np.sqrt(t2s)
    sh = np.sin(dt(0.5) * t)
    a = np.where(small, dt(1.0), np.sin(t) / t).astype(dt)
    b = np.where(small, dt(0.5), ((dt(2.0) * sh) * sh) / t2s).astype(dt)
    cross = lambda x, y: np.stack([x[:, 1] * y[:, 2] - x[:, 2] * y[:, 1], x[:, 2] * y[:, 0] - x[:, 0] * y[:, 2],
                                   x[:, 0] * y[:, 1] - x[:, 1] * y[:, 0]], -1)
    c = cross(v, d)
    e = cross(v, c)
    q = (d + a[:, None] * c) + b[:, None] * e
    dirs = np.stack([(R[k, 0] * q[:, 0] + R[k, 1] * q[:, 1]) + R[k, 2] * q[:, 2] for k in range(3)], -1)
    orig = p[None, :] + s[:, None] * dp[None, :]
    assert dirs.dtype == dt and orig.dtype == dt, (dirs.dtype, orig.dtype)
    n = H * W
    radius = F32(F64(row[4]) * abs(F64(row[3])) / F64(W) * 2.0 / np.sqrt(12.0))          # (in double on the host, rounded once)
    return dict(origins=orig, directions=dirs, viewdirs=dirs.copy(), radii=np.full(n, radius, F32), near=np.full(n, near, F32),
                far=np.full(n, far, F32))


# ---- returns --------------------------------------------------------------------------------------------------------------
def quantile(w, t, p):
    """one ray: weights w [N], t [N+1], 0 < p <= 1 -> (range(p), j*) in float64; (0, -1) when every weight is 0"""
    w, t = np.asarray(w, F64), np.asarray(t, F64)
    c = np.cumsum(w)
    W = c[-1]
    if not W > 0:
        return 0.0, -1
    tau = p * W
    ok = np.nonzero((c >= tau) & (w > 0))[0]
    j = int(ok[0]) if ok.size else int(np.nonzero(w > 0)[0][-1])          # (p -> 1 and rounding: the last non-empty bin)
    cp = c[j - 1] if j > 0 else 0.0
    f = min(max((tau - cp) / w[j], 0.0), 1.0)
    return t[j] + f * (t[j + 1] - t[j]), j


def cdf(w, t, x):
    """the float64 CDF of one ray, piecewise linear over t, at depth x (unnormalised: it ends at sum w)"""
    w, t = np.asarray(w, F64), np.asarray(t, F64)
    c = np.concatenate([[0.0], np.cumsum(w)])
    return float(np.interp(x, t, c))


def returns(weights, t_vals, acc, q=0.5, q_lo=0.16, q_hi=0.84, min_acc=0.5, max_range=np.inf, origins=None, directions=None,
            to_sensor=None):
    """float64 over n rays -> dict range (0 where invalid), range_raw (before the validity rule), bin, range_mean, spread,
    valid, W[, xyz]"""
    w, t, acc = np.asarray(weights, F64), np.asarray(t_vals, F64), np.asarray(acc, F64).reshape(-1)
    n = w.shape[0]
    out = dict(range_raw=np.zeros(n), bin=np.zeros(n, np.int64), range_mean=np.zeros(n), spread=np.zeros(n), W=w.sum(1))
    for r in range(n):
        out['range_raw'][r], out['bin'][r] = quantile(w[r], t[r], q)
        if out['W'][r] > 0:
            out['range_mean'][r] = (w[r] * 0.5 * (t[r, :-1] + t[r, 1:])).sum() / out['W'][r]
            out['spread'][r] = quantile(w[r], t[r], q_hi)[0] - quantile(w[r], t[r], q_lo)[0]
    out['valid'] = (acc >= min_acc) & (out['W'] > 0) & (out['range_raw'] <= max_range)
    out['range'] = np.where(out['valid'], out['range_raw'], 0.0)
    if origins is not None:
        xyz = np.asarray(origins, F64) + out['range'][:, None] * np.asarray(directions, F64)
        if to_sensor is not None:
            M = np.asarray(to_sensor, F64).reshape(3, 4)
            xyz = xyz @ M[:, :3].T + M[:, 3]
        out['xyz'] = xyz
    return out


def xyz_f32(origins, directions, rng, to_sensor=None):
    """the header's fp32 point of a GIVEN range: o + r d per component, then (M_i0 x + M_i1 y) + M_i2 z + M_i3"""
    o, d, r = np.asarray(origins, F32), np.asarray(directions, F32), np.asarray(rng, F32)
    p = (o + r[:, None] * d).astype(F32)
    if to_sensor is not None:
        M = np.asarray(to_sensor, F32).reshape(3, 4)
        p = np.stack([((M[i, 0] * p[:, 0] + M[i, 1] * p[:, 1]) + M[i, 2] * p[:, 2]) + M[i, 3] for i in range(3)], -1).astype(F32)
    return p


# ---- compaction -----------------------------------------------------------------------------------------------------------
def compact(valid, xyz, rng, rgb=None, dyn=None):
    """-> (points [M,8] float32, source [M] int32, M): the rays with valid != 0, in ray order"""
    valid = np.asarray(valid).reshape(-1)
    src = np.nonzero(valid != 0)[0].astype(np.int32)
    n = valid.shape[0]
    rgb = np.zeros((n, 3), F32) if rgb is None else np.asarray(rgb, F32).reshape(n, 3)
    dyn = np.zeros(n, np.int32) if dyn is None else np.asarray(dyn).reshape(n)
    pts = np.concatenate([np.asarray(xyz, F32).reshape(n, 3), np.asarray(rng, F32).reshape(n, 1), rgb, dyn.astype(F32)[:, None]], 1)
    return pts[src], src, int(src.shape[0])
