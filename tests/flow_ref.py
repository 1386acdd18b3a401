"""include/durf_flow.h restated in numpy, written from the header and not from csrc/flow.hip.  Every function takes `dt`:
np.float64 is the oracle; np.float32 is its twin, the header's operations in the header's order in float32 (numpy neither
fuses nor reorders elementwise arithmetic), which says what fp32 in that order costs on a given input.  Inputs are the fp32
values the library is handed; both evaluate on exactly those.

Beside the restatement: a small analytic scene (camera_rays, ray_setup, plant_scene) for the closed-form checks of
tests/test_flow_host.py -- a wall at a fixed depth in front of the camera and boxes whose visible surface is a plane a little
inside them, acc = 1 -- which stands in for the renderer where no GPU is to hand."""
import numpy as np

from tests import camera_ref
from tests.camera_ref import row as camera_row  # noqa: F401

F32, F64 = np.float32, np.float64
POSE_ROW = 12
CONS_SPAN = 4096
WHEEL = 55


def _a(x, dt):
    """the fp32 value the library is handed, in the working precision"""
    return np.asarray(np.asarray(x, F32), dt)


# ---- the pose table ---------------------------------------------------------------------------------------------------------
def aa2matrix(rotvec, dt=F64):
    """world->object matrix of a rotation vector (csrc/aa2matrix.h): safe_norm's clamp, the +1e-12, the skew product"""
    rx, ry, rz = (dt(v) for v in _a(rotvec, dt))
    s = (rx * rx + ry * ry) + rz * rz
    s = dt(1e-12) if s < dt(1e-12) else s
    th = np.sqrt(s) + dt(1e-12)
    a = np.sin(th) / th
    b = (dt(1) - np.cos(th)) / (th * th)
    z = dt(0)
    S = [[z, -rz, ry], [rz, z, -rx], [-ry, rx, z]]
    R = np.zeros((3, 3), dt)
    for i in range(3):
        for j in range(3):
            s2 = (S[i][0] * S[0][j] + S[i][1] * S[1][j]) + S[i][2] * S[2][j]
            R[i, j] = (dt(1 if i == j else 0) + a * S[i][j]) + b * s2
    return R


def _to_world(R, c, P):
    """c + R^T P, per component c_j + ((R[0][j] P_0 + R[1][j] P_1) + R[2][j] P_2); P [m,3]"""
    return np.stack([c[j] + ((R[0, j] * P[:, 0] + R[1, j] * P[:, 1]) + R[2, j] * P[:, 2]) for j in range(3)], 1)


def project(cam, X, dt=F64):
    """(x', y', z) of world points X [m,3] in camera row `cam` (camera_ref's projection)"""
    with np.errstate(all='ignore'):                # (a point at infinity: an invalid pixel's, replaced by NaN afterwards)
        xy, z = camera_ref.project(_a(cam, dt)[None], X[None], dt)
    return xy[0, :, 0], xy[0, :, 1], z[0]


# ---- (a) durf_flow_points ---------------------------------------------------------------------------------------------------
def points(origins_s, dirs_s, hit, t, acc, cam_a, cam_b, pose_a, pose_b, ext, first=0, normalise=True, min_acc=0.5, znear=1e-2,
           inside_tol=1e-3, dt=F64):
    """-> dict: flow [n,2], scene_flow, xyz, target [n,3], zcam [n] (dt; NaN where invalid), moving, valid [n] int32; and, for
    a test's preconditions, P [n,3] (the point in the frame the ray was marched in), nh [n], z_b [n] before the validity select"""
    o, d, t, acc = _a(origins_s, dt), _a(dirs_s, dt), _a(t, dt).reshape(-1), _a(acc, dt).reshape(-1)
    n = o.shape[0]
    K = 0 if pose_a is None else int(np.asarray(pose_a).reshape(-1, 6).shape[0])
    hit = np.zeros((n, 0), np.int32) if K == 0 else np.asarray(hit, np.int32).reshape(n, K)
    with np.errstate(all='ignore'):
        tt = t / acc if normalise else t.copy()
        P = np.stack([o[:, j] + tt * d[:, j] for j in range(3)], 1)
    Xa, Xb = P.copy(), P.copy()
    moving = np.full(n, -1, np.int32)
    nh = (hit != 0).sum(1).astype(np.int32)
    grow = dt(1) + dt(F32(inside_tol))
    for k in range(K):
        h = hit[:, k] != 0
        if not h.any():
            continue
        pa, pb, e = _a(np.asarray(pose_a).reshape(-1, 6)[k], dt), _a(np.asarray(pose_b).reshape(-1, 6)[k], dt), _a(np.asarray(ext)[k], dt)
        with np.errstate(all='ignore'):
            A = _to_world(aa2matrix(pa[3:], dt), pa[:3], P[h])
            B = _to_world(aa2matrix(pb[3:], dt), pb[:3], P[h])
            inside = (np.abs(P[h, 0]) <= e[0] * grow) & (np.abs(P[h, 1]) <= e[1] * grow) & (np.abs(P[h, 2]) <= e[2] * grow)
        Xa[h] = A
        Xb[h] = np.where(inside[:, None], B, A)
        moving[h] = np.where(inside, k, -1)
    cam_a32 = np.asarray(cam_a, F32)
    w = int(cam_a32[camera_ref.W])
    p = first + np.arange(n)
    x, y = (p % w).astype(dt), (p // w).astype(dt)
    xb, yb, zb = project(cam_b, Xb, dt)
    _, _, za = project(cam_a, Xa, dt)
    with np.errstate(invalid='ignore'):
        ok = (acc >= dt(F32(min_acc))) & (nh <= 1) & np.isfinite(tt) & (zb >= dt(F32(znear)))
    nan = dt(np.nan)
    sel = lambda v: np.where(ok if v.ndim == 1 else ok[:, None], v, nan).astype(dt)
    with np.errstate(invalid='ignore'):
        res = dict(flow=sel(np.stack([xb - x, yb - y], 1)), scene_flow=sel(Xb - Xa), xyz=sel(Xa), target=sel(np.stack([xb, yb, zb], 1)),
                   zcam=sel(za))
    res.update(moving=np.where(ok, moving, -2).astype(np.int32), valid=ok.astype(np.int32), P=P, nh=nh, z_b=zb)
    return res


# ---- (b) durf_flow_warp -----------------------------------------------------------------------------------------------------
def warp(target, valid, img_b, zcam_b, occ_rel=0.02, occ_abs=0.0, dt=F64):
    """-> (warped [n,C] dt, NaN where not visible; mask [n] int32)"""
    tg, img, zc = _a(target, dt).reshape(-1, 3), _a(img_b, dt), _a(zcam_b, dt)
    h, w, C = img.shape
    zc = zc.reshape(h, w)
    xp, yp, zb = tg[:, 0], tg[:, 1], tg[:, 2]
    with np.errstate(invalid='ignore'):
        inframe = (xp >= 0) & (xp <= dt(w - 1)) & (yp >= 0) & (yp <= dt(h - 1))
    xs, ys = np.where(inframe, xp, dt(0)), np.where(inframe, yp, dt(0))
    x0 = np.maximum(np.minimum(np.floor(xs).astype(np.int64), w - 2), 0)
    y0 = np.maximum(np.minimum(np.floor(ys).astype(np.int64), h - 2), 0)
    x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
    fx = np.zeros_like(xs) if w == 1 else xs - x0.astype(dt)
    fy = np.zeros_like(ys) if h == 1 else ys - y0.astype(dt)
    zs = zc[np.rint(ys).astype(np.int64), np.rint(xs).astype(np.int64)]
    one = dt(1)
    with np.errstate(invalid='ignore'):
        vis = (np.asarray(valid).reshape(-1) != 0) & inframe & np.isfinite(zs) & (zb <= zs * (one + dt(F32(occ_rel))) + dt(F32(occ_abs)))
        fx_, fy_ = fx[:, None], fy[:, None]
        v = (one - fy_) * ((one - fx_) * img[y0, x0] + fx_ * img[y0, x1]) + fy_ * ((one - fx_) * img[y1, x0] + fx_ * img[y1, x1])
    return np.where(vis[:, None], v, dt(np.nan)).astype(dt), vis.astype(np.int32)


# ---- (c) durf_flow_consistency ----------------------------------------------------------------------------------------------
def consistency(warped, img_a, mask):
    """float64 sums over the masked pixels of the fp32 inputs -> [P,4]: count, sse, sae, psnr"""
    wp, a, mk = _a(warped, F64), _a(img_a, F64), np.asarray(mask) != 0
    P, m, C = wp.shape
    out = np.zeros((P, 4))
    for p in range(P):
        d = wp[p][mk[p]] - a[p][mk[p]]
        cnt, sse, sae = float(mk[p].sum()), float((d * d).sum()), float(np.abs(d).sum())
        psnr = np.nan if cnt == 0 else (np.inf if sse == 0 else -10.0 * np.log10(sse / (cnt * C)))
        out[p] = cnt, sse, sae, psnr
    return out


# ---- (d) durf_flow_color ----------------------------------------------------------------------------------------------------
def colorwheel():
    """the Middlebury wheel [55,3], levels 0..255, from its description: six ramps of 15, 6, 4, 11, 13 and 6 steps"""
    rows = []
    ramps = ((15, (0, 1), +1), (6, (1, 0), -1), (4, (1, 2), +1), (11, (2, 1), -1), (13, (2, 0), +1), (6, (0, 2), -1))
    for steps, (full, ramp), sign in ramps:        # `full` stays at 255; `ramp` rises from 0 (sign +) or falls from 255 (sign -)
        for i in range(steps):
            c = [0, 0, 0]
            c[full] = 255
            c[ramp] = (255 * i) // steps if sign > 0 else 255 - (255 * i) // steps
            rows.append(c)
    return np.asarray(rows, np.int64)


def color(flow, max_mag, dt=F64, dimmed=None):
    """-> (rgb [n,3] dt, 0 where the flow is not finite; the pre-rounding col * 255 [n,3] for a test's rounding margins).
    dimmed: None decides rad <= 1 per pixel as the header does; False / True forces the branch (a test's pixels whose rad is 1
    to rounding, where the two branches differ by a quarter of the colour, are held to either)"""
    f = _a(flow, dt).reshape(-1, 2)
    ok = np.isfinite(f).all(1)
    u, v = np.where(ok, f[:, 0], dt(0)), np.where(ok, f[:, 1], dt(0))
    mm = dt(F32(max_mag))
    pi = dt(F32(np.pi)) if dt is F32 else dt(np.pi)
    rad = np.sqrt(u * u + v * v) / mm
    a = np.arctan2(-v, -u) / pi
    fk = ((a + dt(1)) / dt(2)) * dt(WHEEL - 1)
    k0 = np.clip(fk.astype(np.int64), 0, WHEEL - 1)
    k1 = np.where(k0 + 1 == WHEEL, 0, k0 + 1)
    fr = (fk - k0.astype(dt))[:, None]
    wheel = colorwheel().astype(dt)
    c0, c1 = wheel[k0] / dt(255), wheel[k1] / dt(255)
    col = (dt(1) - fr) * c0 + fr * c1
    r = rad[:, None]
    inner = r <= 1 if dimmed is None else np.full(r.shape, not dimmed)
    col = np.where(inner, dt(1) - r * (dt(1) - col), col * dt(0.75))
    col = np.where(ok[:, None], col, dt(0)).astype(dt)
    return col, col * dt(255)


# ---- an analytic scene for the closed-form checks -----------------------------------------------------------------------------
def camera_rays(cam):
    """origins, directions [h w,3] float64 of a camera row: the pinhole rays of csrc/camera.h (direction's -z camera component 1)"""
    cam = np.asarray(cam, F32).astype(F64)
    h, w = int(cam[camera_ref.H]), int(cam[camera_ref.W])
    y, x = np.divmod(np.arange(h * w), w)
    o, d = camera_ref.rays(cam, x, y)
    return np.tile(o, (h * w, 1)), d


def ray_setup(origins, dirs, pose, ext):
    """the box test of csrc/rays.hip in float64 -> origins_s, dirs_s [n,3], hit [n,K] int32, t_near [n] (entry of the hit box along
    the unit object-frame direction; NaN elsewhere)"""
    n = origins.shape[0]
    pose = np.asarray(pose, F64).reshape(-1, 6)
    K = pose.shape[0]
    so, sd, hit, tnear = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros((n, K), np.int32), np.full(n, np.nan)
    for k in range(K):
        R = aa2matrix(pose[k, 3:])
        po, pd = (origins - pose[k, :3]) @ R.T, dirs @ R.T
        pd = pd / np.linalg.norm(pd, axis=1, keepdims=True)
        with np.errstate(all='ignore'):
            t0, t1 = (-ext[k] - po) / pd, (ext[k] - po) / pd
        tn, tf = np.minimum(t0, t1).max(1), np.maximum(t0, t1).min(1)
        h = (tf > tn) & (tf > 0)
        hit[:, k] = h
        so[h] += po[h]
        sd[h] += pd[h]
        tnear[h] = tn[h]
    none = hit.sum(1) == 0
    so[none], sd[none] = origins[none], dirs[none]
    return so, sd, hit, tnear


def plant_scene(cam, pose, ext, wall_depth, skin=0.05):
    """what a renderer would report for camera row `cam`: rays that hit one box see a surface `skin` (in the box's units) behind
    its entry point, the others a wall at depth wall_depth along the camera's axis; acc = 1.  Valid for a camera whose rotation
    is the identity.  -> dict(origins_s, dirs_s, hit, t, acc) as float32 / int32 arrays"""
    o, d = camera_rays(cam)
    so, sd, hit, tn = ray_setup(o, d, pose, np.asarray(ext, F64)) if len(pose) else (o, d, np.zeros((o.shape[0], 0), np.int32), None)
    t = np.full(o.shape[0], float(wall_depth))
    if len(pose):
        one = hit.sum(1) == 1
        t[one] = tn[one] + skin
    return dict(origins_s=so.astype(F32), dirs_s=sd.astype(F32), hit=hit, t=t.astype(F32), acc=np.ones(o.shape[0], F32))
