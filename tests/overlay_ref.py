"""numpy restatement of the two definitions of csrc/overlay.hip (include/durf_overlay.h: durf_project_boxes, durf_draw_boxes), and the
cases the overlay tests share.  Every function takes the dtype it computes in: np.float64 is the reference, np.float32 its TWIN
-- the same statements, every operation rounded to fp32 -- whose distance from the reference is the error fp32 arithmetic itself
makes on those inputs, and so the measure the device is held to."""
import numpy as np

from tests.camera_ref import FLOATS, project as project_points, row as camera_row, to_camera  # noqa: F401  (the oracle's camera)

EDGES = 12


def edge_corners():
    """[12,2] corner indices: edge e = 4 axis + j joins the corners that differ in bit `axis`, j over the other two bits in
    increasing corner index, from the corner with the bit clear to the one with it set"""
    out = []
    for axis in range(3):
        for lo in range(8):
            if not lo & (1 << axis):
                out.append((lo, lo | (1 << axis)))
    return np.array(out, np.int64)


def aa2matrix(rotvec, ft):
    """box_helpers.aa2matrix as k_ray_setup evaluates it: rotvec [...,3] -> world->object matrices [...,3,3]"""
    r = np.asarray(rotvec, ft)
    rx, ry, rz = r[..., 0], r[..., 1], r[..., 2]
    s = rx * rx + ry * ry + rz * rz
    s = np.where(s < ft(1e-12), ft(1e-12), s)
    th = np.sqrt(s) + ft(1e-12)
    a = np.sin(th) / th
    b = (ft(1.0) - np.cos(th)) / (th * th)
    z = np.zeros_like(rx)
    S = np.stack([np.stack([z, -rz, ry], -1), np.stack([rz, z, -rx], -1), np.stack([-ry, rx, z], -1)], -2)
    R = np.zeros(S.shape, ft)
    for i in range(3):
        for j in range(3):
            s2 = S[..., i, 0] * S[..., 0, j] + S[..., i, 1] * S[..., 1, j] + S[..., i, 2] * S[..., 2, j]
            R[..., i, j] = ft(1.0 if i == j else 0.0) + a * S[..., i, j] + b * s2
    return R


def world_corners(poses, ext, ft):
    """poses [F,K,6], ext [K,3] -> P [F,K,8,3] = c + R^T (s_c * ext)"""
    poses, ext = np.asarray(poses, ft), np.asarray(ext, ft)
    R = aa2matrix(poses[..., 3:], ft)                                  # [F,K,3,3]
    P = np.zeros(poses.shape[:2] + (8, 3), ft)
    for q in range(8):
        v = [ext[:, a] if q & (1 << a) else -ext[:, a] for a in range(3)]
        for a in range(3):
            P[:, :, q, a] = poses[:, :, a] + ((R[:, :, 0, a] * v[0] + R[:, :, 1, a] * v[1]) + R[:, :, 2, a] * v[2])
    return P


def project_boxes(cams, poses, ext, box_enable, znear, ft):
    """-> segments [F,K,12,4], rect [F,K,6] in dtype ft"""
    cams = np.asarray(cams, ft)
    F, K = np.asarray(poses).shape[:2]
    znear = ft(znear)
    pc = to_camera(cams, world_corners(poses, ext, ft), ft)             # [F,K,8,3]
    pcc = to_camera(cams, np.asarray(poses, ft)[..., :3], ft)           # [F,K,3]
    ec = edge_corners()
    seg = np.full((F, K, EDGES, 4), np.nan, ft)
    rect = np.full((F, K, 6), np.nan, ft)
    on = np.ones(K, bool) if box_enable is None else np.asarray(box_enable) != 0
    with np.errstate(all='ignore'):
        for f in range(F):
            focal, ppx, ppy = cams[f, 12], cams[f, 13], cams[f, 14]
            for k in range(K):
                pts = []
                for e in range(EDGES):
                    a, b = pc[f, k, ec[e, 0]], pc[f, k, ec[e, 1]]
                    ax, ay, az = a[0], a[1], -a[2]
                    bx, by, bz = b[0], b[1], -b[2]
                    a_in, b_in = az >= znear, bz >= znear
                    if not on[k] or not (a_in or b_in):
                        continue
                    if not a_in or not b_in:
                        t = (znear - az) / (bz - az)
                        cx, cy = ax + t * (bx - ax), ay + t * (by - ay)
                        if not a_in:
                            ax, ay, az = cx, cy, znear
                        else:
                            bx, by, bz = cx, cy, znear
                    seg[f, k, e] = (ppx + (focal * ax) / az, ppy - (focal * ay) / az, ppx + (focal * bx) / bz, ppy - (focal * by) / bz)
                    pts += [seg[f, k, e, :2], seg[f, k, e, 2:]]
                rect[f, k, 4] = -pcc[f, k, 2]
                rect[f, k, 5] = 0.0
                if pts:
                    pts = np.array(pts, ft)
                    lo = np.maximum(pts.min(0), ft(0.0))
                    hi = np.minimum(pts.max(0), np.array([cams[f, 16] - ft(1.0), cams[f, 15] - ft(1.0)], ft))
                    if lo[0] <= hi[0] and lo[1] <= hi[1]:
                        rect[f, k, :4] = (lo[0], lo[1], hi[0], hi[1])
                        rect[f, k, 5] = 1.0
    assert seg.dtype == ft and rect.dtype == ft
    return seg, rect


def box_distances(segments, h, w, ft):
    """segments [F,K,12,4] -> d [F,K,h,w]: per box the least point-segment distance of every pixel (inf: no kept segment)"""
    s = np.asarray(segments, ft)
    F, K = s.shape[:2]
    py, px = np.meshgrid(np.arange(h, dtype=ft), np.arange(w, dtype=ft), indexing='ij')
    d = np.full((F, K, h, w), np.inf, ft)
    with np.errstate(all='ignore'):
        for f in range(F):
            for k in range(K):
                for e in range(EDGES):
                    ax, ay, bx, by = s[f, k, e]
                    if np.isnan(s[f, k, e]).any():
                        continue
                    ex, ey = bx - ax, by - ay
                    L = ex * ex + ey * ey
                    if L > 0:
                        t = np.minimum(np.maximum(((px - ax) * ex + (py - ay) * ey) / L, ft(0.0)), ft(1.0))
                    else:
                        t = np.zeros_like(px)
                    dx, dy = px - (ax + t * ex), py - (ay + t * ey)
                    de = np.sqrt(dx * dx + dy * dy)
                    d[f, k] = np.where(de < d[f, k], de, d[f, k])           # (a NaN distance never replaces)
    assert d.dtype == ft
    return d


def owners(d, half_width):
    """d [F,K,h,w] -> label [F,h,w] int32: the lowest k with d_k <= half_width, -1 for none"""
    F, K, h, w = d.shape
    lab = np.full((F, h, w), -1, np.int32)
    for k in range(K - 1, -1, -1):
        lab[d[:, k] <= half_width] = k
    return lab


def raster_reference(segments, h, w, half_width):
    """What the rasteriser tests share for one table of fp32 segments: the float64 distances and labels, EDGE = 4 x the twin's
    largest distance error (at least 1e-4 px), the undecided pixels (some box's float64 d_k within EDGE of half_width) and their
    share of the reference's drawn pixels."""
    seg32 = np.asarray(segments, np.float32)
    d64 = box_distances(seg32.astype(np.float64), h, w, np.float64)
    d32 = box_distances(seg32, h, w, np.float32)
    both = np.isfinite(d64) & np.isfinite(d32)
    twin_err = float(np.abs(d32[both].astype(np.float64) - d64[both]).max()) if both.any() else 0.0
    edge = max(4.0 * twin_err, 1e-4)
    label = owners(d64, np.float64(half_width))
    undecided = (np.abs(d64 - np.float64(half_width)) <= edge).any(1) if d64.shape[1] else np.zeros(label.shape, bool)
    drawn = label >= 0
    share = float(undecided.sum()) / max(int(drawn.sum()), 1)
    return dict(d64=d64, label=label, undecided=undecided, drawn=drawn, edge=edge, twin_err=twin_err, share=share)


# ---- the cases of tests/test_gpu_overlay.py (built here so that tests/test_overlay_host.py can hold them to the 5 % cap) -------
def look_at(eye, target, up=(0.0, 0.0, 1.0)):
    """c2w [3,4]: the camera at `eye` looks along its -z at `target`, +y up"""
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    fwd = target - eye
    fwd /= np.linalg.norm(fwd)
    right = np.cross(fwd, np.asarray(up, np.float64))
    right /= np.linalg.norm(right)
    true_up = np.cross(right, fwd)
    return np.concatenate([np.stack([right, true_up, -fwd], 1), eye[:, None]], 1)


SPECIAL = ('zero_rot', 'near_pi', 'straddle', 'behind', 'offscreen', 'edge_on', 'disabled')


def make_case(F, h, w, K, seed):
    """A seeded scene: F cameras near the origin looking down the world's +x, K boxes about 6 units ahead.  The first boxes are
    the special poses of SPECIAL, in that order, as far as K reaches (frame 0's camera is exactly axis-aligned at the origin so
    that the hand-placed ones are what they say); the rest are random.  -> dict of float32 arrays and znear."""
    rng = np.random.default_rng(seed)
    focal = 0.9 * w
    ppx, ppy = (w - 1) / 2.0 + 0.25, (h - 1) / 2.0 - 0.25
    cams = np.zeros((F, FLOATS), np.float32)
    for f in range(F):
        eye = np.zeros(3) if f == 0 else rng.uniform(-0.3, 0.3, 3)
        target = np.array([6.0, 0.0, 0.0]) if f == 0 else np.array([6.0, 0.0, 0.0]) + rng.uniform(-0.5, 0.5, 3)
        cams[f] = camera_row(look_at(eye, target), focal, ppx, ppy, h, w)
    poses = np.zeros((F, K, 6), np.float32)
    ext = rng.uniform(0.3, 0.9, (K, 3)).astype(np.float32)
    enable = np.ones(K, np.int32)
    znear = 0.5
    for k in range(K):
        c = np.array([rng.uniform(4.0, 8.0), rng.uniform(-2.0, 2.0), rng.uniform(-1.5, 1.5)])
        r = rng.normal(size=3)
        r *= rng.uniform(0.1, 2.5) / np.linalg.norm(r)
        kind = SPECIAL[k] if k < len(SPECIAL) and K > 1 else 'random'
        if kind == 'zero_rot':
            r = np.zeros(3)
        elif kind == 'near_pi':
            r *= (np.pi - 1e-3) / np.linalg.norm(r)
        elif kind == 'straddle':                    # around the plane x = znear of frame 0's camera, off the axis
            c, r = np.array([0.4, 0.9, -0.5]), np.array([0.0, 0.0, 0.3])
            ext[k] = (0.6, 0.4, 0.3)
        elif kind == 'behind':
            c = np.array([-5.0, 0.5, 0.2])
        elif kind == 'offscreen':
            c = np.array([5.0, 40.0, 0.0])
        elif kind == 'edge_on':                     # the edge y = z = 0 along the world's x runs through frame 0's camera: a point
            r = np.zeros(3)
            c = np.array([5.0, float(ext[k, 1]), float(ext[k, 2])])
        elif kind == 'disabled':
            enable[k] = 0
        for f in range(F):
            step = 0.0 if kind in ('straddle', 'behind', 'offscreen', 'edge_on') else 0.15 * f
            poses[f, k, :3] = c + step * np.array([0.5, 1.0, 0.2])
            poses[f, k, 3:] = r
    return dict(cams=cams, poses=poses, ext=ext, enable=enable, znear=znear, F=F, h=h, w=w, K=K)


# (name, F, h, w, K, line widths): the sizes tests/test_gpu_overlay.py runs
GPU_CASES = (('k1', 3, 37, 53, 1, (1.5,)), ('k3', 3, 37, 53, 3, (1.5, 3.0)), ('k8', 3, 37, 53, 8, (1.0, 1.5)),
             ('k16', 3, 37, 53, 16, (1.5,)), ('tiny', 1, 5, 7, 3, (1.5,)), ('big', 2, 320, 480, 3, (1.5,)))


def gpu_case(name):
    for i, (n, F, h, w, K, widths) in enumerate(GPU_CASES):
        if n == name:
            return dict(make_case(F, h, w, K, 100 + i), name=n, widths=widths)
    raise KeyError(name)
