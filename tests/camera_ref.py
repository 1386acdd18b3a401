"""The camera row and its projection, restated in numpy for the overlay, flow, raster and tsdf oracles (include/durf_hip.h, THE
CAMERA ROW): an independent restatement -- it calls nothing of durf_amd and reads no library.  Dtype-parametric: float32 gives
the kernels' bits (every operation rounds once, in the header's association), float64 the yardstick."""
import numpy as np

FLOATS, FOCAL, PPX, PPY, H, W = 17, 12, 13, 14, 15, 16


def row(c2w, focal, ppx, ppy, h, w):
    """one camera: c2w [3,4] (or [4,4]) row-major, then focal, principal point x / y, height, width -> float32 [FLOATS]"""
    out = np.zeros(FLOATS, np.float32)
    out[:FOCAL] = np.asarray(c2w, np.float64)[:3, :4].reshape(-1)
    out[FOCAL:] = (focal, ppx, ppy, h, w)
    return out


def look_at(eye, target, up=(0.0, 1.0, 0.0)):
    """c2w [3,4] of a camera at `eye` looking at `target` (camera -z is the view direction)"""
    eye, target, up = (np.asarray(a, np.float64) for a in (eye, target, up))
    zc = eye - target
    zc /= np.linalg.norm(zc)
    xc = np.cross(up, zc)
    xc /= np.linalg.norm(xc)
    yc = np.cross(zc, xc)
    return np.concatenate([np.stack([xc, yc, zc], 1), eye[:, None]], 1)


def _per_frame(cams, nd, ft):
    cams = np.asarray(cams, ft)
    return cams.reshape((cams.shape[0],) + (1,) * (nd - 2) + (FLOATS,))


def to_camera(cams, P, ft):
    """cams [F,FLOATS], P [F,...,3] -> pc [F,...,3] = R_c^T (P - o)"""
    P = np.asarray(P, ft)
    c = _per_frame(cams, P.ndim, ft)
    d0, d1, d2 = P[..., 0] - c[..., 3], P[..., 1] - c[..., 7], P[..., 2] - c[..., 11]
    return np.stack([(c[..., j] * d0 + c[..., 4 + j] * d1) + c[..., 8 + j] * d2 for j in range(3)], -1)


def pixel(cams, pc, z, ft):
    """picture coordinates [F,...,2] of camera-space points pc [F,...,3] at depth z"""
    c = _per_frame(cams, pc.ndim, ft)
    return np.stack([c[..., PPX] + (c[..., FOCAL] * pc[..., 0]) / z, c[..., PPY] - (c[..., FOCAL] * pc[..., 1]) / z], -1)


def project(cams, P, ft):
    """picture coordinates [F,...,2] and camera depth [F,...] of world points (no clipping)"""
    pc = to_camera(cams, P, ft)
    z = -pc[..., 2]
    return pixel(cams, pc, z, ft), z


def rays(cam, x, y):
    """the generator's rays of pixels (x, y) (arrays of one shape, or scalars) of one camera row, in float64: the origin [3] and the
    un-normalised directions [...,3], whose camera-space z is -1, so that the ray parameter is the camera depth"""
    cam = np.asarray(cam, np.float64)
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    m = cam[:FOCAL].reshape(3, 4)
    cd = np.stack([(x - cam[PPX]) / cam[FOCAL], -(y - cam[PPY]) / cam[FOCAL], -np.ones_like(x)], -1)
    return m[:, 3].copy(), cd @ m[:, :3].T
