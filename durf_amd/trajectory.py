"""Camera trajectories on the host: keyframes -> per-frame cameras and times, the trajectory files of the reference's
notebooks/durf_render_traj.ipynb, and binary PPM frames.  numpy only -- the rendering is MipNerfModel.render_trajectory
(one library call for the whole list); this module prepares its `cams` / `times` and stores what it returns."""
import numpy as np

from . import camera


def _quat_from_rot(R):
    """rotation matrix -> unit quaternion (w, x, y, z), the branch with the largest pivot (no division by a small number)"""
    R = np.asarray(R, np.float64)
    tr = R[0, 0] + R[1, 1] + R[2, 2]
    if tr > 0:
        s = 2.0 * np.sqrt(1.0 + tr)
        q = np.array([0.25 * s, (R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s])
    else:
        i = int(np.argmax([R[0, 0], R[1, 1], R[2, 2]]))
        j, k = (i + 1) % 3, (i + 2) % 3
        s = 2.0 * np.sqrt(1.0 + R[i, i] - R[j, j] - R[k, k])
        q = np.zeros(4)
        q[0] = (R[k, j] - R[j, k]) / s
        q[1 + i] = 0.25 * s
        q[1 + j] = (R[j, i] + R[i, j]) / s
        q[1 + k] = (R[k, i] + R[i, k]) / s
    return q / np.linalg.norm(q)


def _rot_from_quat(q):
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def _slerp(q0, q1, u):
    d = float(np.dot(q0, q1))
    if d < 0.0:                       # the shorter of the two arcs between the rotations
        q1, d = -q1, -d
    if d > 1.0 - 1e-12:
        q = q0 + u * (q1 - q0)
        return q / np.linalg.norm(q)
    th = np.arccos(min(d, 1.0))
    return (np.sin((1.0 - u) * th) * q0 + np.sin(u * th) * q1) / np.sin(th)


def make_trajectory(c2w_keys, t_keys, n_frames):
    """Keyframes -> n_frames cameras evenly spaced over the keyframe index: c2w_keys [M,3,4] (or [M,4,4]) camera-to-world
    matrices with orthonormal rotation blocks, t_keys [M] scene times.  Position and time are lerped, rotation is slerped
    through quaternions (every returned rotation block is orthonormal).  -> (c2w [F,3,4] float64, times [F] float64); the
    first and last frame are the first and last keyframe."""
    keys = np.asarray(c2w_keys, np.float64)[:, :3, :4]
    t_keys = np.asarray(t_keys, np.float64).reshape(-1)
    M = keys.shape[0]
    if M < 1 or t_keys.shape[0] != M or n_frames < 1:
        raise ValueError('make_trajectory: %d keyframes, %d times, %d frames' % (M, t_keys.shape[0], n_frames))
    quats = [_quat_from_rot(k[:, :3]) for k in keys]
    c2w = np.zeros((n_frames, 3, 4))
    times = np.zeros(n_frames)
    for f in range(n_frames):
        s = 0.0 if (n_frames == 1 or M == 1) else f * (M - 1) / (n_frames - 1)
        i = min(int(np.floor(s)), max(M - 2, 0))
        u = s - i
        if M == 1 or u == 0.0:
            c2w[f], times[f] = keys[i], t_keys[i]
        elif u == 1.0:
            c2w[f], times[f] = keys[i + 1], t_keys[i + 1]
        else:
            c2w[f, :, :3] = _rot_from_quat(_slerp(quats[i], quats[i + 1], u))
            c2w[f, :, 3] = keys[i, :, 3] + u * (keys[i + 1, :, 3] - keys[i, :, 3])
            times[f] = t_keys[i] + u * (t_keys[i + 1] - t_keys[i])
    return c2w, times


def save_trajectory(path, c2w, times, notebook_format=False):
    """{c2w [F,3,4], times [F]} npz, or -- notebook_format -- the notebook's: np.savez(path, list of [c2w 4x4, ts]) ('arr_0')"""
    c2w, times = np.asarray(c2w, np.float64), np.asarray(times, np.float64).reshape(-1)
    if not notebook_format:
        np.savez(path, c2w=c2w[:, :3, :4], times=times)
        return
    arr = np.empty((len(times), 2), dtype=object)
    for f in range(len(times)):
        m = np.eye(4)
        m[:3, :4] = c2w[f][:3, :4]
        arr[f, 0], arr[f, 1] = m, float(times[f])
    np.savez(path, arr)


def load_trajectory(path):
    """-> (c2w [F,3,4] float64, times [F] float64) from a plain {c2w, times} npz or the notebook's format: an object array
    ('arr_0') of (c2w, ts) pairs, c2w 3x4 or 4x4 (notebooks/durf_render_traj.ipynb: np.savez(path, traj))"""
    with np.load(path, allow_pickle=True) as z:
        if 'c2w' in z.files and 'times' in z.files:
            c2w, times = np.asarray(z['c2w'], np.float64), np.asarray(z['times'], np.float64).reshape(-1)
        else:
            if len(z.files) != 1:
                raise ValueError('%s: expected the arrays c2w and times, or one array of (c2w, ts) pairs; found %s' % (path, z.files))
            pairs = z[z.files[0]]
            c2w = np.stack([np.asarray(p[0], np.float64)[:3, :4] for p in pairs])
            times = np.array([float(p[1]) for p in pairs], np.float64)
    c2w = c2w[:, :3, :4]
    if c2w.shape[0] != times.shape[0] or c2w.shape[1:] != (3, 4):
        raise ValueError('%s: c2w %s against times %s' % (path, c2w.shape, times.shape))
    return c2w, times


camera_rows = camera.rows          # [F,3,4] camera-to-world matrices with shared intrinsics -> the table render_trajectory takes


def write_ppm(path, rgb8):
    """[h,w,3] uint8 (numpy or a tensor) -> binary PPM (P6, maxval 255): no image library needed"""
    a = rgb8.cpu().numpy() if hasattr(rgb8, 'cpu') else np.asarray(rgb8)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
        raise ValueError('write_ppm: [h,w,3] uint8, got %s %s' % (a.dtype, a.shape))
    with open(path, 'wb') as f:
        f.write(b'P6\n%d %d\n255\n' % (a.shape[1], a.shape[0]))
        f.write(np.ascontiguousarray(a).tobytes())
