"""LIDAR sweeps of the scene: what a spinning multi-beam sensor would see from a pose, at a time, with the boxes where they
are then -- the sensor model in front of the renderer, a robust return model behind it (include/durf_lidar.h,
csrc/lidar.hip, libdurf_lidar.so), and the returns as a point cloud on disk.

    sensor = LidarSensor.waymo_top()
    res = render_lidar(model, variables, sensor, pose_start, times, ext, white_bkgd, alpha, near=0.1, far=75.0)
    points, count = point_cloud(res, sweep=0)
    write_ply('sweep.ply', points, count)

Conventions: the sensor frame is x forward, y left, z up; a pose is a [3,4] sensor-to-world row (R | p); ray r = h W + w of
beam h and azimuth column w, so every per-ray output is a range image [H,W].  The sensor moves during a sweep: column w is
seen from R_start rodrigues(s_w omega), p_start + s_w dp with s_w = (w + 0.5) / W; sweep_motion() takes (omega, dp) from the
poses at the sweep's start and end.  The boxes are frozen per sweep at its time."""
import dataclasses
import math

import numpy as np


@dataclasses.dataclass
class LidarSensor:
    """inclinations [H] float32 radians, one per beam, any order; width: azimuth columns W; az0, az_span: radians, signed
    (column w looks along az0 + (w + 0.5) / W az_span); radius_scale: the factor on mip-NeRF's pixel-footprint rule applied to
    the azimuth step; max_range: returns beyond it are invalid."""
    inclinations: np.ndarray
    width: int
    az0: float = math.pi
    az_span: float = -2.0 * math.pi
    radius_scale: float = 1.0
    max_range: float = 75.0

    def __post_init__(self):
        self.inclinations = np.ascontiguousarray(np.asarray(self.inclinations, np.float32).reshape(-1))
        self.width = int(self.width)

    @property
    def height(self):
        return int(self.inclinations.shape[0])

    def row(self):
        """the 6 host floats of durf_lidar.h's sensor row: H, W, az0, az_span, radius_scale, max_range"""
        return np.array([self.height, self.width, self.az0, self.az_span, self.radius_scale, self.max_range], np.float32)

    @classmethod
    def uniform(cls, H, lo, hi, W, **kw):
        """H beams with inclinations evenly spaced over [lo, hi] radians, from the highest beam (row 0, as in a range image) down"""
        return cls(np.linspace(hi, lo, H), W, **kw)

    @classmethod
    def waymo_top(cls):
        """The shape of the Waymo Open Dataset's top sensor: 64 beams x 2650 columns, -17.6 .. +2.4 degrees, azimuth from +pi
        downwards over a full turn, 75 m.  The inclinations are UNIFORM here: the real sensor's per-beam table is calibration
        data that comes with each recording, which this project does not ship -- pass it as `inclinations` where it is to hand."""
        return cls.uniform(64, math.radians(-17.6), math.radians(2.4), 2650, az0=math.pi, az_span=-2.0 * math.pi, max_range=75.0)


def rodrigues(v):
    """rotation matrix of the rotation vector v, float64"""
    v = np.asarray(v, np.float64)
    t = float(np.linalg.norm(v))
    K = np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])
    if t < 1e-12:
        return np.eye(3) + K
    return np.eye(3) + math.sin(t) / t * K + 2.0 * math.sin(0.5 * t) ** 2 / (t * t) * (K @ K)


def sweep_motion(pose_start, pose_end):
    """(omega [3], dp [3]) of a sweep from the sensor poses [3,4] at its start and end, in float64: R_start rodrigues(omega) ==
    R_end, p_start + dp == p_end.  Rotations of up to just under 180 degrees."""
    a, b = np.asarray(pose_start, np.float64).reshape(3, 4), np.asarray(pose_end, np.float64).reshape(3, 4)
    Rr = a[:, :3].T @ b[:, :3]
    skew = 0.5 * np.array([Rr[2, 1] - Rr[1, 2], Rr[0, 2] - Rr[2, 0], Rr[1, 0] - Rr[0, 1]])          # sin(t) axis
    s, c = float(np.linalg.norm(skew)), 0.5 * (float(np.trace(Rr)) - 1.0)
    t = math.atan2(s, c)
    omega = skew * (t / s) if s > 1e-300 else np.zeros(3)
    return omega, b[:, 3] - a[:, 3]


def sweep_rows(pose_start, pose_end=None):
    """[F,18] float32 rows of durf_lidar.h's sweeps (a sensor pose and its motion: a layout of its own, not camera.py's row): pose_start [F,3,4] (or one [3,4]), pose_end likewise or None (the sensor
    stands still: omega = dp = 0)"""
    ps = np.asarray(pose_start, np.float64).reshape(-1, 3, 4)
    rows = np.zeros((ps.shape[0], 18), np.float64)
    rows[:, :12] = ps.reshape(-1, 12)
    if pose_end is not None:
        pe = np.asarray(pose_end, np.float64).reshape(-1, 3, 4)
        if pe.shape != ps.shape:
            raise ValueError('pose_end %s for pose_start %s' % (pe.shape, ps.shape))
        for f in range(ps.shape[0]):
            rows[f, 12:15], rows[f, 15:18] = sweep_motion(ps[f], pe[f])
    return rows.astype(np.float32)


DEFAULT_OUTPUTS = ('range', 'acc', 'rgb', 'spread', 'dynamic', 'valid', 'xyz')


def render_lidar(model, variables, sensor, poses, times, ext, white_bkgd, alpha, *, near, far, pose_end=None, chunk=8192, q=0.5,
                 q_lo=0.16, q_hi=0.84, min_acc=0.5, box_enable=None, outputs=DEFAULT_OUTPUTS):
    """F sweeps of `sensor` through the scene as ONE library call (durf_render_lidar): poses [F,3,4] the sensor at the start of
    every sweep (pose_end: at its end; None: it stands still), times [F] in [0, T - 1] -- fractional times take the boxes
    between two labelled timesteps, from MipNerfModel.render_trajectory's pose interpolation (which renders nothing here).
    -> dict of [F,H,W,.] tensors for `outputs` (ops.LIDAR_OUTPUTS: range -- the q-quantile of the ray's weights, 0 where
    invalid --, range_mean, distance -- the renderer's own --, acc, rgb, spread -- range(q_hi) - range(q_lo) --, dynamic,
    valid, xyz in the world frame) plus box_poses [F,K,6].  Same scope as render_image_one_call (supports_one_call)."""
    import torch
    from . import ops
    rows = sweep_rows(poses, pose_end)
    times = np.asarray(times, np.float32).reshape(-1)
    if times.shape[0] != rows.shape[0]:
        raise ValueError('%d times for %d sweeps' % (times.shape[0], rows.shape[0]))
    variables, args, kw = model._one_call_args('durf_render_lidar', variables, ext, alpha, white_bkgd)
    dev = variables.flat.device
    K, F = variables.layout.K, rows.shape[0]
    if K > 0:
        box_poses = model._trajectory_call(variables, None, times, ext, white_bkgd, alpha, near, far, chunk, None, ())['poses']
    else:
        box_poses = torch.empty(F, 0, 6, device=dev)
    en = ops._enable(box_enable, K, dev) if K > 0 else None
    incl = torch.as_tensor(sensor.inclinations, device=dev)
    res = ops.render_lidar(sensor.row(), incl, rows, box_poses, *args, chunk, near, far, box_enable=en, q=q, q_lo=q_lo, q_hi=q_hi,
                           min_acc=min_acc, outputs=outputs, **kw)
    H, W = sensor.height, sensor.width
    res = {k: v.reshape((F, H, W) + tuple(v.shape[2:])) for k, v in res.items()}
    res['box_poses'] = box_poses
    return res


def point_cloud(result, sweep=0):
    """the valid returns of one sweep of render_lidar's result (it needs valid, xyz and range; rgb and dynamic fill their
    columns when present) -> (points [n,8] float32: x, y, z, range, r, g, b, dynamic -- rows from count on are undefined --,
    count [1] int32 on the device), through durf_lidar_compact: no read-back"""
    from . import ops
    missing = [k for k in ('valid', 'xyz', 'range') if k not in result]
    if missing:
        raise ValueError('point_cloud needs the outputs %s of render_lidar' % missing)
    g = lambda k: result[k][sweep].reshape(-1, *result[k].shape[3:]).contiguous() if k in result else None
    points, _, count = ops.lidar_compact(g('valid'), g('xyz'), g('range'), g('rgb'), g('dynamic'))
    return points, count


PLY_DTYPE = np.dtype([('x', '<f4'), ('y', '<f4'), ('z', '<f4'), ('red', 'u1'), ('green', 'u1'), ('blue', 'u1'), ('range', '<f4'),
                      ('dynamic', 'u1')])


def write_ply(path, points, count):
    """points [n,8] (x, y, z, range, r, g, b, dynamic) and their number -> binary little-endian PLY: xyz float, rgb uchar,
    range float, dynamic uchar.  The one read-back of the pipeline: count first, then that many rows."""
    m = int(count.reshape(-1)[0]) if hasattr(count, 'reshape') else int(count)
    pts = points[:m]
    pts = pts.cpu().numpy() if hasattr(pts, 'cpu') else np.asarray(pts)
    pts = np.asarray(pts, np.float32).reshape(m, 8)
    v = np.zeros(m, PLY_DTYPE)
    v['x'], v['y'], v['z'], v['range'] = pts[:, 0], pts[:, 1], pts[:, 2], pts[:, 3]
    rgb = np.rint(np.clip(np.nan_to_num(pts[:, 4:7]), 0.0, 1.0) * 255.0).astype(np.uint8)
    v['red'], v['green'], v['blue'] = rgb[:, 0], rgb[:, 1], rgb[:, 2]
    v['dynamic'] = np.clip(pts[:, 7], 0, 255).astype(np.uint8)
    header = ('ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n'
              'property uchar red\nproperty uchar green\nproperty uchar blue\nproperty float range\nproperty uchar dynamic\n'
              'end_header\n' % m)
    with open(path, 'wb') as f:
        f.write(header.encode('ascii'))
        f.write(v.tobytes())
    return m
