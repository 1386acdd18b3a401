"""Render LIDAR sweeps of a trained scene to a directory:

    python -m durf_amd.render_lidar --gin_file configs/waymo.gin --data_dir DATA --train_dir CKPT --sweeps sweeps.npz --eval_dir OUT
                                    [--beams 64] [--columns 2650] [--incl_lo -17.6] [--incl_hi 2.4] [--max_range 75]
                                    [--q 0.5] [--min_acc 0.5] [--disable_box k ...] [--chunk 8192]
    python -m durf_amd.render_lidar --synthetic --eval_dir OUT [--sweeps sweeps.npz]

sweeps.npz holds pose_start [F,3,4] (sensor-to-world rows; sensor frame x forward, y left, z up), optionally pose_end [F,3,4]
(the sensor at the end of every sweep; absent: it stands still) and times [F] in [0, T - 1] (fractional times take the boxes
between two labelled timesteps).  The checkpoint in --train_dir is restored and all sweeps are ONE durf_amd.lidar.render_lidar
call; per sweep f the command writes OUT/range_%04d.npy ([H,W] float32, the median return, 0 where there is none),
OUT/range_%04d.ppm (that range image through vis.visualize_depth) and OUT/sweep_%04d.ply (the valid returns: xyz in the world
frame, rgb, range, dynamic).  The sensor is LidarSensor.uniform(--beams, --incl_lo, --incl_hi, --columns) in degrees: the
shape of Waymo's top sensor by default, with uniform inclinations.  --synthetic renders
train_boxpose.SyntheticTimestepDataset's scene instead (no data directory; without --train_dir the freshly initialised model,
without --sweeps two sweeps of a 16 x 128 sensor from the scene's first camera, the second one moving and between two
timesteps), which exercises the command end to end."""
import argparse
import math
import os
import sys

from . import camera
from .render_traj import add_scene_arguments, open_scene, restore_model


def build_parser():
    ap = argparse.ArgumentParser(prog='python -m durf_amd.render_lidar', description=__doc__.split('\n\n')[0])
    add_scene_arguments(ap)
    ap.add_argument('--sweeps', default=None, help='npz: pose_start [F,3,4], optional pose_end [F,3,4], times [F]')
    ap.add_argument('--beams', type=int, default=None, help='beams H (default 64; --synthetic: 16)')
    ap.add_argument('--columns', type=int, default=None, help='azimuth columns W (default 2650; --synthetic: 128)')
    ap.add_argument('--incl_lo', type=float, default=None, help='lowest inclination in degrees (default -17.6; --synthetic: -20)')
    ap.add_argument('--incl_hi', type=float, default=None, help='highest inclination in degrees (default 2.4; --synthetic: 20)')
    ap.add_argument('--max_range', type=float, default=75.0, help='returns beyond it are dropped (scene units)')
    ap.add_argument('--q', type=float, default=0.5, help='the quantile of the ray\'s weights that is the return')
    ap.add_argument('--min_acc', type=float, default=0.5, help='rays with less accumulated opacity give no return')
    ap.add_argument('--disable_box', type=int, action='append', default=[], help='box index to switch off (repeatable)')
    return ap


# camera axes (x right, y up, looking along -z) <- sensor axes (x forward, y left, z up)
CAM_FROM_SENSOR = ((0.0, -1.0, 0.0), (0.0, 0.0, 1.0), (-1.0, 0.0, 0.0))


def main(argv=None):
    args = build_parser().parse_args(argv)
    import numpy as np
    from . import lidar, trajectory, vis
    if not args.synthetic and (args.data_dir is None or args.train_dir is None or args.sweeps is None):
        raise SystemExit('render_lidar: --data_dir, --train_dir and --sweeps are required (or --synthetic)')
    dev, config, dataset = open_scene(args)
    dflt = (16, 128, -20.0, 20.0) if args.synthetic else (64, 2650, -17.6, 2.4)
    H, W, lo, hi = [d if v is None else v for v, d in zip((args.beams, args.columns, args.incl_lo, args.incl_hi), dflt)]
    sensor = lidar.LidarSensor.uniform(H, math.radians(lo), math.radians(hi), W, max_range=args.max_range)
    ext = dataset.ext if args.synthetic else dataset.peek()['ext']
    model, variables, alpha = restore_model(args, config, dataset, dev)
    if args.sweeps is not None:
        with np.load(args.sweeps) as z:
            pose_start = np.asarray(z['pose_start'], np.float64).reshape(-1, 3, 4)
            pose_end = np.asarray(z['pose_end'], np.float64).reshape(-1, 3, 4) if 'pose_end' in z.files else None
            times = np.asarray(z['times'], np.float32).reshape(-1)
    else:
        c2w = camera.c2w(dataset.ts_data[0].cams[0]).astype(np.float64)
        p0 = np.concatenate([c2w[:, :3] @ np.asarray(CAM_FROM_SENSOR), c2w[:, 3:]], 1)
        p1 = p0.copy()
        p1[:, :3] = p0[:, :3] @ lidar.rodrigues([0.0, 0.0, 0.1])
        p1[:, 3] += 0.05 * p0[:, 0]
        pose_start, pose_end = np.stack([p0, p0]), np.stack([p0, p1])
        times = np.array([0.0, min(0.5, dataset.T - 1.0)], np.float32)
    K = variables.layout.K
    enable = None
    if args.disable_box:
        bad = [k for k in args.disable_box if not 0 <= k < K]
        if bad:
            raise SystemExit('render_lidar: --disable_box %s of K = %d boxes' % (bad, K))
        enable = [0 if k in args.disable_box else 1 for k in range(K)]
    res = lidar.render_lidar(model, variables, sensor, pose_start, times, ext, config.white_bkgd, alpha, near=config.near,
                             far=config.far, pose_end=pose_end, chunk=args.chunk, q=args.q, min_acc=args.min_acc, box_enable=enable)
    os.makedirs(args.eval_dir, exist_ok=True)
    pics = vis.visualize_depth(res['range'], res['acc'], out8=True).cpu().numpy()
    rng = res['range'].cpu().numpy()
    total = 0
    for f in range(rng.shape[0]):
        np.save(os.path.join(args.eval_dir, 'range_%04d.npy' % f), rng[f])
        trajectory.write_ppm(os.path.join(args.eval_dir, 'range_%04d.ppm' % f), pics[f])
        points, count = lidar.point_cloud(res, f)
        total += lidar.write_ply(os.path.join(args.eval_dir, 'sweep_%04d.ply' % f), points, count)
    print('render_lidar: %d sweeps of %d x %d, %d returns, written to %s' % (rng.shape[0], H, W, total, args.eval_dir))
    return 0


if __name__ == '__main__':
    sys.exit(main())
