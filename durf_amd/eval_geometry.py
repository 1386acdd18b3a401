"""Measure a trained scene's geometry against the LIDAR depth of a split -- accuracy, completeness, Chamfer distance and
precision / recall / F-score at thresholds (durf_amd.geometry):

    python -m durf_amd.eval_geometry --gin_file configs/waymo.gin --data_dir DATA --train_dir CKPT --split test --eval_dir OUT
                                     --grid "ox,oy,oz;nu,nv,nw;step" [--iso V] [--source mesh|frames|lidar] [--samples 200000]
                                     [--max_dist 0.5] [--thresholds 0.05,0.1,0.2] [--keep_objects] [--sweeps sweeps.npz]
                                     [--min_component N] [--largest K] [--exact]
    python -m durf_amd.eval_geometry --synthetic --eval_dir OUT [--source ...]

Truth: the union over the split's frames of geometry.depth_points of the frame's LIDAR depth plane (eval_set()['depth']: its
positive pixels).  Points inside any box at their frame's timestep are dropped unless --keep_objects is given: the background
mesh is static.  Prediction (--source): `mesh` (default) extract_mesh's background mesh (--grid, --iso, --sigma: every box
disabled; --min_component, --largest: without its floaters, as extract_mesh) sampled with --samples area-uniform points; `frames` the rendered distance maps of the same cameras, back-projected
at the truth's pixels; `lidar` the returns of rendered sweeps (--sweeps and the sensor arguments of render_lidar; the boxes are
switched off unless --keep_objects).  Written: OUT/geometry.json (everything geometry.cloud_distance returns, the grids, the
source and the point counts), OUT/accuracy.ply (the prediction coloured by its distance to the truth) and OUT/completeness.ply
(the truth coloured by its distance to the prediction), turbo over [0, --max_dist].  --synthetic measures
train_boxpose.SyntheticTimestepDataset's scene (no data directory; without --train_dir the freshly initialised model), which
exercises the command end to end.  --exact (--source mesh only) measures completeness against the mesh itself, not its samples
(geometry.surface_distance: the point-to-triangle distance of durf_amd.closest); geometry.json then holds "exact": true and
completeness.ply is coloured by the exact distances."""
import argparse
import json
import math
import os
import sys

from . import camera
from .query_field import build_parser as _field_parser, parse_grid
from .render_traj import add_scene_arguments, open_scene, restore_model


def default_iso():
    """query_field's --threshold default, as extract_mesh's"""
    return _field_parser().get_default('threshold')


def build_parser():
    ap = argparse.ArgumentParser(prog='python -m durf_amd.eval_geometry', description=__doc__.split('\n\n')[0])
    add_scene_arguments(ap)
    ap.add_argument('--split', choices=('test', 'render'), default='test', help='the frames whose LIDAR depth is the truth')
    ap.add_argument('--source', choices=('mesh', 'frames', 'lidar'), default='mesh', help='what is measured against the truth')
    ap.add_argument('--samples', type=int, default=200000, help='--source mesh: surface samples')
    ap.add_argument('--exact', action='store_true', help='--source mesh: completeness against the mesh itself (point-to-triangle), not its samples')
    ap.add_argument('--max_dist', type=float, default=0.5, help='distances are looked for up to here (scene units)')
    ap.add_argument('--thresholds', default=None, help='comma-separated, at most 8, each <= --max_dist (default: 0.05,0.1,0.2,0.5 up to it)')
    ap.add_argument('--keep_objects', action='store_true', help='keep the truth points inside boxes (and the boxes in a lidar prediction)')
    ap.add_argument('--grid', default=None, help='--source mesh: "ox,oy,oz;nu,nv,nw;step" (--synthetic default: "-2,-2,-1;32,32,16;0.125")')
    ap.add_argument('--iso', type=float, default=default_iso(), help='--source mesh: density at which a point is solid')
    ap.add_argument('--ts', type=float, default=0.0, help='--source mesh: timestep of the box poses')
    ap.add_argument('--sigma', type=float, default=0.0, help='--source mesh: standard deviation of the Gaussian at every lattice point')
    ap.add_argument('--min_component', type=int, default=0, help='--source mesh: drop connected solid regions of fewer lattice points')
    ap.add_argument('--largest', type=int, default=None, help='--source mesh: keep only this many of the biggest connected solid regions')
    ap.add_argument('--sweeps', default=None, help='--source lidar: npz as for render_lidar')
    ap.add_argument('--beams', type=int, default=None, help='--source lidar: beams (default 64; --synthetic: 16)')
    ap.add_argument('--columns', type=int, default=None, help='--source lidar: azimuth columns (default 2650; --synthetic: 128)')
    ap.add_argument('--incl_lo', type=float, default=None, help='--source lidar: lowest inclination in degrees')
    ap.add_argument('--incl_hi', type=float, default=None, help='--source lidar: highest inclination in degrees')
    ap.add_argument('--max_range', type=float, default=75.0, help='--source lidar: returns beyond it are dropped')
    return ap


def truth_cloud(es, config, poses, keep_objects):
    """-> (points [n,3], per frame the [h,w] bool plane of the pixels that gave a truth point)"""
    import numpy as np
    import torch
    from . import geometry
    clouds, planes = [], []
    for f in range(len(es['ts'])):
        cam = es['cams'][f]
        h, w = camera.size(cam)
        d = es['depth'][f].reshape(h * w)
        plane = d > 0
        pts = geometry.depth_points(cam, d, config.near, config.far)
        if not keep_objects and poses is not None and poses.shape[1] > 0:
            ext = np.asarray(torch.as_tensor(es['ext'][f]).detach().cpu().numpy(), np.float64)
            out = geometry.outside_boxes(pts, poses[int(es['ts'][f])], ext)
            plane = plane.clone()
            plane[plane.clone()] = out
            pts = pts[out]
        clouds.append(pts)
        planes.append(plane.reshape(h, w))
    return torch.cat(clouds).contiguous(), planes


def frames_cloud(model, config, variables, es, alpha, chunk, planes):
    """the rendered distance maps of the split's cameras, back-projected at the truth's pixels"""
    import torch
    from . import geometry
    cams, ts = es['cams'], [int(t) for t in es['ts']]
    groups = {}
    for f in range(len(ts)):
        groups.setdefault(camera.size(cams[f]) + (ts[f],), []).append(f)
    clouds = [None] * len(ts)
    for (h, w, t), members in groups.items():
        out = model.render_trajectory(variables, cams[members], [float(t)] * len(members), es['ext'][members[0]], config.white_bkgd, alpha,
                                      near=config.near, far=config.far, chunk=chunk, outputs=('rgb', 'distance', 'acc'))
        for i, f in enumerate(members):
            clouds[f] = geometry.depth_points(cams[f], out['distance'][i], config.near, config.far, mask=planes[f])
    return torch.cat(clouds).contiguous()


def lidar_cloud(args, model, config, variables, dataset, alpha, ext):
    """the valid returns of the rendered sweeps, as python -m durf_amd.render_lidar renders them"""
    import numpy as np
    import torch
    from . import lidar
    from .render_lidar import CAM_FROM_SENSOR
    dflt = (16, 128, -20.0, 20.0) if args.synthetic else (64, 2650, -17.6, 2.4)
    H, W, lo, hi = [d if v is None else v for v, d in zip((args.beams, args.columns, args.incl_lo, args.incl_hi), dflt)]
    sensor = lidar.LidarSensor.uniform(H, math.radians(lo), math.radians(hi), W, max_range=args.max_range)
    if args.sweeps is not None:
        with np.load(args.sweeps) as z:
            pose_start = np.asarray(z['pose_start'], np.float64).reshape(-1, 3, 4)
            pose_end = np.asarray(z['pose_end'], np.float64).reshape(-1, 3, 4) if 'pose_end' in z.files else None
            times = np.asarray(z['times'], np.float32).reshape(-1)
    else:
        c2w = camera.c2w(dataset.ts_data[0].cams[0]).astype(np.float64)
        p0 = np.concatenate([c2w[:, :3] @ np.asarray(CAM_FROM_SENSOR), c2w[:, 3:]], 1)
        pose_start, pose_end, times = p0[None], None, np.zeros(1, np.float32)
    K = variables.layout.K
    res = lidar.render_lidar(model, variables, sensor, pose_start, times, ext, config.white_bkgd, alpha, near=config.near, far=config.far,
                             pose_end=pose_end, chunk=args.chunk, box_enable=None if args.keep_objects or not K else [0] * K)
    clouds = []
    for f in range(len(times)):
        points, count = lidar.point_cloud(res, f)
        clouds.append(points[:int(count.reshape(-1)[0]), :3])
    return torch.cat(clouds).contiguous()


def _json(x):
    if isinstance(x, dict):
        return {k: _json(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [_json(v) for v in x]
    if isinstance(x, float):
        return x if math.isfinite(x) else None
    return x


def main(argv=None):
    args = build_parser().parse_args(argv)
    from . import geometry, mesh
    if not args.synthetic and (args.data_dir is None or args.train_dir is None):
        raise SystemExit('eval_geometry: --data_dir and --train_dir are required (or --synthetic)')
    if args.source == 'mesh' and not args.synthetic and args.grid is None:
        raise SystemExit('eval_geometry: --source mesh needs --grid')
    if args.source == 'lidar' and not args.synthetic and args.sweeps is None:
        raise SystemExit('eval_geometry: --source lidar needs --sweeps')
    if args.exact and args.source != 'mesh':
        raise SystemExit('eval_geometry: --exact needs --source mesh')
    try:
        thresholds = (geometry.DEFAULT_THRESHOLDS if args.thresholds is None else
                      tuple(float(t) for t in args.thresholds.split(',') if t.strip()))
        origin, shape, step = parse_grid(args.grid if args.grid is not None else '-2,-2,-1;32,32,16;0.125')
    except ValueError as e:
        raise SystemExit('eval_geometry: %s' % e)
    dev, config, dataset = open_scene(args, split=args.split)
    ext = dataset.ext if args.synthetic else dataset.peek()['ext']
    model, variables, alpha = restore_model(args, config, dataset, dev)
    K = variables.layout.K
    es = dataset.eval_set()
    poses = variables['params']['box_centers'].detach().cpu().numpy() if K else None       # [T,K,6]: the one read of the poses
    truth, planes = truth_cloud(es, config, poses, args.keep_objects)
    if args.source == 'mesh':
        cleaning = args.min_component or args.largest is not None
        ckw = dict(min_points=args.min_component, largest=args.largest) if cleaning else {}
        bg = mesh.extract(model, variables, origin, shape, step=step, iso=args.iso, colour=None, ts=args.ts, ext=ext if K else None,
                          box_enable=[0] * K if K else None, sigma=args.sigma, alpha=alpha, chunk=max(args.chunk, 1), **ckw)
        pred = None if args.exact else geometry.sample_mesh(bg, args.samples)[0]
        source = dict(kind='mesh', vertices=int(bg['vertices'].shape[0]), triangles=int(bg['triangles'].shape[0]), iso=args.iso,
                      samples=args.samples, frame=bg['frame'])
        if cleaning:
            source.update(min_component=args.min_component, largest=args.largest, **bg['cleaning'])
    elif args.source == 'frames':
        pred = frames_cloud(model, config, variables, es, alpha, args.chunk, planes)
        source = dict(kind='frames', frames=len(es['ts']))
    else:
        pred = lidar_cloud(args, model, config, variables, dataset, alpha, ext)
        source = dict(kind='lidar', sweeps=args.sweeps)
    try:
        if args.exact:
            res = geometry.surface_distance(bg, truth, args.max_dist, thresholds=thresholds, samples=args.samples, keep=True)
            pred = res['pred']
        else:
            res = geometry.cloud_distance(pred, truth, args.max_dist, thresholds=thresholds, keep=True)
    except ValueError as e:
        raise SystemExit('eval_geometry: %s' % e)
    os.makedirs(args.eval_dir, exist_ok=True)
    geometry.write_error_ply(os.path.join(args.eval_dir, 'accuracy.ply'), pred, res['pred_dist'], args.max_dist)
    geometry.write_error_ply(os.path.join(args.eval_dir, 'completeness.ply'), truth, res['truth_dist'], args.max_dist)
    doc = {k: v for k, v in res.items() if k not in ('pred', 'pred_dist', 'pred_index', 'truth_dist', 'truth_index', 'truth_bary')}
    if args.exact:
        doc['exact'] = True
    doc.update(source=source, pred_points=int(pred.shape[0]), truth_points=int(truth.shape[0]), frames=len(es['ts']), split=args.split,
               keep_objects=bool(args.keep_objects))
    with open(os.path.join(args.eval_dir, 'geometry.json'), 'w') as fh:
        json.dump(_json(doc), fh, indent=1)
    print('eval_geometry: %s, %d points against %d LIDAR points: accuracy %s, completeness %s (truncated at %g: %s, %s) -> %s'
          % (args.source, pred.shape[0], truth.shape[0], doc['accuracy'], doc['completeness'], args.max_dist, doc['accuracy_truncated'],
             doc['completeness_truncated'], os.path.join(args.eval_dir, 'geometry.json')))
    return 0


if __name__ == '__main__':
    sys.exit(main())
