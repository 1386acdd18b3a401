"""Fuse the rendered depth of a trained scene into TSDF volumes and write their zero levels as triangle meshes:

    python -m durf_amd.fuse_tsdf --gin_file configs/waymo.gin --data_dir DATA --train_dir CKPT --traj traj.npz
                                 --grid "ox,oy,oz;nu,nv,nw;step" --eval_dir OUT [--trunc D] [--objects] [--obj_step S]
                                 [--min_weight 1] [--min_component N] [--largest K] [--cam 0] [--carve]
                                 [--smooth N] [--smooth_lambda 0.5] [--smooth_mu -0.53] [--smooth_boundary pin|slide]
    python -m durf_amd.fuse_tsdf --synthetic --objects --eval_dir OUT [--frames 8] [--grid ...]

The cameras and times come from --traj (render_traj's file), the intrinsics from image --cam of the test split.  Every frame is
rendered once with its layers (durf_amd.tsdf.fuse_scene): the background volume over --grid takes the depth of the scene with
every box switched off, and with --objects every box gets a volume in its own frame (spacing --obj_step, default half the
grid's) that follows it through the frames, fed by the pixels the instance map gives it.  --trunc: the half width of the band in
scene units (default: three steps; the object volumes use three of theirs).  A voxel counts as observed from --min_weight on.
Written: OUT/background.ply, OUT/object_%02d.ply (box k in its canonical frame), OUT/poses.npy ([T,K,6], as extract_mesh writes
it: render_mesh --poses takes it) and OUT/tsdf.json (the shapes, trunc, the observed voxels and the vertices and triangles of
every mesh).  --min_component / --largest: as for extract_mesh (durf_amd.parts).  --smooth N: N Taubin iterations on every mesh after the
cleaning (durf_amd.smooth; vertices and normals change, triangles and colours stay); tsdf.json then gains `smooth` and a `census`
per mesh.  --synthetic fuses
train_boxpose.SyntheticTimestepDataset's scene instead (no data directory), which exercises the command end to end; like
render_traj it needs the one-call inference path (bf16 object MLPs: --gin_param 'MipNerfModel.no_pose_opt = True' --gin_param
'MipNerfModel.no_yaw_opt = True' for a freshly initialised model)."""
import argparse
import json
import os
import sys

from .query_field import parse_grid
from .render_traj import add_scene_arguments, open_scene, restore_model

SYNTHETIC_GRID = '-2,-2,-1;24,24,12;0.17'


def build_parser():
    ap = argparse.ArgumentParser(prog='python -m durf_amd.fuse_tsdf', description=__doc__.split('\n\n')[0], conflict_handler='resolve')
    add_scene_arguments(ap)
    ap.add_argument('--objects', dest='write_objects', action='store_true', help='also fuse one volume per box, in the box\'s frame')
    ap.add_argument('--synthetic_boxes', type=int, default=3, help='dynamic boxes of the synthetic scene')
    ap.add_argument('--traj', default=None, help='trajectory npz: the notebook\'s (c2w, ts) pairs or {c2w, times}')
    ap.add_argument('--cam', type=int, default=0, help='index into the dataset\'s image list: the frames use that image\'s intrinsics')
    ap.add_argument('--frames', type=int, default=8, help='--synthetic without --traj: frames of the generated sweep')
    ap.add_argument('--grid', default=None, help='"ox,oy,oz;nu,nv,nw;step" (--synthetic default: "%s")' % SYNTHETIC_GRID)
    ap.add_argument('--trunc', type=float, default=None, help='half width of the band in scene units (default: 3 steps)')
    ap.add_argument('--obj_step', type=float, default=None, help='--objects: spacing of the object lattices (default: half the grid\'s)')
    ap.add_argument('--pad', type=float, default=0.05, help='--objects: the object lattice reaches ext (1 + pad)')
    ap.add_argument('--carve', action='store_true', help='--objects: a pixel of another label beyond the voxel counts as free space')
    ap.add_argument('--min_weight', type=float, default=1.0, help='a voxel is observed from this weight on')
    ap.add_argument('--min_acc', type=float, default=0.5, help='a pixel below this opacity is no observation')
    ap.add_argument('--batch', type=int, default=8, help='frames staged per integrate call')
    ap.add_argument('--min_component', type=int, default=0, help='drop connected regions of fewer lattice points (0: keep all)')
    ap.add_argument('--largest', type=int, default=None, help='keep only this many of the biggest connected regions')
    from . import smooth
    smooth.add_arguments(ap)
    return ap


def check_args(args):
    """the refusals of the command line, before anything is read -> (origin, shape, step), or SystemExit"""
    if not args.synthetic and (args.data_dir is None or args.train_dir is None or args.traj is None or args.grid is None):
        raise SystemExit('fuse_tsdf: --data_dir, --train_dir, --traj and --grid are required (or --synthetic)')
    try:
        origin, shape, step = parse_grid(args.grid if args.grid is not None else SYNTHETIC_GRID)
    except ValueError as e:
        raise SystemExit('fuse_tsdf: %s' % e)
    if min(shape) < 2:
        raise SystemExit('fuse_tsdf: --grid needs at least two points along every axis, got %s' % (shape,))
    if args.trunc is not None and not args.trunc > 0:
        raise SystemExit('fuse_tsdf: --trunc %g' % args.trunc)
    if args.obj_step is not None and not args.obj_step > 0:
        raise SystemExit('fuse_tsdf: --obj_step %g' % args.obj_step)
    if args.batch < 1 or args.frames < 1:
        raise SystemExit('fuse_tsdf: --batch %d --frames %d' % (args.batch, args.frames))
    if args.min_weight != args.min_weight:
        raise SystemExit('fuse_tsdf: --min_weight %r' % args.min_weight)
    return origin, shape, step


def _record(m, vol):
    census = dict(census=m['census']) if 'census' in m else {}                # (only with --smooth)
    return dict(vertices=int(m['vertices'].shape[0]), triangles=int(m['triangles'].shape[0]), observed=int(m['observed']),
                shape=list(vol['shape']), trunc=vol['trunc'], frame=vol['frame'], **m.get('cleaning', {}), **census)


def main(argv=None):
    args = build_parser().parse_args(argv)
    origin, shape, step = check_args(args)
    import numpy as np
    from . import camera, mesh, smooth, trajectory, tsdf
    sm = smooth.from_args(args, 'fuse_tsdf')
    dev, config, dataset = open_scene(args, boxes=args.synthetic_boxes)  # (--objects is this command's switch, not the box count)
    cam_rows, ext, key_c2w, key_t = camera.scene_cameras(args, dataset, 'fuse_tsdf')
    focal, ppx, ppy, h, w = camera.intrinsics(cam_rows[args.cam])
    model, variables, alpha = restore_model(args, config, dataset, dev)
    if args.traj is not None:
        c2w, times = trajectory.load_trajectory(args.traj)
    else:
        c2w, times = trajectory.make_trajectory(key_c2w, key_t, args.frames)
    cams = trajectory.camera_rows(c2w, focal, (ppx, ppy), int(h), int(w))
    K = variables.layout.K
    obj_step = args.obj_step if args.obj_step is not None else 0.5 * step
    s = tsdf.fuse_scene(model, variables, cams, times, ext if K else None, config.white_bkgd, alpha, origin, shape, step,
                        args.trunc if args.trunc is not None else 3.0 * step, obj_step=obj_step, pad=args.pad, carve=args.carve,
                        near=config.near, far=config.far, chunk=max(args.chunk, 1), batch=args.batch, min_acc=args.min_acc,
                        min_weight=args.min_weight, min_points=args.min_component, largest=args.largest, objects=args.write_objects)
    if sm is not None:                                                       # (after the cleaning; the colours stay the fused ones)
        s['background'] = mesh.smoothed(s['background'], sm)
        s['objects'] = [mesh.smoothed(o, sm) for o in s['objects']]
    os.makedirs(args.eval_dir, exist_ok=True)
    mesh.write_ply(os.path.join(args.eval_dir, 'background.ply'), s['background'])
    meta = dict(frames=int(cams.shape[0]), h=int(h), w=int(w), min_weight=args.min_weight, step=step,
                background=_record(s['background'], s['volumes']['background']), objects=[],
                **(dict(smooth=s['background']['smooth']) if sm is not None else {}))
    for k, (o, v) in enumerate(zip(s['objects'], s['volumes']['objects'])):
        mesh.write_ply(os.path.join(args.eval_dir, 'object_%02d.ply' % k), o)
        meta['objects'].append(dict(_record(o, v), box=k, step=obj_step))
    np.save(os.path.join(args.eval_dir, 'poses.npy'), s['poses'])
    with open(os.path.join(args.eval_dir, 'tsdf.json'), 'w') as f:
        json.dump(meta, f, indent=1)
    print('fuse_tsdf: %d frames; background %d vertices, %d triangles from %d observed voxels; %d object meshes; written to %s'
          % (meta['frames'], meta['background']['vertices'], meta['background']['triangles'], meta['background']['observed'],
             len(meta['objects']), args.eval_dir))
    return 0


if __name__ == '__main__':
    sys.exit(main())
