"""Render a camera trajectory of a trained scene to a directory -- the reference's `--eval_dir` ('where to render traj to',
internal/utils.py:155) and the loop of notebooks/durf_render_traj.ipynb as a command:

    python -m durf_amd.render_traj --gin_file configs/waymo.gin --data_dir DATA --train_dir CKPT --traj traj.npz --eval_dir OUT
                                   [--cam 0] [--disable_box k ...] [--chunk 8192] [--vis [--vis_near N] [--vis_far F]]
                                   [--boxes [--box_width W] [--box_opacity A]] [--flow]
    python -m durf_amd.render_traj --synthetic --eval_dir OUT [--frames 8] [--traj traj.npz] [--synthetic_size H W]

The checkpoint in --train_dir is restored, the intrinsics (focal, principal point, image size) are those of image --cam of the
dataset's test split, the half extents of the boxes are one timestep's for every frame, and the cameras and times come from
--traj (durf_amd.trajectory.load_trajectory: the notebook's npz or a plain {c2w, times} one; fractional times render the
boxes between two labelled timesteps).  The whole trajectory is ONE
MipNerfModel.render_trajectory call; OUT/%04d.ppm (binary P6) and OUT/distance.npy [F,h,w] are written.  --vis adds the
depth pictures of the reference's evaluation block (vis.visualize_suite) for every frame: OUT/depth_%04d.ppm,
OUT/depth_mod_%04d.ppm and OUT/normals_%04d.ppm, from ONE batched 8-bit durf_amd.vis.visualize_suite call over the
trajectory's distance and acc planes (--vis_near / --vis_far: the planes of the depth picture; unset, every frame takes its
own least and greatest depth).  --boxes adds the frames with the scene's boxes drawn on them, OUT/boxes_%04d.ppm, and the
boxes' 2D rectangles OUT/boxes2d.npy [F,K,6] (xmin, ymin, xmax, ymax, depth of the centre, visible), from
durf_amd.overlay.overlay_trajectory on the call's own poses (a box switched off with --disable_box is not drawn; --box_width:
the lines' width in pixels, --box_opacity: how much of the picture they cover).  --flow adds how the scene moves from every
frame to the next (durf_amd.flow, from the call's own distance, acc and poses: no second render): OUT/flow_%04d.flo (Middlebury
format, unknown where invalid), OUT/flow_%04d.ppm (the Middlebury colour wheel, one scale for the trajectory) and
OUT/consistency.json -- per pair the count, MSE and PSNR of frame f + 1 warped back onto frame f under the occlusion mask, and
their means.  --synthetic renders
train_boxpose.SyntheticTimestepDataset's scene instead (no data directory; without --train_dir the freshly initialised
model, without --traj a sweep between the scene's first and last camera), which exercises the command end to end."""
import argparse
import os
import sys


def add_scene_arguments(ap):
    """the arguments that name a trained scene and where to write: shared with python -m durf_amd.eval_set"""
    ap.add_argument('--gin_file', action='append', default=[])
    ap.add_argument('--gin_param', action='append', default=[])
    ap.add_argument('--train_dir', default=None, help='checkpoint directory (required unless --synthetic)')
    ap.add_argument('--data_dir', default=None, help='dataset directory (loaders: durf_amd.datasets)')
    ap.add_argument('--eval_dir', required=True, help='where to render traj to')
    ap.add_argument('--chunk', type=int, default=8192)
    ap.add_argument('--synthetic', action='store_true', help='render the synthetic scene (no data directory needed)')
    ap.add_argument('--objects', type=int, default=3, help='dynamic boxes of the synthetic scene')
    ap.add_argument('--synthetic_size', type=int, nargs=2, default=None, metavar=('H', 'W'),
                    help='image size of the synthetic scene (default: the dataset\'s own, 64 x 96)')
    return ap


def build_parser():
    ap = argparse.ArgumentParser(prog='python -m durf_amd.render_traj', description=__doc__.split('\n\n')[0])
    add_scene_arguments(ap)
    ap.add_argument('--traj', default=None, help='trajectory npz: the notebook\'s (c2w, ts) pairs or {c2w, times}')
    ap.add_argument('--cam', type=int, default=0, help='index into the dataset\'s image list: the frames use that image\'s intrinsics')
    ap.add_argument('--disable_box', type=int, action='append', default=[], help='box index to switch off (repeatable)')
    ap.add_argument('--frames', type=int, default=8, help='--synthetic without --traj: frames of the generated sweep')
    ap.add_argument('--vis', action='store_true', help='also write depth_%%04d.ppm, depth_mod_%%04d.ppm and normals_%%04d.ppm')
    ap.add_argument('--vis_near', type=float, default=None, help='--vis: near plane of the depth picture (default: per frame, automatic)')
    ap.add_argument('--vis_far', type=float, default=None, help='--vis: far plane of the depth picture (default: per frame, automatic)')
    ap.add_argument('--boxes', action='store_true', help='also write boxes_%%04d.ppm (the frames with the boxes drawn on) and boxes2d.npy')
    ap.add_argument('--box_width', type=float, default=1.5, help='--boxes: width of the lines in pixels')
    ap.add_argument('--box_opacity', type=float, default=1.0, help='--boxes: opacity of the lines, 0..1')
    ap.add_argument('--flow', action='store_true', help='also write flow_%%04d.flo, flow_%%04d.ppm (frame f to f + 1) and consistency.json')
    return ap


def open_scene(args, split='test', boxes=None):
    """-> device, config and the `split` dataset the scene arguments name (the synthetic scene with --synthetic; boxes: its count
    of dynamic boxes, for a command whose --objects means something else; None: args.objects)"""
    import torch
    from . import train_boxpose, utils
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    utils.clear_gin()
    config = utils.load_config(args.gin_file, args.gin_param)
    if args.synthetic:
        size = dict(hw=tuple(args.synthetic_size)) if getattr(args, 'synthetic_size', None) else {}
        dataset = train_boxpose.SyntheticTimestepDataset(config, K=args.objects if boxes is None else int(boxes), device=dev, split=split, **size)
    else:
        from . import datasets
        dataset = datasets.get_dataset(split, args.data_dir, config, device=dev)
    return dev, config, dataset


def restore_model(args, config, dataset, dev):
    """the scene's model with the checkpoint of --train_dir restored (none: freshly initialised) -> (model, variables, alpha:
    the frequency schedule's value at the checkpoint's step)"""
    from . import checkpoints, obbpose_model as om, train_boxpose
    model, variables = om.construct_mipnerf(20200823, dataset.peek(), device=dev)
    state = train_boxpose.create_train_state(variables)
    if args.train_dir is not None:
        state = checkpoints.restore_checkpoint(args.train_dir, state)
    alpha = train_boxpose.make_schedules(config)[2](max(int(state.step), 1))
    return model, state.variables, alpha


def write_pictures(eval_dir, pics):
    """pics {depth, depth_mod, depth_normals}: [F,h,w,3] uint8 host arrays -> depth_%04d.ppm, depth_mod_%04d.ppm, normals_%04d.ppm"""
    from . import trajectory
    for name, key in (('depth', 'depth'), ('depth_mod', 'depth_mod'), ('normals', 'depth_normals')):
        for f in range(len(pics[key])):
            trajectory.write_ppm(os.path.join(eval_dir, '%s_%04d.ppm' % (name, f)), pics[key][f])


def write_flow(eval_dir, out, cams, ext, near, far, enable, chunk):
    """--flow: the motion from every frame to the next (durf_amd.flow) -> flow_%04d.flo, flow_%04d.ppm (one colour scale for
    the whole trajectory) and consistency.json: per pair the count, MSE and PSNR of frame f + 1 warped onto frame f under the
    occlusion mask, and their means over the pairs that have any visible pixel"""
    import json
    import math
    from . import flow, trajectory
    kw = dict(near=near, far=far, box_enable=enable, chunk=chunk)
    fl = flow.render_flow(out, cams, ext, outputs=('flow', 'valid', 'moving', 'target'), **kw)
    P = len(fl['pairs'])
    if P == 0:
        return
    cons = flow.consistency(flow.warp(fl, out['rgb'], flow.frame_depth(out, cams, ext, **kw)), out['rgb'], fl['pairs'])
    pics = flow.flow_to_color(fl['flow'], out8=True).cpu().numpy()
    flows, valid = fl['flow'].cpu().numpy(), fl['valid'].cpu().numpy()
    for p in range(P):
        flow.write_flo(os.path.join(eval_dir, 'flow_%04d.flo' % p), flows[p], valid[p])
        trajectory.write_ppm(os.path.join(eval_dir, 'flow_%04d.ppm' % p), pics[p])
    cols = {k: [float(x) for x in cons[k].cpu().numpy()] for k in ('count', 'mse', 'psnr')}
    rows = [dict(source=int(fl['pairs'][p][0]), target=int(fl['pairs'][p][1]), count=cols['count'][p], mse=cols['mse'][p],
                 psnr=cols['psnr'][p]) for p in range(P)]
    seen = [r for r in rows if r['count'] > 0]
    finite = [r['psnr'] for r in seen if math.isfinite(r['psnr'])]
    mean = dict(count=sum(r['count'] for r in rows) / P, mse=sum(r['mse'] for r in seen) / len(seen) if seen else float('nan'),
                psnr=sum(finite) / len(finite) if finite else float('nan'))
    with open(os.path.join(eval_dir, 'consistency.json'), 'w') as f:
        json.dump(dict(pairs=rows, mean=mean), f, indent=1)


def main(argv=None):
    args = build_parser().parse_args(argv)
    import numpy as np
    from . import camera, trajectory
    if not args.synthetic and (args.data_dir is None or args.train_dir is None or args.traj is None):
        raise SystemExit('render_traj: --data_dir, --train_dir and --traj are required (or --synthetic)')
    dev, config, dataset = open_scene(args)
    cam_rows, ext, key_c2w, key_t = camera.scene_cameras(args, dataset, 'render_traj')
    focal, ppx, ppy, h, w = camera.intrinsics(cam_rows[args.cam])
    model, variables, alpha = restore_model(args, config, dataset, dev)
    if args.traj is not None:
        c2w, times = trajectory.load_trajectory(args.traj)
    else:
        c2w, times = trajectory.make_trajectory(key_c2w, key_t, args.frames)
    K = variables.layout.K
    enable = None
    if args.disable_box:
        bad = [k for k in args.disable_box if not 0 <= k < K]
        if bad:
            raise SystemExit('render_traj: --disable_box %s of K = %d boxes' % (bad, K))
        enable = [0 if k in args.disable_box else 1 for k in range(K)]
    cams = trajectory.camera_rows(c2w, focal, (ppx, ppy), int(h), int(w))
    outputs = ('rgb8', 'distance', 'acc') if args.vis else ('rgb8', 'distance')
    if args.flow:
        outputs = ('rgb8', 'rgb', 'distance', 'acc')
    out = model.render_trajectory(variables, cams, times, ext, config.white_bkgd, alpha, near=config.near, far=config.far,
                                  chunk=args.chunk, box_enable=enable, outputs=outputs)
    os.makedirs(args.eval_dir, exist_ok=True)
    rgb8 = out['rgb8'].cpu().numpy()
    for f in range(rgb8.shape[0]):
        trajectory.write_ppm(os.path.join(args.eval_dir, '%04d.ppm' % f), rgb8[f])
    np.save(os.path.join(args.eval_dir, 'distance.npy'), out['distance'].cpu().numpy())
    if args.vis:
        from . import vis
        shape = (rgb8.shape[0], int(h), int(w))
        dist, acc = out['distance'].reshape(shape), out['acc'].reshape(shape)
        if args.vis_near is None and args.vis_far is None:
            pics = vis.visualize_suite(dist, acc, out8=True)
        else:
            pics = dict(depth=vis.visualize_depth(dist, acc, near=args.vis_near, far=args.vis_far, out8=True),
                        depth_mod=vis.visualize_depth(dist, acc, modulus=0.1, out8=True),
                        depth_normals=vis.visualize_normals(dist, acc, out8=True))
        write_pictures(args.eval_dir, {k: v.cpu().numpy() for k, v in pics.items()})
    if args.boxes:
        from . import overlay
        drawn = overlay.overlay_trajectory(dict(rgb8=out['rgb8'], poses=out['poses']), cams, ext, box_enable=enable,
                                           width=args.box_width, opacity=args.box_opacity)
        boxes8 = drawn['rgb8'].reshape(rgb8.shape[0], int(h), int(w), 3).cpu().numpy()
        for f in range(boxes8.shape[0]):
            trajectory.write_ppm(os.path.join(args.eval_dir, 'boxes_%04d.ppm' % f), boxes8[f])
        np.save(os.path.join(args.eval_dir, 'boxes2d.npy'), drawn['rect'].cpu().numpy())
    if args.flow:
        write_flow(args.eval_dir, out, cams, ext, config.near, config.far, enable, args.chunk)
    print('render_traj: %d frames of %d x %d written to %s' % (rgb8.shape[0], int(h), int(w), args.eval_dir))
    return 0


if __name__ == '__main__':
    sys.exit(main())
