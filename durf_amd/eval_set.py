"""Evaluate a trained scene on a whole split -- the loop of the reference's notebooks/render_eval_durf.ipynb and of the
evaluation block of train_boxpose.py:535-575 as a command:

    python -m durf_amd.eval_set --gin_file configs/waymo.gin --data_dir DATA --train_dir CKPT --split test --eval_dir OUT
                                [--obj_mask boxes] [--vis] [--frames] [--chunk 8192]
    python -m durf_amd.eval_set --synthetic --eval_dir OUT [--vis] [--frames]

The checkpoint in --train_dir is restored as python -m durf_amd.render_traj restores it, every image of the split ('test': the
held-out images, 'render': every image) is rendered and measured by train_boxpose.evaluate_set -- per group of frames one
MipNerfModel.render_trajectory call and one two-launch durf_eval_frames call -- and the table is read back ONCE.
OUT/metrics.json holds {"fields": [...], "per_frame": [[...], ...], "mean": {psnr, ssim, depth_abs, depth_rmse, obj_psnr},
"frames": F, "rays": n}; a value that is not finite (the object fields without --obj_mask, a frame without a LIDAR return) is
null.  --obj_mask boxes measures the object PSNR over the pixels whose ray hits a box.  --frames writes OUT/%04d.ppm, --vis
the depth pictures OUT/depth_%04d.ppm, OUT/depth_mod_%04d.ppm and OUT/normals_%04d.ppm (render_traj's names).  --synthetic
evaluates train_boxpose.SyntheticTimestepDataset's scene (no data directory; without --train_dir the freshly initialised
model), which exercises the command end to end."""
import argparse
import json
import math
import os
import sys

from . import render_traj


def build_parser():
    ap = argparse.ArgumentParser(prog='python -m durf_amd.eval_set', description=__doc__.split('\n\n')[0])
    render_traj.add_scene_arguments(ap)
    ap.add_argument('--split', choices=('test', 'render'), default='test', help='the images to evaluate: held out, or all')
    ap.add_argument('--obj_mask', choices=('boxes',), default=None, help='object PSNR over the pixels whose ray hits a box')
    ap.add_argument('--vis', action='store_true', help='also write depth_%%04d.ppm, depth_mod_%%04d.ppm and normals_%%04d.ppm')
    ap.add_argument('--frames', action='store_true', help='also write the rendered frames, %%04d.ppm')
    return ap


def _finite(x):
    x = float(x)
    return x if math.isfinite(x) else None


def main(argv=None):
    args = build_parser().parse_args(argv)
    import torch
    from . import train_boxpose, trajectory
    if not args.synthetic and (args.data_dir is None or args.train_dir is None):
        raise SystemExit('eval_set: --data_dir and --train_dir are required (or --synthetic)')
    dev, config, dataset = render_traj.open_scene(args, split=args.split)
    model, variables, alpha = render_traj.restore_model(args, config, dataset, dev)
    res = train_boxpose.evaluate_set(model, config, variables, dataset, alpha, chunk=args.chunk, obj_mask=args.obj_mask,
                                     vis=args.vis, frames=args.frames)
    # the table's one read-back: its rows, then the means
    names = list(res['mean'])
    flat = torch.cat([res['per_frame'].reshape(-1), torch.stack([res['mean'][k] for k in names])]).cpu().tolist()
    n = len(res['fields'])
    rows, means = [flat[f * n:(f + 1) * n] for f in range(res['frames'])], flat[res['frames'] * n:]
    os.makedirs(args.eval_dir, exist_ok=True)
    doc = dict(fields=list(res['fields']), per_frame=[[_finite(v) for v in row] for row in rows],
               mean={k: _finite(v) for k, v in zip(names, means)}, frames=res['frames'], rays=res['rays'])
    with open(os.path.join(args.eval_dir, 'metrics.json'), 'w') as fh:
        json.dump(doc, fh, indent=1)
    if args.frames:
        for f, frame in enumerate(res['rgb8']):
            trajectory.write_ppm(os.path.join(args.eval_dir, '%04d.ppm' % f), frame.cpu().numpy())
    if args.vis:
        render_traj.write_pictures(args.eval_dir, {k: [p[k].cpu().numpy() for p in res['vis']]
                                                  for k in ('depth', 'depth_mod', 'depth_normals')})
    print('eval_set: %d frames, %d rays: psnr %s, ssim %s -> %s' % (res['frames'], res['rays'], doc['mean']['psnr'],
                                                                  doc['mean']['ssim'], os.path.join(args.eval_dir, 'metrics.json')))
    return 0


if __name__ == '__main__':
    sys.exit(main())
