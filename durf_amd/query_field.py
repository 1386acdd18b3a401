"""Query the field of a trained scene over a regular grid and write it to a directory:

    python -m durf_amd.query_field --gin_file configs/waymo.gin --data_dir DATA --train_dir CKPT --grid "ox,oy,oz;nu,nv,nw;step"
                                   --ts T --eval_dir OUT [--sigma 0] [--threshold 1.0] [--disable_box k ...] [--chunk 65536]
    python -m durf_amd.query_field --synthetic --eval_dir OUT [--grid ...]

--grid: the origin of cell (0, 0, 0), the cell counts along x, y, z and one spacing, in scene units; the grid's last axis (z)
is the one the top-down maps look along.  --ts: the timestep whose box poses hold (a fractional one interpolates them).  The
checkpoint in --train_dir is restored and the whole grid is ONE durf_amd.field.grid call (density only: no view direction).
Written: OUT/density.npy ([nu,nv,nw] float32, NaN where a cell lies in several boxes), OUT/owner.npy ([nu,nv,nw] int32: the box
that owns a cell, -1 background, -2 several), OUT/bev_opacity.ppm (1 - exp(-step sum density) per column through turbo),
OUT/bev_height.npy ([nu,nv] int32: the first cell along z whose density reaches --threshold, -1 for none) and OUT/grid.json
(the grid's frame).  --synthetic queries train_boxpose.SyntheticTimestepDataset's scene instead (no data directory; without
--train_dir the freshly initialised model, without --grid a 32 x 32 x 16 grid around the origin), which exercises the command
end to end."""
import argparse
import json
import os
import sys

from .render_traj import add_scene_arguments, open_scene, restore_model


def parse_grid(text):
    """"ox,oy,oz;nu,nv,nw;step" -> (origin [3] floats, shape (nu, nv, nw), step)"""
    parts = text.split(';')
    if len(parts) != 3:
        raise ValueError('--grid: expected "ox,oy,oz;nu,nv,nw;step", got %r' % text)
    origin = [float(x) for x in parts[0].split(',')]
    shape = tuple(int(x) for x in parts[1].split(','))
    step = float(parts[2])
    if len(origin) != 3 or len(shape) != 3 or min(shape) < 1 or not step > 0:
        raise ValueError('--grid: three origin coordinates, three positive counts and a positive step, got %r' % text)
    return origin, shape, step


def build_parser():
    ap = argparse.ArgumentParser(prog='python -m durf_amd.query_field', description=__doc__.split('\n\n')[0])
    add_scene_arguments(ap)
    ap.add_argument('--grid', default=None, help='"ox,oy,oz;nu,nv,nw;step" (--synthetic default: "-2,-2,-1;32,32,16;0.125")')
    ap.add_argument('--ts', type=float, default=0.0, help='timestep of the box poses (fractional: interpolated)')
    ap.add_argument('--sigma', type=float, default=0.0, help='standard deviation of the isotropic Gaussian at every cell')
    ap.add_argument('--threshold', type=float, default=1.0, help='density a cell must reach to count for bev_height')
    ap.add_argument('--disable_box', type=int, action='append', default=[], help='box index to switch off (repeatable)')
    return ap


def main(argv=None):
    args = build_parser().parse_args(argv)
    import numpy as np
    from . import field, trajectory, vis
    if not args.synthetic and (args.data_dir is None or args.train_dir is None or args.grid is None):
        raise SystemExit('query_field: --data_dir, --train_dir and --grid are required (or --synthetic)')
    try:
        origin, shape, step = parse_grid(args.grid if args.grid is not None else '-2,-2,-1;32,32,16;0.125')
    except ValueError as e:
        raise SystemExit('query_field: %s' % e)
    dev, config, dataset = open_scene(args)
    ext = dataset.ext if args.synthetic else dataset.peek()['ext']
    model, variables, alpha = restore_model(args, config, dataset, dev)
    K = variables.layout.K
    enable = None
    if args.disable_box:
        bad = [k for k in args.disable_box if not 0 <= k < K]
        if bad:
            raise SystemExit('query_field: --disable_box %s of K = %d boxes' % (bad, K))
        enable = [0 if k in args.disable_box else 1 for k in range(K)]
    g = field.grid(model, variables, origin, shape, step=step, sigma=args.sigma, ts=args.ts, alpha=alpha, box_enable=enable,
                   chunk=max(args.chunk, 1), ext=ext if K else None)
    m = field.columns(g, threshold=args.threshold)
    os.makedirs(args.eval_dir, exist_ok=True)
    field.write_density(os.path.join(args.eval_dir, 'density'), g)
    np.save(os.path.join(args.eval_dir, 'owner.npy'), g['owner'].cpu().numpy())
    np.save(os.path.join(args.eval_dir, 'bev_height.npy'), m['first'].cpu().numpy())
    # opacity in [0, 1] through turbo: far = 1 is blue under the identity curve, so show 1 - opacity's complement as "depth"
    pic = vis.visualize_depth(1.0 - m['opacity'], None, near=1e-6, far=1.0, curve_fn='identity', out8=True)
    trajectory.write_ppm(os.path.join(args.eval_dir, 'bev_opacity.ppm'), pic.cpu().numpy())
    with open(os.path.join(args.eval_dir, 'grid.json'), 'w') as f:
        json.dump(dict(g['frame'], ts=args.ts, sigma=args.sigma, threshold=args.threshold, step=step), f, indent=1)
    own = g['owner']
    print('query_field: %d x %d x %d cells, %d in boxes, %d in several, written to %s'
          % (shape + (int((own >= 0).sum()), int((own == -2).sum()), args.eval_dir)))
    return 0


if __name__ == '__main__':
    sys.exit(main())
