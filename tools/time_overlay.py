#!/usr/bin/env python3
"""What drawing the boxes costs: durf_amd.overlay.project_boxes + draw_boxes (B: csrc/overlay.hip, two launches) on
F = 20 uint8 frames of 320 x 480, K = 3 boxes, lines 1.5 px wide, beside the MipNerfModel.render_trajectory call that produced
those frames (A), in the same run: the synthetic eval scene `bench.py --mode eval` builds (cfg3: K = 3, N = 128, chunk 8192),
tools/time_trajectory.py's cameras and times.  B draws in place on a scratch copy made outside the timed region, from the poses
A returned; B' is the two launches behind overlay_trajectory's copy of the frames.

HIP events around each call, warm-up, the median of --repeats calls per block and of --blocks blocks per variant, the variants
interleaved so that clock drift hits all alike.  Prints one text report (--out profiles/overlay_time.txt keeps it).

    python tools/time_overlay.py [--frames 20] [--blocks 5] [--repeats 3] [--chunk 8192] [--out FILE]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=20)
    ap.add_argument('--blocks', type=int, default=5)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--chunk', type=int, default=8192)
    ap.add_argument('--width', type=float, default=1.5)
    ap.add_argument('--out', default=None, help='also write the report to this file')
    args = ap.parse_args()
    import numpy as np
    import torch
    import bench
    from durf_amd import overlay, synthetic, trajectory
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    w = bench.setup_workload('cfg3', dev)
    config, model, variables = w['config'], w['model'], w['state'].variables
    H, W, F = 320, 480, args.frames
    lay = variables.layout
    ext = torch.tensor(synthetic.make_batch(1024, w['K'], seed=7, far=w['far'])['ext'], device=dev)
    yaw = np.deg2rad(10.0)
    keys = np.zeros((2, 3, 4))
    keys[0, :, :3] = np.eye(3)
    keys[1, :, :3] = [[np.cos(yaw), 0, np.sin(yaw)], [0, 1, 0], [-np.sin(yaw), 0, np.cos(yaw)]]
    keys[1, :, 3] = [0.3, 0.0, 0.0]
    c2w, _ = trajectory.make_trajectory(keys, [0.0, 1.0], F)
    times = [(0.5 * f) % (lay.T - 1.0) if lay.T > 1 else 0.0 for f in range(F)]
    cams = trajectory.camera_rows(c2w, 515.0, (W / 2.0, H / 2.0), H, W)
    cams_dev = torch.tensor(cams, device=dev)
    near, far, alpha, white = 0.0, float(w['far']), w['alpha'], config.white_bkgd

    def render():                                 # A
        return model.render_trajectory(variables, cams, times, ext, white, alpha, near=near, far=far, chunk=args.chunk,
                                       outputs=('rgb8', 'distance'))

    out = render()
    frames = out['rgb8'].reshape(F, H, W, 3)
    scratch = frames.clone()
    poses = out['poses']

    def draw():                                   # B: the two launches
        p = overlay.project_boxes(cams_dev, poses, ext)
        return overlay.draw_boxes(scratch, p['segments'], width=args.width, inplace=True), p['rect']

    def draw_copy():                              # B': behind a copy of the frames, as overlay_trajectory does
        p = overlay.project_boxes(cams_dev, poses, ext)
        return overlay.draw_boxes(frames, p['segments'], width=args.width), p['rect']

    drawn, rect = draw_copy()
    touched = int((drawn != frames).any(-1).sum())
    visible = int((rect[..., 5] > 0.5).sum())
    variants = {'A: render_trajectory': render, 'B: project + draw': draw, 'B\': project + copy + draw': draw_copy}
    for fn in variants.values():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()

    def one(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    blocks = {k: [] for k in variants}
    for _ in range(args.blocks):
        t = {k: [] for k in variants}
        for _ in range(args.repeats):
            for k, fn in variants.items():        # interleaved
                t[k].append(one(fn))
        for k in variants:
            blocks[k].append(statistics.median(t[k]))
    med = {k: statistics.median(v) for k, v in blocks.items()}
    ka, kb, kc = list(variants)
    L = ['box overlay, %d uint8 frames of %d x %d, K = %d, lines %.1f px wide, %s' % (F, H, W, w['K'], args.width, torch.cuda.get_device_name(dev)),
         'visible boxes over the trajectory: %d of %d; pixels the lines change: %d of %d' % (visible, F * w['K'], touched, F * H * W),
         'ms per call: median over %d blocks of the median of %d calls each; [min .. max] of the block medians' % (args.blocks, args.repeats)]
    for k in variants:
        L.append('  %-28s %10.4f   [%.4f .. %.4f]' % (k, med[k], min(blocks[k]), max(blocks[k])))
    L += ['B / A  = %.6f' % (med[kb] / med[ka]), 'B\' / A = %.6f' % (med[kc] / med[ka])]
    text = '\n'.join(L)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, 'w').write(text + '\n')


if __name__ == '__main__':
    main()
