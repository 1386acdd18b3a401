#!/usr/bin/env python3
"""What the motion products cost: one durf_amd.flow.render_flow over the 19 consecutive pairs of F = 20 frames of
320 x 480 (B: flow, valid, moving, target), the warp of every pair's target frame back onto its source with the occlusion test
(C: frame_depth + warp) and the consistency reduction (D), beside the MipNerfModel.render_trajectory call that produced the
frames (A), in the same run: the synthetic eval scene `bench.py --mode eval` builds (cfg3: K = 3, N = 128, chunk 8192),
tools/time_trajectory.py's cameras and times.  The feature adds work beside the renderer and replaces none of it: B, C and D
are reported against A, not against an earlier way of doing the same.

HIP events around each call, warm-up, the median of --repeats calls per block and of --blocks blocks per variant, the variants
interleaved so that clock drift hits all alike.  Prints one text report (--out profiles/flow_time.txt keeps it).

    python tools/time_flow.py [--frames 20] [--blocks 5] [--repeats 3] [--chunk 8192] [--out FILE]
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
    ap.add_argument('--out', default=None, help='also write the report to this file')
    args = ap.parse_args()
    import numpy as np
    import torch
    import bench
    from durf_amd import flow, synthetic, trajectory
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
    near, far, alpha, white = 0.0, float(w['far']), w['alpha'], config.white_bkgd
    kw = dict(near=near, far=far, chunk=args.chunk)

    def render():                                 # A
        return model.render_trajectory(variables, cams, times, ext, white, alpha, near=near, far=far, chunk=args.chunk,
                                       outputs=('rgb', 'distance', 'acc'))

    out = render()
    state = {}

    def flows():                                  # B: P pairs, one library call
        state['fl'] = flow.render_flow(out, cams, ext, outputs=('flow', 'valid', 'moving', 'target'), **kw)

    def warps():                                  # C: every frame's own depth (F more pairs), then one launch per pair
        state['wp'] = flow.warp(state['fl'], out['rgb'], flow.frame_depth(out, cams, ext, **kw))

    def cons():                                   # D: two launches
        state['cons'] = flow.consistency(state['wp'], out['rgb'], state['fl']['pairs'])

    variants = {'A: render_trajectory': render, 'B: render_flow': flows, 'C: frame_depth + warp': warps, 'D: consistency': cons}
    for fn in variants.values():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    fl, cn = state['fl'], state['cons']
    P = len(fl['pairs'])
    valid, riding, seen = int(fl['valid'].sum()), int((fl['moving'] >= 0).sum()), int(cn['count'].sum())

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
    ka = list(variants)[0]
    L = ['motion between frames, %d pairs of %d x %d, K = %d, %s' % (P, H, W, w['K'], torch.cuda.get_device_name(dev)),
         'valid pixels: %d of %d; riding a box: %d; visible after the warp: %d' % (valid, P * H * W, riding, seen),
         'ms per call: median over %d blocks of the median of %d calls each; [min .. max] of the block medians' % (args.blocks, args.repeats)]
    for k in variants:
        L.append('  %-28s %10.4f   [%.4f .. %.4f]' % (k, med[k], min(blocks[k]), max(blocks[k])))
    L += ['%s / A = %.6f' % (k[0], med[k] / med[ka]) for k in list(variants)[1:]]
    text = '\n'.join(L)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, 'w').write(text + '\n')


if __name__ == '__main__':
    main()
