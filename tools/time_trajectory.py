#!/usr/bin/env python3
"""What a rendered camera trajectory costs: ONE MipNerfModel.render_trajectory call (B) against the loop a
user needed before it, on the same build (A) -- per frame raygen.generate_batch rays of the whole image,
render_layers(pose=...) and the 8-bit conversion in torch -- on the synthetic eval scene `bench.py --mode eval` builds
(320 x 480, cfg3: K = 3, N = 128, chunk 8192), F = 20 frames, every second frame time fractional.  A is given its
in-between poses and its per-camera tables for free (built outside the timed region).

HIP events around each trajectory, warm-up, the median of --repeats trajectories per block and of --blocks blocks per
variant, the variants interleaved so that clock drift hits both alike; the spread of A's block medians is the yardstick
for "B is not slower than A".  Peak device memory of each variant is measured in a pass of its own.  Prints one text
report (--out profiles/trajectory_time.txt keeps it; no such run is on record yet).

    python tools/time_trajectory.py [--frames 20] [--blocks 5] [--repeats 3] [--chunk 8192] [--out FILE]
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
    from durf_amd import camera, raygen, synthetic, trajectory
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    w = bench.setup_workload('cfg3', dev)
    config, model, variables = w['config'], w['model'], w['state'].variables
    H, W, F = 320, 480, args.frames
    lay = variables.layout
    init = variables['params']['box_centers']
    ext = torch.tensor(synthetic.make_batch(1024, w['K'], seed=7, far=w['far'])['ext'], device=dev)      # (tools/time_layers.py's boxes)
    yaw = np.deg2rad(10.0)
    keys = np.zeros((2, 3, 4))
    keys[0, :, :3] = np.eye(3)
    keys[1, :, :3] = [[np.cos(yaw), 0, np.sin(yaw)], [0, 1, 0], [-np.sin(yaw), 0, np.cos(yaw)]]
    keys[1, :, 3] = [0.3, 0.0, 0.0]
    c2w, _ = trajectory.make_trajectory(keys, [0.0, 1.0], F)
    times = [(0.5 * f) % (lay.T - 1.0) if lay.T > 1 else 0.0 for f in range(F)]      # every second one fractional
    cams = camera.rows(c2w, 515.0, (W / 2.0, H / 2.0), H, W)          # synthetic.make_batch's camera
    near, far, alpha, white = 0.0, float(w['far']), w['alpha'], config.white_bkgd
    tables = [raygen.TimestepData([camera.c2w(c)], [515.0], [(W / 2.0, H / 2.0)], [H], [W], device=dev) for c in cams]
    poses = model.render_trajectory(variables, cams, times, ext, white, alpha, near=near, far=far, chunk=args.chunk, outputs=())['poses']

    def loop():                                   # A: what a user had before
        frames, dists, accs = [], [], []
        for f in range(F):
            rays, _, _, _ = raygen.generate_batch(tables[f], None, near, far)
            img = type(rays)(*[r.reshape(H, W, -1) for r in rays])
            out = model.render_layers(variables, img, init, ext, int(times[f]), white, alpha, chunk=args.chunk, pose=poses[f], layers=())
            frames.append(torch.round(out['rgb'].clamp(0, 1) * 255).to(torch.uint8))
            dists.append(out['distance'])
            accs.append(out['acc'])
        return torch.stack(frames), torch.stack(dists), torch.stack(accs)

    def one_call():                               # B
        out = model.render_trajectory(variables, cams, times, ext, white, alpha, near=near, far=far, chunk=args.chunk,
                                      outputs=('rgb8', 'distance', 'acc'))
        return out['rgb8'], out['distance'], out['acc']

    variants = {'A: per-frame loop': loop, 'B: render_trajectory': one_call}
    a, b = loop(), one_call()
    same = all(torch.equal(x, y) for x, y in zip(a, b))
    del a, b
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
    peak = {}
    for k, fn in variants.items():
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        res = fn()
        torch.cuda.synchronize()
        peak[k] = (torch.cuda.max_memory_allocated() - base, sum(x.numel() * x.element_size() for x in res))
        del res
    ka, kb = list(variants)
    spread = (max(blocks[ka]) - min(blocks[ka])) / med[ka]
    ratio = med[kb] / med[ka]
    L = ['trajectory render, %d frames of %d x %d, K = %d, N = %d, chunk %d, %s' % (F, H, W, w['K'], w['N'], args.chunk, torch.cuda.get_device_name(dev)),
         'frame times: %s' % ' '.join('%g' % t for t in times),
         'A and B return the same bytes (rgb8, distance, acc): %s' % same,
         'ms per trajectory: median over %d blocks of the median of %d trajectories each; [min .. max] of the block medians' % (args.blocks, args.repeats)]
    for k in variants:
        L.append('  %-24s %9.3f   [%.3f .. %.3f]   %.3f ms per frame' % (k, med[k], min(blocks[k]), max(blocks[k]), med[k] / F))
    L += ['B / A                                  = %.4f' % ratio,
          'spread of A (max - min of its block medians / median) = %.4f' % spread,
          'B is not slower than A by more than A\'s own spread: %s' % (ratio <= 1.0 + spread),
          'peak device memory during one trajectory, above what was allocated before it (of which: the returned outputs)']
    for k in variants:
        L.append('  %-24s %8.2f MiB   (%.2f MiB)' % (k, peak[k][0] / 2 ** 20, peak[k][1] / 2 ** 20))
    text = '\n'.join(L)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, 'w').write(text + '\n')


if __name__ == '__main__':
    main()
