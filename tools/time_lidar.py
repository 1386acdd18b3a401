#!/usr/bin/env python3
"""What a LIDAR sweep costs: ONE durf_amd.lidar.render_lidar call (A) on a 64 x 1024 sweep of the synthetic eval
scene `bench.py --mode eval` builds (cfg3: K = 3, N = 128, chunk 8192), beside MipNerfModel.render_layers on the same rays
precomputed into a buffer (B: what a user had to do before the sensor model existed -- and it yields no return model), in the
same run, and the three new kernels on their own: durf_lidar_rays, durf_lidar_returns and durf_lidar_compact on the sweep's
65536 rays.

HIP events around each call, warm-up, A and B interleaved: the median of --repeats calls per block and of --blocks blocks per
variant, with the [min .. max] of the block medians as the run-to-run spread; the kernels: the median of 20 calls after 5
warm-ups.  Prints one text report (--out profiles/lidar_time.txt keeps it).

    python tools/time_lidar.py [--blocks 5] [--repeats 3] [--chunk 8192] [--out FILE]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--blocks', type=int, default=5)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--chunk', type=int, default=8192)
    ap.add_argument('--out', default=None, help='also write the report to this file')
    args = ap.parse_args()
    import numpy as np
    import torch
    import bench
    from durf_amd import lidar, ops, synthetic, utils
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    w = bench.setup_workload('cfg3', dev)
    config, model, variables = w['config'], w['model'], w['state'].variables
    H, W = 64, 1024
    n = H * W
    N = model.num_samples
    ext = torch.tensor(synthetic.make_batch(1024, w['K'], seed=7, far=w['far'])['ext'], device=dev)
    near, far, alpha, white = 0.05, float(w['far']), w['alpha'], config.white_bkgd
    sensor = lidar.LidarSensor.uniform(H, np.deg2rad(-17.6), np.deg2rad(2.4), W, max_range=far)
    start = np.array([[0.0, -1.0, 0.0, 0.0], [0.0, 0.0, 1.0, 0.0], [-1.0, 0.0, 0.0, 0.0]])      # x forward along the world's -z
    end = start.copy()
    end[:, :3] = start[:, :3] @ lidar.rodrigues([0.0, 0.0, 0.05])
    end[:, 3] += [0.0, 0.0, -0.5]
    outs = ('range', 'spread', 'valid', 'xyz', 'distance', 'acc', 'rgb', 'dynamic')

    def sweep():                                  # A
        return lidar.render_lidar(model, variables, sensor, start[None], [0.0], ext, white, alpha, near=near, far=far,
                                  pose_end=end[None], chunk=args.chunk, outputs=outs)

    res = sweep()
    incl = torch.tensor(sensor.inclinations, device=dev)
    row = lidar.sweep_rows(start, end)[0]
    o, d, v, r, nr, fr = ops.lidar_rays(sensor.row(), incl, row, near, far)
    rays = utils.BoxRays(*[x.reshape(H, W, -1) for x in (o, d, v, r, torch.ones(n, device=dev), nr, fr)])

    def layers():                                 # B
        return model.render_layers(variables, rays, None, ext, 0, white, alpha, chunk=args.chunk, pose=res['box_poses'][0], layers=())

    same = all(torch.equal(layers()[k], res[k][0]) for k in ('rgb', 'distance', 'acc'))
    variants = {'A: render_lidar (one call)': sweep, 'B: render_layers on the rays': layers}
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
    med = {k: statistics.median(x) for k, x in blocks.items()}

    # the three kernels on their own, on planted inputs of the sweep's shape
    g = torch.Generator(device=dev).manual_seed(0)
    wts = torch.rand(n, N, device=dev, generator=g)
    tv = torch.cumsum(torch.rand(n, N + 1, device=dev, generator=g) + 0.1, 1)
    acc = torch.rand(n, device=dev, generator=g)
    ret = ops.lidar_returns(wts, tv, acc, o, d, max_range=float(tv.max()))
    rgb = torch.rand(n, 3, device=dev, generator=g)
    dyn = torch.zeros(n, dtype=torch.int32, device=dev)
    points, source = torch.empty(n, 8, device=dev), torch.empty(n, dtype=torch.int32, device=dev)
    kernels = {
        'durf_lidar_rays': lambda: ops.lidar_rays(sensor.row(), incl, row, near, far),
        'durf_lidar_returns': lambda: ops.lidar_returns(wts, tv, acc, o, d, max_range=float(far)),
        'durf_lidar_compact (3 launches)': lambda: ops.lidar_compact(ret['valid'], ret['xyz'], ret['range'], rgb, dyn, points, source),
    }
    kt = {}
    for k, fn in kernels.items():
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        kt[k] = statistics.median(one(fn) for _ in range(20))
    ka, kb = list(variants)
    spread_b = max(blocks[kb]) - min(blocks[kb])
    L = ['LIDAR sweep, %d x %d rays, K = %d, N = %d, chunk %d, %s' % (H, W, w['K'], N, args.chunk, torch.cuda.get_device_name(dev)),
         'returns in the sweep: %d of %d rays; rgb / distance / acc of A == B bit for bit: %s' % (int(res['valid'].sum()), n, same),
         'ms per call: median over %d blocks of the median of %d calls each; [min .. max] of the block medians' % (args.blocks, args.repeats)]
    for k in variants:
        L.append('  %-34s %10.4f   [%.4f .. %.4f]' % (k, med[k], min(blocks[k]), max(blocks[k])))
    L += ['A - B = %+.4f ms; B\'s own run-to-run spread (max - min of its block medians) = %.4f ms' % (med[ka] - med[kb], spread_b),
          'the new kernels alone, ms per call (HIP events around one stand-alone call, allocation of its outputs included;',
          'median of 20 after 5 warm-ups); durf_lidar_returns reads n (2 N + 1) 4 = %.1f MB once:' % (n * (2 * N + 1) * 4 / 1e6)]
    for k in kernels:
        L.append('  %-34s %10.4f' % (k, kt[k]))
    L.append('sum of the three = %.4f ms = %.4f of B' % (sum(kt.values()), sum(kt.values()) / med[kb]))
    text = '\n'.join(L)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, 'w').write(text + '\n')


if __name__ == '__main__':
    main()
