#!/usr/bin/env python3
"""What evaluating a whole split costs: train_boxpose.evaluate_set -- per group of frames one
render_trajectory call and one two-launch durf_eval_frames call, nothing read back until the end -- against the loop it
replaces: evaluate() per image with float() on both metrics, as train_loop does, on 20 frames of 320 x 480 of
SyntheticTimestepDataset (10 timesteps of 2 cameras) under cfg3's model (K = 3, N = 128, chunk 8192).  The loop is timed
twice: over test cases built beforehand, and with each image's rays generated inside it as next(test_dataset) does.

Also the metrics alone: ops.eval_frames over the 20 rendered frames against per-frame ((rgb - gt) ** 2).mean() +
metrics.compute_ssim, both without a read-back.

HIP events around each pass over the set, warm-up, the variants interleaved in --blocks blocks so that clock drift hits all
of them alike; reported: the median of the blocks and their [min .. max].  Prints one text report
(profiles/eval_set_time.txt is such a run).

    python tools/time_eval_set.py [--blocks 5] [--chunk 8192]
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
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--chunk', type=int, default=8192)
    ap.add_argument('--timesteps', type=int, default=10)
    args = ap.parse_args()
    import torch
    import bench
    from durf_amd import metrics, obbpose_model, ops, raygen, train_boxpose, utils
    from durf_amd import math as dmath
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    w = bench.setup_workload('cfg3', dev)                      # the gin bindings of the eval benchmark's model
    config, alpha = w['config'], w['alpha']
    H, W, n_cams = 320, 480, 2
    ds = train_boxpose.SyntheticTimestepDataset(config, K=w['K'], T=args.timesteps, hw=(H, W), n_cams=n_cams, device=dev, split='test')
    model, variables = obbpose_model.construct_mipnerf(0, ds.peek(), device=dev)
    es = ds.eval_set()
    F = len(es['ts'])

    def test_case(f):
        t, c = f // n_cams, f % n_cams
        rays, px, dp, sk = raygen.generate_batch(ds.ts_data[t], None, config.near, config.far)
        img = lambda x: x[c * H * W:(c + 1) * H * W].reshape(H, W, -1)
        return dict(rays=utils.namedtuple_map(img, rays), pixels=img(px), depth=img(dp), sky=img(sk), init=ds.init, ext=ds.ext, ts=t)

    def loop(cases):
        out = []
        for f in range(F):
            ev = train_boxpose.evaluate(model, config, variables, cases[f] if cases else test_case(f), alpha, chunk=args.chunk)
            out.append((float(ev['psnr']), float(ev['ssim'])))
        return out

    prebuilt = [test_case(f) for f in range(F)]
    first = train_boxpose.evaluate_set(model, config, variables, ds, alpha, chunk=args.chunk)
    frames = [train_boxpose.evaluate(model, config, variables, c, alpha, chunk=args.chunk) for c in prebuilt]
    rgb = torch.stack([e['rgb'] for e in frames]).contiguous()
    dist = torch.stack([e['distance'] for e in frames]).contiguous()
    gt = torch.stack([c['pixels'][..., :3] for c in prebuilt]).contiguous()
    gd = torch.stack([c['depth'][..., 0] for c in prebuilt]).contiguous()

    def metrics_loop():
        return [(dmath.mse_to_psnr(((rgb[f] - gt[f]) ** 2).mean()), metrics.compute_ssim(rgb[f], gt[f], 1.0)) for f in range(F)]

    variants = {
        'evaluate_set (one pass)': lambda: train_boxpose.evaluate_set(model, config, variables, ds, alpha, chunk=args.chunk)['per_frame'].cpu(),
        'loop: evaluate() + float(), cases prebuilt': lambda: loop(prebuilt),
        'loop: evaluate() + float(), rays per image': lambda: loop(None),
        'metrics: eval_frames, 2 launches': lambda: ops.eval_frames(rgb, gt, dist, gd),
        'metrics: mean + compute_ssim per frame': metrics_loop,
    }
    ref = loop(prebuilt)
    table = first['per_frame'].cpu()
    gap_psnr = max(abs(float(table[f, 1]) - ref[f][0]) for f in range(F))
    gap_ssim = max(abs(float(table[f, 2]) - ref[f][1]) for f in range(F))
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
        for k, fn in variants.items():            # interleaved
            blocks[k].append(one(fn))
    med = {k: statistics.median(v) for k, v in blocks.items()}
    print('whole-set evaluation, %d frames of %d x %d, K = %d, N = %d, chunk %d, %s' % (F, H, W, w['K'], model.num_samples, args.chunk,
                                                                                  torch.cuda.get_device_name(dev)))
    print('ms per pass over the set: median of %d interleaved blocks; [min .. max] of the blocks' % args.blocks)
    for k in variants:
        print('  %-46s %10.3f   [%.3f .. %.3f]   %8.3f per frame' % (k, med[k], min(blocks[k]), max(blocks[k]), med[k] / F))
    base = 'loop: evaluate() + float(), cases prebuilt'
    spread = (max(blocks[base]) - min(blocks[base])) / med[base]
    print('evaluate_set / loop (cases prebuilt)        = %.4f' % (med['evaluate_set (one pass)'] / med[base]))
    print('evaluate_set / loop (rays per image)        = %.4f' % (med['evaluate_set (one pass)'] / med['loop: evaluate() + float(), rays per image']))
    print('block-to-block spread of the loop (max - min / median) = %.4f' % spread)
    print('eval_frames / (mean + compute_ssim per frame) = %.4f' % (med['metrics: eval_frames, 2 launches'] /
                                                                  med['metrics: mean + compute_ssim per frame']))
    print('largest difference between the two over the set: psnr %.2e dB, ssim %.2e' % (gap_psnr, gap_ssim))


if __name__ == '__main__':
    main()
