#!/usr/bin/env python3
"""What a cloud comparison costs: one durf_amd.geometry.cloud_distance of --samples area-uniform samples of a
sphere mesh (mesh.surface of an analytic field on a 129^3 lattice, radius 1.3) against --points noisy points on the sphere,
both directions with their statistics -- A with the queries handed over in the order of their own cell keys, B as they come
-- beside C, the brute-force yardstick on the same device over the same sets: torch.cdist in chunks of at most 2^30
distances, .min(1), both directions.  The per-stage times of A (keys + sort of the reference set, the search, the statistics)
are listed for the larger direction.  Nothing is promised or asserted: nobody had measured this; the file records what was
seen.

HIP events around each call, warm-up, the median over --blocks interleaved blocks.  Prints one text report
(--out profiles/geometry_time.txt keeps it).

    python tools/time_geometry.py [--samples 1000000] [--points 200000] [--max_dist 0.05] [--blocks 3] [--out FILE]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--samples', type=int, default=1000000)
    ap.add_argument('--points', type=int, default=200000)
    ap.add_argument('--max_dist', type=float, default=0.05)
    ap.add_argument('--noise', type=float, default=0.01, help='standard deviation of the points around the sphere')
    ap.add_argument('--blocks', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--no_cdist', action='store_true', help='skip the brute-force yardstick')
    ap.add_argument('--out', default=None, help='also write the report to this file')
    args = ap.parse_args()
    import numpy as np
    import torch
    from durf_amd import geometry, mesh, ops
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    n1, R = 129, 1.3
    h = 4.0 / (n1 - 1)
    ax = torch.arange(n1, device=dev, dtype=torch.float32) * h - 2.0
    X = torch.stack(torch.meshgrid(ax, ax, ax, indexing='ij'), -1)
    fr = dict(origin=[-2.0, -2.0, -2.0], du=[h, 0.0, 0.0], dv=[0.0, h, 0.0], dw=[0.0, 0.0, h])
    m = mesh.surface(dict(density=(R - X.norm(dim=-1)).contiguous(), valid=None, frame=fr), 0.0)
    pred = geometry.sample_mesh(m, args.samples)[0]
    g = torch.Generator(device=dev).manual_seed(0)
    d = torch.randn(args.points, 3, device=dev, generator=g)
    truth = (d / d.norm(dim=1, keepdim=True) * (R + args.noise * torch.randn(args.points, 1, device=dev, generator=g))).contiguous()
    th = tuple(t for t in (0.01, 0.02, 0.05) if t <= args.max_dist)
    state = {}

    def run(sort):
        def fn():
            state['res', sort] = geometry.cloud_distance(pred, truth, args.max_dist, thresholds=th, sort_queries=sort)
        return fn

    def brute():
        out = []
        for q, r in ((pred, truth), (truth, pred)):
            rows = max(1, (1 << 30) // max(r.shape[0], 1))
            best = torch.empty(q.shape[0], device=dev)
            for lo in range(0, q.shape[0], rows):
                best[lo:lo + rows] = torch.cdist(q[lo:lo + rows], r).min(1)[0]
            out.append(best.clamp(max=args.max_dist).double().mean())
        state['brute'] = [float(x) for x in torch.stack(out).cpu()]

    # the stages of the larger direction (pred -> truth has more queries; truth -> pred the larger reference set)
    grid = geometry.make_grid(pred, args.max_dist)

    def stage_ref():
        state['prep'] = geometry.sort_reference(pred, grid)

    def stage_search_sorted():
        state['dn'] = geometry.nearest(truth, pred, args.max_dist, sort_queries=True, grid=grid, prepared=state['prep'])

    def stage_search_unsorted():
        geometry.nearest(truth, pred, args.max_dist, sort_queries=False, grid=grid, prepared=state['prep'])

    def stage_stats():
        ops.geom_stats(state['dn'][0], state['dn'][1], th)

    variants = {'A: cloud_distance, sorted queries': run(True), 'B: cloud_distance, unsorted queries': run(False)}
    if not args.no_cdist:
        variants['C: chunked torch.cdist(...).min, both directions'] = brute
    stages = {'  sort_reference (keys, torch.sort, gather) of %d' % pred.shape[0]: stage_ref,
              '  nearest, %d queries sorted (keys, sort, search, scatter)' % truth.shape[0]: stage_search_sorted,
              '  nearest, %d queries unsorted (search)' % truth.shape[0]: stage_search_unsorted,
              '  geom_stats of %d' % truth.shape[0]: stage_stats}
    every = dict(variants, **stages)
    for fn in every.values():
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

    t = {k: [] for k in every}
    for _ in range(args.blocks):
        for k, fn in every.items():               # interleaved
            t[k].append(one(fn))
    med = {k: statistics.median(v) for k, v in t.items()}
    a, b = state['res', True], state['res', False]
    same = all(a[k] == b[k] for k in a if k != 'grids')
    L = ['cloud comparison: %d mesh samples (%d triangles) against %d points, max_dist = %g, %s'
         % (pred.shape[0], m['triangles'].shape[0], truth.shape[0], args.max_dist, torch.cuda.get_device_name(dev)),
         'grids: %s and %s cells' % (a['grids']['pred_to_truth']['dims'], a['grids']['truth_to_pred']['dims']),
         'accuracy %.6f (truncated %.6f), completeness %.6f (truncated %.6f), found %d / %d and %d / %d; sorted and unsorted agree: %s'
         % (a['accuracy'], a['accuracy_truncated'], a['completeness'], a['completeness_truncated'], a['pred_found'], a['pred_usable'],
            a['truth_found'], a['truth_usable'], same),
         'ms per call: median over %d interleaved blocks; [min .. max]' % args.blocks]
    for k in every:
        L.append('  %-66s %10.3f   [%.3f .. %.3f]' % (k, med[k], min(t[k]), max(t[k])))
    if not args.no_cdist:
        L.append('C\'s truncated means: %.6f, %.6f (fp32 cdist; beside A\'s %.6f, %.6f)'
                 % (state['brute'][0], state['brute'][1], a['accuracy_truncated'], a['completeness_truncated']))
        L.append('C / A = %.1f, B / A = %.2f (A and B include two reads of six bounds and the one read of the statistics)'
                 % (med[list(variants)[2]] / med[list(variants)[0]], med[list(variants)[1]] / med[list(variants)[0]]))
    text = '\n'.join(L)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, 'w').write(text + '\n')


if __name__ == '__main__':
    main()
