#!/usr/bin/env python3
"""What the closest point of a mesh costs, on tools/time_raster.py's scene -- the surface of the synthetic scene's
128^3 density grid at its median density, about 9.7 M triangles -- for 2 x 10^5 LIDAR-like points: the returns of one 64 x 3125
sweep of the mesh from inside it (durf_amd.cast.lidar), each moved by measurement noise of --noise standard deviation:

  A  durf_amd.closest.points, the queries sorted by their Morton keys (the default);
  B  the same, unsorted (the sweep's own order: beam by beam);
  C  what it replaces: durf_amd.geometry.sample_mesh for 10^6 samples and geometry.nearest of the points against them.

The tree (cast.build) is built once outside the timed calls, as the grid of C is part of C.  The report also gives the byte
model's input -- the node boxes a query tests and the leaves it enters, counted by the numpy walk tests/closest_ref.walk32 of
the same tree on --sample of the points -- and how far C's sampled distance lies above A's exact one.  The tool FAILS unless the
device equals the numpy walk on those points in every bit.

HIP events around each call, warm-up, the median of --repeats calls per block and of --blocks blocks per variant, the variants
interleaved.  Prints one text report (--out profiles/closest_time.txt keeps it).

    python tools/time_closest.py [--cells 128] [--points 200000] [--samples 1000000] [--blocks 5] [--repeats 3] [--out FILE]
"""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cells', type=int, default=128)
    ap.add_argument('--points', type=int, default=200000)
    ap.add_argument('--samples', type=int, default=1000000)
    ap.add_argument('--max_dist', type=float, default=0.1)
    ap.add_argument('--noise', type=float, default=0.01)
    ap.add_argument('--blocks', type=int, default=5)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--sample', type=int, default=256, help='points the numpy walk counts nodes for and is compared on')
    ap.add_argument('--out', default=None, help='also write the report to this file')
    args = ap.parse_args()
    import torch
    import bench
    from durf_amd import cast, closest, field, geometry, lidar, mesh, synthetic
    from tests import closest_ref as R
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    wl = bench.setup_workload('cfg3', dev)
    model, variables = wl['model'], wl['state'].variables
    ext = torch.tensor(synthetic.make_batch(1024, wl['K'], seed=7, far=wl['far'])['ext'], device=dev)
    n1, half = args.cells, 2.0
    g = field.grid(model, variables, (-half, -half, -half), (n1, n1, n1), step=2 * half / n1, ext=ext, chunk=65536)
    m = mesh.surface(g, float(g['density'][g['valid'] != 0].median()))
    m = dict(vertices=m['vertices'], triangles=m['triangles'])
    V, T = int(m['vertices'].shape[0]), int(m['triangles'].shape[0])
    b = cast.build(m)
    columns = -(-args.points // 64)
    sensor = lidar.LidarSensor.uniform(64, np.deg2rad(-17.6), np.deg2rad(2.4), columns, max_range=float(wl['far']))
    s = cast.lidar(b, sensor, np.concatenate([np.eye(3), np.zeros((3, 1))], 1)[None], near=0.1, far=float(wl['far']))
    xyz = s['xyz'][0].reshape(-1, 3)[s['valid'][0].reshape(-1) > 0][:args.points]
    torch.manual_seed(0)
    p = (xyz + args.noise * torch.randn_like(xyz)).contiguous()
    md, state = args.max_dist, {}

    def sorted_():
        state['a'] = closest.points(b, p, md, sort_queries=True)

    def unsorted():
        state['b'] = closest.points(b, p, md, sort_queries=False)

    def sampled():
        state['c'] = geometry.nearest(p, geometry.sample_mesh(m, args.samples)[0], md)

    variants = {'A: closest.points, sorted': sorted_, 'B: closest.points, unsorted': unsorted, 'C: sample_mesh + nearest': sampled}
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
            for k, fn in variants.items():                # interleaved
                t[k].append(one(fn))
        for k in variants:
            blocks[k].append(statistics.median(t[k]))
    med = {k: statistics.median(x) for k, x in blocks.items()}
    a, u, (cd, ci) = state['a'], state['b'], state['c']
    same = all(bool(torch.equal(a[k].view(torch.int32) if a[k].dtype == torch.float32 else a[k], u[k].view(torch.int32) if u[k].dtype == torch.float32 else u[k]))
               for k in ('tri', 'dist', 'bary', 'point'))
    both = a['mask'] & (ci >= 0)
    L = ['the closest point of a mesh, %s' % torch.cuda.get_device_name(dev),
         'the surface of the synthetic scene\'s %d^3 grid at its median density: %d vertices, %d triangles; workspace %d bytes (%.1f per triangle)'
         % (n1, V, T, b['ws'].numel(), b['ws'].numel() / max(T, 1)),
         'queries: %d returns of a 64 x %d sweep of the mesh, moved by noise of %g; max_dist %g: %d find a triangle, %d find a sample of %d'
         % (p.shape[0], columns, args.noise, md, int(a['mask'].sum()), int((ci >= 0).sum()), args.samples),
         'sorted and unsorted queries give the same bits: %s' % same,
         'where both find something (%d points): exact mean %.6f, sampled mean %.6f, the sampled distance lies %.6f above on average, %.6f at most'
         % (int(both.sum()), float(a['dist'][both].double().mean()), float(cd[both].double().mean()), float((cd - a['dist'])[both].double().mean()),
            float((cd - a['dist'])[both].max())),
         'ms per call: median over %d blocks of the median of %d calls each; [min .. max] of the block medians' % (args.blocks, args.repeats), '']
    for k in variants:
        L.append('  %-30s %10.3f   [%.3f .. %.3f]' % (k, med[k], min(blocks[k]), max(blocks[k])))
    L.append('  A / C = %.3f, B / A = %.3f' % (med['A: closest.points, sorted'] / med['C: sample_mesh + nearest'],
                                             med['B: closest.points, unsorted'] / med['A: closest.points, sorted']))
    # the byte model: the numpy walk of the same tree on a sample of the points
    v, t = m['vertices'].cpu().numpy(), m['triangles'].cpu().numpy()
    pick = np.linspace(0, p.shape[0] - 1, args.sample).astype(np.int64)
    stats = {}
    want = R.walk32(v, t, b['order'].cpu().numpy(), p.cpu().numpy()[pick], md, stats=stats)
    got = tuple(a[k].cpu().numpy()[pick] for k in ('tri', 'dist', 'bary', 'point'))
    walk_equal = all(np.array_equal(R.bits(x), R.bits(y)) for x, y in zip(got, want))
    L += ['', 'the numpy walk of the same tree on %d of the points: %.1f node boxes tested and %.1f leaves entered per query (max %d, %d):'
          % (len(pick), stats['nodes'].mean(), stats['leaves'].mean(), stats['nodes'].max(), stats['leaves'].max()),
          '  %.0f bytes of nodes and %.0f of leaf records per query; the walk and the device agree on these points in every bit: %s'
          % (32 * stats['nodes'].mean(), 160 * stats['leaves'].mean(), walk_equal)]
    text = '\n'.join(L)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, 'w').write(text + '\n')
    if not (walk_equal and same):
        sys.exit('time_closest: %s' % ('the numpy walk and the device differ' if not walk_equal else 'sorted and unsorted queries differ'))


if __name__ == '__main__':
    main()
