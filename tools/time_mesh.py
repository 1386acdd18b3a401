#!/usr/bin/env python3
"""What the surface costs: durf_amd.mesh.surface on a 128^3 grid (B: count, the one read of the two counts,
exact allocation, emit with normals) beside the durf_amd.field.grid call that made the grid (A: density only, K = 3 boxes,
chunk 65536), in the same process.  iso is the median of the grid's valid densities, so about half the lattice is in: a
freshly initialised field is noise and its surface far larger than a trained scene's, which makes B an upper bound.  No time
is promised: the feature replaces nothing; the MLP query that fills the grid bounds the product.

HIP events around each call, warm-up, the median of --repeats calls per block and of --blocks blocks per variant, the variants
interleaved so that clock drift hits all alike.  Prints one text report (--out profiles/mesh_time.txt keeps it).

    python tools/time_mesh.py [--cells 128] [--blocks 5] [--repeats 1] [--chunk 65536] [--out FILE]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cells', type=int, default=128)
    ap.add_argument('--blocks', type=int, default=5)
    ap.add_argument('--repeats', type=int, default=1)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--chunk', type=int, default=65536)
    ap.add_argument('--out', default=None, help='also write the report to this file')
    args = ap.parse_args()
    import torch
    import bench
    from durf_amd import field, mesh, synthetic
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    w = bench.setup_workload('cfg3', dev)
    model, variables = w['model'], w['state'].variables
    ext = torch.tensor(synthetic.make_batch(1024, w['K'], seed=7, far=w['far'])['ext'], device=dev)
    n1 = args.cells
    half = 2.0
    step = 2 * half / n1
    state = {}

    def grid():                                   # A
        state['g'] = field.grid(model, variables, (-half, -half, -half), (n1, n1, n1), step=step, ext=ext, chunk=args.chunk)

    grid()
    torch.cuda.synchronize()
    g = state['g']
    iso = float(g['density'][g['valid'] != 0].median())

    def surface():                                # B
        state['m'] = mesh.surface(g, iso)

    variants = {'A: field.grid': grid, 'B: mesh.surface': surface}
    for fn in variants.values():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    nv, nt = (int(x) for x in state['m']['counts'].cpu())

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
    a, b = (med[k] for k in variants)
    L = ['surface extraction, %d^3 = %d lattice points, K = %d, iso = %.4f (the median density), %s'
         % (n1, n1 ** 3, w['K'], iso, torch.cuda.get_device_name(dev)),
         'vertices: %d; triangles: %d' % (nv, nt),
         'ms per call: median over %d blocks of the median of %d calls each; [min .. max] of the block medians' % (args.blocks, args.repeats)]
    for k in variants:
        L.append('  %-28s %10.3f   [%.3f .. %.3f]' % (k, med[k], min(blocks[k]), max(blocks[k])))
    L.append('B / A = %.4f: the surface beside the query that made its grid (B includes the read of the two counts and the allocation)' % (b / a))
    L.append('lattice points per second: B %.3e' % (n1 ** 3 / b * 1e3))
    text = '\n'.join(L)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, 'w').write(text + '\n')


if __name__ == '__main__':
    main()
