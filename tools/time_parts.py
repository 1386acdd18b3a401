#!/usr/bin/env python3
"""What the connected components cost: durf_amd.parts.components (label + number + the one read of the count +
stats) on a 128^3 lattice beside the durf_amd.mesh.surface call on the same lattice at the same iso, in the same process --
a classify-scan-emit pipeline over the same n points, which is the yardstick: labelling that costs several times as much
means the tile pass is not doing its job.  Two fillings: the synthetic scene's density grid at its median density (as
tools/time_mesh.py), and rng.random < 0.3, which gives the most unions.  The three stages of components are also timed one by
one, and scipy.ndimage.label on the host copy, the copy included, stands beside them for scale (wall clock; skipped where
scipy is missing).  No time is promised: the feature replaces nothing.

HIP events around each call, warm-up, the median of --repeats calls per block and of --blocks blocks per variant, the variants
interleaved so that clock drift hits all alike.  Prints one text report (--out profiles/parts_time.txt keeps it).

    python tools/time_parts.py [--cells 128] [--blocks 5] [--repeats 3] [--chunk 65536] [--out FILE]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cells', type=int, default=128)
    ap.add_argument('--blocks', type=int, default=5)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--chunk', type=int, default=65536)
    ap.add_argument('--out', default=None, help='also write the report to this file')
    args = ap.parse_args()
    import numpy as np
    import torch
    import bench
    from durf_amd import field, mesh, ops, parts, synthetic
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    w = bench.setup_workload('cfg3', dev)
    model, variables = w['model'], w['state'].variables
    ext = torch.tensor(synthetic.make_batch(1024, w['K'], seed=7, far=w['far'])['ext'], device=dev)
    n1 = args.cells
    half = 2.0
    scene = field.grid(model, variables, (-half, -half, -half), (n1, n1, n1), step=2 * half / n1, ext=ext, chunk=args.chunk)
    scene_iso = float(scene['density'][scene['valid'] != 0].median())
    rnd = torch.as_tensor((np.random.default_rng(0).random((n1, n1, n1)) < 0.3).astype(np.float32)).to(dev)
    fillings = (('the synthetic scene\'s grid, iso = its median density', scene, scene_iso),
                ('rng.random < 0.3', dict(density=rnd, valid=None, frame=scene['frame']), 0.5))

    def one(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    L = ['connected components, %d^3 = %d lattice points, %s' % (n1, n1 ** 3, torch.cuda.get_device_name(dev)),
         'ms per call: median over %d blocks of the median of %d calls each; [min .. max] of the block medians' % (args.blocks, args.repeats)]
    for name, g, iso in fillings:
        d = g['density'].contiguous()
        v = None if g.get('valid') is None else g['valid'].to(torch.uint8).contiguous()
        shape = tuple(d.shape)
        state = {}

        def surface():
            state['m'] = mesh.surface(g, iso)

        def components():
            state['p'] = parts.components(g, iso)

        def label():
            state['labels'], state['ws'] = ops.parts_label(d, v, shape, iso, ws=state.get('ws'))

        def number():
            state['comp'], state['count'] = ops.parts_number(state['labels'], state['ws'])

        def stats():
            ops.parts_stats(state['comp'], shape, state['p']['n'])

        variants = {'A: mesh.surface': surface, 'B: parts.components': components, '   durf_parts_label': label,
                    '   durf_parts_number': number, '   durf_parts_stats': stats}
        for fn in variants.values():
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize()
        blocks = {k: [] for k in variants}
        for _ in range(args.blocks):
            t = {k: [] for k in variants}
            for _ in range(args.repeats):
                for k, fn in variants.items():        # interleaved
                    t[k].append(one(fn))
            for k in variants:
                blocks[k].append(statistics.median(t[k]))
        med = {k: statistics.median(x) for k, x in blocks.items()}
        p = state['p']
        nv, nt = (int(x) for x in state['m']['counts'].cpu())
        L += ['', '%s: %d points in, %d components, the largest of %d points; surface of %d vertices, %d triangles'
              % (name, int((p['comp'] >= 0).sum()), p['n'], int(p['size'].max()) if p['n'] else 0, nv, nt)]
        for k in variants:
            L.append('  %-28s %10.3f   [%.3f .. %.3f]' % (k, med[k], min(blocks[k]), max(blocks[k])))
        a, b = med['A: mesh.surface'], med['B: parts.components']
        L.append('  B / A = %.3f (both include one read-back and their allocations); lattice points per second: B %.3e' % (b / a, n1 ** 3 / b * 1e3))
        try:
            from scipy import ndimage
            from tests import parts_ref
            st = parts_ref.scipy_structure()
            walls = []
            for _ in range(3):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                hd = d.cpu().numpy()
                inn = parts_ref.in_points(hd, None if v is None else v.cpu().numpy(), iso)
                _, count = ndimage.label(inn, structure=st)
                walls.append((time.perf_counter() - t0) * 1e3)
            L.append('  %-28s %10.3f   (wall clock, the copy to the host included; %d components)' % ('scipy.ndimage.label', statistics.median(walls), count))
        except ImportError:
            L.append('  scipy.ndimage.label: scipy is not installed here')
    text = '\n'.join(L)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, 'w').write(text + '\n')


if __name__ == '__main__':
    main()
