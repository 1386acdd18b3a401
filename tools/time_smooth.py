"""What smoothing an extracted mesh costs on the device: smooth.adjacency (the keys, the two sorts, the CSR build, the classes),
10 Taubin iterations (20 steps: a step's time is the call's over 20) and smooth.normals on the surface of the synthetic scene's
128^3 density grid at its median density (tools/time_raster.py's extraction), beside the mesh.surface call that made the mesh, in the same process.  HIP events on the
stream, warm-up, medians of 5 interleaved blocks.  It reports V, T, the mean and maximum degree, the bytes one step must move
(12 V in, 12 V out, 8 per adjacency entry, 4 per offset) and, from the step's time, the bytes per second achieved.  It fails
unless the device equals the numpy oracle (tests/smooth_ref.py) on the first 256 vertices, bit for bit.  No time is promised: the
feature replaces nothing.

    python tools/time_smooth.py [--cells 128] [--iters 10] [--blocks 5] [--repeats 3] [--out FILE]
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
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--blocks', type=int, default=5)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--out', default=None, help='also write the report to this file')
    args = ap.parse_args()
    import numpy as np
    import torch
    import bench
    from durf_amd import field, mesh, ops, smooth, synthetic
    from tests import smooth_ref as S
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    wl = bench.setup_workload('cfg3', dev)
    model, variables = wl['model'], wl['state'].variables
    ext = torch.tensor(synthetic.make_batch(1024, wl['K'], seed=7, far=wl['far'])['ext'], device=dev)
    n1, half = args.cells, 2.0
    g = field.grid(model, variables, (-half, -half, -half), (n1, n1, n1), step=2 * half / n1, ext=ext, chunk=65536)
    iso = float(g['density'][g['valid'] != 0].median())
    m = mesh.surface(g, iso)
    V, T = int(m['vertices'].shape[0]), int(m['triangles'].shape[0])
    adj = smooth.adjacency(m)
    census = smooth.census(adj)
    entries = int(adj['offsets'][-1])
    deg = (adj['offsets'][1:] - adj['offsets'][:-1])
    state = {}

    def taubin():
        state['x'] = ops.smooth_taubin(adj, adj['vertices'], args.iters, 0.5, -0.53)

    variants = {'mesh.surface (count, read, emit)': lambda: mesh.surface(g, iso),
                'smooth.adjacency (two sorts)': lambda: smooth.adjacency(m),
                '%d Taubin iterations' % args.iters: taubin,
                'smooth.normals': lambda: state.__setitem__('n', ops.smooth_normals(adj, state['x'], adj['triangles']))}
    for fn in variants.values():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()

    # the device against the oracle on the first 256 vertices, bit for bit (the oracle runs on the whole mesh: a step reads neighbours)
    v, t = m['vertices'].cpu().numpy(), m['triangles'].cpu().numpy()
    a = S.adjacency(v, t)
    U = int(a['offsets'][-1])
    want_x = S.taubin(a, v, args.iters, 0.5, -0.53)
    want_n = S.normals(a, want_x)
    k = min(256, V)
    same = (np.array_equal(adj['offsets'].cpu().numpy(), a['offsets']) and np.array_equal(adj['neighbours'].cpu().numpy()[:U], a['neighbours'])
            and np.array_equal(adj['multiplicity'].cpu().numpy()[:U], a['multiplicity']) and np.array_equal(adj['vertex_class'].cpu().numpy(), a['vertex_class'])
            and np.array_equal(S.bits(state['x'].cpu().numpy()[:k]), S.bits(want_x[:k])) and np.array_equal(S.bits(state['n'].cpu().numpy()[:k]), S.bits(want_n[:k])))
    if not same:
        sys.exit('time_smooth: the device differs from tests/smooth_ref.py on the first %d vertices' % k)

    def one(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    blocks = {k_: [] for k_ in variants}
    for _ in range(args.blocks):
        tt = {k_: [] for k_ in variants}
        for _ in range(args.repeats):
            for k_, fn in variants.items():               # interleaved
                tt[k_].append(one(fn))
        for k_ in variants:
            blocks[k_].append(statistics.median(tt[k_]))
    med = {k_: statistics.median(x) for k_, x in blocks.items()}
    step_bytes = 12 * V + 12 * V + 8 * entries + 4 * (V + 1)
    L = ['smoothing an extracted mesh, %s' % torch.cuda.get_device_name(dev),
         'the surface of the synthetic scene\'s %d^3 grid at its median density: %d vertices, %d triangles' % (n1, V, T),
         'adjacency entries %d: degree mean %.3f, maximum %d; census: %s' % (entries, entries / max(V, 1), int(deg.max()) if V else 0,
                                                                              ', '.join('%s %s' % kv for kv in census.items())),
         'the device equals tests/smooth_ref.py on the first %d vertices, bit for bit (adjacency, classes, %d iterations, normals)' % (k, args.iters),
         'ms per call: median over %d blocks of the median of %d calls each; [min .. max] of the block medians' % (args.blocks, args.repeats), '']
    for k_ in variants:
        L.append('  %-34s %10.3f   [%.3f .. %.3f]' % (k_, med[k_], min(blocks[k_]), max(blocks[k_])))
    L.append('')
    per = med['%d Taubin iterations' % args.iters] / (2 * args.iters)
    L.append('one step must move %d bytes (12 V in, 12 V out, 8 per adjacency entry, 4 per offset); a step of the Taubin call takes'
             % step_bytes)
    L.append('%.3f ms (its time over %d steps): %.1f GB/s' % (per, 2 * args.iters, step_bytes / (per * 1e-3) / 1e9))
    L.append('time only: an untrained field meshed at its median density; the gather re-reads neighbours through the caches, so the')
    L.append('bytes above are the least a step can move, not what it moves')
    text = '\n'.join(L)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, 'w').write(text + '\n')


if __name__ == '__main__':
    main()
