#!/usr/bin/env python3
"""What a field query costs: one durf_amd.field.grid call over 128^3 cells with K = 3 boxes (A: density only,
chunk 65536) beside ops.mlp_fwd_f32 alone on the same number of pre-made background rows in the same chunks (B), in the same
process.  The expectation under test: classify, lists, encode and activate together add little beside the exact-fp32 MLP --
about 1 MFLOP per row against 60 sines.  (A also runs the object MLPs on the cells inside boxes and the constant term; B is
the background MLP on every row: the share below is A's extra over the MLP it cannot do without.)

HIP events around each call, warm-up, the median of --repeats calls per block and of --blocks blocks per variant, the variants
interleaved so that clock drift hits all alike.  Prints one text report (--out profiles/field_time.txt keeps it).

    python tools/time_field.py [--cells 128] [--blocks 5] [--repeats 1] [--chunk 65536] [--out FILE]
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
    from durf_amd import field, ops, synthetic
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    w = bench.setup_workload('cfg3', dev)
    model, variables = w['model'], w['state'].variables
    ext = torch.tensor(synthetic.make_batch(1024, w['K'], seed=7, far=w['far'])['ext'], device=dev)
    n1 = args.cells
    n = n1 ** 3
    half = 2.0
    step = 2 * half / n1
    state = {}

    def grid():                                   # A
        state['g'] = field.grid(model, variables, (-half, -half, -half), (n1, n1, n1), step=step, ext=ext, chunk=args.chunk)

    B = min(args.chunk, n)
    bk = variables.mlp_flat('MLP_0')
    ws = ops.mlp_f32_pack(256, 60, bk)
    enc = torch.rand(B, 60, device=dev) * 2 - 1
    v27 = torch.zeros(B, 27, device=dev)
    raw = torch.empty(B, 4, device=dev)

    def mlp():                                    # B: the same rows through the background MLP alone, chunk by chunk
        for i in range(0, n, B):
            ops.mlp_fwd_f32(256, 60, min(B, n - i), 1, enc, v27, bk, wstream=ws, raw=raw)

    variants = {'A: field.grid': grid, 'B: mlp_fwd_f32 alone': mlp}
    for fn in variants.values():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    own = state['g']['owner']
    inbox, multi = int((own >= 0).sum()), int((own == -2).sum())

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
    L = ['field query, %d^3 = %d cells, K = %d, chunk %d, %s' % (n1, n, w['K'], args.chunk, torch.cuda.get_device_name(dev)),
         'cells inside a box: %d; inside several: %d' % (inbox, multi),
         'ms per call: median over %d blocks of the median of %d calls each; [min .. max] of the block medians' % (args.blocks, args.repeats)]
    for k in variants:
        L.append('  %-28s %10.3f   [%.3f .. %.3f]' % (k, med[k], min(blocks[k]), max(blocks[k])))
    L.append('(A - B) / A = %.4f: the share of a query that is not the background MLP' % ((a - b) / a))
    L.append('rows per second: A %.3e, B %.3e' % (n / a * 1e3, n / b * 1e3))
    text = '\n'.join(L)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, 'w').write(text + '\n')


if __name__ == '__main__':
    main()
