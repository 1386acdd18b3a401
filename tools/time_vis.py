#!/usr/bin/env python3
"""What the depth visualisations cost: durf_amd.vis.visualize_suite (B: csrc/vis.hip, six launches for any
number of frames) against the same three pictures composed from torch operators on the device (A: what a user would write
from internal/vis.py -- sort for the planes, a table gather, conv2d for the normals), for 1 and for 20 frames of 320 x 480,
float and 8-bit output.  Depths are smooth in [1, 40], acc is random.

HIP events around each call, warm-up, the median of --repeats calls per block and of --blocks blocks per variant, the variants
interleaved so that clock drift hits all alike.  A's launches are counted as the aten operators it dispatches (each is at
least one launch; sort and cumsum are several).  For scale: one 320 x 480 image render is 36.2 ms.  Prints one text
report (--out profiles/vis_time.txt keeps it; no such run is on record yet).

    python tools/time_vis.py [--blocks 5] [--repeats 5] [--out FILE]
"""
import argparse
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def torch_suite(depth, acc, lut, out8):
    """internal/vis.py's visualize_suite from torch operators, batched over frames ([F,H,W] -> three [F,H,W,3])"""
    import torch
    import torch.nn.functional as Fn
    eps = float(torch.finfo(torch.float32).eps)
    F, H, W = depth.shape
    nan = torch.isnan(depth)
    a = torch.where(nan, torch.zeros_like(acc), acc)[..., None]
    ds = torch.sort(depth.reshape(F, -1), dim=1).values                      # NaNs last
    near, far = ds[:, :1] - eps, ds[:, -1:] + eps
    curve = lambda x: -torch.log(x + eps)                                    # noqa: E731
    d, n, f = curve(depth), curve(near)[..., None], curve(far)[..., None]
    value = torch.nan_to_num(torch.clamp((d - torch.minimum(n, f)) / torch.abs(f - n), 0, 1))
    pic_depth = lut[torch.clamp((value * 256).long(), max=255)] * a + (1 - a)
    h = (torch.remainder(d, 0.1) / 0.1)[..., None]
    bow = torch.sin(math.pi * (torch.tensor([3 / 6, 5 / 6, 7 / 6], device=depth.device) - h)) ** 2
    pic_mod = bow * a + (1 - a)
    ok = ~nan
    cnt = ok.sum((1, 2), keepdim=True).double()
    x = torch.arange(W, device=depth.device, dtype=torch.float64).expand(F, H, W)
    y = torch.arange(H, device=depth.device, dtype=torch.float64)[:, None].expand(F, H, W)

    def var(v):
        v = torch.where(ok, v, torch.zeros_like(v))
        m = v.sum((1, 2), keepdim=True) / cnt
        return (torch.where(ok, (v - m) ** 2, torch.zeros_like(v))).sum((1, 2), keepdim=True) / cnt
    scale = torch.sqrt((var(x) + var(y)) / 2 / var(depth.double())).float()
    s = (scale * depth)[:, None]
    blur, edge = torch.tensor([1., 2., 1.], device=depth.device) / 4, torch.tensor([-1., 0., 1.], device=depth.device) / 2
    ky = (blur[None, :] * edge[:, None]).flip(0, 1)[None, None]              # conv2d correlates: flip for a true convolution
    kx = (blur[:, None] * edge[None, :]).flip(0, 1)[None, None]
    dy, dx = Fn.conv2d(s, ky, padding=1)[:, 0], Fn.conv2d(s, kx, padding=1)[:, 0]
    inv = 1 / torch.sqrt(1 + dx ** 2 + dy ** 2)
    nrm = torch.stack([dx * inv, dy * inv, inv], -1)
    pic_n = torch.isnan(nrm).float() + torch.nan_to_num((nrm + 1) / 2)
    pic_n = pic_n * acc[..., None] + (1 - acc[..., None])
    pics = {'depth': pic_depth, 'depth_mod': pic_mod, 'depth_normals': pic_n}
    if out8:
        pics = {k: torch.round(torch.nan_to_num(v).clamp(0, 1) * 255).to(torch.uint8) for k, v in pics.items()}
    return pics


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--blocks', type=int, default=5)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--out', default=None, help='also write the report to this file')
    args = ap.parse_args()
    import numpy as np
    import torch
    from torch.utils._python_dispatch import TorchDispatchMode
    from durf_amd import ops, vis
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    H, W = 320, 480
    lut = torch.tensor(ops.vis_turbo_lut(), device=dev)

    class Count(TorchDispatchMode):
        n = 0

        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            Count.n += 1
            return func(*args, **(kwargs or {}))

    def one(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    L = ['depth visualisations (depth, depth_mod, depth_normals), frames of %d x %d, %s' % (H, W, torch.cuda.get_device_name(dev)),
         'ms per call: median over %d blocks of the median of %d calls each; [min .. max] of the block medians' % (args.blocks, args.repeats),
         'A: torch operators   B: durf_amd.vis.visualize_suite (3 statistics launches + 3 picture launches)']
    for F in (1, 20):
        rs = np.random.default_rng(F)
        yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
        depth = np.stack([20.5 + 19.0 * np.sin(0.01 * (f + 1) * xx + 0.013 * yy + f) * np.cos(0.007 * yy) for f in range(F)]).astype(np.float32)
        d = torch.tensor(depth, device=dev)
        a = torch.tensor(rs.uniform(0, 1, depth.shape).astype(np.float32), device=dev)
        variants = {}
        for out8 in (False, True):
            tag = '8-bit' if out8 else 'float'
            variants['A %s' % tag] = lambda out8=out8: torch_suite(d, a, lut, out8)
            variants['B %s' % tag] = lambda out8=out8: vis.visualize_suite(d, a, out8=out8)
        # the two agree (A is fp32 torch arithmetic: a colour-map pixel on a step of the table may differ by a row)
        pa, pb = variants['A float'](), variants['B float']()
        agree = {k: float((torch.nan_to_num(pa[k] - pb[k]).abs().amax(-1) <= 1e-4).float().mean()) for k in pa}
        del pa, pb
        with Count():
            Count.n = 0
            variants['A float']()
            n_float = Count.n
            Count.n = 0
            variants['A 8-bit']()
            n_u8 = Count.n
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
        med = {k: statistics.median(v) for k, v in blocks.items()}
        L.append('F = %d   (pixels within 1e-4 of each other, A against B: %s)' % (F, ', '.join('%s %.4f' % kv for kv in agree.items())))
        for k in variants:
            launches = '6 launches' if k.startswith('B') else '%d aten operators' % (n_u8 if '8-bit' in k else n_float)
            L.append('  %-10s %9.3f   [%.3f .. %.3f]   %s' % (k, med[k], min(blocks[k]), max(blocks[k]), launches))
        L.append('  B / A: float %.4f, 8-bit %.4f' % (med['B float'] / med['A float'], med['B 8-bit'] / med['A 8-bit']))
    text = '\n'.join(L)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, 'w').write(text + '\n')


if __name__ == '__main__':
    main()
