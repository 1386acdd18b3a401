#!/usr/bin/env python3
"""What fusing depth frames costs: 20 synthetic frames of 320 x 480 (rgb, distance, acc) into a 128^3 and a 256^3
TSDF volume with colour.
  A  the MipNerfModel.render_trajectory call that made the frames
  B  ONE durf_amd.tsdf.integrate call over all of them
  C  a frame-by-frame torch restatement of the same rule (torch_integrate below: one pass of indexing per frame over the whole
     volume); its result must agree with B to within float tolerance (compare() below: asserted, the tool fails
     otherwise) -- bit equality is not expected of it
and durf_tsdf_lattice alone.  Beside B the byte model: the volume's bytes read once and written once (24 per voxel with colour, each way)
over the measured time, as a fraction of 6.29 TB/s.  There is no pass mark: the library replaces nothing, C is the comparison.

HIP events around each call, warm-up, the median of --repeats calls per block and of --blocks blocks per variant, the variants
interleaved so that clock drift hits all alike.  Prints one text report (--out profiles/tsdf_time.txt keeps it).

    python tools/time_tsdf.py [--frames 20] [--blocks 5] [--repeats 3] [--chunk 8192] [--out FILE]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK = 6.29e12


TOL = 2e-5          # |dD| and |dC| allowed between B and C: the 20 updates of a voxel cost a few u = 6e-8 each when every operation
                    # of C rounds as B's does; C's operations are torch's, which need not (a division, a product kept in a register)
FLIPS = 1e-4        # the fraction of the observed voxels allowed beyond TOL: a voxel for which C's rounding of x, y or sdf falls on
                    # the other side of a pixel or band boundary reads another pixel, or takes another rule


def torch_integrate(vol, P, cams, depth, acc, rgb, min_acc=0.5, max_weight=64.0, znear=1e-2):
    """include/durf_tsdf.h's rule without label, xform and frame weights, one frame at a time over all voxels P [n,3], every
    operation written out in the header's order (no matrix product: its order of summation is the library's own)"""
    import torch
    from durf_amd import ops
    D, W, C = vol['tsdf'].reshape(-1), vol['weight'].reshape(-1), vol['colour'].reshape(-1, 4)
    F, h, w = depth.shape
    trunc = vol['trunc']
    for f in range(F):
        c = cams[f]
        d0, d1, d2 = P[:, 0] - c[3], P[:, 1] - c[7], P[:, 2] - c[11]
        pc = [(c[j] * d0 + c[4 + j] * d1) + c[8 + j] * d2 for j in range(3)]
        z = -pc[2]
        x, y = c[ops.CAM_PPX] + (c[ops.CAM_FOCAL] * pc[0]) / z, c[ops.CAM_PPY] - (c[ops.CAM_FOCAL] * pc[1]) / z
        px, py = torch.round(x), torch.round(y)                              # ties to even, as rintf
        ok = torch.isfinite(pc[0]) & torch.isfinite(pc[1]) & torch.isfinite(pc[2]) & (z >= znear) & (x.abs() <= 2 ** 20) & (y.abs() <= 2 ** 20)
        ok &= (px >= 0) & (px < w) & (py >= 0) & (py < h)
        p = torch.where(ok, py * w + px, torch.zeros_like(px)).long()
        dep = depth[f].reshape(-1)[p]
        sdf = dep - z
        ok &= torch.isfinite(dep) & (dep > 0) & (acc[f].reshape(-1)[p] >= min_acc) & ~(sdf < -trunc)
        dn = torch.clamp(sdf / trunc, max=1.0)
        Wn = W + 1.0
        D.copy_(torch.where(ok, (W * D + 1.0 * dn) / Wn, D))
        W.copy_(torch.where(ok, torch.clamp(Wn, max=max_weight), W))
        okc = (ok & (sdf <= trunc))[:, None]
        Wc = C[:, 3:].clone()
        Wcn = Wc + 1.0
        C[:, :3] = torch.where(okc, (Wc * C[:, :3] + 1.0 * rgb[f].reshape(-1, 3)[p]) / Wcn, C[:, :3])
        C[:, 3:] = torch.where(okc, torch.clamp(Wcn, max=max_weight), Wc)


def compare(vb, vc):
    """B's state against C's after ONE call each on new volumes -> dict of the figures the report prints; raises when C does
    not restate B: more than FLIPS of the observed voxels beyond TOL in D, W or colour, or any voxel observed by one alone"""
    import torch
    seen_b, seen_c = vb['weight'] > 0, vc['weight'] > 0
    gap = lambda a, b: torch.where(torch.isnan(a) & torch.isnan(b), torch.zeros_like(a), (a - b).abs())       # NaN where one alone is NaN
    dD, dW, dC = gap(vb['tsdf'], vc['tsdf']), gap(vb['weight'], vc['weight']), gap(vb['colour'], vc['colour']).amax(-1)
    off = ~(dD <= TOL) | ~(dW == 0) | ~(dC <= TOL)                           # a NaN in one alone is a difference
    n_seen, n_off = int(seen_b.sum()), int(off.sum())
    r = dict(seen=n_seen, off=n_off, only_one=int((seen_b != seen_c).sum()), bits=int((~(dD == 0) | ~(dC == 0)).sum()),
             nan=int(torch.isnan(vb['colour']).any(-1).sum()), dD=float(dD[~off].max()), dC=float(dC[~off].max()),
             worst=float(torch.nan_to_num(dD, nan=float('inf')).max()))
    if n_seen == 0 or n_off > FLIPS * n_seen:
        raise SystemExit('time_tsdf: the torch restatement does not restate the library: %d of %d observed voxels differ by more than %g '
                         '(allowed: %g of them); %r' % (n_off, n_seen, TOL, FLIPS, r))
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=20)
    ap.add_argument('--blocks', type=int, default=5)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--chunk', type=int, default=8192)
    ap.add_argument('--out', default=None, help='also write the report to this file')
    args = ap.parse_args()
    import numpy as np
    import torch
    import bench
    from durf_amd import ops, synthetic, trajectory, tsdf
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    wl = bench.setup_workload('cfg3', dev)
    config, model, variables = wl['config'], wl['model'], wl['state'].variables
    ext = torch.tensor(synthetic.make_batch(1024, wl['K'], seed=7, far=wl['far'])['ext'], device=dev)
    H, W, F = 320, 480, args.frames
    yaw = np.deg2rad(10.0)
    keys = np.zeros((2, 3, 4))
    keys[0, :, :3] = np.eye(3)
    keys[1, :, :3] = [[np.cos(yaw), 0, np.sin(yaw)], [0, 1, 0], [-np.sin(yaw), 0, np.cos(yaw)]]
    keys[1, :, 3] = [0.3, 0.0, 0.0]
    c2w, _ = trajectory.make_trajectory(keys, [0.0, 1.0], F)                      # tools/time_trajectory.py's sweep
    cams = trajectory.camera_rows(c2w, 515.0, (W / 2.0, H / 2.0), H, W)
    times = [0.0] * F
    near, far, alpha, white = 0.0, float(wl['far']), wl['alpha'], config.white_bkgd
    state = {}

    def volumetric():
        state['frames'] = model.render_trajectory(variables, cams, times, ext, white, alpha, near=near, far=far, chunk=args.chunk,
                                                  outputs=('rgb', 'distance', 'acc'))

    volumetric()
    fr = state['frames']
    depth, acc, rgb = fr['distance'].reshape(F, H, W).contiguous(), fr['acc'].reshape(F, H, W).contiguous(), fr['rgb'].reshape(F, H, W, 3).contiguous()
    cams_dev = torch.as_tensor(cams).to(dev)
    half = 2.0
    L = ['%d frames of %d x %d fused into TSDF volumes with colour, %s' % (F, H, W, torch.cuda.get_device_name(dev)),
         'pixels of the rendered frames that are not finite: rgb %d, distance %d, acc %d (the rule passes a NaN colour on as it is)'
         % tuple(int((~torch.isfinite(t)).sum()) for t in (rgb, depth, acc)),
         'ms per call: median over %d blocks of the median of %d calls each; [min .. max] of the block medians' % (args.blocks, args.repeats), '']
    for n1 in (128, 256):
        step = 2 * half / (n1 - 1)
        mk = lambda: tsdf.volume((-half, -half, -2 * half), (n1, n1, n1), step=step, trunc=3 * step, device=dev)
        vb, vc = mk(), mk()
        P = torch.stack(torch.meshgrid(*[torch.arange(n1, device=dev, dtype=torch.float32) * step + o for o in (-half, -half, -2 * half)],
                                       indexing='ij'), -1).reshape(-1, 3)

        def fused():
            tsdf.integrate(vb, cams_dev, depth, acc=acc, rgb=rgb)

        def restated():
            torch_integrate(vc, P, cams_dev, depth, acc, rgb)

        def lattice():
            ops.tsdf_lattice(vb['tsdf'], vb['weight'], vb['colour'], vb['shape'], 1.0)

        fused(), restated()
        torch.cuda.synchronize()
        cmp = compare(vb, vc)                                                # after one call each on new volumes; raises when C is no restatement
        variants = {'B: tsdf.integrate': fused, 'C: torch, frame by frame': restated, '   durf_tsdf_lattice': lattice}
        if n1 == 128:
            variants = dict({'A: render_trajectory': volumetric}, **variants)
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
        if 'A: render_trajectory' in med:
            state['A'] = med['A: render_trajectory']
        n = n1 ** 3
        L.append('%d^3 voxels, step %.4f, band 3 steps; after one call %d voxels observed' % (n1, step, cmp['seen']))
        L.append('  B against C (asserted): %d voxels (allowed %d) beyond %g in D, colour or any difference in W, the worst |dD| %.3e; all others'
                 % (cmp['off'], int(FLIPS * cmp['seen']), TOL, cmp['worst']))
        L.append('  within |dD| %.3e, |dC| %.3e; %d voxels differ in any bit; %d observed by one of the two alone; %d voxels hold a NaN colour in both'
                 % (cmp['dD'], cmp['dC'], cmp['bits'], cmp['only_one'], cmp['nan']))
        for k in variants:
            L.append('  %-28s %10.3f   [%.3f .. %.3f]' % (k, med[k], min(blocks[k]), max(blocks[k])))
        b = med['B: tsdf.integrate']
        L.append('  B / A = %.4f, B / C = %.4f; byte model of B: %d bytes (the state read once and written once, 24 per voxel each way) in %.3f ms = %.1f %% of 6.29 TB/s'
                 % (b / state['A'], b / med['C: torch, frame by frame'], 2 * 24 * n, b, 100.0 * 2 * 24 * n / (b * 1e-3) / PEAK))
        L.append('')
        del vb, vc, P
    L.append('time only: the frames are an untrained field\'s; every call of B and C adds the same 20 frames to the volume once more')
    text = '\n'.join(L)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, 'w').write(text + '\n')


if __name__ == '__main__':
    main()
