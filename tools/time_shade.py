#!/usr/bin/env python3
"""What a shaded picture costs, on tools/time_raster.py's scene -- the surface of the synthetic scene's 128^3 density
grid at its median density, about 9.7 M triangles, 20 frames of 320 x 480 with the camera inside it; 64 directions, reach 2 % of
the bounding diagonal:

  A  durf_amd.cast.cameras for the 20 frames (depth and ids only): what a picture cost before;
  B  durf_amd.shade.cameras for them: the cast, the surface, the occlusion, the sun and the colour (its waves take 8 x 8 tiles);
  C  the occlusion launch alone (durf_shade_occlusion on B's points and normals), samples in row order;
  D  the same launch with the samples in the order of 8 x 8 pixel tiles, a wave per tile: the one design question a number
     settles -- does a wave that is compact in space beat a wave that is a piece of a row?  (It does: the camera entry keeps
     the tiles, and C stays here as the record of the alternative.)

No time is promised: the feature replaces nothing.  The report also gives the node boxes a secondary ray tests and the leaves it
enters, counted by the numpy walk (tests/shade_ref.occlusion32 over tests/cast_ref.bvh32) of the same tree on --sample pixels of
frame 0, and the tool FAILS unless the device and that walk agree on those pixels' two integers.

HIP events around each call, warm-up, the median of --repeats calls per block and of --blocks blocks per variant, the variants
interleaved.  Prints one text report (--out profiles/shade_time.txt keeps it).

    python tools/time_shade.py [--cells 128] [--frames 20] [--blocks 5] [--repeats 3] [--out FILE]
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
    ap.add_argument('--frames', type=int, default=20)
    ap.add_argument('--dirs', type=int, default=64)
    ap.add_argument('--blocks', type=int, default=5)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--sample', type=int, default=256, help='pixels of frame 0 the numpy walk counts nodes for')
    ap.add_argument('--out', default=None, help='also write the report to this file')
    args = ap.parse_args()
    import torch
    import bench
    from durf_amd import cast, field, mesh, ops, shade, synthetic, trajectory
    from tests import cast_ref as R, shade_ref as S
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
    H, W, F = 320, 480, args.frames
    yaw = np.deg2rad(10.0)
    keys = np.zeros((2, 3, 4))
    keys[0, :, :3] = np.eye(3)
    keys[1, :, :3] = [[np.cos(yaw), 0, np.sin(yaw)], [0, 1, 0], [-np.sin(yaw), 0, np.cos(yaw)]]
    keys[1, :, 3] = [0.3, 0.0, 0.0]
    c2w, _ = trajectory.make_trajectory(keys, [0.0, 1.0], F)                      # tools/time_raster.py's sweep
    cams = trajectory.camera_rows(c2w, 515.0, (W / 2.0, H / 2.0), H, W)
    b = cast.build(m)
    reach = shade.default_reach(m['vertices'])
    bias = reach / 1024.0
    dirs = torch.as_tensor(shade.directions(args.dirs)).to(dev)
    state = {}

    def plain():
        state['c'] = cast.cameras(b, cams, attrs=(), label=None)

    def shaded():
        state['s'] = shade.cameras(b, cams, dirs=dirs, reach=reach, albedo=None)

    shaded()
    s = state['s']
    toward = torch.as_tensor(np.stack([R.pinhole32(cams[f], H, W)[1] for f in range(F)]).reshape(F, H, W, 3)).to(dev)
    bary = ops.cast_cameras(b['ws'], b['T'], torch.as_tensor(cams).to(dev).contiguous(), H, W)[2]
    point, normal = ops.shade_surface(b['vertices'], b['triangles'], s['tri'], bary, toward)
    assert torch.equal(normal.view(torch.int32), s['normal'].view(torch.int32)), 'the separate surface call and the one call differ'
    rows = (point.reshape(-1, 3), normal.reshape(-1, 3))
    perm = torch.arange(F * H * W, device=dev).reshape(F, H // 8, 8, W // 8, 8).permute(0, 1, 3, 2, 4).reshape(-1)
    tiles = (rows[0][perm].contiguous(), rows[1][perm].contiguous())

    def occlusion_rows():
        state['o'] = ops.shade_occlusion(b['ws'], b['T'], rows[0], rows[1], dirs, bias, reach)

    def occlusion_tiles():
        state['t'] = ops.shade_occlusion(b['ws'], b['T'], tiles[0], tiles[1], dirs, bias, reach)

    variants = {'A: cast.cameras': plain, 'B: shade.cameras': shaded, 'C: occlusion, row order': occlusion_rows, 'D: occlusion, 8 x 8 tiles': occlusion_tiles}
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
    used, blocked = s['ao_used'].reshape(-1), s['ao_blocked'].reshape(-1)
    same_rows = torch.equal(state['o'][0], used) and torch.equal(state['o'][1], blocked)
    same_tiles = torch.equal(state['t'][0], used[perm]) and torch.equal(state['t'][1], blocked[perm])
    rays = int(used.sum())
    L = ['a shaded picture of a mesh, %s' % torch.cuda.get_device_name(dev),
         'the surface of the synthetic scene\'s %d^3 grid at its median density: %d vertices, %d triangles' % (n1, V, T),
         '%d frames of %d x %d, %d directions, reach %.5f (2 %% of the bounding diagonal), bias %.3g' % (F, H, W, args.dirs, reach, bias),
         'primary hits %d of %d pixels; secondary rays used %d (%.1f per hit), blocked %d (%.1f %%)'
         % (int(s['mask'].sum()), F * H * W, rays, rays / max(int(s['mask'].sum()), 1), int(blocked.sum()), 100.0 * int(blocked.sum()) / max(rays, 1)),
         'ms per call: median over %d blocks of the median of %d calls each; [min .. max] of the block medians' % (args.blocks, args.repeats), '']
    for k in variants:
        L.append('  %-28s %10.3f   [%.3f .. %.3f]' % (k, med[k], min(blocks[k]), max(blocks[k])))
    a, bb, c, d = (med[k] for k in variants)
    L.append('  B / A = %.2f, D / B = %.2f, D / C = %.3f; %.1f M secondary rays per second in C, %.1f M in D' % (bb / a, d / bb, d / c, rays / c / 1e3, rays / d / 1e3))
    L.append('  the separate occlusion calls equal the one call in both integers: row order %s, tile order %s' % (same_rows, same_tiles))
    # the byte model: the numpy walk of the same tree on a sample of frame 0's pixels
    v, t = m['vertices'].cpu().numpy(), m['triangles'].cpu().numpy()
    pick = np.linspace(0, H * W - 1, args.sample).astype(np.int64)
    p0, n0 = point[0].reshape(-1, 3).cpu().numpy()[pick], normal[0].reshape(-1, 3).cpu().numpy()[pick]
    stats = {}
    wu, wb = S.occlusion32(v, t, p0, n0, dirs.cpu().numpy(), bias, reach, order=b['order'].cpu().numpy(), stats=stats)
    du, db = used.cpu().numpy()[pick], blocked.cpu().numpy()[pick]
    walk_equal = bool(np.array_equal(wu, du) and np.array_equal(wb, db))
    if len(stats['nodes']):
        L += ['', 'the numpy walk of the same tree on %d pixels of frame 0 (%d used rays): %.1f node boxes tested and %.1f leaves entered per ray (max %d, %d):'
              % (len(pick), len(stats['nodes']), stats['nodes'].mean(), stats['leaves'].mean(), stats['nodes'].max(), stats['leaves'].max()),
              '  %.0f bytes of nodes and %.0f of leaf records per ray; the walk and the device agree on these pixels in both integers: %s'
              % (32 * stats['nodes'].mean(), 160 * stats['leaves'].mean(), walk_equal)]
    text = '\n'.join(L)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, 'w').write(text + '\n')
    if not (walk_equal and same_rows and same_tiles):
        sys.exit('time_shade: the numpy walk and the device differ, or the separate calls and the one call do')


if __name__ == '__main__':
    main()
