#!/usr/bin/env python3
"""What casting rays at a mesh costs, on tools/time_raster.py's scene -- the surface of the synthetic scene's 128^3
density grid at its median density, about 9.7 M triangles, 20 frames of 320 x 480 with the camera inside it:

  A  durf_amd.cast.build on its own: bounds, keys, the stable sort, the build;
  B  durf_amd.cast.cameras for the 20 frames, beside
  C  durf_amd.raster.render_mesh for them (depth and ids only, as B);
  D  one 64 x 1024 sweep by durf_amd.cast.lidar, beside
  E  durf_amd.lidar.render_lidar's volumetric sweep of the same sensor and pose.

No time is promised: the feature replaces nothing.  The report also gives the byte model's input -- the node boxes a ray tests
and the leaves it enters, counted by the numpy walk tests/cast_ref.bvh32 of the same tree on a sample of frame 0's rays -- and
the tool FAILS unless the cast and raster pictures agree under the GPU test's rule (tests/cast_ref.rasteriser_comparison), applied
to --windows windows of frame 0: every triangle that a ray of the window can reach is found by a frustum test in float64, the
float64 twins of both pictures are computed on those, and the rule is applied to the pixels whose nearest triangle the
rasteriser draws at all (one that crosses its near plane it drops by its own rule: those pixels are counted and left out).

HIP events around each call, warm-up, the median of --repeats calls per block and of --blocks blocks per variant, the variants
interleaved.  Prints one text report (--out profiles/cast_time.txt keeps it).

    python tools/time_cast.py [--cells 128] [--frames 20] [--blocks 5] [--repeats 3] [--out FILE]
"""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def window_camera(cam, x0, y0, size):
    """the camera row of the size x size window at (x0, y0) of cam's picture: the same rays, bit for bit, while x0, y0 and the
    principal point are multiples of 1/2 (the differences x - ppx are then exact either way)"""
    c = np.array(cam, np.float32)
    c[13], c[14], c[15], c[16] = c[13] - x0, c[14] - y0, size, size
    return c


def reachable(cam, vertices, triangles, margin=2.0):
    """the triangles a ray of cam's picture (widened by `margin` pixels) can reach, by a float64 frustum test in camera space
    that holds for triangles behind and across the camera too -> (ids int64 [m], zmin float64 [m]: their smallest camera depth)"""
    c = np.asarray(cam, np.float64)
    R, o = c[:12].reshape(3, 4)[:, :3], c[:12].reshape(3, 4)[:, 3]
    pc = (np.asarray(vertices, np.float64) - o) @ R
    z = -pc[:, 2]
    f, ppx, ppy, h, w = c[12:17]
    planes = [f * pc[:, 0] - (-margin - ppx) * z, (w - 1 + margin - ppx) * z - f * pc[:, 0],
              -f * pc[:, 1] - (-margin - ppy) * z, (h - 1 + margin - ppy) * z + f * pc[:, 1], z]
    t = np.asarray(triangles, np.int64)
    keep = np.ones(t.shape[0], bool)
    for p in planes:                                                         # not all three vertices outside one plane
        keep &= (p[t] >= 0).any(1)
    ids = np.nonzero(keep)[0]
    return ids, z[t[ids]].min(1)


def check_window(cam, x0, y0, size, vertices, triangles, rast, cst, znear, cull=0):
    """rasteriser_comparison on one window of one frame.  rast, cst: dict tri, depth [h,w] of the whole frame (host arrays)
    -> the rule's result plus candidates and left_out, or an AssertionError"""
    from tests import cast_ref as R, raster_ref
    wc = window_camera(cam, x0, y0, size)
    ids, zmin = reachable(wc, vertices, triangles)
    v, t = np.asarray(vertices, np.float32), np.asarray(triangles, np.int64)[ids]
    used, sub = np.unique(t, return_inverse=True)                            # the sub-mesh in its own numbering
    vs, ts = v[used], sub.reshape(-1, 3).astype(np.int32)
    back = lambda tri: np.where(tri >= 0, np.append(ids, -1)[np.maximum(tri, 0)], tri)                   # (-1 appended: ids may be empty)
    if len(ids):
        r64 = raster_ref.draw64(wc[None], size, size, vs, ts, znear, cull)
        o, d = R.pinhole32(wc, size, size)
        parts = [R.cast64(vs, ts, o[a:a + 64], d[a:a + 64], cull=cull) for a in range(0, size * size, 64)]
        c64 = {k: np.concatenate([p[k] for p in parts]).reshape(1, size, size) for k in ('tri', 't', 'edge')}
    else:                                                                    # the window looks at nothing
        none = np.full((1, size, size), -1, np.int64)
        r64, c64 = dict(tri=none, depth=np.zeros((1, size, size))), dict(tri=none, t=np.zeros((1, size, size)), edge=np.full((1, size, size), np.inf))
    win = lambda a: np.asarray(a)[None, y0:y0 + size, x0:x0 + size]
    crossing = np.zeros(np.asarray(triangles).shape[0] + 1, bool)            # (the last entry: no triangle)
    crossing[ids] = zmin < znear
    names = lambda tri: crossing[np.where(tri >= 0, tri, -1)]
    left_out = names(win(cst['tri'])) | names(back(c64['tri']))
    res = R.rasteriser_comparison(dict(tri=win(rast['tri']), depth=win(rast['depth'])), dict(tri=win(cst['tri']), depth=win(cst['depth'])),
                                  dict(tri=back(r64['tri']), depth=r64['depth']), dict(tri=back(c64['tri']), depth=c64['t']),
                                  np.asarray(triangles), judged=~left_out, edge=c64['edge'])
    res.update(candidates=int(len(ids)), left_out=int(left_out.sum()))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cells', type=int, default=128)
    ap.add_argument('--frames', type=int, default=20)
    ap.add_argument('--blocks', type=int, default=5)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--windows', type=int, default=2, help='16 x 16 windows of frame 0 the pictures are compared on')
    ap.add_argument('--sample', type=int, default=256, help='rays of frame 0 the numpy walk counts nodes for')
    ap.add_argument('--out', default=None, help='also write the report to this file')
    args = ap.parse_args()
    import torch
    import bench
    from durf_amd import cast, field, lidar, mesh, raster, synthetic, trajectory
    from tests import cast_ref as R
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    wl = bench.setup_workload('cfg3', dev)
    config, model, variables = wl['config'], wl['model'], wl['state'].variables
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
    sensor = lidar.LidarSensor.uniform(64, np.deg2rad(-17.6), np.deg2rad(2.4), 1024, max_range=float(wl['far']))
    pose = np.concatenate([np.eye(3), np.zeros((3, 1))], 1)[None]
    near, far, alpha, white, znear = 0.1, float(wl['far']), wl['alpha'], config.white_bkgd, 1e-2
    state = {}

    def build():
        state['b'] = cast.build(m)

    def cameras():
        state['c'] = cast.cameras(state['b'], cams, attrs=(), label=None)

    def rendered():
        state['r'] = raster.render_mesh(m, cams, znear=znear, attrs=(), label=None)

    def sweep():
        state['s'] = cast.lidar(state['b'], sensor, pose, near=near, far=far)

    def volumetric():
        state['l'] = lidar.render_lidar(model, variables, sensor, pose, [0.0], ext, white, alpha, near=near, far=far, outputs=('range', 'valid'))

    variants = {'A: cast.build': build, 'B: cast.cameras': cameras, 'C: raster.render_mesh': rendered, 'D: cast.lidar, one sweep': sweep,
                'E: render_lidar, one sweep': volumetric}
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
    b, c, r, s = state['b'], state['c'], state['r'], state['s']
    tally = dict(zip(raster.COUNT_FIELDS, (int(x) for x in r['counts'].sum(0))))
    L = ['rays against a mesh, %s' % torch.cuda.get_device_name(dev),
         'the surface of the synthetic scene\'s %d^3 grid at its median density: %d vertices, %d triangles; workspace %d bytes (%.1f per triangle)'
         % (n1, V, T, b['ws'].numel(), b['ws'].numel() / max(T, 1)),
         'cameras: %d frames of %d x %d, cast hits %d of %d pixels, the rasteriser covers %d (its tallies: %s)'
         % (F, H, W, int(c['mask'].sum()), F * H * W, int(r['mask'].sum()), ', '.join('%s %d' % kv for kv in tally.items())),
         'sweep: 64 x 1024, %d returns from the mesh, %d from the field' % (int(s['valid'].sum()), int(state['l']['valid'].sum())),
         'ms per call: median over %d blocks of the median of %d calls each; [min .. max] of the block medians' % (args.blocks, args.repeats), '']
    for k in variants:
        L.append('  %-28s %10.3f   [%.3f .. %.3f]' % (k, med[k], min(blocks[k]), max(blocks[k])))
    L.append('  B / C = %.3f, D / E = %.3f' % (med['B: cast.cameras'] / med['C: raster.render_mesh'], med['D: cast.lidar, one sweep'] / med['E: render_lidar, one sweep']))
    # the byte model: the numpy walk of the same tree on a sample of frame 0's rays
    v, t = m['vertices'].cpu().numpy(), m['triangles'].cpu().numpy()
    o, d = R.pinhole32(cams[0], H, W)
    pick = np.linspace(0, H * W - 1, args.sample).astype(np.int64)
    stats = {}
    tri_s, t_s, _ = R.bvh32(v, t, b['order'].cpu().numpy(), o[pick], d[pick], stats=stats)
    dev_tri, dev_t = c['tri'][0].reshape(-1).cpu().numpy()[pick], c['depth'][0].reshape(-1).cpu().numpy()[pick]
    walk_equal = bool(np.array_equal(tri_s, dev_tri) and np.array_equal(R.bits(t_s), R.bits(dev_t)))
    L += ['', 'the numpy walk of the same tree on %d rays of frame 0: %.1f node boxes tested and %.1f leaves entered per ray (max %d, %d):'
          % (len(pick), stats['nodes'].mean(), stats['leaves'].mean(), stats['nodes'].max(), stats['leaves'].max()),
          '  %.0f bytes of nodes and %.0f of leaf records per ray; the walk and the device agree on these rays in every bit: %s'
          % (32 * stats['nodes'].mean(), 160 * stats['leaves'].mean(), walk_equal)]
    # the pictures, under the GPU test's rule
    host = lambda p: dict(tri=p['tri'][0].cpu().numpy(), depth=p['depth'][0].cpu().numpy())
    rast0, cst0 = host(r), host(c)
    results, failure = [], None
    for i in range(args.windows):
        x0, y0 = (W - 16) * (i + 1) // (args.windows + 1) // 2 * 2, (H - 16) * (i + 1) // (args.windows + 1) // 2 * 2
        try:
            res = check_window(cams[0], x0, y0, 16, v, t, rast0, cst0, znear)
            results.append(res)
            L.append('  window 16 x 16 at (%d, %d) of frame 0: %s' % (x0, y0, res))
        except AssertionError as e:
            failure = 'window at (%d, %d): %r' % (x0, y0, e.args)
            L.append('  FAILED ' + failure)
    text = '\n'.join(L)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, 'w').write(text + '\n')
    if failure or not walk_equal:
        sys.exit('time_cast: the cast and raster pictures do not agree under the rule: %s' % (failure or 'the numpy walk and the device differ'))


if __name__ == '__main__':
    main()
