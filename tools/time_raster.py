#!/usr/bin/env python3
"""What looking at a mesh costs: ONE durf_amd.raster.render_mesh call -- the surface of the synthetic scene's
128^3 density grid at its median density (tools/time_mesh.py's extraction), depth, normals and nothing else, over 20 frames of
320 x 480 -- beside the MipNerfModel.render_trajectory call for the same cameras in the same process: the volumetric frames a
mesh preview stands in for.  The stages of ONE call of render_mesh are also timed one by one (setup, draw at the exact size,
the normals' gather): over the frames of its first call, which is the whole trajectory only where that fits the workspace
bound -- the report says how many frames that is.  No time is promised: the feature replaces nothing.  The report measures
time only: the scene is an untrained field meshed at its median density with the camera inside it, so the difference it
prints between the mesh's depth and the volumetric distance says nothing about how well the two agree on a real surface.

HIP events around each call, warm-up, the median of --repeats calls per block and of --blocks blocks per variant, the variants
interleaved so that clock drift hits all alike.  Prints one text report (--out profiles/raster_time.txt keeps it).

    python tools/time_raster.py [--cells 128] [--frames 20] [--blocks 5] [--repeats 3] [--chunk 8192] [--out FILE]
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
    from durf_amd import field, mesh, ops, raster, synthetic, trajectory
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    wl = bench.setup_workload('cfg3', dev)
    config, model, variables = wl['config'], wl['model'], wl['state'].variables
    ext = torch.tensor(synthetic.make_batch(1024, wl['K'], seed=7, far=wl['far'])['ext'], device=dev)
    n1, half = args.cells, 2.0
    g = field.grid(model, variables, (-half, -half, -half), (n1, n1, n1), step=2 * half / n1, ext=ext, chunk=65536)
    m = mesh.surface(g, float(g['density'][g['valid'] != 0].median()))
    V, T = int(m['vertices'].shape[0]), int(m['triangles'].shape[0])
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
    cams_dev = torch.as_tensor(cams).to(dev)
    state = {}

    def volumetric():
        state['frames'] = model.render_trajectory(variables, cams, times, ext, white, alpha, near=near, far=far, chunk=args.chunk,
                                                  outputs=('rgb8', 'distance', 'acc'))

    def rendered():
        state['r'] = raster.render_mesh(m, cams, attrs=('normals',), label=None)

    per = min(raster.default_frames_per_call(F, T, H, W), F)
    cams_one = cams_dev[:per].contiguous()                # the frames of render_mesh's first call: the stages are timed on these

    def setup():
        state['counts'], state['ws'] = ops.raster_setup(cams_one, H, W, m['vertices'], m['triangles'], 1e-2, ws=state.get('ws'))

    def draw():
        state['tri'], state['depth'], state['bary'] = ops.raster_draw(per, T, H, W, state['ws'], state['n_pairs'], pairs=state.get('pairs'))

    def interp():
        ops.raster_interp(m['triangles'], state['tri'], state['bary'], V, attr_f=m['normals'])

    setup()
    state['n_pairs'] = int(state['counts'].cpu()[0])
    state['pairs'] = torch.empty(max(state['n_pairs'], 1), dtype=torch.int32, device=dev)
    stage_names = ('   durf_raster_setup', '   durf_raster_draw', '   durf_raster_interp')
    variants = {'A: render_trajectory': volumetric, 'B: raster.render_mesh': rendered}
    variants.update(zip(stage_names, (setup, draw, interp)))
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
    r = state['r']
    tally = dict(zip(raster.COUNT_FIELDS, (int(x) for x in r['counts'].sum(0))))
    e = raster.depth_error(r['depth'], state['frames']['distance'].reshape(F, H, W), state['frames']['acc'].reshape(F, H, W))
    L = ['a mesh through %d cameras of %d x %d, %s' % (F, H, W, torch.cuda.get_device_name(dev)),
         'the surface of the synthetic scene\'s %d^3 grid at its median density: %d vertices, %d triangles; %d frames per call' % (n1, V, T, per),
         'counts over all frames: %s' % ', '.join('%s %d' % kv for kv in tally.items()),
         'covered pixels: %d of %d; against the volumetric distance where acc >= 0.5: %d pixels, mean |d| %s, median |d| %s'
         % (int(r['mask'].sum()), F * H * W, e['both'], e['abs_mean'], e['abs_median']),
         'ms per call: median over %d blocks of the median of %d calls each; [min .. max] of the block medians' % (args.blocks, args.repeats), '']
    for k in variants:
        nf = per if k in stage_names else F
        L.append('  %-28s %10.3f   [%.3f .. %.3f]   %8.3f ms per frame over %d frames' % (k, med[k], min(blocks[k]), max(blocks[k]), med[k] / nf, nf))
    a, b = med['A: render_trajectory'], med['B: raster.render_mesh']
    L.append('  B / A = %.4f (B includes its read-back of the counts and its allocations; A renders rgb8, distance and acc)' % (b / a))
    L.append('  the three stages are one call of B: its first %d frames, %d (tile, pair) entries' % (per, state['n_pairs']))
    L.append('time only: an untrained field meshed at its median density, the camera inside it -- the depth difference above says')
    L.append('nothing about how well a mesh\'s depth and the volumetric distance agree on a real surface')
    text = '\n'.join(L)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, 'w').write(text + '\n')


if __name__ == '__main__':
    main()
