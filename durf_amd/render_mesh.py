"""Render triangle meshes through the cameras of a trajectory -- depth and id pictures, no network involved:

    python -m durf_amd.render_mesh --ply OUT/background.ply [--ply OUT/object_00.ply ...] [--poses OUT/poses.npy --ts T]
                                   --traj traj.npz --focal F --size H W [--pp X Y] --eval_dir OUT2
                                   [--znear 0.01] [--cull none|back|front] [--ids component|part|tri]
    python -m durf_amd.render_mesh --synthetic --eval_dir OUT2 [--frames 8]

--ply: what durf_amd.extract_mesh wrote (durf_amd.mesh.read_ply); several are merged (durf_amd.raster.merge).  With --poses
(extract_mesh's poses.npy, [T,K,6]) the first file is taken as the world-frame background and file 1 + k as box k in its own
frame, placed at its pose of timestep --ts.  --traj: the {c2w, times} npz (or the notebook's pairs) render_traj takes; the
intrinsics come from --focal, --size and --pp (default: the frame's centre).  Written per frame f: OUT2/depth_%04d.npy (camera
depth, float32, 0 where no triangle covers), depth_%04d.ppm, ids_%04d.ppm (--ids: the PLY's per-vertex component, the file a
vertex came from -- the default with several files -- or the triangle id) and OUT2/raster.json (the counts per frame: pairs,
drawn, invalid, behind, crossing, range, degenerate, culled).  A triangle crossing the near plane is dropped, not clipped.
--shade [--ao_dirs 64 --ao_reach R --light X Y Z --ambient 0.5 --no_sun] adds shade_%04d.ppm, ao_%04d.ppm and normals_%04d.ppm
per frame and ao_dirs, ao_reach, bias and light to raster.json: the rasteriser's hits, shaded by any-hit rays through a cast tree
of the same mesh (durf_amd.shade.primaries; R defaults to 2 % of the merged mesh's bounding diagonal).
--synthetic renders a sphere's iso-surface (durf_amd.mesh.surface of an analytic density lattice) from an orbit of --frames
cameras instead: no data, no checkpoint, the command end to end."""
import argparse
import json
import os
import sys

CULL = dict(none=0, back=1, front=2)


def build_parser():
    ap = argparse.ArgumentParser(prog='python -m durf_amd.render_mesh', description=__doc__.split('\n\n')[0])
    ap.add_argument('--ply', action='append', default=[], help='a mesh file (repeatable; merged)')
    ap.add_argument('--poses', default=None, help='poses.npy [T,K,6]: file 1 + k is box k in its own frame')
    ap.add_argument('--ts', type=int, default=0, help='--poses: the timestep whose poses hold')
    ap.add_argument('--traj', default=None, help='trajectory npz: {c2w, times} or the notebook\'s (c2w, ts) pairs')
    ap.add_argument('--focal', type=float, default=None, help='focal length in pixels')
    ap.add_argument('--size', type=int, nargs=2, default=None, metavar=('H', 'W'), help='frame size')
    ap.add_argument('--pp', type=float, nargs=2, default=None, metavar=('X', 'Y'), help='principal point (default: the centre)')
    ap.add_argument('--eval_dir', required=True, help='where the pictures go')
    ap.add_argument('--znear', type=float, default=1e-2, help='near plane: a triangle with a vertex nearer is dropped')
    ap.add_argument('--cull', choices=sorted(CULL), default='none', help='faces to drop')
    ap.add_argument('--ids', choices=('component', 'part', 'tri'), default=None, help='what ids_%%04d.ppm shows')
    ap.add_argument('--synthetic', action='store_true', help='render a synthetic sphere from an orbit (no data needed)')
    ap.add_argument('--frames', type=int, default=8, help='--synthetic: cameras of the orbit')
    from . import shade
    shade.add_arguments(ap)
    return ap


def check_args(args):
    """the refusals of the command line, before anything is read -> the message, or None"""
    if args.shade:
        from . import shade
        why = shade.check_arguments(args)
        if why:
            return why
    if args.synthetic:
        return None if args.frames >= 1 else '--frames %d' % args.frames
    if not args.ply:
        return '--ply is required (or --synthetic)'
    if args.traj is None or args.focal is None or args.size is None:
        return '--traj, --focal and --size are required (or --synthetic)'
    if not args.focal > 0 or min(args.size) < 1:
        return '--focal %g --size %d %d' % (args.focal, args.size[0], args.size[1])
    if not args.znear > 0:
        return '--znear %g' % args.znear
    if args.poses is None and args.ts != 0:
        return '--ts needs --poses'
    return None


def synthetic_scene(frames, cells=32, size=(48, 64), focal=56.0):
    """a sphere of radius 1 as the iso-surface of a distance lattice, and an orbit around it -> (mesh, c2w [F,3,4], focal, h, w)"""
    import numpy as np
    import torch
    from . import mesh
    dev = torch.device('cuda', torch.cuda.current_device())
    step = 3.0 / (cells - 1)
    ax = torch.arange(cells, device=dev, dtype=torch.float32) * step - 1.5
    r = torch.sqrt(ax[:, None, None] ** 2 + ax[None, :, None] ** 2 + ax[None, None, :] ** 2)
    frame = dict(origin=[-1.5, -1.5, -1.5], du=[step, 0.0, 0.0], dv=[0.0, step, 0.0], dw=[0.0, 0.0, step])
    m = mesh.surface(dict(density=(1.0 - r).contiguous(), valid=None, frame=frame), 0.0)
    m['rgb'] = (0.5 + 0.5 * m['normals']).contiguous()
    c2w = np.zeros((frames, 3, 4))
    for f in range(frames):
        a = 2.0 * np.pi * f / frames
        eye = np.array([4.0 * np.sin(a), 1.0, 4.0 * np.cos(a)])
        zc = eye / np.linalg.norm(eye)
        xc = np.cross([0.0, 1.0, 0.0], zc)
        xc /= np.linalg.norm(xc)
        c2w[f] = np.concatenate([np.stack([xc, np.cross(zc, xc), zc], 1), eye[:, None]], 1)
    return m, c2w, focal, size[0], size[1]


def main(argv=None):
    args = build_parser().parse_args(argv)
    why = check_args(args)
    if why:
        raise SystemExit('render_mesh: %s' % why)
    import numpy as np
    from . import mesh, raster, trajectory
    if args.synthetic:
        m, c2w, focal, h, w = synthetic_scene(args.frames)
        names = ['synthetic sphere']
    else:
        meshes = [mesh.read_ply(p) for p in args.ply]
        poses = None
        if args.poses is not None:
            table = np.load(args.poses)
            if table.ndim != 3 or table.shape[2] < 6 or not 0 <= args.ts < table.shape[0] or table.shape[1] < len(meshes) - 1:
                raise SystemExit('render_mesh: --poses of shape %s for %d object files at --ts %d' % (table.shape, len(meshes) - 1, args.ts))
            poses = [None] + [table[args.ts, k, :6] for k in range(len(meshes) - 1)]
        m = raster.merge(meshes, poses)
        c2w, _ = trajectory.load_trajectory(args.traj)
        focal, (h, w), names = args.focal, args.size, list(args.ply)
    pp = args.pp if args.pp is not None else ((w - 1) / 2.0, (h - 1) / 2.0)
    cams = trajectory.camera_rows(c2w, focal, pp, h, w)
    ids = args.ids or ('part' if m.get('part') is not None and len(names) > 1 else 'component' if m.get('component') is not None else 'tri')
    if ids != 'tri' and m.get(ids) is None:
        raise SystemExit('render_mesh: --ids %s, but the mesh has no per-vertex %s' % (ids, ids))
    r = raster.render_mesh(m, cams, znear=args.znear, attrs=(), label=None if ids == 'tri' else ids, cull=CULL[args.cull], frames_per_call=1)
    os.makedirs(args.eval_dir, exist_ok=True)
    picture = r['tri'] if ids == 'tri' else r[ids]
    for f in range(cams.shape[0]):
        raster.write_depth(os.path.join(args.eval_dir, 'depth_%04d' % f), r['depth'][f], r['mask'][f])
        raster.write_ids(os.path.join(args.eval_dir, 'ids_%04d.ppm' % f), picture[f])
    covered = r['mask'].reshape(cams.shape[0], -1).sum(1).cpu().numpy()
    meta = dict(meshes=names, vertices=int(m['vertices'].shape[0]), triangles=int(m['triangles'].shape[0]), h=int(h), w=int(w), focal=float(focal),
                principal_point=[float(pp[0]), float(pp[1])], znear=args.znear, cull=args.cull, ids=ids,
                frames=[dict(dict(zip(raster.COUNT_FIELDS, (int(x) for x in row))), covered=int(c)) for row, c in zip(r['counts'], covered)])
    if args.shade:
        # the rasteriser's primaries, the cast's secondaries: a tree for the any-hit rays, the surface from the rasteriser's tri / bary
        import torch
        from . import cast, raygen, shade
        b = cast.build(m)
        kw = shade.arguments(args, m['vertices'])
        for f in range(cams.shape[0]):
            toward = raygen.camera_rays(cams[f], 0.0, 1.0, device=b['ws'].device).directions.reshape(h, w, 3).contiguous()
            s = shade.primaries(b, r['tri'][f].contiguous(), r['bary'][f].contiguous(), toward, cull=CULL[args.cull], **kw)
            shade.write_pictures(args.eval_dir, f, {k: (v[None] if torch.is_tensor(v) else v) for k, v in s.items()}, 0)
        meta.update(shade.meta(args, s))
    with open(os.path.join(args.eval_dir, 'raster.json'), 'w') as fjson:
        json.dump(meta, fjson, indent=1)
    print('render_mesh: %d frames of %d x %d, %d triangles; written to %s' % (cams.shape[0], h, w, meta['triangles'], args.eval_dir))
    return 0


if __name__ == '__main__':
    sys.exit(main())
