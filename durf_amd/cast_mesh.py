"""Cast rays at triangle meshes -- pinhole pictures without a near plane, or LIDAR sweeps of the surface; no network involved:

    python -m durf_amd.cast_mesh --ply OUT/background.ply [--ply OUT/object_00.ply ...] [--poses OUT/poses.npy --ts T]
                                 --traj traj.npz --focal F --size H W [--pp X Y] --eval_dir OUT2 [--cull none|back|front] [--ids ...]
    python -m durf_amd.cast_mesh --ply ... --sweeps sensor_poses.npy [--beams 64 --columns 2650 --incl -17.6 2.4] [--near 0.1 --far 75]
                                 --eval_dir OUT2
    python -m durf_amd.cast_mesh --synthetic --eval_dir OUT2 [--frames 8]

The meshes, --poses / --ts, --traj, --focal, --size, --pp, --cull and --ids are durf_amd.render_mesh's, and so are the files of
a camera run: OUT2/depth_%04d.npy, depth_%04d.ppm, ids_%04d.ppm per frame -- cast along the pixel's ray (durf_amd.cast.cameras),
so a camera that stands on or inside the mesh loses nothing to a near plane.  --shade [--ao_dirs 64 --ao_reach R --light X Y Z
--ambient 0.5 --no_sun] adds shade_%04d.ppm (the mesh's colours under a sun with its shadow and ambient occlusion:
durf_amd.shade.cameras), ao_%04d.ppm and normals_%04d.ppm per frame, and ao_dirs, ao_reach, bias and light to cast.json; R
defaults to 2 % of the merged mesh's bounding diagonal.  --sweeps: sensor-to-world poses [F,3,4] (npy), one
standing sweep each, of a sensor with --beams uniform inclinations over --incl degrees and --columns azimuth columns; written
per sweep as durf_amd.render_lidar names them: range_%04d.npy ([H,W] float32, 0 where nothing is hit) and sweep_%04d.ply.  Either
way OUT2/cast.json holds the counts of rays, hits and unusable rays per frame or sweep.  --synthetic casts at
render_mesh's synthetic sphere both ways, no data needed: the --frames cameras of its orbit, and one sweep of a 16 x 180 sensor
(inclinations -40 .. 40 degrees; --beams, --columns and --incl are not read) standing at its centre."""
import argparse
import json
import math
import os
import sys

from .render_mesh import CULL


def build_parser():
    ap = argparse.ArgumentParser(prog='python -m durf_amd.cast_mesh', description=__doc__.split('\n\n')[0])
    ap.add_argument('--ply', action='append', default=[], help='a mesh file (repeatable; merged)')
    ap.add_argument('--poses', default=None, help='poses.npy [T,K,6]: file 1 + k is box k in its own frame')
    ap.add_argument('--ts', type=int, default=0, help='--poses: the timestep whose poses hold')
    ap.add_argument('--traj', default=None, help='trajectory npz: {c2w, times} or the notebook\'s (c2w, ts) pairs')
    ap.add_argument('--focal', type=float, default=None, help='focal length in pixels')
    ap.add_argument('--size', type=int, nargs=2, default=None, metavar=('H', 'W'), help='frame size')
    ap.add_argument('--pp', type=float, nargs=2, default=None, metavar=('X', 'Y'), help='principal point (default: the centre)')
    ap.add_argument('--sweeps', default=None, help='sensor poses [F,3,4] (npy): LIDAR sweeps instead of cameras')
    ap.add_argument('--beams', type=int, default=64, help='--sweeps: beams H')
    ap.add_argument('--columns', type=int, default=2650, help='--sweeps: azimuth columns W')
    ap.add_argument('--incl', type=float, nargs=2, default=(-17.6, 2.4), metavar=('LO', 'HI'), help='--sweeps: inclinations in degrees')
    ap.add_argument('--near', type=float, default=0.1, help='--sweeps: the nearest return')
    ap.add_argument('--far', type=float, default=75.0, help='--sweeps: the farthest return')
    ap.add_argument('--eval_dir', required=True, help='where the files go')
    ap.add_argument('--cull', choices=sorted(CULL), default='none', help='cameras: faces to drop')
    ap.add_argument('--ids', choices=('component', 'part', 'tri'), default=None, help='cameras: what ids_%%04d.ppm shows')
    ap.add_argument('--synthetic', action='store_true', help='cast at a synthetic sphere: an orbit of cameras and one sweep from its centre (no data needed)')
    ap.add_argument('--frames', type=int, default=8, help='--synthetic: cameras of the orbit')
    from . import shade
    shade.add_arguments(ap)
    return ap


def check_args(args):
    """the refusals of the command line, before anything is read -> the message, or None"""
    if args.beams < 1 or args.columns < 1 or not args.incl[0] <= args.incl[1]:
        return '--beams %d --columns %d --incl %g %g' % (args.beams, args.columns, args.incl[0], args.incl[1])
    if not 0 <= args.near <= args.far:
        return '--near %g --far %g' % (args.near, args.far)
    if args.shade:
        from . import shade
        why = shade.check_arguments(args)
        if why:
            return why
        if not args.synthetic and args.sweeps is not None:
            return '--shade shades the pictures of cameras (--traj), not --sweeps'
    if args.synthetic:
        return None if args.frames >= 1 else '--frames %d' % args.frames
    if not args.ply:
        return '--ply is required (or --synthetic)'
    if (args.sweeps is None) == (args.traj is None):
        return 'one of --traj (cameras) and --sweeps (LIDAR) is required (or --synthetic)'
    if args.traj is not None:
        if args.focal is None or args.size is None:
            return '--traj needs --focal and --size'
        if not args.focal > 0 or min(args.size) < 1:
            return '--focal %g --size %d %d' % (args.focal, args.size[0], args.size[1])
    if args.poses is None and args.ts != 0:
        return '--ts needs --poses'
    return None


def _counts(tri):
    n = tri.reshape(tri.shape[0], -1)
    return [dict(rays=int(n.shape[1]), hits=int(h), unusable=int(u)) for h, u in zip((n >= 0).sum(1).cpu().numpy(), (n == -2).sum(1).cpu().numpy())]


def main(argv=None):
    args = build_parser().parse_args(argv)
    why = check_args(args)
    if why:
        raise SystemExit('cast_mesh: %s' % why)
    import numpy as np
    from . import cast, lidar, mesh, raster, render_mesh, trajectory
    sweeps = cams = None
    beams, columns, incl = args.beams, args.columns, args.incl
    if args.synthetic:
        m, c2w, focal, h, w = render_mesh.synthetic_scene(args.frames)
        names = ['synthetic sphere']
        sweeps = np.concatenate([np.eye(3), np.zeros((3, 1))], 1)[None]
        beams, columns, incl = 16, 180, (-40.0, 40.0)
    else:
        meshes = [mesh.read_ply(p) for p in args.ply]
        poses = None
        if args.poses is not None:
            table = np.load(args.poses)
            if table.ndim != 3 or table.shape[2] < 6 or not 0 <= args.ts < table.shape[0] or table.shape[1] < len(meshes) - 1:
                raise SystemExit('cast_mesh: --poses of shape %s for %d object files at --ts %d' % (table.shape, len(meshes) - 1, args.ts))
            poses = [None] + [table[args.ts, k, :6] for k in range(len(meshes) - 1)]
        m = raster.merge(meshes, poses)
        names = list(args.ply)
        if args.sweeps is not None:
            sweeps = np.load(args.sweeps)
            if sweeps.ndim < 2 or sweeps.shape[-2:] != (3, 4):
                raise SystemExit('cast_mesh: --sweeps of shape %s, expected [F,3,4]' % (sweeps.shape,))
            sweeps = sweeps.reshape(-1, 3, 4)
        else:
            c2w, _ = trajectory.load_trajectory(args.traj)
            focal, (h, w) = args.focal, args.size
    b = cast.build(m)
    os.makedirs(args.eval_dir, exist_ok=True)
    meta = dict(meshes=names, vertices=b['V'], triangles=b['T'])
    done = []
    if sweeps is not None:
        sensor = lidar.LidarSensor.uniform(beams, math.radians(incl[0]), math.radians(incl[1]), columns, max_range=args.far)
        s = cast.lidar(b, sensor, sweeps, near=args.near, far=args.far)
        for f in range(sweeps.shape[0]):
            np.save(os.path.join(args.eval_dir, 'range_%04d.npy' % f), s['range'][f].cpu().numpy().astype(np.float32))
            lidar.write_ply(os.path.join(args.eval_dir, 'sweep_%04d.ply' % f), *cast.point_cloud(s, f))
        meta.update(beams=sensor.height, columns=sensor.width, near=args.near, far=args.far, sweeps=_counts(s['tri']))
        done.append('%d sweeps of %d x %d' % (sweeps.shape[0], sensor.height, sensor.width))
    if args.synthetic or sweeps is None:
        pp = args.pp if args.pp is not None else ((w - 1) / 2.0, (h - 1) / 2.0)
        cams = trajectory.camera_rows(c2w, focal, pp, h, w)
        ids = args.ids or ('part' if m.get('part') is not None and len(names) > 1 else 'component' if m.get('component') is not None else 'tri')
        if ids != 'tri' and m.get(ids) is None:
            raise SystemExit('cast_mesh: --ids %s, but the mesh has no per-vertex %s' % (ids, ids))
        r = cast.cameras(b, cams, attrs=(), label=None if ids == 'tri' else ids, cull=CULL[args.cull])
        picture = r['tri'] if ids == 'tri' else r[ids]
        for f in range(cams.shape[0]):
            raster.write_depth(os.path.join(args.eval_dir, 'depth_%04d' % f), r['depth'][f], r['mask'][f])
            raster.write_ids(os.path.join(args.eval_dir, 'ids_%04d.ppm' % f), picture[f])
        meta.update(h=int(h), w=int(w), focal=float(focal), principal_point=[float(pp[0]), float(pp[1])], cull=args.cull, ids=ids,
                    frames=_counts(r['tri']))
        if args.shade:
            from . import shade
            s = shade.cameras(b, cams, cull=CULL[args.cull], **shade.arguments(args, m['vertices']))
            for f in range(cams.shape[0]):
                shade.write_pictures(args.eval_dir, f, s)
            meta.update(shade.meta(args, s))
        done.append('%d frames of %d x %d' % (cams.shape[0], h, w))
    with open(os.path.join(args.eval_dir, 'cast.json'), 'w') as fjson:
        json.dump(meta, fjson, indent=1)
    print('cast_mesh: %s, %d triangles; written to %s' % (' and '.join(done), b['T'], args.eval_dir))
    return 0


if __name__ == '__main__':
    sys.exit(main())
