"""A shaded picture of a triangle mesh, on the device (include/durf_shade.h, csrc/shade.hip, libdurf_shade.so): flat normals that
face the viewer, a sun shadow and ambient occlusion from short any-hit rays at the primary hits -- the picture in which floaters,
holes, the staircase of a coarse lattice and a vehicle that hovers above the street show, where a depth ramp hides them.

    b = cast.build(m)                                              # the tree the secondary rays walk
    r = cameras(b, cams, dirs=64, reach=0.3)                       # tri, depth, mask, normal, ao, shaded, shaded8
    p, n = surface(b, tri, bary, toward=directions)                # any primary hits: the rasteriser's, the cast's, closest's
    used, blocked = occlusion(b, p, n, directions(64), reach=0.3)
    rgb, rgb8 = compose(tri, n, used, blocked, light=(0, 1, 0))

Every output is defined in the header with no reference to a tree, in integers or written-out fp32: tests/shade_ref.py holds the
device to every bit.  The set of directions is fixed in world space, so a picture has no noise and two runs write the same bytes."""
import math

import numpy as np

from . import trimesh

MAX_DIRS = 256                         # DURF_SHADE_MAX_DIRS (tests/test_shade_host.py holds the two together)
LIGHT = (0.35, 0.85, 0.4)              # the default sun: from above, a little to the side


def directions(S, seed=0):
    """S unit vectors [S,3] float32 spread evenly over the sphere: a Fibonacci sphere computed in float64 and rounded once.
    seed turns the spiral about its axis by the golden angle times seed: another fixed set."""
    if not isinstance(S, (int, np.integer)) or isinstance(S, bool) or not 1 <= S <= MAX_DIRS:
        raise ValueError('shade.directions: S = %r, expected a count in 1 .. %d' % (S, MAX_DIRS))
    if not isinstance(seed, (int, np.integer)) or isinstance(seed, bool):
        raise ValueError('shade.directions: seed = %r, expected a whole number' % (seed,))
    k = np.arange(S, dtype=np.float64)
    z = 1.0 - (2.0 * k + 1.0) / S
    rho = np.sqrt(np.maximum(1.0 - z * z, 0.0))
    phi = (k + float(seed)) * (math.pi * (3.0 - math.sqrt(5.0)))
    d = np.stack([rho * np.cos(phi), rho * np.sin(phi), z], 1)
    return (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)


def _three(entry, name, x):
    try:
        a = np.asarray(x, np.float64).reshape(-1)
    except (TypeError, ValueError):
        a = np.zeros(0)
    if a.size != 3 or not np.isfinite(a).all():
        raise ValueError('%s: %s = %r, expected three finite numbers' % (entry, name, x))
    return [float(v) for v in a]


def _check_rays(entry, reach, bias, cull):
    """-> (reach, bias) as floats; bias defaults to reach / 1024 and must be given with an infinite reach"""
    if isinstance(reach, bool) or not isinstance(reach, (int, float, np.floating, np.integer)) or not reach > 0:
        raise ValueError('%s: reach = %r, expected +inf or a number > 0' % (entry, reach))
    if bias is None:
        if math.isinf(reach):
            raise ValueError('%s: bias must be given when reach is infinite' % entry)
        bias = float(reach) / 1024.0
    if isinstance(bias, bool) or not isinstance(bias, (int, float, np.floating, np.integer)) or not bias >= 0:
        raise ValueError('%s: bias = %r, expected a number >= 0' % (entry, bias))
    if cull not in (0, 1, 2):
        raise ValueError('%s: cull = %r, expected 0 (both faces), 1 (drop back faces) or 2 (drop front faces)' % (entry, cull))
    return float(reach), float(bias)


def _check_look(entry, light, ambient, background):
    if isinstance(ambient, bool) or not isinstance(ambient, (int, float, np.floating, np.integer)) or not 0 <= ambient <= 1:
        raise ValueError('%s: ambient = %r, expected a number in [0, 1]' % (entry, ambient))
    return _three(entry, 'light', light), float(ambient), _three(entry, 'background', background)


def _check_dirs(entry, dirs):
    """a count (the Fibonacci set) or an array [S,3] -> float32 [S,3] on the host, or the tensor as it is"""
    if isinstance(dirs, (int, np.integer)) and not isinstance(dirs, bool):
        if not 1 <= dirs <= MAX_DIRS:
            raise ValueError('%s: dirs = %d, expected a count in 1 .. %d or an array [S,3]' % (entry, dirs, MAX_DIRS))
        return directions(int(dirs))
    shape = tuple(getattr(dirs, 'shape', ()))
    if len(shape) != 2 or shape[1] != 3 or not 1 <= shape[0] <= MAX_DIRS:
        raise ValueError('%s: dirs of shape %s, expected [S,3] with S in 1 .. %d' % (entry, shape, MAX_DIRS))
    return dirs


def _tree(entry, b):
    if not isinstance(b, dict) or any(b.get(k) is None for k in ('ws', 'T', 'V', 'vertices', 'triangles')):
        raise ValueError("%s: b is cast.build's dict (vertices, triangles, V, T, ws)" % entry)
    return b


def surface(b, tri, bary, toward=None):
    """The primary hits (tri [...] int32, bary [...,3] = (w, u, v): the cast's, the rasteriser's or closest's) on cast.build's b
    -> (point [...,3], normal [...,3]); toward [...,3]: the rays' directions, the normal then faces their origin.  Zero where
    nothing was hit; a zero normal on a triangle without area."""
    entry = 'shade.surface'
    _tree(entry, b)
    lead = tuple(getattr(tri, 'shape', ()))
    if tuple(getattr(bary, 'shape', ())) != lead + (3,) or (toward is not None and tuple(getattr(toward, 'shape', ())) != lead + (3,)):
        raise ValueError('%s: tri of shape %s, bary of shape %s and toward of shape %s, expected [...], [...,3] and [...,3]' % (
            entry, lead, tuple(getattr(bary, 'shape', ())), None if toward is None else tuple(getattr(toward, 'shape', ()))))
    import torch
    from . import ops
    dev = b['ws'].device
    return ops.shade_surface(b['vertices'], b['triangles'], trimesh.upload(tri, torch.int32, dev), trimesh.upload(bary, torch.float32, dev),
                             None if toward is None else trimesh.upload(toward, torch.float32, dev))


def occlusion(b, points, normals, dirs, reach, bias=None, cull=0):
    """points, normals [...,3] against cast.build's b -> (used, blocked) int32 [...]: of the directions dirs ([S,3], or a count for
    directions(count)) that leave the surface, how many there are and how many meet a triangle within `reach` (+inf: anywhere)
    of the point lifted by bias (default reach / 1024) along its normal"""
    entry = 'shade.occlusion'
    _tree(entry, b)
    reach, bias = _check_rays(entry, reach, bias, cull)
    dirs = _check_dirs(entry, dirs)
    ps, ns = tuple(getattr(points, 'shape', ())), tuple(getattr(normals, 'shape', ()))
    if len(ps) < 1 or ps[-1] != 3 or ps != ns:
        raise ValueError('%s: points of shape %s and normals of shape %s, expected the same [..., 3]' % (entry, ps, ns))
    import torch
    from . import ops
    dev = b['ws'].device
    return ops.shade_occlusion(b['ws'], b['T'], trimesh.upload(points, torch.float32, dev), trimesh.upload(normals, torch.float32, dev), trimesh.upload(dirs, torch.float32, dev),
                               bias, reach, cull)


def compose(tri, normals, used, blocked, light=LIGHT, ambient=0.5, background=(1.0, 1.0, 1.0), sun_blocked=None, albedo=None):
    """-> (shaded [...,3] float, shaded8 [...,3] uint8): ambient * ao + (1 - ambient) * lambert * sun, times albedo [...,3] where
    given, the background where tri < 0.  light is used as given (normalise it for a Lambert term in [0, 1]); normals may be
    the caller's own interpolated ones; sun_blocked [...] int32: the `blocked` of an occlusion along the light."""
    entry = 'shade.compose'
    light, ambient, background = _check_look(entry, light, ambient, background)
    lead = tuple(getattr(tri, 'shape', ()))
    shapes = dict(normals=(normals, lead + (3,)), used=(used, lead), blocked=(blocked, lead))
    if sun_blocked is not None:
        shapes['sun_blocked'] = (sun_blocked, lead)
    if albedo is not None:
        shapes['albedo'] = (albedo, lead + (3,))
    for name, (a, want) in shapes.items():
        if tuple(getattr(a, 'shape', ())) != want:
            raise ValueError('%s: %s of shape %s for tri of shape %s' % (entry, name, tuple(getattr(a, 'shape', ())), lead))
    import torch
    from . import ops
    dev = trimesh.device_of(tri)
    i32 = lambda a: None if a is None else trimesh.upload(a, torch.int32, dev)
    f32 = lambda a: None if a is None else trimesh.upload(a, torch.float32, dev)
    return ops.shade_compose(i32(tri), f32(normals), i32(used), i32(blocked), light, ambient, background, i32(sun_blocked), f32(albedo))


def default_reach(vertices):
    """2 % of the bounding diagonal of the finite vertices (host arrays or tensors; one read-back of six floats) -> float"""
    import torch
    v = torch.as_tensor(vertices).reshape(-1, 3).to(torch.float64)
    v = v[torch.isfinite(v).all(1)]
    if v.shape[0] == 0:
        return 1.0
    diag = float((v.max(0)[0] - v.min(0)[0]).norm())
    return 0.02 * diag if diag > 0 else 1.0


def ao_plane(used, blocked):
    """the two counts -> ao [...] float: the share of the used directions that are free, 1 where none was used"""
    import torch
    return torch.where(used > 0, (used - blocked).to(torch.float32) / used.clamp(min=1).to(torch.float32), torch.ones((), device=used.device))


def cameras(b, cams, dirs=64, reach=None, bias=None, light=LIGHT, sun=True, ambient=0.5, albedo='rgb', background=(1.0, 1.0, 1.0),
            tmin=0.0, tmax=float('inf'), cull=0):
    """cast.build's b through the cameras cams [F,CAM_FLOATS] of one frame size, shaded, in one call of durf_shade_cameras -> dict
    tri [F,h,w] int32, depth [F,h,w], mask, normal [F,h,w,3] (facing the camera), ao_used, ao_blocked [F,h,w] int32, ao [F,h,w]
    float, shaded [F,h,w,3] float, shaded8 [F,h,w,3] uint8.  dirs: a count (directions(count)) or [S,3]; reach: how far an
    occluder counts (default: 2 % of the mesh's bounding diagonal, one small read-back); light: towards the sun, normalised
    here; sun: cast its shadow; albedo: the key of a per-vertex colour of b ([V,3]; uint8 as [0, 1]), or None for white."""
    from . import camera, cast
    entry = 'shade.cameras'
    _tree(entry, b)
    cams, h, w = camera.as_rows(cams, entry)
    if not np.isfinite(cams).all():
        raise ValueError('%s: a camera row that is not finite' % entry)
    cast._check_bounds(entry, tmin, tmax, cull)
    dirs = _check_dirs(entry, dirs)
    light, ambient, background = _check_look(entry, light, ambient, background)
    norm = math.sqrt(sum(x * x for x in light))
    if not norm > 0:
        raise ValueError('%s: light = %r, expected a direction' % (entry, light))
    light = [x / norm for x in light]
    if albedo is not None and not isinstance(albedo, str):
        raise ValueError('%s: albedo = %r, expected the key of a per-vertex colour of the mesh or None' % (entry, albedo))
    if cams.shape[0] * h * w >= 2 ** 31:
        raise ValueError('%s: %d frames of %d x %d: frames x pixels must stay below 2^31' % (entry, cams.shape[0], h, w))
    if reach is None:
        reach = default_reach(b['vertices'])
    reach, bias = _check_rays(entry, reach, bias, cull)
    import torch
    from . import ops
    dev = b['ws'].device
    a = trimesh.vertex_attributes(b, (albedo,), None, b['V'], dev)[0].get(albedo) if albedo is not None else None
    if a is not None:
        if a.shape[1] != 3:
            raise ValueError('%s: albedo %r of shape %s, expected [V,3]' % (entry, albedo, tuple(a.shape)))
    r = ops.shade_cameras(b['ws'], b['vertices'], b['triangles'], torch.as_tensor(cams).to(dev).contiguous(), h, w, trimesh.upload(dirs, torch.float32, dev),
                          bias, reach, light, bool(sun), ambient, background, albedo_vertex=a, tmin=tmin, tmax=tmax, cull=cull)
    return dict(tri=r['tri'], depth=r['depth'], mask=r['tri'] >= 0, normal=r['normal'], ao_used=r['ao_used'], ao_blocked=r['ao_blocked'],
                ao=ao_plane(r['ao_used'], r['ao_blocked']), shaded=r['out_f'], shaded8=r['out_u8'], reach=reach, bias=bias, light=light)


def primaries(b, tri, bary, toward, dirs=64, reach=None, bias=None, light=LIGHT, sun=True, ambient=0.5, albedo='rgb',
              background=(1.0, 1.0, 1.0), cull=0):
    """cameras()'s dict for primary hits found elsewhere -- the rasteriser's tri [...] and bary [...,3] with the pixels' ray
    directions toward [...,3] -- through the three separate entries: durf_shade_surface, durf_shade_occlusion for dirs and, with
    sun, for the light, durf_raster_interp for the albedo, durf_shade_compose."""
    from . import cast
    entry = 'shade.primaries'
    _tree(entry, b)
    dirs = _check_dirs(entry, dirs)
    light, ambient, background = _check_look(entry, light, ambient, background)
    norm = math.sqrt(sum(x * x for x in light))
    if not norm > 0:
        raise ValueError('%s: light = %r, expected a direction' % (entry, light))
    light = [x / norm for x in light]
    if reach is None:
        reach = default_reach(b['vertices'])
    reach, bias = _check_rays(entry, reach, bias, cull)
    point, normal = surface(b, tri, bary, toward)
    used, blocked = occlusion(b, point, normal, dirs, reach, bias, cull)
    sun_blocked = occlusion(b, point, normal, np.asarray([light], np.float32), float('inf'), bias, cull)[1] if sun else None
    tri = tri.to(point.device)
    a = cast.attributes_at(b, tri, bary.to(point.device), (albedo,), None, {}).get(albedo) if albedo is not None else None
    shaded, shaded8 = compose(tri, normal, used, blocked, light, ambient, background, sun_blocked, a)
    return dict(tri=tri, mask=tri >= 0, normal=normal, ao_used=used, ao_blocked=blocked, ao=ao_plane(used, blocked), shaded=shaded, shaded8=shaded8,
                reach=reach, bias=bias, light=light)


def add_arguments(ap):
    """--shade and what goes with it, for the commands that write pictures of a mesh (cast_mesh, render_mesh)"""
    ap.add_argument('--shade', action='store_true', help='also write shade_%%04d.ppm, ao_%%04d.ppm and normals_%%04d.ppm per frame')
    ap.add_argument('--ao_dirs', type=int, default=64, help='--shade: directions of the ambient occlusion (1 .. %d)' % MAX_DIRS)
    ap.add_argument('--ao_reach', type=float, default=None, help='--shade: how far an occluder counts (default: 2 %% of the bounding diagonal)')
    ap.add_argument('--light', type=float, nargs=3, default=LIGHT, metavar=('X', 'Y', 'Z'), help='--shade: the direction towards the sun')
    ap.add_argument('--ambient', type=float, default=0.5, help='--shade: the share of the ambient term, in [0, 1]')
    ap.add_argument('--no_sun', action='store_true', help='--shade: no sun shadow')


def check_arguments(args):
    """the refusals of --shade's arguments -> the message, or None"""
    if not 1 <= args.ao_dirs <= MAX_DIRS:
        return '--ao_dirs %d' % args.ao_dirs
    if args.ao_reach is not None and not (args.ao_reach > 0 and math.isfinite(args.ao_reach)):
        return '--ao_reach %g' % args.ao_reach
    if not 0 <= args.ambient <= 1:
        return '--ambient %g' % args.ambient
    if not all(math.isfinite(x) for x in args.light) or not any(args.light):
        return '--light %g %g %g' % tuple(args.light)
    return None


def arguments(args, vertices):
    """-> the keywords of cameras() / primaries() the command line asks for; the reach from the mesh where none is given"""
    reach = args.ao_reach if args.ao_reach is not None else default_reach(vertices)
    return dict(dirs=args.ao_dirs, reach=reach, light=tuple(args.light), sun=not args.no_sun, ambient=args.ambient)


def meta(args, r):
    """what the command's json gains"""
    return dict(ao_dirs=args.ao_dirs, ao_reach=float(r['reach']), bias=float(r['bias']), light=[float(x) for x in r['light']])


def to_u8(x):
    """rgb8's rule (csrc/durf_common.h) in torch: round-half-even of clamp(x, 0, 1) * 255, 0 for a NaN -> uint8"""
    import torch
    return torch.round(torch.nan_to_num(x, nan=0.0).clamp(0.0, 1.0) * 255.0).to(torch.uint8)


def write_pictures(eval_dir, f, r, k=None):
    """shade_%04d.ppm, ao_%04d.ppm and normals_%04d.ppm of frame f from cameras()'s r (frame k of r, default f)"""
    import os
    from . import trajectory
    k = f if k is None else k
    trajectory.write_ppm(os.path.join(eval_dir, 'shade_%04d.ppm' % f), r['shaded8'][k])
    trajectory.write_ppm(os.path.join(eval_dir, 'ao_%04d.ppm' % f), to_u8(r['ao'][k])[..., None].expand(-1, -1, 3).contiguous())
    trajectory.write_ppm(os.path.join(eval_dir, 'normals_%04d.ppm' % f), to_u8((r['normal'][k] + 1.0) / 2.0))
