"""The scene's surface as triangle meshes: the iso-surface of a density lattice, extracted on the device (include/durf_mesh.h,
csrc/mesh.hip, libdurf_mesh.so) -- marching tetrahedra on the Kuhn subdivision with welded vertices: closed and consistently
oriented wherever the lattice is usable, deterministic, no atomics.

    m = surface(field.grid(model, variables, origin, shape, step=0.25, ext=ext), iso=5.0)     # any dict(density=, valid=, frame=)
    m = extract(model, variables, origin, shape, step=0.25, iso=5.0, ext=ext, ts=3)           # + owner and colour per vertex
    o = extract_object(model, variables, k, ext, step=0.05, iso=5.0, ts=3)                    # box k in its own frame
    s = extract_scene(model, variables, origin, shape, step=0.25, iso=5.0, ext=ext, obj_step=0.05)
    write_ply('out/background.ply', s['background'])

The street is one network and every vehicle its own network in its own canonical frame, with its pose at every timestep a
parameter: the scene comes out as a static background mesh plus one mesh per object in the object's frame, with the poses
[T,K,6] alongside -- an asset to replay and edit.  `iso` has no default: it is the density at which the caller calls a point
solid.  A vertex next to an unusable lattice point (a cell in several boxes, a NaN) may belong to no triangle; holes there are
documented, not repaired."""
import numpy as np

from . import lattice
from .lattice import _host


def aa2matrix(rotvec):
    """the world->object matrix of a pose's rotation vector in float64 (csrc/aa2matrix.h: safe_norm's clamp, the +1e-12)"""
    r = np.asarray(rotvec, np.float64).reshape(3)
    s = max(float(r @ r), 1e-12)
    th = np.sqrt(s) + 1e-12
    S = np.array([[0.0, -r[2], r[1]], [r[2], 0.0, -r[0]], [-r[1], r[0], 0.0]])
    return np.eye(3) + (np.sin(th) / th) * S + ((1.0 - np.cos(th)) / (th * th)) * (S @ S)


def host_frame(frame, entry='mesh.surface'):
    """lattice.host under the name callers know: (origin, du, dv, dw, A, flip)"""
    return lattice.host(frame, entry)


def _iso(iso, entry):
    if iso is None or not float(iso) == float(iso):
        raise ValueError('%s: iso = %r; the library has no default (it is the density the caller calls solid)' % (entry, iso))
    return float(iso)


def surface(g, iso, normals=True, attrs=()):
    """The iso-surface of the lattice g: field.grid's dict, or any dict(density= [nu,nv,nw] float32 on the device, valid=
    uint8 or None, frame= dict(origin, du, dv, dw)).  A point is in when density >= iso.  durf_mesh_count, ONE read of the two
    counts (the pipeline's only read-back, as render_layers reads its hit count), exact allocation, durf_mesh_emit -> dict
    vertices [V,3], normals [V,3] (None with normals=False; they point from in to out), triangles [T,3] int32, vertex_edge
    [V,2] int32 (the lattice point and which of its seven edges), vertex_t [V], counts (the device tensor), frame, iso, shape.
    attrs: keys of g holding float lattice attributes [nu,nv,nw(,C)] to carry to the vertices (a + t (b - a)), returned
    under the same keys as [V,C]."""
    import torch
    from . import ops
    iso = _iso(iso, 'mesh.surface')
    d, v, shape, (o, du, dv, dw, A, flip) = lattice.device_lattice(g, 'mesh.surface', with_frame=True)
    counts, ws = ops.mesh_count(d, v, shape, iso)
    nv_, nt_ = (int(x) for x in counts.cpu())
    m = ops.mesh_emit(d, v, shape, iso, o, du, dv, dw, ws, nv_, nt_, normal_xform=A if normals else None, flip=flip)
    out = dict(m, counts=counts, frame=dict(g['frame']), iso=iso, shape=shape)
    for key in attrs:
        a = g[key].to(torch.float32).contiguous()
        out[key] = ops.mesh_gather(shape, counts, m['vertex_edge'], m['vertex_t'], attr_f=a)[0]
    return out


def _owner(m, g, iso):
    from . import ops
    d, shape = g['density'].contiguous(), m['shape']
    return ops.mesh_gather(shape, m['counts'], m['vertex_edge'], m['vertex_t'], attr_i=g['owner'].contiguous().reshape(-1), density=d,
                           valid=g['valid'].contiguous(), iso=iso)[1]


def view_of_normals(normals):
    """the direction looking straight at the surface: -n; a zero normal gets (0, 0, -1)"""
    import torch
    vd = -normals
    zero = (normals == 0).all(1, keepdim=True)
    return torch.where(zero, torch.tensor([0.0, 0.0, -1.0], device=normals.device).expand_as(vd), vd).contiguous()


def _colour(m, g, colour, model, variables, kw, entry):
    from . import field
    if colour is None:
        return None
    if colour == 'query':
        q = {k: v for k, v in kw.items() if k != 'view'}
        return field.query(model, variables, m['vertices'], view_of_normals(m['normals']), **q)['rgb']
    return m['rgb']


def _clean(m, g, iso, min_points, largest):
    """the opt-in cleaning of extract, extract_object and extract_scene (durf_amd.parts): with the defaults m as it is"""
    if not min_points and largest is None:
        return m
    from . import parts
    m, m['cleaning'] = parts.clean(m, g, iso, min_points=min_points, largest=largest)
    return m


def smoothed(m, sm):
    """the opt-in smoothing of extract, extract_object and extract_scene (durf_amd.smooth.taubin, after _clean): with smooth=0 m
    as it is.  Adds `smooth` (the arguments used) and `census` (of the mesh that was smoothed: closed? manifold?).  sm: None, or
    smooth.options' dict.  fuse_tsdf applies it to tsdf.fuse_scene's meshes."""
    if sm is None:
        return m
    from . import smooth
    adj = smooth.adjacency(m)
    out = smooth.taubin(m, adj=adj, **sm)
    out['smooth'] = dict(dict(iters=10, lam=0.5, mu=-0.53, boundary='pin'), **{k: v for k, v in sm.items() if k != 'fixed'})
    out['census'] = smooth.census(adj)
    return out


def extract(model, variables, origin, shape, step=None, axes=None, iso=None, colour='query', view=(0.0, 0.0, -1.0), min_points=0,
            largest=None, smooth=0, **kw):
    """field.grid over the lattice (its arguments: sigma, ts, alpha, pose, box_enable, chunk, inside_tol, ext), then surface
    -> surface's dict plus owner [V] int32 (the owner of each edge's in end: the box a vertex belongs to, -1 background) and
    rgb [V,3].  colour='query' (default): field.query(vertices, viewdirs=-normals), the colour seen looking straight at the
    surface; 'grid': the grid's own rgb, seen along `view`, interpolated along each edge; None: no colour.
    min_points, largest (opt-in; durf_amd.parts.keep): drop the connected solid regions of the lattice with fewer points, or all
    but the `largest` biggest, from the mesh -- a compaction: what stays keeps its bits; adds component [V] int32 and `cleaning`
    (components, kept, dropped_points, sizes).  With the defaults nothing of this runs.
    smooth (opt-in; durf_amd.smooth.taubin): a number of Taubin iterations, or a dict of taubin's arguments (iters, lam, mu,
    boundary, fixed); it runs after the cleaning, replaces vertices and normals, keeps the triangles, and adds `smooth` and
    `census`.  colour='query' then asks the colour at the smoothed vertices with the fresh normals.  With smooth=0 nothing of
    this runs."""
    from . import field, smooth as smooth_
    iso = _iso(iso, 'mesh.extract')
    sm = smooth_.options(smooth, 'mesh.extract')
    if colour not in ('query', 'grid', None):
        raise ValueError('mesh.extract: colour = %r, expected \'query\', \'grid\' or None' % (colour,))
    g = field.grid(model, variables, origin, shape, step=step, axes=axes, view=view if colour == 'grid' else None, **kw)
    m = surface(g, iso, normals=True, attrs=('rgb',) if colour == 'grid' else ())
    m['owner'] = _owner(m, g, iso)
    later = sm is not None and colour == 'query'                              # the colour is asked once, where the vertices end up
    m['rgb'] = _colour(m, g, None if later else colour, model, variables, kw, 'mesh.extract')
    m = smoothed(_clean(m, g, iso, min_points, largest), sm)
    if later:
        m['rgb'] = _colour(m, g, colour, model, variables, kw, 'mesh.extract')
    return m


def object_lattice(c, R, ext_k, step, pad):
    """the lattice of a box in its own frame, centred, inside |P_j| <= ext_kj (1 + pad) -> (object frame, world frame, shape)"""
    half = np.asarray(ext_k, np.float64).reshape(3) * (1.0 + float(pad))
    step = float(step)
    if not step > 0 or not (half > 0).all():
        raise ValueError('mesh.extract_object: step = %r, ext (1 + pad) = %s' % (step, half.tolist()))
    shape = tuple(int(np.floor(2.0 * h / step * (1.0 - 1e-6))) + 1 for h in half)
    if min(shape) < 3:
        raise ValueError('mesh.extract_object: step = %g leaves a lattice of %s points over half extents %s' % (step, shape, half.tolist()))
    o_obj = np.array([-(n - 1) * step / 2.0 for n in shape])
    # X = c + R^T P: the image of object axis j is row j of R
    return (lattice.frame(o_obj, step=step, entry='mesh.extract_object'),
            lattice.frame(c + R.T @ o_obj, axes=step * R, entry='mesh.extract_object'), shape)


def extract_object(model, variables, k, ext, step, iso, ts=0, pad=0.05, colour='query', pose=None, min_points=0, largest=None, smooth=0,
                   **kw):
    """Box k as a mesh in the box's own (canonical) frame.  The 24 bytes of its pose are read once; the lattice is built in
    the box's frame (spacing `step`, centred, inside |P_j| <= ext_kj (1 + pad)) and the WORLD field is queried at c_k + R_k^T P;
    the density is set to 0 where the owner is not k, and on the lattice's outermost layer, so the object closes at its faces;
    the surface is then taken in the object frame: vertices and normals are canonical coordinates.  -> extract's dict plus
    `grid` (the world-frame lattice that was meshed: density, valid, owner, frame) and `pose` (c [3], R [3,3] float64).
    colour='query' asks the world field at the vertices' world positions.  min_points, largest, smooth: as for extract."""
    import torch
    from . import field, smooth as smooth_
    iso = _iso(iso, 'mesh.extract_object')
    sm = smooth_.options(smooth, 'mesh.extract_object')
    K = variables.layout.K if hasattr(variables, 'layout') else 0
    if not 0 <= int(k) < K:
        raise ValueError('mesh.extract_object: box %r of K = %d boxes' % (k, K))
    if colour not in ('query', 'grid', None):
        raise ValueError('mesh.extract_object: colour = %r, expected \'query\', \'grid\' or None' % (colour,))
    field._refuse(model, variables, 'mesh.extract_object')
    if pose is None and float(ts) != int(ts):
        pose = model.interpolate_pose(variables, float(ts))
    p = model._scene_edit(variables, int(ts), pose, None)[0]
    row = p[int(k)].cpu().numpy().astype(np.float64)                         # the one read of the pose
    c, R = row[:3], aa2matrix(row[3:])
    e = np.asarray(torch.as_tensor(ext).detach().cpu().numpy(), np.float64).reshape(-1, 3)
    obj, world, shape = object_lattice(c, R, e[int(k)], step, pad)
    view = kw.pop('view', (0.0, 0.0, -1.0))
    g = field.grid(model, variables, world['origin'], shape, axes=(world['du'], world['dv'], world['dw']),
                   view=view if colour == 'grid' else None, ts=ts, pose=p, ext=ext, **kw)
    mine = g['owner'] == int(k)
    mine[0], mine[-1], mine[:, 0], mine[:, -1], mine[:, :, 0], mine[:, :, -1] = False, False, False, False, False, False
    g['density'] = torch.where(mine, g['density'], torch.zeros_like(g['density']))
    g['valid'] = torch.where(mine, g['valid'], torch.ones_like(g['valid']))
    m = surface(dict(g, frame=dict(obj, shape=list(shape))), iso, normals=True, attrs=('rgb',) if colour == 'grid' else ())
    m['owner'] = _owner(m, g, iso)

    def ask(m):
        Rt = torch.tensor(R, dtype=torch.float32, device=m['vertices'].device)           # row vectors: X = c + P R
        X = (torch.tensor(c, dtype=torch.float32, device=Rt.device) + m['vertices'] @ Rt).contiguous()
        vd = view_of_normals(m['normals'] @ Rt)
        return field.query(model, variables, X, vd, ts=ts, pose=p, ext=ext, **kw)['rgb']
    later = sm is not None and colour == 'query'                              # the colour is asked once, where the vertices end up
    if colour == 'query' and not later:
        m['rgb'] = ask(m)
    elif colour is None or later:
        m['rgb'] = None
    m = smoothed(_clean(m, g, iso, min_points, largest), sm)
    if later:
        m['rgb'] = ask(m)
    m['grid'], m['pose'] = g, (c, R)
    return m


def extract_scene(model, variables, origin, shape, step=None, axes=None, iso=None, ext=None, obj_step=None, ts=0, pad=0.05,
                  colour='query', min_points=0, largest=None, smooth=0, **kw):
    """The whole scene as an asset: `background` (extract with every box disabled), `objects` (extract_object of every box,
    each in its own frame, at spacing obj_step) and `poses` [T,K,6] (the boxes' centres and rotation vectors at every timestep,
    a host array): place object k at time t with X = c + R^T P.  min_points, largest, smooth: as for extract, for every mesh."""
    iso = _iso(iso, 'mesh.extract_scene')
    K = variables.layout.K
    if K and (obj_step is None or ext is None):
        raise ValueError('mesh.extract_scene: obj_step and ext are needed for K = %d boxes' % K)
    bg = extract(model, variables, origin, shape, step=step, axes=axes, iso=iso, colour=colour, ts=ts, ext=ext,
                 box_enable=[0] * K if K else None, min_points=min_points, largest=largest, smooth=smooth, **kw)
    objs = [extract_object(model, variables, k, ext, obj_step, iso, ts=ts, pad=pad, colour=colour, min_points=min_points, largest=largest,
                           smooth=smooth, **kw)
            for k in range(K)]
    poses = variables['params']['box_centers'].detach().cpu().numpy()
    return dict(background=bg, objects=objs, poses=poses)


# ---- PLY ------------------------------------------------------------------------------------------------------------------------
_VERTEX = np.dtype([('x', '<f4'), ('y', '<f4'), ('z', '<f4'), ('nx', '<f4'), ('ny', '<f4'), ('nz', '<f4'), ('red', 'u1'),
                    ('green', 'u1'), ('blue', 'u1')])
_VERTEX_COMPONENT = np.dtype(_VERTEX.descr + [('component', '<i4')])
_FACE = np.dtype([('n', 'u1'), ('v', '<i4', (3,))])


def write_ply(path, m):
    """m: dict vertices [V,3], triangles [T,3], normals [V,3] or None (zeros), rgb [V,3] or None (grey; float in [0, 1] or
    uint8) -> binary little-endian PLY: vertices x y z nx ny nz (float) red green blue (uchar), faces as uchar-int lists.
    A dict with the key `component` [V] (durf_amd.parts.select's) gets one more vertex property, component (int), and only then."""
    X, tri = _host(m['vertices']).astype('<f4').reshape(-1, 3), _host(m['triangles']).astype('<i4').reshape(-1, 3)
    with_component = m.get('component') is not None
    V = np.zeros(X.shape[0], _VERTEX_COMPONENT if with_component else _VERTEX)
    if with_component:
        V['component'] = _host(m['component']).astype('<i4').reshape(-1)
    for c, name in enumerate('xyz'):
        V[name] = X[:, c]
    if m.get('normals') is not None:
        N = _host(m['normals']).astype('<f4')
        for c, name in enumerate(('nx', 'ny', 'nz')):
            V[name] = N[:, c]
    rgb = m.get('rgb')
    if rgb is None:
        rgb8 = np.full((X.shape[0], 3), 200, np.uint8)
    else:
        rgb = _host(rgb)
        rgb8 = rgb if rgb.dtype == np.uint8 else np.rint(np.clip(np.nan_to_num(rgb.astype(np.float64)), 0.0, 1.0) * 255.0).astype(np.uint8)
    for c, name in enumerate(('red', 'green', 'blue')):
        V[name] = rgb8[:, c]
    F = np.zeros(tri.shape[0], _FACE)
    F['n'], F['v'] = 3, tri
    head = ('ply\nformat binary_little_endian 1.0\ncomment durf_amd.mesh\nelement vertex %d\n' % X.shape[0] +
            ''.join('property float %s\n' % n for n in ('x', 'y', 'z', 'nx', 'ny', 'nz')) +
            ''.join('property uchar %s\n' % n for n in ('red', 'green', 'blue')) + ('property int component\n' if with_component else '') +
            'element face %d\nproperty list uchar int vertex_indices\nend_header\n' % tri.shape[0])
    with open(path, 'wb') as f:
        f.write(head.encode('ascii'))
        f.write(V.tobytes())
        f.write(F.tobytes())


def read_ply(path):
    """what write_ply wrote -> dict vertices [V,3] float32, normals [V,3] float32, rgb [V,3] uint8, triangles [T,3] int32, and
    component [V] int32 when the file has that property"""
    blob = open(path, 'rb').read()
    end = blob.index(b'end_header\n') + len(b'end_header\n')
    lines = blob[:end].decode('ascii').split('\n')
    if lines[0] != 'ply' or 'format binary_little_endian 1.0' not in lines:
        raise ValueError('read_ply: %s is not a binary little-endian PLY' % path)
    nv = int([l for l in lines if l.startswith('element vertex')][0].split()[-1])
    nf = int([l for l in lines if l.startswith('element face')][0].split()[-1])
    props = [l.split()[-1] for l in lines if l.startswith('property') and ' list ' not in l]
    vertex = _VERTEX_COMPONENT if props == list(_VERTEX_COMPONENT.names) else _VERTEX
    if props != list(vertex.names):
        raise ValueError('read_ply: vertex properties %s, expected %s (write_ply\'s)' % (props, list(_VERTEX.names)))
    if len(blob) != end + nv * vertex.itemsize + nf * _FACE.itemsize:
        raise ValueError('read_ply: %s holds %d bytes, its header promises %d' % (path, len(blob), end + nv * vertex.itemsize + nf * _FACE.itemsize))
    V = np.frombuffer(blob, vertex, nv, end)
    F = np.frombuffer(blob, _FACE, nf, end + nv * vertex.itemsize)
    if nf and not (F['n'] == 3).all():
        raise ValueError('read_ply: a face that is no triangle')
    out = dict(vertices=np.stack([V['x'], V['y'], V['z']], 1), normals=np.stack([V['nx'], V['ny'], V['nz']], 1),
               rgb=np.stack([V['red'], V['green'], V['blue']], 1), triangles=np.array(F['v'], np.int32).reshape(-1, 3))
    if vertex is _VERTEX_COMPONENT:
        out['component'] = np.array(V['component'], np.int32)
    return out
