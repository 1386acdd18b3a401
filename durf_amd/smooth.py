"""Which vertices of a mesh are neighbours, whether the mesh is closed and manifold, Laplacian / Taubin smoothing and fresh vertex
normals, on the device (include/durf_smooth.h, csrc/smooth.hip, libdurf_smooth.so).  Marching tetrahedra on a lattice leaves a
surface terraced at the lattice's period; a few Taubin iterations take the staircase out without the shrinkage of plain Laplacian
smoothing, and the triangles stay what they are.

    adj = adjacency(m)                                   # one-ring and corner lists in CSR form, vertex_class; two sorts, no read-back
    c = census(adj)                                      # closed? manifold? Euler characteristic (the one read-back)
    s = taubin(m, iters=10, adj=adj)                     # a new mesh dict: vertices replaced, normals recomputed when m had them
    s = laplacian(m, iters=5, factor=0.5)                # plain Laplacian smoothing: it shrinks
    n = normals(s, adj)                                  # area-weighted vertex normals

Every output is defined in the header in integers or written-out fp32 with a stated order of summation: tests/smooth_ref.py
holds the device to every bit, and two runs write the same bytes."""
import numpy as np

from . import trimesh
from . import _smooth_sigs as _H       # generated from include/durf_smooth.h: the constants are written there once

MAX_TRIANGLES = _H.DURF_SMOOTH_MAX_TRIANGLES
LIMIT_WORDS = 'the limit is 6 T < 2^31'
CENSUS_FIELDS = ('isolated', 'interior', 'boundary', 'nonmanifold', 'triangles', 'edges', 'boundary_edges', 'nonmanifold_edges')
assert len(CENSUS_FIELDS) == _H.DURF_SMOOTH_CENSUS_INTS
BOUNDARY = dict(pin=_H.DURF_SMOOTH_PIN, slide=_H.DURF_SMOOTH_SLIDE)
ADJ_KEYS = ('vertices', 'triangles', 'V', 'T', 'offsets', 'neighbours', 'multiplicity', 'corner_offsets', 'corner_tri', 'vertex_class')


def _number(entry, name, x, lo, hi, words, open_lo=False):
    if isinstance(x, bool) or not isinstance(x, (int, float, np.floating, np.integer)) or not (lo <= x <= hi) or (open_lo and x == lo):
        raise ValueError('%s: %s = %r, expected a number in %s' % (entry, name, x, words))
    return float(x)


def _iters(entry, iters):
    if isinstance(iters, bool) or not isinstance(iters, (int, np.integer)) or not 0 <= iters < 2 ** 30:
        raise ValueError('%s: iters = %r, expected a whole number >= 0' % (entry, iters))
    return int(iters)


def _boundary(entry, boundary):
    if boundary not in BOUNDARY:
        raise ValueError("%s: boundary = %r, expected 'pin' or 'slide'" % (entry, boundary))
    return BOUNDARY[boundary]


def _adj(entry, adj, V, T):
    if not isinstance(adj, dict) or any(adj.get(k) is None for k in ADJ_KEYS):
        raise ValueError("%s: adj is smooth.adjacency's dict (%s)" % (entry, ', '.join(ADJ_KEYS)))
    if (V, T) != (None, None) and (adj['V'], adj['T']) != (V, T):
        raise ValueError('%s: adj of %d vertices and %d triangles for a mesh of %d and %d' % (entry, adj['V'], adj['T'], V, T))
    return adj


def _fixed(entry, fixed, V, dev):
    if fixed is None:
        return None
    if tuple(getattr(fixed, 'shape', ())) != (V,):
        raise ValueError('%s: fixed of shape %s, expected [%d]' % (entry, tuple(getattr(fixed, 'shape', ())), V))
    import torch
    f = fixed if torch.is_tensor(fixed) else torch.as_tensor(np.ascontiguousarray(np.asarray(fixed) != 0))
    return (f != 0).to(device=dev, dtype=torch.uint8).contiguous()


def adjacency(m):
    """The one-ring of every vertex of the mesh dict m -> dict vertices [V,3] and triangles [T,3] on the device, V, T, offsets
    [V+1], neighbours and multiplicity [6T] (ascending within a vertex; entries past offsets[V] are not written), corner_offsets
    [V+1], corner_tri [3T] and vertex_class uint8 [V] (0 isolated, 1 interior, 2 boundary, 3 non-manifold).  Adjacency is
    combinatorial: a triangle with an index outside 0 .. V-1 or a repeated index takes no part.  Two torch.sort calls on the keys,
    as cast.build sorts its Morton keys; nothing is read back."""
    entry = 'smooth.adjacency'
    V, T = trimesh.arrays(m, entry, MAX_TRIANGLES, LIMIT_WORDS)
    import torch
    from . import ops
    v, t = trimesh.on_device(m, V, T, trimesh.device_of(m['vertices']))
    ek, ck = ops.smooth_keys(t, V)
    a = ops.smooth_adjacency(torch.sort(ek).values, torch.sort(ck).values, V, T)
    a['vertex_class'] = ops.smooth_classify(a['offsets'], a['multiplicity'])
    return dict(a, vertices=v, triangles=t, V=V, T=T)


def census(adj):
    """What the adjacency says about the mesh -> dict of ints isolated, interior, boundary, nonmanifold (vertices of each class),
    triangles (contributing), edges (undirected), boundary_edges (in one triangle), nonmanifold_edges (in more than two), plus
    closed (no boundary and no non-manifold edge) and euler ((V - isolated) - edges + triangles).  The one read-back."""
    from . import ops
    adj = _adj('smooth.census', adj, None, None)
    c = dict(zip(CENSUS_FIELDS, (int(x) for x in ops.smooth_census(adj).cpu())))
    c['closed'] = c['boundary_edges'] == 0 and c['nonmanifold_edges'] == 0
    c['euler'] = (adj['V'] - c['isolated']) - c['edges'] + c['triangles']
    return c


def normals(m, adj=None):
    """Area-weighted vertex normals [V,3] of m's vertices over adj's corner lists: the sum of e1 x e2 of the triangles at a vertex
    in ascending triangle id, scaled to unit length; zero where nothing contributes.  Oriented as the triangles are."""
    entry = 'smooth.normals'
    V, T = trimesh.arrays(m, entry, MAX_TRIANGLES, LIMIT_WORDS)
    adj = adjacency(m) if adj is None else _adj(entry, adj, V, T)
    import torch
    from . import ops
    v = trimesh.upload(m['vertices'], torch.float32, adj['vertices'].device).reshape(V, 3)
    return ops.smooth_normals(adj, v, adj['triangles'])


def _smoothed(entry, m, adj, fixed, boundary, run):
    V, T = trimesh.arrays(m, entry, MAX_TRIANGLES, LIMIT_WORDS)
    b = _boundary(entry, boundary)
    adj = adjacency(m) if adj is None else _adj(entry, adj, V, T)
    import torch
    dev = adj['vertices'].device
    v = trimesh.upload(m['vertices'], torch.float32, dev).reshape(V, 3)
    out = dict(m)
    out['vertices'] = run(adj, v, b, _fixed(entry, fixed, V, dev))
    if m.get('normals') is not None:
        from . import ops
        out['normals'] = ops.smooth_normals(adj, out['vertices'], adj['triangles'])
    return out


def step(m, factor, boundary='pin', fixed=None, adj=None):
    """One smoothing step: every free vertex moves by factor times the way to the mean of its neighbours.  An interior vertex
    uses all its neighbours; a boundary vertex stays (boundary='pin') or uses its neighbours along the boundary ('slide');
    isolated and non-manifold vertices, vertices with fixed[i] != 0 and vertices that are not finite stay, bit for bit.
    -> a new mesh dict with `vertices` replaced and `normals` recomputed when m had them; everything else as it is."""
    from . import ops
    entry = 'smooth.step'
    f = _number(entry, 'factor', factor, -1.0, 1.0, '[-1, 1]')
    return _smoothed(entry, m, adj, fixed, boundary, lambda a, v, b, fx: ops.smooth_step(a, v, f, b, fx))


def taubin(m, iters=10, lam=0.5, mu=-0.53, boundary='pin', fixed=None, adj=None):
    """Taubin smoothing: iters times a step with lam (it shrinks) then a step with mu (it inflates), which damps the staircase
    and keeps the volume; mu = 0 leaves the lam steps alone.  -> as step."""
    from . import ops
    entry = 'smooth.taubin'
    n = _iters(entry, iters)
    la, mm = _number(entry, 'lam', lam, 0.0, 1.0, '(0, 1]', True), _number(entry, 'mu', mu, -1.0, 0.0, '[-1, 0]')
    return _smoothed(entry, m, adj, fixed, boundary, lambda a, v, b, fx: ops.smooth_taubin(a, v, n, la, mm, b, fx))


def laplacian(m, iters, factor=0.5, boundary='pin', fixed=None, adj=None):
    """Plain Laplacian smoothing: iters steps with `factor`.  It shrinks what it smooths; taubin does not.  -> as step."""
    from . import ops
    entry = 'smooth.laplacian'
    n = _iters(entry, iters)
    f = _number(entry, 'factor', factor, 0.0, 1.0, '(0, 1]', True)
    return _smoothed(entry, m, adj, fixed, boundary, lambda a, v, b, fx: ops.smooth_taubin(a, v, n, f, 0.0, b, fx))


def options(smooth, entry):
    """the `smooth` argument of mesh.extract and its kin: 0 / None (nothing), a number of Taubin iterations, or a dict of taubin's
    arguments -> None or that dict"""
    if smooth is None or (isinstance(smooth, (int, np.integer)) and not isinstance(smooth, bool) and smooth == 0):
        return None
    if isinstance(smooth, dict):
        bad = set(smooth) - {'iters', 'lam', 'mu', 'boundary', 'fixed'}
        if bad:
            raise ValueError('%s: smooth has no %s (iters, lam, mu, boundary, fixed)' % (entry, ', '.join(sorted(map(repr, bad)))))
        return dict(smooth)
    return dict(iters=_iters(entry, smooth))


# ---- the commands' flags (extract_mesh, fuse_tsdf) ------------------------------------------------------------------------------
def add_arguments(ap):
    ap.add_argument('--smooth', type=int, default=0, help='Taubin iterations on every mesh after the cleaning (0: none; durf_amd.smooth)')
    ap.add_argument('--smooth_lambda', type=float, default=0.5, help='--smooth: the shrinking factor, in (0, 1]')
    ap.add_argument('--smooth_mu', type=float, default=-0.53, help='--smooth: the inflating factor, in [-1, 0] (0: plain Laplacian smoothing)')
    ap.add_argument('--smooth_boundary', choices=tuple(BOUNDARY), default='pin', help='--smooth: boundary vertices stay, or slide along the boundary')


def from_args(args, prog):
    """the four flags -> None (no --smooth) or taubin's arguments as a dict, refused under the command's name"""
    if not args.smooth:
        return None
    try:
        return dict(iters=_iters(prog, args.smooth), lam=_number(prog, '--smooth_lambda', args.smooth_lambda, 0.0, 1.0, '(0, 1]', True),
                    mu=_number(prog, '--smooth_mu', args.smooth_mu, -1.0, 0.0, '[-1, 0]'), boundary=args.smooth_boundary)
    except ValueError as e:
        raise SystemExit(str(e))
