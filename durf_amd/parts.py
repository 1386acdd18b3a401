"""The connected solid regions of a density lattice, on the device (include/durf_parts.h, csrc/parts.hip, libdurf_parts.so):
label them, measure them, keep the large ones, and drop the rest -- the floaters a radiance field leaves in free space --
from the lattice's surface.

    g = field.grid(model, variables, origin, shape, step=0.25, ext=ext)          # any dict(density=, valid=, frame=)
    p = components(g, iso=5.0)                                                   # labels, comp, n, size, bbox, touches_border
    k = keep(p, min_points=50)                                                   # bool [n]; largest=, seeds= combine with AND
    m = select(mesh.surface(g, 5.0), g, p, k)                                    # the same mesh without the dropped shells
    v = mask(p, k)                                                               # uint8 lattice of the kept components' points

Two IN points are connected along the seven lattice edges a point owns and the seven that end at it: the edges of the Kuhn
tetrahedra mesh.surface marches.  Points the surface does not separate share a component, points it separates do not, and every
triangle belongs to exactly one component, so dropping a component is a compaction of the mesh: positions, normals and colours
are untouched, nothing is re-meshed and no density is overwritten.  Everything stays on the device; the one
value read back by components is the number of components, as mesh.surface reads its two counts."""


from .lattice import device_lattice as _lattice


def components(g, iso):
    """The components of the lattice g (field.grid's dict, or any dict(density= [nu,nv,nw] float32 on the device, valid= uint8 or
    None)) at `iso`: durf_parts_label, durf_parts_number, ONE read of the count, durf_parts_stats -> dict labels [nu,nv,nw]
    int32 (the smallest index of the point's component, -1 where the point is not in), comp [nu,nv,nw] int32 (the component's
    number, in ascending order of the labels, or -1), count (the device tensor), n (int), size [n] int32 (points), bbox [n,6]
    int32 (imin, jmin, kmin, imax, jmax, kmax, inclusive), touches_border [n] bool, iso, shape."""
    from . import ops
    from .mesh import _iso
    iso = _iso(iso, 'parts.components')
    d, v, shape = _lattice(g, 'parts.components')
    labels, ws = ops.parts_label(d, v, shape, iso)
    comp, count = ops.parts_number(labels, ws)
    n = int(count.cpu())
    size, bbox = ops.parts_stats(comp, shape, n)
    hi = bbox.new_tensor([s - 1 for s in shape])
    touches = ((bbox[:, :3] == 0) | (bbox[:, 3:] == hi)).any(1)
    return dict(labels=labels.view(shape), comp=comp.view(shape), count=count, n=n, size=size, bbox=bbox, touches_border=touches, iso=iso,
                shape=shape)


def keep(parts, min_points=0, largest=None, seeds=None):
    """Which components stay -> bool [n] where parts['size'] lives.  min_points: the component has at least that many points;
    largest: it is among the `largest` biggest, ties broken by the smaller number; seeds [m,3] int: it contains one of those
    lattice points (i, j, k).  The rules given are combined with AND."""
    import torch
    size = parts['size']
    n = int(size.shape[0])
    k = size >= int(min_points)
    if largest is not None:
        if int(largest) < 0:
            raise ValueError('parts.keep: largest = %r' % (largest,))
        order = torch.sort(size, descending=True, stable=True)[1]              # equal sizes stay in ascending number
        top = torch.zeros(n, dtype=torch.bool, device=size.device)
        top[order[:int(largest)]] = True
        k = k & top
    if seeds is not None:
        s = torch.as_tensor(seeds).detach().cpu().to(torch.int64).reshape(-1, 3)
        shape = parts['shape']
        if s.numel() and not bool(((s >= 0) & (s < torch.tensor(shape))).all()):
            raise ValueError('parts.keep: a seed outside the lattice of %s points' % (tuple(shape),))
        comp = parts['comp']
        s = s.to(comp.device)
        c = comp[s[:, 0], s[:, 1], s[:, 2]].to(torch.int64)
        hit = torch.zeros(n + 1, dtype=torch.bool, device=size.device)          # slot n takes the seeds that are not in
        hit[torch.where(c >= 0, c, torch.full_like(c, n)).to(size.device)] = True
        k = k & hit[:n]
    return k


def mask(parts, keep):
    """uint8 [nu,nv,nw]: 1 at the IN points of kept components -- to clean a field.columns map, or as the `valid` of another
    call"""
    import torch
    comp = parts['comp']
    k = torch.cat([keep.to(device=comp.device, dtype=torch.uint8), torch.zeros(1, dtype=torch.uint8, device=comp.device)])
    return k[torch.where(comp >= 0, comp, torch.full_like(comp, parts['n'])).to(torch.int64)]


def vertex_components(m, g, parts):
    """the component of every vertex of m = mesh.surface(g, parts['iso']): that of its edge's IN end (durf_mesh_gather) -> int32 [V]"""
    import torch
    from . import ops
    d, v, shape = _lattice(g, 'parts.select')
    if tuple(m['shape']) != shape or tuple(parts['shape']) != shape or float(m['iso']) != float(parts['iso']):
        raise ValueError('parts.select: the mesh (shape %s, iso %r), the lattice %s and the components (shape %s, iso %r) do not belong together'
                         % (tuple(m['shape']), m['iso'], shape, tuple(parts['shape']), parts['iso']))
    V = int(m['vertex_edge'].shape[0])
    if V == 0:
        return torch.empty(0, dtype=torch.int32, device=d.device)
    return ops.mesh_gather(shape, m['counts'], m['vertex_edge'], m['vertex_t'], attr_i=parts['comp'].contiguous().reshape(-1), density=d, valid=v,
                           iso=m['iso'])[1]


def _select(m, vertex_comp, keep):
    import torch
    from . import ops
    V = int(vertex_comp.shape[0])
    k = keep.to(device=vertex_comp.device, dtype=torch.uint8).contiguous()
    vmap, vsrc, tri, counts = ops.parts_select_mesh(m['counts'], vertex_comp, m['triangles'].contiguous(), k)
    nv, nt = (int(x) for x in counts.cpu())
    src = vsrc[:nv].to(torch.int64)
    out = {}
    for key, val in m.items():
        per_vertex = torch.is_tensor(val) and key not in ('triangles', 'counts') and val.dim() >= 1 and val.shape[0] == V
        out[key] = val.index_select(0, src) if per_vertex else val
    out.update(triangles=tri[:nt], counts=counts, component=vertex_comp.index_select(0, src))
    return out


def select(m, g, parts, keep):
    """The mesh m = mesh.surface(g, iso) (or extract's) without the components keep drops: durf_parts_select_mesh, ONE read of
    the two new counts, then every per-vertex array (vertices, normals, vertex_edge, vertex_t, owner, rgb, attributes) gathered
    with index_select -> a dict of m's keys with new `counts`, plus component [V'] int32.  Kept vertices and triangles keep
    their order and their bits."""
    return _select(m, vertex_components(m, g, parts), keep)


def split(m, g, parts, keep):
    """one mesh per kept component, in ascending number -> list of select's dicts"""
    import torch
    vc = vertex_components(m, g, parts)
    out = []
    for c in torch.nonzero(keep).reshape(-1).cpu().tolist():
        one = torch.zeros_like(keep, dtype=torch.bool)
        one[c] = True
        out.append(_select(m, vc, one))
    return out


def clean(m, g, iso, min_points=0, largest=None):
    """mesh.extract's opt-in cleaning: components, keep, select -> (the selected mesh, a host summary dict components (the count
    before), kept, dropped_points, sizes (the kept ones))"""
    p = components(g, iso)
    k = keep(p, min_points=min_points, largest=largest)
    size, kk = p['size'].cpu(), k.cpu()
    summary = dict(components=p['n'], kept=int(kk.sum()), dropped_points=int(size[~kk].sum()), sizes=[int(s) for s in size[kk]])
    return select(m, g, p, k), summary
