"""The CPU oracle of libdurf_parts.so: include/durf_parts.h restated in numpy and plain Python, with none of the library's
structure -- no tiles, no passes, no atomics: one union-find over every owned edge whose two ends are IN, by minimum index."""
import numpy as np

from tests import lattice_ref

OFFSETS = tuple(lattice_ref.edge(e) for e in range(7))       # o_e: the bits of e + 1


def in_points(density, valid, iso):
    """IN: usable (valid != 0, density not NaN) and density >= iso"""
    d = np.asarray(density, np.float32)
    with np.errstate(invalid='ignore'):
        inn = ~np.isnan(d) & (d >= np.float32(iso))
    return inn if valid is None else inn & (np.asarray(valid) != 0)


def labels_of(inn):
    """bool [nu,nv,nw] -> int32 [nu,nv,nw]: the smallest index of each point's component, -1 where it is not in"""
    nu, nv, nw = inn.shape
    idx = np.arange(inn.size, dtype=np.int64).reshape(inn.shape)
    parent = list(range(inn.size))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for di, dj, dk in OFFSETS:
        a, b = (slice(0, nu - di), slice(0, nv - dj), slice(0, nw - dk)), (slice(di, nu), slice(dj, nv), slice(dk, nw))
        both = inn[a] & inn[b]
        for x, y in zip(idx[a][both].tolist(), idx[b][both].tolist()):
            rx, ry = find(x), find(y)
            if rx != ry:
                parent[max(rx, ry)] = min(rx, ry)
    flat = inn.reshape(-1)
    return np.array([find(g) if flat[g] else -1 for g in range(inn.size)], np.int32).reshape(inn.shape)


def labels(density, valid, iso):
    return labels_of(in_points(density, valid, iso))


def number(lab):
    """labels -> (comp int32 of the same shape: the rank of each point's label among the labels, -1; the count)"""
    flat = lab.reshape(-1)
    roots = np.flatnonzero(flat == np.arange(flat.size))
    rank = np.full(flat.size, -1, np.int32)
    rank[roots] = np.arange(roots.size, dtype=np.int32)
    comp = np.where(flat >= 0, rank[np.maximum(flat, 0)], -1).astype(np.int32)
    return comp.reshape(lab.shape), int(roots.size)


def stats(comp, count):
    """-> size int32 [count], bbox int32 [count,6]: imin, jmin, kmin, imax, jmax, kmax (inclusive)"""
    size, bbox = np.zeros(count, np.int32), np.zeros((count, 6), np.int32)
    ijk = np.stack(np.meshgrid(*[np.arange(s) for s in comp.shape], indexing='ij'), -1)
    for c in range(count):
        at = ijk[comp == c]
        size[c] = at.shape[0]
        bbox[c, :3], bbox[c, 3:] = at.min(0), at.max(0)
    return size, bbox


def components(density, valid, iso):
    lab = labels(density, valid, iso)
    comp, count = number(lab)
    size, bbox = stats(comp, count)
    return dict(labels=lab, comp=comp, count=count, size=size, bbox=bbox)


def scipy_structure():
    """the centro-symmetric 3 x 3 x 3 structure of the 14 offsets +-o_e plus the centre, for scipy.ndimage.label"""
    s = np.zeros((3, 3, 3), bool)
    s[1, 1, 1] = True
    for di, dj, dk in OFFSETS:
        s[1 + di, 1 + dj, 1 + dk] = s[1 - di, 1 - dj, 1 - dk] = True
    return s


def min_index_labels(numbered):
    """any labelling with 0 = background, 1 .. C = components (scipy's) -> the minimum-index labelling, -1 = background"""
    flat = numbered.reshape(-1)
    out = np.full(flat.size, -1, np.int32)
    for c in range(1, int(flat.max()) + 1 if flat.size else 1):
        at = np.flatnonzero(flat == c)
        out[at] = at[0]
    return out.reshape(numbered.shape)


def vertex_component(comp, vertex_edge, inn):
    """the component of each vertex's IN end: vertex_edge [V,2] = (g, e)"""
    g, e = vertex_edge[:, 0].astype(np.int64), vertex_edge[:, 1].astype(np.int64)
    gb = lattice_ref.edge_end(g, e, comp.shape)
    return np.where(inn.reshape(-1)[g], comp.reshape(-1)[g], comp.reshape(-1)[gb]).astype(np.int32)


def select_mesh(vertex_comp, triangles, keep):
    """-> vertex_map [V] (new id or -1), vertex_src [V'], triangles_out [T',3], (V', T')"""
    keep = np.asarray(keep).astype(bool)
    kv = np.array([0 <= c < keep.size and keep[c] for c in vertex_comp.tolist()], bool).reshape(-1)
    vmap = np.where(kv, np.cumsum(kv) - 1, -1).astype(np.int32)
    kt = kv[triangles[:, 0]] if triangles.shape[0] else np.zeros(0, bool)
    return vmap, np.flatnonzero(kv).astype(np.int32), vmap[triangles[kt]].astype(np.int32).reshape(-1, 3), (int(kv.sum()), int(kt.sum()))


def serpentine(shape):
    """a one-point-wide path through the lattice, as the (i, j, k) of its points in path order: runs along k on the even rows j
    of the even planes i, joined by two-step links along j at alternating ends, the planes joined by two-step links along i --
    so no two points of different runs are adjacent and the path's order is the only connection"""
    nu, nv, nw = shape
    path, fwd_k, fwd_j = [], True, True
    planes = list(range(0, nu, 2))
    for pi, i in enumerate(planes):
        rows = list(range(0, nv, 2))
        rows = rows if fwd_j else rows[::-1]
        for rj, j in enumerate(rows):
            ks = list(range(nw)) if fwd_k else list(range(nw - 1, -1, -1))
            path += [(i, j, k) for k in ks]
            if rj + 1 < len(rows):
                path.append((i, (j + rows[rj + 1]) // 2, ks[-1]))
            fwd_k = not fwd_k
        if pi + 1 < len(planes):
            path.append((i + 1, rows[-1], path[-1][2]))
        fwd_j = not fwd_j
    return path
