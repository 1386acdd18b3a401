"""The iso-surface of include/durf_mesh.h restated in numpy: a float64 oracle with a float32 twin that performs the header's
operations in the header's order (what tests/flow_ref.py is to durf_flow.h).  The integer side -- which edges are active, the
vertex ids, which tetrahedra emit, the split of each case into triangles, the triangle order -- is restated from the header's
rules.  The WINDING is not a table here: for every (tetrahedron, case) the oracle places each crossing at its edge midpoint in
index space and demands (X1 - X0) x (X2 - X0) . (mean(O) - mean(I)) > 0, swapping the last two vertices when it is not; a wrong
entry of the kernel's compile-time table can therefore not be mirrored.

    m = surface(density, valid, iso, frame, flip=False, dt=np.float64)
        -> counts (V, T), vertex_edge [V,2], triangles [T,3], t [V], vertices [V,3], normals [V,3], mask [n], voff [n], toff [n]

frame: dict(origin, du, dv, dw); the values are rounded to float32 first (they reach the library as host floats)."""
import itertools

import numpy as np

from tests import lattice_ref
from tests.lattice_ref import host_frame  # noqa: F401  (the frame and its inverse are lattice_ref's)

PERMS = ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0))
POP8 = np.array([bin(x).count('1') for x in range(256)], np.int64)


def offset(code):
    """(di, dj, dk): the bits of code = 4 di + 2 dj + dk"""
    return code >> 2 & 1, code >> 1 & 1, code & 1


def tet_corners(perm):
    """cell-corner codes of v0 = p, v1 = p + e_x, v2 = p + e_x + e_y, v3 = p + (1,1,1)"""
    x, y, _ = perm
    return 0, 4 >> x, (4 >> x) | (4 >> y), 7


def case_triangles(perm, case):
    """the triangles of one tetrahedron case (bit l: local corner l is in) -> list of triples of local-corner pairs (a, b),
    a < b, wound so that the normal points from the in corners to the out corners in index space (a right-handed frame)"""
    I = [l for l in range(4) if case >> l & 1]
    O = [l for l in range(4) if not case >> l & 1]
    e = lambda a, b: (min(a, b), max(a, b))
    if len(I) in (0, 4):
        return []
    if len(I) == 1 or len(O) == 1:
        a = I[0] if len(I) == 1 else O[0]
        b, c, d = [l for l in range(4) if l != a]
        tris = [(e(a, b), e(a, c), e(a, d))]
    else:
        (a, b), (c, d) = I, O
        tris = [(e(a, c), e(a, d), e(b, d)), (e(a, c), e(b, d), e(b, c))]
    pos = np.array([offset(c) for c in tet_corners(perm)], np.float64)
    want = pos[O].mean(0) - pos[I].mean(0)
    out = []
    for tri in tris:
        X = [0.5 * (pos[a] + pos[b]) for a, b in tri]
        s = float(np.dot(np.cross(X[1] - X[0], X[2] - X[0]), want))
        assert abs(s) > 1e-9, (perm, case)
        out.append(tri if s > 0 else (tri[0], tri[2], tri[1]))
    return out


def lattice_state(density, valid, iso):
    """-> usable, inn [nu,nv,nw] bool (the exact float32 comparison)"""
    d = np.asarray(density, np.float32)
    usable = ~np.isnan(d)
    if valid is not None:
        usable &= np.asarray(valid) != 0
    with np.errstate(invalid='ignore'):
        inn = usable & (d >= np.float32(iso))
    return usable, inn


def _shift(a, off, fill):
    """a[p + off] at every p, `fill` where p + off is outside"""
    out = np.full(a.shape, fill, a.dtype)
    di, dj, dk = off
    nu, nv, nw = a.shape
    out[:nu - di, :nv - dj, :nw - dk] = a[di:, dj:, dk:]
    return out


def topology(density, valid, iso, flip=False):
    """the integer side of the header -> dict mask, voff, toff [n], vertex_edge [V,2] (g, e), triangles [T,3], counts"""
    usable, inn = lattice_state(density, valid, iso)
    nu, nv, nw = usable.shape
    n = nu * nv * nw
    mask = np.zeros((nu, nv, nw), np.int64)
    for e in range(7):
        o = offset(e + 1)
        ub, ib = _shift(usable, o, False), _shift(inn, o, False)
        mask |= (usable & ub & (inn != ib)).astype(np.int64) << e
    mask = mask.reshape(-1)
    cnt = POP8[mask]
    voff = np.cumsum(cnt) - cnt
    bits = (mask[:, None] >> np.arange(7)[None]) & 1
    g_of, e_of = np.nonzero(bits)                                   # g-major, then e: the id order
    vertex_edge = np.stack([g_of, e_of], 1).astype(np.int32)
    # cells
    gi = np.arange(n).reshape(nu, nv, nw)[:nu - 1, :nv - 1, :nw - 1].reshape(-1)
    stride = np.array([nv * nw, nw, 1])
    uf, nf = usable.reshape(-1), inn.reshape(-1)
    rows, keys = [], []
    ntri = np.zeros(n, np.int64)
    for t, perm in enumerate(PERMS):
        codes = tet_corners(perm)
        cg = [gi + int(np.dot(offset(c), stride)) for c in codes]
        ok = uf[cg[0]] & uf[cg[1]] & uf[cg[2]] & uf[cg[3]]
        case = sum(nf[cg[l]].astype(np.int64) << l for l in range(4))
        for cs in range(1, 15):
            tris = case_triangles(perm, cs)
            sel = np.nonzero(ok & (case == cs))[0]
            if sel.size == 0:
                continue
            ntri[gi[sel]] += len(tris)
            for r, tri in enumerate(tris):
                ids = []
                for a, b in tri:
                    owner = cg[a][sel]
                    e = codes[b] - codes[a] - 1
                    assert (mask[owner] >> e & 1).all()
                    ids.append(voff[owner] + POP8[mask[owner] & ((1 << e) - 1)])
                if flip:
                    ids = [ids[0], ids[2], ids[1]]
                rows.append(np.stack(ids, 1))
                keys.append((gi[sel] * 6 + t) * 2 + r)
    if rows:
        rows, keys = np.concatenate(rows), np.concatenate(keys)
        triangles = rows[np.argsort(keys, kind='stable')].astype(np.int32)
    else:
        triangles = np.zeros((0, 3), np.int32)
    toff = np.cumsum(ntri) - ntri
    return dict(mask=mask.astype(np.uint8), voff=voff.astype(np.int32), toff=toff.astype(np.int32), vertex_edge=vertex_edge,
                triangles=triangles, counts=(int(cnt.sum()), int(triangles.shape[0])))


def gradient(density, valid, dt):
    """the index-space gradient at every lattice point [nu,nv,nw,3]: central where both neighbours exist and are usable,
    one-sided towards the usable one, else 0"""
    d = np.asarray(density, np.float32).astype(dt)
    usable, _ = lattice_state(density, valid, 0.0)
    out = np.zeros(d.shape + (3,), dt)
    with np.errstate(invalid='ignore'):
        for x in range(3):
            dp, dm = np.roll(d, -1, x), np.roll(d, 1, x)
            up, um = np.roll(usable, -1, x), np.roll(usable, 1, x)
            idx = np.arange(d.shape[x]).reshape([-1 if y == x else 1 for y in range(3)])
            up = up & (idx + 1 < d.shape[x])
            um = um & (idx > 0)
            g = np.where(up & um, dt(0.5) * (dp - dm), np.where(up, dp - d, np.where(um, d - dm, dt(0))))
            out[..., x] = g
    return out


def geometry(density, valid, iso, frame, vertex_edge, dt=np.float64, normals=True):
    """t [V], vertices [V,3], normals [V,3] of the vertices on edges vertex_edge, in dtype dt, the header's order of operations"""
    d = np.asarray(density, np.float32)
    A = host_frame(frame)[4].astype(dt)
    g, e = vertex_edge[:, 0].astype(np.int64), vertex_edge[:, 1].astype(np.int64)
    (i, j, k), (di, dj, dk), gb = lattice_ref.ijk(g, d.shape), lattice_ref.edge(e), lattice_ref.edge_end(g, e, d.shape)
    flat = d.reshape(-1).astype(dt)
    da, db = flat[g], flat[gb]
    with np.errstate(all='ignore'):
        t = (dt(np.float32(iso)) - da) / (db - da)
        t = np.fmin(np.fmax(t, dt(0)), dt(1))
    X = lattice_ref.place(frame, [i.astype(dt) + t * di.astype(dt), j.astype(dt) + t * dj.astype(dt), k.astype(dt) + t * dk.astype(dt)], dt)
    nrm = None
    if normals:
        G = gradient(density, valid, dt).reshape(-1, 3)
        gr = G[g] + t[:, None] * (G[gb] - G[g])
        m = np.stack([(A[c, 0] * gr[:, 0] + A[c, 1] * gr[:, 1]) + A[c, 2] * gr[:, 2] for c in range(3)], 1)
        with np.errstate(all='ignore'):
            ln = np.sqrt((m[:, 0] * m[:, 0] + m[:, 1] * m[:, 1]) + m[:, 2] * m[:, 2])
            nrm = -m / ln[:, None]
        bad = ~np.isfinite(nrm).all(1) | (nrm == 0).all(1)
        nrm[bad] = 0
    return t, X, nrm


def surface(density, valid, iso, frame, flip=False, dt=np.float64, normals=True):
    top = topology(density, valid, iso, flip)
    t, X, nrm = geometry(density, valid, iso, frame, top['vertex_edge'], dt, normals)
    return dict(top, t=t, vertices=X, normals=nrm)


def gather_float(attr, vertex_edge, t, shape, dt=np.float64):
    """attr [n,C] at the vertices: a + t (b - a)"""
    g, e = vertex_edge[:, 0].astype(np.int64), vertex_edge[:, 1].astype(np.int64)
    gb = lattice_ref.edge_end(g, e, shape)
    a, b = np.asarray(attr, np.float32).astype(dt)[g], np.asarray(attr, np.float32).astype(dt)[gb]
    return a + np.asarray(t, dt)[:, None] * (b - a)


def gather_label(label, vertex_edge, density, valid, iso):
    """the label of each edge's in end"""
    _, inn = lattice_state(density, valid, iso)
    g, e = vertex_edge[:, 0].astype(np.int64), vertex_edge[:, 1].astype(np.int64)
    gb = lattice_ref.edge_end(g, e, inn.shape)
    return np.where(inn.reshape(-1)[g], np.asarray(label).reshape(-1)[g], np.asarray(label).reshape(-1)[gb])


# ---- what a closed surface satisfies ------------------------------------------------------------------------------------------
def edge_census(triangles):
    """-> (directed edge count per undirected edge [E,2]: forward, backward; E)"""
    tri = np.asarray(triangles, np.int64)
    a = np.concatenate([tri[:, 0], tri[:, 1], tri[:, 2]])
    b = np.concatenate([tri[:, 1], tri[:, 2], tri[:, 0]])
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    key = lo * (int(tri.max()) + 1 if tri.size else 1) + hi
    uniq, inv = np.unique(key, return_inverse=True)
    fwd = np.bincount(inv, weights=(a < b), minlength=uniq.size).astype(np.int64)
    bwd = np.bincount(inv, weights=(a > b), minlength=uniq.size).astype(np.int64)
    same = np.bincount(inv, weights=(a == b), minlength=uniq.size).astype(np.int64)
    return fwd, bwd, same


def is_closed(triangles):
    """every undirected edge in exactly two triangles, once in each direction"""
    fwd, bwd, same = edge_census(triangles)
    return bool((fwd == 1).all() and (bwd == 1).all() and (same == 0).all())


def euler(triangles):
    """V - E + F over the vertices the triangles reference"""
    tri = np.asarray(triangles, np.int64)
    fwd, _, _ = edge_census(tri)
    return int(np.unique(tri).size - fwd.size + tri.shape[0])


def signed_volume(vertices, triangles):
    """the divergence theorem: sum X0 . (X1 x X2) / 6"""
    X = np.asarray(vertices, np.float64)
    tri = np.asarray(triangles, np.int64)
    return float((X[tri[:, 0]] * np.cross(X[tri[:, 1]], X[tri[:, 2]])).sum() / 6.0)


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(np.float32)).astype(np.float64)


# ---- planted fields -------------------------------------------------------------------------------------------------------------
def lattice_points(frame, shape):
    """float64 from the frame's values AS GIVEN (the planted fields' bits hang on it): not the libraries' rule, lattice_ref.points"""
    o, du, dv, dw = (np.asarray(frame[k], np.float64) for k in ('origin', 'du', 'dv', 'dw'))
    i, j, k = np.meshgrid(*[np.arange(s, dtype=np.float64) for s in shape], indexing='ij')
    return o + i[..., None] * du + j[..., None] * dv + k[..., None] * dw


def sphere_field(frame, shape, centre, R):
    X = lattice_points(frame, shape)
    return (R - np.linalg.norm(X - np.asarray(centre, np.float64), axis=-1)).astype(np.float32)


def torus_field(frame, shape, centre, R, r):
    X = lattice_points(frame, shape) - np.asarray(centre, np.float64)
    ring = np.sqrt(X[..., 0] ** 2 + X[..., 1] ** 2) - R
    return (r - np.sqrt(ring ** 2 + X[..., 2] ** 2)).astype(np.float32)


def sign_field(shape, seed, border=False):
    """random +-1; border: a one-point shell of -1 (out) around it"""
    d = np.where(np.random.default_rng(seed).integers(0, 2, shape) > 0, 1.0, -1.0).astype(np.float32)
    if border:
        d[0], d[-1], d[:, 0], d[:, -1], d[:, :, 0], d[:, :, -1] = -1, -1, -1, -1, -1, -1
    return d


def corner_patterns(density, iso):
    """the set of 8-bit corner-sign patterns over the cells of a lattice"""
    inn = np.asarray(density, np.float32) >= np.float32(iso)
    nu, nv, nw = inn.shape
    pat = np.zeros((nu - 1, nv - 1, nw - 1), np.int64)
    for c, (di, dj, dk) in enumerate(itertools.product((0, 1), repeat=3)):
        pat |= inn[di:nu - 1 + di, dj:nv - 1 + dj, dk:nw - 1 + dk].astype(np.int64) << c
    return set(np.unique(pat).tolist())


def unit_frame(step=1.0, origin=(0.0, 0.0, 0.0)):
    return lattice_ref.frame_of(origin, step)
