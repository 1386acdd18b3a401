"""Brute-force oracles of include/durf_raster.h in NumPy: every (frame, triangle) pair, every pixel of its bounds.

    draw32   Python / int64 edge functions and np.float32 arithmetic in exactly the order the header states: what
             libdurf_raster.so must reproduce bit for bit (every NumPy ufunc is one rounding: nothing is fused).
    draw64   the same snapped coordinates, hence the same coverage, with the projection (the z of every vertex), the weights
             E_i / |A2| and the depth in float64, no float32 rounding anywhere: what draw32's depth is held to; it also gives
             the relative gap between the nearest two candidates of every pixel.

Scenes shared by the host and the device tests: camera(), random_scene(), fan() and grid() (tilings of a rectangle)."""
import numpy as np

from tests import camera_ref
from tests.camera_ref import look_at  # noqa: F401

SUB = 256
MAX_COORD = 1 << 29
TILE = 16
COUNT_FIELDS = ('pairs', 'drawn', 'invalid', 'behind', 'crossing', 'range', 'degenerate', 'culled')
F32 = np.float32


def camera(h, w, focal, c2w=None, pp=None):
    """one camera row (identity pose: looking down -z, y up; the principal point at the picture's centre)"""
    ppx, ppy = ((w - 1) / 2.0, (h - 1) / 2.0) if pp is None else pp
    return camera_ref.row(np.eye(4) if c2w is None else c2w, focal, ppx, ppy, h, w)


def _setup(cam, vertices, triangles, znear, cull, dtype):
    """project, cull, snap: rules 1-6 of the header for one camera -> why [T] (1 drawn, 2 .. 7 the culls), X, Y int64 [T,3]
    (float32 route whatever `dtype`: the snap is part of the definition), z [T,3] in `dtype`"""
    cam = np.asarray(cam, np.float32).reshape(1, -1)
    vertices = np.asarray(vertices, np.float32).reshape(-1, 3)
    tri = np.asarray(triangles, np.int64).reshape(-1, 3)
    V, T = vertices.shape[0], tri.shape[0]
    ok_id = ((tri >= 0) & (tri < V)).all(1) if T else np.zeros(0, bool)
    P32 = vertices[np.clip(tri, 0, max(V - 1, 0))] if V else np.zeros((T, 3, 3), np.float32)
    with np.errstate(all='ignore'):
        pc = camera_ref.to_camera(cam, P32[None], np.float32)
        finite = np.isfinite(P32).all(2) & np.isfinite(pc[0]).all(2)
        valid = ok_id & finite.all(1)
        z = -pc[0, ..., 2]
        xy = camera_ref.pixel(cam, pc, z[None], np.float32)[0]
        x, y = xy[..., 0], xy[..., 1]
        near = (z < F32(znear)).sum(1)
        sx, sy = F32(SUB) * x, F32(SUB) * y
        rng = (~(np.abs(sx) <= F32(MAX_COORD)) | ~(np.abs(sy) <= F32(MAX_COORD))).any(1)
        snap = valid[:, None] & ~rng[:, None] & np.isfinite(sx) & np.isfinite(sy)
        X = np.where(snap, np.rint(np.where(snap, sx, 0)), 0).astype(np.int64)
        Y = np.where(snap, np.rint(np.where(snap, sy, 0)), 0).astype(np.int64)
        z_out = z if dtype == np.float32 else -camera_ref.to_camera(cam, P32[None], np.float64)[0, ..., 2]
    A2 = (X[:, 1] - X[:, 0]) * (Y[:, 2] - Y[:, 0]) - (Y[:, 1] - Y[:, 0]) * (X[:, 2] - X[:, 0])
    why = np.full(T, 1)
    why[(cull == 1) & (A2 > 0) | (cull == 2) & (A2 < 0)] = 7
    why[A2 == 0] = 6
    why[rng] = 5
    why[near > 0] = 4
    why[near == 3] = 3
    why[~valid] = 2                         # (assigned last: the first rule that applies wins)
    return why, X, Y, z_out, A2


def _bounds(X, Y, h, w):
    x0, x1 = max(-(-int(X.min()) // SUB), 0), min(int(X.max()) // SUB, w - 1)
    y0, y1 = max(-(-int(Y.min()) // SUB), 0), min(int(Y.max()) // SUB, h - 1)
    return x0, x1, y0, y1


def _coverage(X, Y, A2, x0, x1, y0, y1):
    """vertices already exchanged so that A2 > 0 -> (E [3] int64 arrays over the bounds, covered)"""
    cx = (np.arange(x0, x1 + 1, dtype=np.int64) * SUB)[None, :]
    cy = (np.arange(y0, y1 + 1, dtype=np.int64) * SUB)[:, None]
    E, cov = [], True
    for e in range(3):
        a, b = (e + 1) % 3, (e + 2) % 3
        dX, dY = int(X[b] - X[a]), int(Y[b] - Y[a])
        Ee = dX * (cy - int(Y[a])) - dY * (cx - int(X[a]))
        allow = dY > 0 or (dY == 0 and dX < 0)
        cov = cov & ((Ee > 0) | ((Ee == 0) & allow))
        E.append(Ee)
    assert ((E[0] + E[1] + E[2]) == A2).all()
    return E, cov


def _draw(cams, h, w, vertices, triangles, znear, cull, dtype):
    cams = np.asarray(cams, np.float32).reshape(-1, camera_ref.FLOATS)
    triangles = np.asarray(triangles, np.int64).reshape(-1, 3)
    F, T = cams.shape[0], triangles.shape[0]
    tri = np.full((F, h, w), -1, np.int32)
    depth = np.zeros((F, h, w), dtype)
    second = np.full((F, h, w), np.inf)                      # draw64: the depth of the next candidate
    bary = np.zeros((F, h, w, 3), dtype)
    cover = np.zeros((F, h, w), np.int64)                    # how many triangles cover each pixel
    counts = np.zeros(len(COUNT_FIELDS), np.int64)
    key = np.full((F, h, w), np.iinfo(np.uint64).max, np.uint64) if dtype == np.float32 else None
    one = dtype(1)
    for f in range(F):
        why, X, Y, z, A2 = _setup(cams[f], vertices, triangles, znear, cull, dtype)
        for c in range(1, 8):
            counts[c] += int((why == c).sum())
        for t in np.nonzero(why == 1)[0]:
            x0, x1, y0, y1 = _bounds(X[t], Y[t], h, w)
            if x0 > x1 or y0 > y1:
                continue
            counts[0] += (x1 // TILE - x0 // TILE + 1) * (y1 // TILE - y0 // TILE + 1)
            order = [0, 2, 1] if A2[t] < 0 else [0, 1, 2]
            E, cov = _coverage(X[t][order], Y[t][order], abs(int(A2[t])), x0, x1, y0, y1)
            if not cov.any():
                continue
            with np.errstate(all='ignore'):
                area = dtype(abs(int(A2[t])))
                wz = [(E[e].astype(dtype) / area) * (one / z[t][order[e]]) for e in range(3)]
                dep = one / ((wz[0] + wz[1]) + wz[2])
                q = [wz[e] * dep for e in range(3)]
            win = (slice(f, f + 1), slice(y0, y1 + 1), slice(x0, x1 + 1))
            cover[win][0][cov] += 1
            if dtype == np.float32:
                k = (dep.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.uint64(t)
                upd = cov & (k < key[win][0])
                key[win][0][upd] = k[upd]
            else:
                d0, t0 = depth[win][0], tri[win][0]
                s0 = second[win][0]
                upd = cov & ((t0 < 0) | (dep < d0))           # (t ascends: an equal depth keeps the lower id)
                lose = cov & ~upd
                s0[upd & (t0 >= 0)] = d0[upd & (t0 >= 0)]
                s0[lose] = np.minimum(s0[lose], dep[lose])
            tri[win][0][upd] = t
            depth[win][0][upd] = dep[upd]
            for e in range(3):
                bary[win][0][..., order[e]][upd] = q[e][upd]
    return dict(tri=tri, depth=depth, bary=bary, counts=counts.astype(np.int32), cover=cover, second=second)


def draw32(cams, h, w, vertices, triangles, znear, cull=0):
    """-> dict tri int32 [F,h,w], depth float32 [F,h,w], bary float32 [F,h,w,3], counts int32 [8] (COUNT_FIELDS), cover
    int64 [F,h,w]: the number of triangles covering each pixel"""
    out = _draw(cams, h, w, vertices, triangles, znear, cull, np.float32)
    del out['second']
    return out


def draw64(cams, h, w, vertices, triangles, znear, cull=0):
    """-> dict tri, depth float64, bary float64, counts, cover, gap [F,h,w]: (second - depth) / depth of the nearest two
    candidates (inf with fewer than two)"""
    out = _draw(cams, h, w, vertices, triangles, znear, cull, np.float64)
    with np.errstate(all='ignore'):
        out['gap'] = np.where(out['tri'] >= 0, (out.pop('second') - out['depth']) / out['depth'], np.inf)
    return out


def gamma(cams, vertices, triangles):
    """max over frames and referenced vertices with z > 0 of sum_j |R_c[j][2] d_j| / z in float64: how much the projection's
    cancellation magnifies its roundings in z"""
    cams = np.asarray(cams, np.float64).reshape(-1, camera_ref.FLOATS)
    P = np.asarray(vertices, np.float64)[np.unique(np.asarray(triangles).reshape(-1))]
    g = 0.0
    for c in cams:
        d = P - c[[3, 7, 11]]
        terms = d * c[[2, 6, 10]]
        z = -terms.sum(1)
        ok = z > 0
        g = max(g, float((np.abs(terms).sum(1)[ok] / z[ok]).max()))
    return g


# ---- scenes ----------------------------------------------------------------------------------------------------------------------
def random_scene(seed=0, n=2000, stacked=600, h=48, w=64):
    """n small random triangles in front of three cameras of h x w, `stacked` of them over the pixels of tile (1, 1) of the first
    camera at different depths -> (cams: 3 rows, vertices [3n,3], triangles [n,3])"""
    rng = np.random.default_rng(seed)
    focal = 64.0
    cams = np.stack([camera(h, w, focal),
                     camera(h, w, focal, look_at((0.9, 0.2, 0.3), (0.0, 0.0, -4.0))),
                     camera(h, w, 48.0, look_at((-1.2, -0.4, 0.5), (0.2, 0.0, -4.0)), pp=(w / 2.0 - 0.25, h / 2.0 + 0.125))])
    z = rng.uniform(2.5, 6.0, n)
    # centres as camera 0 sees them: anywhere on (and a little off) the frame; the stacked ones inside tile (1, 1)
    px = rng.uniform(-4.0, w + 3.0, n)
    py = rng.uniform(-4.0, h + 3.0, n)
    px[:stacked] = rng.uniform(TILE + 2.0, 2 * TILE - 3.0, stacked)
    py[:stacked] = rng.uniform(TILE + 2.0, 2 * TILE - 3.0, stacked)
    centre = np.stack([(px - cams[0, 13]) / focal * z, -(py - cams[0, 14]) / focal * z, -z], 1)
    size = rng.uniform(0.5, 4.0, n)[:, None, None] * (z / focal)[:, None, None]          # half a pixel to four pixels
    corners = centre[:, None, :] + size * rng.normal(size=(n, 3, 3)) * np.array([1.0, 1.0, 0.5])
    vertices = corners.reshape(-1, 3).astype(np.float32)
    triangles = np.arange(3 * n, dtype=np.int32).reshape(n, 3)
    return cams, vertices, triangles


def fan(x0, y0, x1, y1, cx, cy, n_edge, z=-4.0):
    """the rectangle [x0, x1] x [y0, y1] (picture coordinates of camera(h, w, focal) at depth -z, see to_world) as a fan of
    triangles around (cx, cy), n_edge boundary segments per side -> (points [m,2] picture coordinates, triangles)"""
    xs, ys = np.linspace(x0, x1, n_edge + 1), np.linspace(y0, y1, n_edge + 1)
    ring = [(x, y0) for x in xs[:-1]] + [(x1, y) for y in ys[:-1]] + [(x, y1) for x in xs[:0:-1]] + [(x0, y) for y in ys[:0:-1]]
    pts = np.array([(cx, cy)] + ring, np.float64)
    m = len(ring)
    tris = np.array([(0, 1 + i, 1 + (i + 1) % m) for i in range(m)], np.int32)
    return pts, tris


def grid(x0, y0, x1, y1, nx, ny, flip_every=2):
    """the rectangle as nx x ny cells of two triangles each, the diagonal alternating -> (points [m,2], triangles)"""
    xs, ys = np.linspace(x0, x1, nx + 1), np.linspace(y0, y1, ny + 1)
    pts = np.array([(x, y) for y in ys for x in xs], np.float64)
    tris = []
    for j in range(ny):
        for i in range(nx):
            a, b, c, d = j * (nx + 1) + i, j * (nx + 1) + i + 1, (j + 1) * (nx + 1) + i + 1, (j + 1) * (nx + 1) + i
            tris += [(a, b, c), (a, c, d)] if (i + j) % flip_every else [(a, b, d), (b, c, d)]
    return pts, np.array(tris, np.int32)


def to_world(cam, pts, z):
    """picture coordinates at camera depth z -> world points for a camera with identity rotation: exact in float32 when the
    focal length and z are powers of two and the coordinates are multiples of 2^-8"""
    cam = np.asarray(cam, np.float64)
    pts = np.asarray(pts, np.float64)
    z = np.broadcast_to(np.asarray(z, np.float64), pts.shape[:1])
    focal, ppx, ppy = cam[camera_ref.FOCAL], cam[camera_ref.PPX], cam[camera_ref.PPY]
    return np.stack([(pts[:, 0] - ppx) / focal * z + cam[3], -(pts[:, 1] - ppy) / focal * z + cam[7], -z + cam[11]], 1).astype(np.float32)
