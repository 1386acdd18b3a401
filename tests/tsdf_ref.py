"""Oracles of include/durf_tsdf.h in NumPy, every voxel at once, frame after frame.

    integrate32   np.float32 arithmetic in exactly the order the header states: what libdurf_tsdf.so must reproduce bit for bit
                  (every NumPy ufunc is one rounding: nothing is fused).  Also `why` [F,n]: 0 where the pair updated, else the
                  number of the skip rule.
    lattice32, sample32   likewise.
    integrate64   the same rules in float64 on the same float32 inputs, and per (frame, voxel) pair the MARGIN of every
                  decision that was taken: the distance of x and y from a rounding boundary (in pixels), of z from znear, of
                  sdf from -trunc and from +trunc (in scene units).  A pair whose margins are large decides alike in both.

Scenes shared by the host and the device tests: ring_cameras(), sphere_depth() (a sphere standing on a plane, analytic camera
depth), holes(), random_extras() and random_scene()."""
import numpy as np

from tests import camera_ref
from tests.lattice_ref import frame_of, inverse_of, points as voxels  # noqa: F401  (the lattice is lattice_ref's)
from tests.raster_ref import camera, look_at  # noqa: F401  (the camera rows are the rasteriser's)
from tests.trimesh_ref import icosphere  # noqa: F401  (the same sphere bit for bit; box_mesh below numbers its vertices its own way and stays)

F32 = np.float32
MAX_COORD = float(1 << 20)
RULES = ('updated', 'invalid', 'behind', 'range', 'outside', 'hole', 'faint', 'occluded', 'other', 'weight')


def new_state(shape, colour=True):
    n = int(np.prod(shape))
    return dict(tsdf=np.zeros(n, F32), weight=np.zeros(n, F32), colour=np.zeros((n, 4), F32) if colour else None)


def _integrate(dtype, state, frame, shape, cams, depth, trunc, acc, min_acc, rgb, label, select, other_mode, xform, frame_weight,
               max_weight, znear, margins):
    cams = np.asarray(cams, F32).reshape(-1, camera_ref.FLOATS)
    depth = np.asarray(depth, F32)
    F, h, w = depth.shape
    T = dtype
    P = voxels(frame, shape, T)
    n = P.shape[0]
    D, W = state['tsdf'].astype(T).copy(), state['weight'].astype(T).copy()
    col = None if state.get('colour') is None else state['colour'].astype(T).copy()
    keep_colour = col is not None and rgb is not None
    why = np.zeros((F, n), np.int8)
    margin = np.full((F, n, 5), np.inf) if margins else None                # x, y, z - znear, sdf + trunc, sdf - trunc
    trunc_, maxw, zn = T(F32(trunc)), T(F32(max_weight)), T(F32(znear))
    with np.errstate(all='ignore'):
        for f in range(F):
            c = cams[f].astype(T)
            if xform is not None:
                M = np.asarray(xform, F32)[f].astype(T)
                X = np.stack([((M[r, 0] * P[:, 0] + M[r, 1] * P[:, 1]) + M[r, 2] * P[:, 2]) + M[r, 3] for r in range(3)], 1)
            else:
                X = P
            pcs = camera_ref.to_camera(c[None], X[None], T)
            pc = [pcs[0, :, j] for j in range(3)]
            y_ = np.zeros(n, np.int8)                                        # the rule that stopped the pair; 0: none yet
            live = np.ones(n, bool)

            def stop(cond, rule):
                nonlocal live
                hit = live & cond
                y_[hit] = rule
                live = live & ~cond
            stop(~(np.isfinite(X).all(1) & np.isfinite(pc[0]) & np.isfinite(pc[1]) & np.isfinite(pc[2])), 1)
            z = -pc[2]
            if margins:
                margin[f, live, 2] = np.abs(z - zn)[live]
            stop(~(z >= zn), 2)
            x, y = np.moveaxis(camera_ref.pixel(c[None], pcs, z[None], T)[0], -1, 0)
            stop(~(np.abs(x) <= T(MAX_COORD)) | ~(np.abs(y) <= T(MAX_COORD)), 3)
            xs, ys = np.where(live, x, T(0)), np.where(live, y, T(0))
            if margins:
                margin[f, live, 0] = np.abs(xs - np.floor(xs) - 0.5)[live]
                margin[f, live, 1] = np.abs(ys - np.floor(ys) - 0.5)[live]
            px, py = np.rint(xs).astype(np.int64), np.rint(ys).astype(np.int64)
            stop((px < 0) | (px >= w) | (py < 0) | (py >= h), 4)
            pxs, pys = np.where(live, px, 0), np.where(live, py, 0)
            dep = depth[f, pys, pxs].astype(T)
            stop(~np.isfinite(dep) | ~(dep > 0), 5)
            if acc is not None:
                stop(~(np.asarray(acc, F32)[f, pys, pxs] >= F32(min_acc)), 6)
            sdf = dep - z
            if margins:
                margin[f, live, 3] = np.abs(sdf + trunc_)[live]
                margin[f, live, 4] = np.abs(sdf - trunc_)[live]
            stop(sdf < -trunc_, 7)
            mine = np.ones(n, bool)
            if label is not None:
                mine = np.asarray(label)[f, pys, pxs] == int(select)
                stop(~mine & (np.ones(n, bool) if other_mode == 0 else ~(sdf >= trunc_)), 8)
            wf = T(F32(1.0) if frame_weight is None else np.asarray(frame_weight, F32)[f])
            stop(np.full(n, not (np.isfinite(wf) and wf > 0)), 9)
            why[f] = y_
            u = live
            dn = np.minimum(sdf[u] / trunc_, T(1))
            Wn = W[u] + wf
            D[u] = (W[u] * D[u] + wf * dn) / Wn
            W[u] = np.minimum(Wn, maxw)
            if keep_colour:
                cu = live & mine & (sdf <= trunc_)
                q = np.asarray(rgb, F32)[f, pys[cu], pxs[cu]].astype(T)
                Wc = col[cu, 3]
                Wcn = Wc + wf
                for ch in range(3):
                    col[cu, ch] = (Wc * col[cu, ch] + wf * q[:, ch]) / Wcn
                col[cu, 3] = np.minimum(Wcn, maxw)
    out = dict(tsdf=D, weight=W, colour=col, why=why, tally=np.bincount(why.reshape(-1), minlength=len(RULES)))
    if margins:
        out['margin'] = margin
    return out


def integrate32(state, frame, shape, cams, depth, trunc, acc=None, min_acc=0.5, rgb=None, label=None, select=0, other_mode=0, xform=None,
                frame_weight=None, max_weight=64.0, znear=1e-2):
    """-> dict tsdf [n], weight [n], colour [n,4] or None (float32: the new state; `state` is left as it is), why int8 [F,n], tally"""
    return _integrate(F32, state, frame, shape, cams, depth, trunc, acc, min_acc, rgb, label, select, other_mode, xform, frame_weight,
                      max_weight, znear, False)


def integrate64(state, frame, shape, cams, depth, trunc, acc=None, min_acc=0.5, rgb=None, label=None, select=0, other_mode=0, xform=None,
                frame_weight=None, max_weight=64.0, znear=1e-2):
    """the same in float64, plus margin [F,n,5]: |frac(x) - 0.5|, |frac(y) - 0.5| (pixels), |z - znear|, |sdf + trunc|, |sdf - trunc|
    (scene units); inf where the pair stopped before the decision was taken"""
    return _integrate(np.float64, state, frame, shape, cams, depth, trunc, acc, min_acc, rgb, label, select, other_mode, xform, frame_weight,
                      max_weight, znear, True)


def lattice32(state, min_weight=1.0):
    """-> density [n] = -D, valid uint8 [n], rgb [n,3] (None without colour)"""
    col = state.get('colour')
    rgb = None if col is None else np.where(col[:, 3:4] > 0, col[:, :3], F32(0)).astype(F32)
    return (-state['tsdf']).astype(F32), (state['weight'] >= F32(min_weight)).astype(np.uint8), rgb


def _lerp(a, b, t):
    return a + t * (b - a)


def sample32(state, frame, shape, trunc, points, min_weight=1.0):
    """-> sdf [m] float32 (NaN where not ok), ok uint8 [m], rgb [m,3] (None without colour)"""
    nu, nv, nw = shape
    dims = (nu, nv, nw)
    P = np.asarray(points, F32).reshape(-1, 3)
    m = P.shape[0]
    o, inv = np.asarray(frame['origin'], F32), inverse_of(frame)
    Dv, Wv = state['tsdf'].reshape(-1), state['weight'].reshape(-1)
    col = state.get('colour')
    with np.errstate(all='ignore'):
        e = [P[:, c] - o[c] for c in range(3)]
        q = [(inv[c, 0] * e[0] + inv[c, 1] * e[1]) + inv[c, 2] * e[2] for c in range(3)]
        inside = np.ones(m, bool)
        for c in range(3):
            inside &= np.isfinite(q[c]) & (q[c] >= 0) & (q[c] <= F32(dims[c] - 1))
        cell = [np.minimum(np.floor(np.where(inside, q[c], F32(0))).astype(np.int64), dims[c] - 2) for c in range(3)]
        t = [(np.where(inside, q[c], F32(0)) - cell[c].astype(F32)).astype(F32) for c in range(3)]
        idx = [((cell[0] + (a >> 2)) * nv + (cell[1] + ((a >> 1) & 1))) * nw + (cell[2] + (a & 1)) for a in range(8)]

        def tri(vals):
            v00, v01 = _lerp(vals[0], vals[1], t[2]), _lerp(vals[2], vals[3], t[2])
            v10, v11 = _lerp(vals[4], vals[5], t[2]), _lerp(vals[6], vals[7], t[2])
            return _lerp(_lerp(v00, v01, t[1]), _lerp(v10, v11, t[1]), t[0])
        ok = inside.copy()
        for a in range(8):
            ok &= Wv[idx[a]] >= F32(min_weight)
        sdf = np.where(ok, tri([Dv[idx[a]] for a in range(8)]) * F32(trunc), F32(np.nan)).astype(F32)
        rgb = None
        if col is not None:
            has = inside.copy()
            for a in range(8):
                has &= col[idx[a], 3] > 0
            rgb = np.stack([np.where(has, tri([col[idx[a], ch] for a in range(8)]), F32(0)) for ch in range(3)], 1).astype(F32)
    return sdf, ok.astype(np.uint8), rgb


# ---- scenes ---------------------------------------------------------------------------------------------------------------------
def ring_cameras(F, h, w, focal, radius=4.0, height=1.0, target=(0.0, 0.0, 0.0), phase=0.1):
    """F cameras on a ring around `target`, looking at it -> [F] camera rows"""
    rows = []
    for f in range(F):
        a = phase + 2.0 * np.pi * f / F
        eye = np.array([radius * np.sin(a), height, radius * np.cos(a)]) + np.asarray(target, np.float64)
        rows.append(camera(h, w, focal, look_at(eye, target)))
    return np.stack(rows)


def sphere_depth(cams, h, w, radius=1.0, centre=(0.0, 0.0, 0.0), plane=True):
    """the analytic camera depth [F,h,w] float32 of a sphere standing on the plane y = centre_y - radius (0 where a ray meets
    neither).  The rays are durf_camera_rays': direction ((px - ppx) / focal, -(py - ppy) / focal, -1) in the camera, so the
    ray parameter IS the camera depth."""
    cams = np.asarray(cams, np.float64).reshape(-1, camera_ref.FLOATS)
    ctr = np.asarray(centre, np.float64)
    out = np.zeros((cams.shape[0], h, w))
    py, px = np.mgrid[0:h, 0:w].astype(np.float64)
    for f, c in enumerate(cams):
        o, d = camera_ref.rays(c, px, py)
        oc = o - ctr
        A, B, C = (d * d).sum(-1), 2.0 * (d @ oc), oc @ oc - radius * radius
        disc = B * B - 4.0 * A * C
        with np.errstate(all='ignore'):
            t = np.where(disc >= 0, (-B - np.sqrt(np.maximum(disc, 0.0))) / (2.0 * A), np.inf)
            t = np.where(t > 0, t, np.inf)
            if plane:
                tp = (ctr[1] - radius - o[1]) / d[..., 1]
                t = np.minimum(t, np.where(tp > 0, tp, np.inf))
        out[f] = np.where(np.isfinite(t), t, 0.0)
    return out.astype(F32)


def holes(depth, rng, fraction=0.05):
    """a copy of depth with `fraction` of its pixels replaced by 0, NaN, inf and a negative value, in equal parts"""
    d = np.array(depth, F32)
    bad = rng.random(d.shape) < fraction
    kind = rng.integers(0, 4, d.shape)
    for i, v in enumerate((0.0, np.nan, np.inf, -1.5)):
        d[bad & (kind == i)] = v
    return d


def rigid(rng, angle=0.3, shift=0.2):
    """a random rigid map [3,4]: a rotation by up to `angle` about a random axis, and a translation"""
    ax = rng.normal(size=3)
    ax /= np.linalg.norm(ax)
    a = rng.uniform(-angle, angle)
    S = np.array([[0.0, -ax[2], ax[1]], [ax[2], 0.0, -ax[0]], [-ax[1], ax[0], 0.0]])
    R = np.eye(3) + np.sin(a) * S + (1.0 - np.cos(a)) * (S @ S)
    return np.concatenate([R, rng.uniform(-shift, shift, (3, 1))], 1)


def random_extras(rng, F, h, w, labels=3):
    """acc, rgb, label, frame_weight and xform for F frames of h x w: every optional input of durf_tsdf_integrate"""
    return dict(acc=rng.random((F, h, w)).astype(F32), rgb=rng.random((F, h, w, 3)).astype(F32),
                label=rng.integers(-1, labels, (F, h, w)).astype(np.int32), frame_weight=rng.uniform(0.5, 2.0, F).astype(F32),
                xform=np.stack([rigid(rng) for _ in range(F)]).astype(F32))


def random_scene(seed, F=6, h=48, w=64, shape=(14, 12, 13), step=0.25, focal=52.0):
    """the sphere on its plane seen from a ring, with holes, and a lattice around it -> dict frame, shape, trunc, cams, depth and
    the extras of random_extras (the label is mostly 1 with patches of others, so that both label rules occur)"""
    rng = np.random.default_rng(seed)
    cams = ring_cameras(F, h, w, focal, radius=4.0 + 0.3 * rng.random(), height=1.0 + 0.5 * rng.random(), phase=rng.random())
    depth = holes(sphere_depth(cams, h, w), rng)
    ex = random_extras(rng, F, h, w)
    ex['label'] = np.where(rng.random((F, h, w)) < 0.8, 1, ex['label']).astype(np.int32)
    ex['xform'] = np.stack([rigid(rng, 0.05, 0.05) for _ in range(F)]).astype(F32)
    origin = [-(n - 1) * step / 2.0 + 0.01 * rng.normal() for n in shape]
    return dict(frame=frame_of(origin, step), shape=tuple(shape), trunc=3.0 * step, cams=cams, depth=depth, **ex)


def six_cameras(h, w, focal, dist, target=(0.0, 0.0, 0.0)):
    """one camera on each half axis at `dist`, looking at `target` -> 6 camera rows"""
    rows = []
    for ax in range(3):
        for s in (1.0, -1.0):
            eye = np.asarray(target, np.float64).copy()
            eye[ax] += s * dist
            rows.append(camera(h, w, focal, look_at(eye, target, up=(0.0, 0.0, 1.0) if ax == 1 else (0.0, 1.0, 0.0))))
    return np.stack(rows)


EDGES = [(0, 0, 1), (0, 1, 0), (0, 1, 1), (1, 0, 0), (1, 0, 1), (1, 1, 0), (1, 1, 1)]        # durf_mesh.h's seven edges of a point


def crossings(D, W, P, shape, min_weight=1.0):
    """where the zero level meets the lattice edges mesh.surface puts vertices on: both ends observed (W >= min_weight), exactly
    one of them in (-D >= 0); the point at t = (0 - d_a) / (d_b - d_a) with d = -D -> [m,3] float64"""
    shape = tuple(shape)
    D, W, P = np.asarray(D, np.float64).reshape(shape), np.asarray(W).reshape(shape), np.asarray(P, np.float64).reshape(shape + (3,))
    pts = []
    for e in EDGES:
        sa, sb = tuple(slice(0, s - o) for s, o in zip(shape, e)), tuple(slice(o, None) for o in e)
        a, b = D[sa], D[sb]
        ok = (W[sa] >= min_weight) & (W[sb] >= min_weight) & ((-a >= 0) != (-b >= 0))
        t = a[ok] / (a[ok] - b[ok])
        pts.append(P[sa][ok] + t[:, None] * (P[sb][ok] - P[sa][ok]))
    return np.concatenate(pts)


def box_mesh(half):
    """the box |P_c| <= half_c as twelve triangles wound outward -> (vertices [8,3] float32, triangles [12,3] int32)"""
    hx, hy, hz = (float(x) for x in half)
    v = np.array([(sx * hx, sy * hy, sz * hz) for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], F32)       # index 4 a + 2 b + c
    q = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]                       # -x +x -y +y -z +z
    t = [(a, b, c) for a, b, c, d in q] + [(a, c, d) for a, b, c, d in q]
    return v, np.asarray(t, np.int32)


def box_surface_distance(P, half):
    """the distance of points [m,3] to the surface of the box |P_c| <= half_c (float64)"""
    d = np.abs(np.asarray(P, np.float64)) - np.asarray(half, np.float64)
    outside = np.linalg.norm(np.maximum(d, 0.0), axis=1)
    inside = np.minimum(d.max(1), 0.0)
    return np.abs(outside + inside)
