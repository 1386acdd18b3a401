"""include/durf_field.h restated for the CPU: the field at world points.  The truth is composed from oracle.durf_ref
(new_space, integrated_pos_enc, weighted_ipe, mlp_apply, pos_enc) in float64 under tests.enc_rows_ref._reference_wrap() -- safe_sin
with the float32-rounded period, the cosine half at fl32(y + fl32(pi/2)) --; the box test and the grid are numpy restatements
written from the header.  Every function takes `dt`: float64 is the oracle, float32 its twin, the header's operations in the
header's order in float32, which says what fp32 in that order costs on a given input.  Inputs are the fp32 values the library
is handed; both evaluate on exactly those.  tests/test_field_host.py pins it without a device, tests/test_gpu_field.py uses it
on one.

The contraction is the reference's (internal/mip360.py:47-60, oracle.durf_ref.contract): it switches at norm 0.1, not at 1.

Yardstick: the twin's distances from the truth (YARDSTICK, written by `python -m tests.field_ref`, held to a fresh run by
tests/test_field_host.py):
  local        the box-frame point of the planted classification set, in ulp32 of the largest |X_j - c_j|:      2.61
  act density  softplus(raw + bias), relative, raw in [-40, 40] (the rounding of raw + bias at 40, through exp):  2.1e-06
  act rgb      sigmoid(raw), absolute:                                                                          8.8e-08
  encoding     per label, over twin_cloud(), (dx in ulp32 of max(|x|, 1), relative dvar), plain | contracted:
      origin      (0.00, 4.3e-08) | (0.00, 4.3e-08)
      n05         (0.00, 4.3e-08) | (2.09, 6.5e-04)
      n1_lo       (0.00, 4.3e-08) | (0.72, 9.6e-07)
      n1          (0.00, 4.3e-08) | (0.50, 8.2e-07)
      n1_hi       (0.00, 4.3e-08) | (0.99, 7.4e-07)
      n2          (0.00, 4.3e-08) | (1.24, 1.9e-06)
      n1e3        (0.00, 4.3e-08) | (2.25, 1.9e-05)
      n1e6        (0.00, 4.3e-08) | (1.86, 1.2e-04)
      switch_lo   (0.00, 4.3e-08) | (1.89, 1.7e-04)
      switch_hi   (0.00, 4.3e-08) | (2.34, 2.9e-04)
(plain: the object rows and the background rows without DURF_ENC_CONTRACT: x is the input itself, var one fp32 product.)"""
import math

import numpy as np
import torch

from oracle import durf_ref as R
from tests import enc_rows_ref as E
from tests import flow_ref as FR

F32, F64 = np.float32, np.float64
SIGMAS = (0.0, 1e-3, 0.1, 10.0)
SIZES = (1, 63, 64, 65, 257)
MARGIN = 1e-2


def _a(x, dt):
    return np.asarray(np.asarray(x, F32), dt)


def _tdt(dt):
    return torch.float64 if dt in (F64, torch.float64) else torch.float32


def ulp32(v):
    """spacing of float32 at |v| (numpy float64 in and out)"""
    a = np.maximum(np.abs(np.asarray(v, F64)), 2.0 ** -126)
    return np.exp2(np.floor(np.log2(a)) - 23)


# ---- which box ----------------------------------------------------------------------------------------------------------------
def classify(points, pose, ext, enable=None, inside_tol=0.0, dt=F64, exact=False):
    """-> dict: owner [n] int32 (-1 none, -2 several), local [n,3] (P of the owner, else X), P [n,K,3], inside [n,K] bool,
    margin [n]: the least | |P_j| / (ext_kj (1 + tol)) - 1 | over the enabled boxes and axes (inf for K = 0), dscale [n,K]: the
    largest |X_j - c_j| (the unit of the twin's distance).  exact: the points are float64 values taken as they are (the
    semantics pin against the oracle's model, whose samples are not fp32 values)"""
    X = np.asarray(points, F64).reshape(-1, 3) if exact else _a(points, dt).reshape(-1, 3)
    n = X.shape[0]
    pose = np.zeros((0, 6), F32) if pose is None else np.asarray(pose, F32).reshape(-1, 6)
    K = pose.shape[0]
    ext = _a(ext, dt).reshape(-1, 3) if K else np.zeros((0, 3), dt)
    en = np.ones(K, bool) if enable is None else np.asarray(enable).reshape(-1) != 0
    grow = dt(1) + dt(F32(inside_tol))
    P = np.zeros((n, K, 3), dt)
    inside = np.zeros((n, K), bool)
    margin = np.full(n, np.inf)
    dscale = np.zeros((n, K))
    for k in range(K):
        Rm, c = FR.aa2matrix(pose[k, 3:], dt), _a(pose[k, :3], dt)
        d = [X[:, j] - c[j] for j in range(3)]
        for i in range(3):
            P[:, k, i] = (Rm[i, 0] * d[0] + Rm[i, 1] * d[1]) + Rm[i, 2] * d[2]
        dscale[:, k] = np.max(np.abs(np.stack(d, 1)), 1)
        if not en[k]:
            continue
        lim = ext[k] * grow
        inside[:, k] = (np.abs(P[:, k]) <= lim).all(1)
        margin = np.minimum(margin, np.abs(np.abs(P[:, k]).astype(F64) / lim.astype(F64) - 1).min(1))
    nin = inside.sum(1)
    last = np.where(inside.any(1), K - 1 - np.argmax(inside[:, ::-1], 1), -1) if K else np.full(n, -1)
    owner = np.where(nin == 0, -1, np.where(nin == 1, last, -2)).astype(np.int32)
    local = X.copy()
    sel = owner >= 0
    local[sel] = P[sel, owner[sel]]
    return dict(owner=owner, local=local, P=P, inside=inside, margin=margin, dscale=dscale)


def lists(owner, K):
    """the stable partition durf_field_lists computes -> (list of K + 1 index arrays; list K: owner -1)"""
    owner = np.asarray(owner)
    return [np.nonzero(owner == (c if c < K else -1))[0].astype(np.int32) for c in range(K + 1)]


# ---- the Gaussian and the two encodings ---------------------------------------------------------------------------------------
def gaussian(x, sigma, contraction, dt=F64, exact=False):
    """(x, var) [n,3] torch tensors as the encoder sees them: var = sigma * sigma (one fp32 product in the twin, the product of
    the fp32 sigma in float64 in the truth), new_space when `contraction`"""
    t = _tdt(dt)
    mean = torch.tensor(np.asarray(x, F64 if exact else F32)).to(t).reshape(-1, 1, 3)
    s = torch.tensor(F32(sigma)).to(t)
    cov = (s * s) * torch.eye(3, dtype=t).expand(mean.shape[0], 1, 3, 3)
    if contraction:
        mean, cov = R.new_space((mean, cov))
    return mean[:, 0], torch.diagonal(cov, dim1=-2, dim2=-1)[:, 0]


def _cov(var):
    return torch.diag_embed(var)[:, None]


def encode_bkgd(x, sigma, contraction, dt=F64, exact=False):
    """-> dict x, var [n,3], enc [n,60]"""
    m, v = gaussian(x, sigma, contraction, dt, exact)
    with E._reference_wrap():
        enc = R.integrated_pos_enc((m[:, None], _cov(v)), 0, 10)[:, 0]
    return dict(x=m, var=v, enc=enc)


def encode_obj(x, sigma, alpha, dt=F64, exact=False):
    """-> dict x, var [n,3], enc [n,63]"""
    m, v = gaussian(x, sigma, False, dt, exact)
    with E._reference_wrap():
        enc = R.weighted_ipe((m[:, None], _cov(v)), 0, 10, alpha)[:, 0]
    return dict(x=m, var=v, enc=enc)


def enc_bound(t, dxu, dvr, weights=None):
    """the per-feature budget [n,60] of encoding rows against the truth `t` (encode_*'s dict in float64), from the reference
    side only: 4 x (twin dx ulp32(max(|x|, 1)) cond_x + twin dvar cond_v) (tests.enc_rows_ref.conditioning) + 4 ulp32 of the feature +
    where the sine argument is wrapped (|y| >= T32) the rounding of the wrapped argument itself, e ulp32(T32): jnp.remainder
    in float32 adds the period to a negative remainder, half an ulp of up to 100 pi, and the product with e follows."""
    e, cx, cv, y = E.conditioning(t['x'], t['var'])
    ux = torch.tensor(ulp32(t['x'].abs().clamp(min=1.0).numpy()))[..., None, :].expand(*t['x'].shape[:-1], 10, 3).reshape(*t['x'].shape[:-1], 30)
    cond = 4 * (dxu * ux * cx + dvr * cv)
    yy = torch.cat([y, (y + E.HALF_PI32).float().double()], -1)
    ee = torch.cat([e, e], -1)
    wrap = (yy.abs() >= E.T32).double() * ee * float(ulp32(E.T32))
    w = torch.ones(60, dtype=torch.float64) if weights is None else weights
    feat = t['enc'][..., -60:].abs()
    return torch.cat([cond, cond], -1) * w + 4 * torch.tensor(ulp32(feat.numpy())) + wrap * w


# ---- MLPs, merge, activations -------------------------------------------------------------------------------------------------
def view_enc(viewdirs, dt=F64, exact=False):
    return R.pos_enc(torch.tensor(np.asarray(viewdirs, F64 if exact else F32)).to(_tdt(dt)), 0, 4, True)


def mlp(params, name, enc, view27):
    """the oracle MLP on encoding rows [n,F] -> raw [n,4] = (r, g, b, density)"""
    cfg = R.MLP_BKGD if name == 'MLP_0' else R.MLP_BOX
    rgb, dens = R.mlp_apply(params[name], enc[:, None], view27, cfg)
    return torch.cat([rgb[:, 0], dens[:, 0]], -1)


def activations(raw, density_bias, dt=F64):
    """(density [n], rgb [n,3]) of raw [n,4]: softplus(x) = max(x, 0) + log1p(exp(-|x|)), sigmoid(x) = 1 / (1 + exp(-x))"""
    r = np.asarray(np.asarray(raw), dt)
    x = r[:, 3] + dt(F32(density_bias))
    with np.errstate(over='ignore'):
        dens = np.maximum(x, dt(0)) + np.log1p(np.exp(-np.abs(x)))
        rgb = dt(1) / (dt(1) + np.exp(-r[:, :3]))
    return dens.astype(dt), rgb.astype(dt)


def query(params, points, viewdirs, pose, ext, enable=None, sigma=0.0, alpha=10.0, contraction=True, density_bias=-1.0,
          inside_tol=0.0, drop_const=False, exact=False):
    """the float64 field at points -> dict raw [n,4], density [n], rgb [n,3] (numpy; NaN where owner == -2), owner, valid.
    params: the oracle's tree in float64.  drop_const: leave the background's constant term out of object-owned points (a
    test's control: the wrong merge rule).  exact: float64 points and view directions as they are."""
    c = classify(points, pose, ext, enable, inside_tol, exact=exact)
    n, owner = c['owner'].shape[0], c['owner']
    K = 0 if pose is None else int(np.asarray(pose).reshape(-1, 6).shape[0])
    vd = np.zeros((n, 3), F64) if viewdirs is None else np.asarray(viewdirs, F64 if exact else F32)
    v27 = view_enc(vd, exact=exact)
    raw = torch.full((n, 4), float('nan'), dtype=torch.float64)
    with torch.no_grad():
        b = np.nonzero(owner == -1)[0]
        if b.size:
            raw[b] = mlp(params, 'MLP_0', encode_bkgd(c['local'][b], sigma, contraction, exact=exact)['enc'], v27[b])
        for k in range(K):
            o = np.nonzero(owner == k)[0]
            if not o.size:
                continue
            r = mlp(params, 'BoxMLP_%d' % k, encode_obj(c['local'][o], sigma, alpha, exact=exact)['enc'], v27[o])
            if not drop_const:
                r = r + mlp(params, 'MLP_0', encode_bkgd(np.zeros((o.size, 3), F32), 0.0, contraction)['enc'], v27[o])
            raw[o] = r
    dens, rgb = activations(raw.numpy(), density_bias)
    return dict(raw=raw.numpy(), density=dens, rgb=rgb, owner=owner, valid=(owner != -2).astype(np.uint8), local=c['local'])


# ---- grids and columns --------------------------------------------------------------------------------------------------------
def columns(density, valid, shape, step, threshold):
    """-> col_max [nu,nv] float32 (exact: a maximum of the inputs), sum [nu,nv] float64 of the counted densities, opacity
    float64 = 1 - exp(-step sum), first [nu,nv] int32"""
    nu, nv, nw = shape
    d = np.asarray(density, F32).reshape(nu, nv, nw)
    ok = (np.asarray(valid).reshape(nu, nv, nw) != 0) & ~np.isnan(d)
    cmax = np.where(ok.any(2), np.max(np.where(ok, d, -np.inf), 2), np.nan).astype(F32)
    s = np.where(ok, d.astype(F64), 0.0).sum(2)
    hit = ok & (d >= F32(threshold))
    first = np.where(hit.any(2), np.argmax(hit, 2), -1).astype(np.int32)
    return cmax, s, 1.0 - np.exp(-float(F32(step)) * s), first


# ---- the planted sets ---------------------------------------------------------------------------------------------------------
def scene():
    """K = 3 boxes: 0 and 1 overlap, 2 is switched off -> (pose [3,6], ext [3,3], enable [3]) float32 / int32"""
    pose = np.array([[0.40, -0.20, 0.10, 0.00, 0.70, 0.00],
                     [0.62, -0.15, 0.22, 0.30, -0.40, 0.20],
                     [-0.90, 0.50, -0.30, 0.00, 0.00, 1.20]], F32)
    ext = np.array([[0.20, 0.17, 0.45], [0.25, 0.15, 0.30], [0.22, 0.20, 0.18]], F32)
    return pose, ext, np.array([1, 1, 0], np.int32)


def _world(pose, P):
    return FR._to_world(FR.aa2matrix(pose[3:]), np.asarray(pose[:3], F64), np.asarray(P, F64).reshape(-1, 3))


def planted_points(n=SIZES[-1], seed=5):
    """-> (points [n,3] float32, tags): centres, 0.99 and 1.01 of each face along each axis, the overlap of boxes 0 and 1, the
    inside of the disabled box, then seeded points of the neighbourhood; every one at least MARGIN (relative to the half
    extent, to the rounding of a planted coordinate) from every enabled face.  The first n of one fixed list."""
    pose, ext, en = scene()
    pts, tags = [], []
    for k in range(3):
        pts.append(_world(pose[k], [0, 0, 0])[0]); tags.append('centre%d' % k)
    for k in range(3):
        for j in range(3):
            for s in (1, -1):
                for f in (0.99, 1.01):
                    P = np.array([0.31, -0.23, 0.17]) * ext[k]
                    P[j] = s * f * ext[k, j]
                    pts.append(_world(pose[k], P)[0]); tags.append('face%d' % k)
    both = 0.5 * (pose[0, :3].astype(F64) + pose[1, :3].astype(F64))
    for d in ((0, 0, 0), (0.01, -0.02, 0.015), (-0.015, 0.01, -0.01)):
        pts.append(both + np.array(d)); tags.append('overlap')
    for P in ((0.5, -0.5, 0.5), (-0.7, 0.2, 0.1)):
        pts.append(_world(pose[2], np.array(P) * ext[2])[0]); tags.append('disabled')
    rng = np.random.default_rng(seed)
    while len(pts) < 4 * n:
        pts.append(rng.uniform(-1.2, 1.2, 3)); tags.append('random')
    pts = np.asarray(pts, F32)
    c = classify(pts, pose, ext, en)
    keep = c['margin'] >= MARGIN - 1e-6
    planted = np.array([t != 'random' for t in tags])
    assert keep[planted].all(), 'a planted point sits within %g of a face' % MARGIN
    idx = np.nonzero(keep)[0][:n]
    assert idx.size == n
    return pts[idx], [tags[i] for i in idx]


def enc_points():
    """-> (points [m,3] float32, labels): the origin, |X| = 0.5, 1 -/+ 1e-3, exactly 1, 2, 1e3, 1e6, and one coordinate at the
    lane encoder's branch switch -/+ 1e-3, each along several directions and both signs"""
    u = np.array([0.6, -0.64, 0.48])
    out = [('origin', (0, 0, 0))]
    for label, r in (('n05', 0.5), ('n1_lo', 1 - 1e-3), ('n1_hi', 1 + 1e-3), ('n2', 2.0), ('n1e3', 1e3), ('n1e6', 1e6)):
        out += [(label, u * r), (label, -u * r), (label, (0, 0, -r)), (label, (r, 0, 0))]
    out += [('n1', (1, 0, 0)), ('n1', (0, -1, 0)), ('n1', (0, 0, 1))]
    for label, s in (('switch_lo', E.SWITCH - 1e-3), ('switch_hi', E.SWITCH + 1e-3)):
        out += [(label, (s, 0.3, -1.2)), (label, (0.3, -s, 0.7)), (label, (-0.2, 0.1, s))]
    return np.asarray([p for _, p in out], F32), [l for l, _ in out]


ENC_LABELS = ('origin', 'n05', 'n1_lo', 'n1', 'n1_hi', 'n2', 'n1e3', 'n1e6', 'switch_lo', 'switch_hi')


# ---- the twin's distances -----------------------------------------------------------------------------------------------------
def twin_local():
    pose, ext, en = scene()
    pts, _ = planted_points()
    a, b = classify(pts, pose, ext, en, dt=F64), classify(pts, pose, ext, en, dt=F32)
    assert (a['owner'] == b['owner']).all()
    unit = ulp32(np.maximum(a['dscale'], 2.0 ** -20))[:, :, None]
    return float((np.abs(b['P'].astype(F64) - a['P']) / unit).max())


def twin_act():
    raw = np.zeros((4001, 4), F32)
    raw[:, :] = np.linspace(-40, 40, 4001, dtype=F32)[:, None]
    d64, c64 = activations(raw, -1.0, F64)
    d32, c32 = activations(raw, -1.0, F32)
    return float((np.abs(d32 - d64) / d64).max()), float(np.abs(c32 - c64).max())


RADII = {'origin': 0.0, 'n05': 0.5, 'n1_lo': 1 - 1e-3, 'n1': 1.0, 'n1_hi': 1 + 1e-3, 'n2': 2.0, 'n1e3': 1e3, 'n1e6': 1e6}


def twin_cloud(cloud=256, seed=17):
    """the points the twin's encoding distance is measured on: enc_points() and, per label, `cloud` seeded points of the same
    class (the label's radius along random directions; the switch coordinate on a random axis beside random others) -- a
    handful of points says little about the rounding of a norm, a few hundred say what fp32 costs on the class"""
    pts, labels = enc_points()
    rng = np.random.default_rng(seed)
    more, ml = [], []
    for l in ENC_LABELS:
        if l == 'origin':
            continue
        for _ in range(cloud):
            if l in RADII:
                u = rng.normal(size=3)
                more.append(u / np.linalg.norm(u) * RADII[l])
            else:
                p = rng.uniform(-1.5, 1.5, 3)
                p[rng.integers(3)] = (E.SWITCH + (1e-3 if l == 'switch_hi' else -1e-3)) * rng.choice([-1, 1])
                more.append(p)
            ml.append(l)
    return np.concatenate([pts, np.asarray(more, F32)]), labels + ml


def twin_enc():
    """{(label, contracted): (dx in ulp32 of max(|x|, 1), relative dvar)}: the largest over the label's points of twin_cloud()
    and SIGMAS.  The floor of 1: 2 - 1/n cancels at n = 0.5, where the contracted point is 0 to rounding and its own ulp
    measures nothing."""
    pts, labels = twin_cloud()
    out = {}
    for con in (False, True):
        for sg in SIGMAS:
            x64, v64 = gaussian(pts, sg, con, F64)
            x32, v32 = gaussian(pts, sg, con, F32)
            x32, v32 = x32.double(), v32.double()
            dx = ((x32 - x64).abs() / torch.tensor(ulp32(torch.maximum(x64.abs(), x32.abs()).clamp(min=1.0).numpy()))).amax(-1)
            dx = torch.where((x32 == x64).all(-1), torch.zeros_like(dx), dx)
            assert bool((v32[v64 == 0] == 0).all())
            dv = torch.where(v64 != 0, (v32 - v64).abs() / v64.abs().clamp(min=1e-300), torch.zeros_like(v64)).amax(-1)
            for i, l in enumerate(labels):
                a, b = out.get((l, con), (0.0, 0.0))
                out[(l, con)] = (max(a, float(dx[i])), max(b, float(dv[i])))
    return out


# the twin's figures (see the module docstring), rounded UP to the digits shown
YARDSTICK = {
    'local': 2.61,
    'act': (2.1e-06, 8.8e-08),
    'enc': {
        ('origin', False): (0.00, 4.3e-08),
        ('origin', True): (0.00, 4.3e-08),
        ('n05', False): (0.00, 4.3e-08),
        ('n05', True): (2.09, 6.5e-04),
        ('n1_lo', False): (0.00, 4.3e-08),
        ('n1_lo', True): (0.72, 9.6e-07),
        ('n1', False): (0.00, 4.3e-08),
        ('n1', True): (0.50, 8.2e-07),
        ('n1_hi', False): (0.00, 4.3e-08),
        ('n1_hi', True): (0.99, 7.4e-07),
        ('n2', False): (0.00, 4.3e-08),
        ('n2', True): (1.24, 1.9e-06),
        ('n1e3', False): (0.00, 4.3e-08),
        ('n1e3', True): (2.25, 1.9e-05),
        ('n1e6', False): (0.00, 4.3e-08),
        ('n1e6', True): (1.86, 1.2e-04),
        ('switch_lo', False): (0.00, 4.3e-08),
        ('switch_lo', True): (1.89, 1.7e-04),
        ('switch_hi', False): (0.00, 4.3e-08),
        ('switch_hi', True): (2.34, 2.9e-04),
    },
}


def enc_yardstick(labels, contracted):
    """(dxu [m,1], dvr [m,1]) tensors of YARDSTICK['enc'] for a list of labels"""
    rows = [YARDSTICK['enc'][(l, contracted)] for l in labels]
    return (torch.tensor([r[0] for r in rows], dtype=torch.float64)[:, None],
            torch.tensor([r[1] for r in rows], dtype=torch.float64)[:, None])


def _up(v, digits):
    return math.ceil(v * 10 ** digits - 1e-9) / 10 ** digits


if __name__ == '__main__':
    print("    'local': %.2f," % _up(twin_local(), 2))
    a = twin_act()
    print("    'act': (%.1e, %.1e)," % (float('%.1e' % (a[0] * 1.05)), float('%.1e' % (a[1] * 1.05))))
    t = twin_enc()
    for l in ENC_LABELS:
        for con in (False, True):
            dx, dv = t[(l, con)]
            print("        (%r, %r): (%.2f, %.1e)," % (l, con, _up(dx, 2), float('%.1e' % (dv * 1.05))))
