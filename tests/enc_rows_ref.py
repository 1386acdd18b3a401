"""Engineered rays for the sample encoders (csrc/rays.hip k_encode / k_encode_lane, csrc/enc_lane.h, csrc/gauss.h) and
their float64 truth: the oracle's own cast_rays, 1 - sum(hit) mask, new_space, integrated_pos_enc and weighted_ipe
(oracle/durf_ref.py) in float64, under the flags the kernels take.  CPU only; tests/test_enc_rows_ref.py holds the conditions,
tests/test_gpu_enc_edges.py uses it on the device.

The base set is one list of rays (N = 32 samples each), every ray built for one LABEL (RAYS below).  A GROUP is one launch
configuration: (kind 'bkgd' | 'obj', flags, hit columns 3 | 0, alpha); every ray is run in every group, and `PROPS` says in
which groups a label means something and which property of the float64 Gaussian its samples must then have (`classify`
asserts it sample by sample).  A sample's class is its ray's label.

safe_sin.  The reference runs in float32, so its wrap `x % (100 pi)` is by the float32-rounded 100 pi = 314.15927124...
(internal/math.py:35-46); oracle.durf_ref.safe_sin in float32 does the same (torch rounds the Python scalar to the tensor's
type), in float64 it would wrap by the double 100 pi, 5.9e-6 rad per wrap away.  The truth is the reference's meaning: the
float64 run swaps in a safe_sin whose period AND threshold are T32 (`_reference_wrap`); the same goes for the float32 sum
fl32(y + fl32(pi/2)) under the cosine half (`_reference_sin`).  tests/test_enc_rows_ref.py checks
both statements.

Conditioning.  Feature (deg, axis) is e sin(2^deg x [+ pi/2]) with e = exp(-0.5 var 4^deg): `cond_x` = 2^deg e is its
sensitivity to x, `cond_v` = 0.5 4^deg var e its sensitivity to the relative error of var.  The yardstick is the oracle's
float32 twin: per label, the largest distance of its Gaussian from float64 in ulps of x and relative in var (YARDSTICK,
written by `python -m tests.enc_rows_ref`, held to a fresh run by tests/test_enc_rows_ref.py):

  label       plain: dx [ulp]  dvar [rel]   contracted: dx [ulp]  dvar [rel]
  axis                   2.08     1.2e-07                   2.06     6.4e-06
  dzero                  0.00     9.8e-08                   4.68     6.4e-07
  hit1                   0.98     2.1e-07                   2.51     5.6e-07
  huge                   0.00     8.5e-08                   1.09     4.0e-05
  n01_hi                 0.73     1.4e-07                   2.72     6.6e-07
  n01_lo                 0.73     1.4e-07                   0.73     1.4e-07
  n1                     0.78     1.7e-07                   1.89     6.9e-07
  n1e3                   0.50     1.8e-07                   1.78     1.4e-04
  n1e6                   0.80     1.2e-07                   1.43     2.3e-04
  n2                     0.78     1.6e-07                   2.22     3.9e-07
  nonunit                1.35     2.1e-07                   2.67     4.7e-07
  obj40                  0.50     1.6e-07                   1.92     4.7e-07
  plain                  0.98     2.1e-07                   2.51     5.6e-07
  radius0                0.98     2.0e-07                   2.51     5.8e-07
  switch_hi              0.49     1.1e-07                   1.90     3.2e-06
  switch_lo              0.49     1.1e-07                   1.94     4.3e-06
  t_equal                0.50     1.1e-07                   0.83     1.9e-07
  thick                  1.51     1.8e-07                   1.97     4.5e-07
  thin                   0.74     1.7e-07                   1.45     4.5e-07
  tiny                   1.14     1.5e-07                   1.14     1.5e-07
  var0                   0.50     0.0e+00                   0.83     0.0e+00
  var_big                1.00     1.5e-07                   1.63     4.0e-07
  var_cross              1.00     2.3e-07                   1.63     4.8e-07
  wrap                   0.50     9.9e-08                   5.18     1.6e-04
  zero                   0.00     8.5e-08                   0.00     8.5e-08
(contracted: the background groups with DURF_ENC_CONTRACT; the contraction's JVP cancels at large norms, and 2 - 1/n
cancels near n = 0.5.)
Out of domain, declared: label `hit2` (two boxes hit: mask -1, negative variance) in the groups with hit columns."""
import contextlib
import itertools
import math

import numpy as np
import torch

from oracle import durf_ref as R

N = 32
T32 = float(np.float32(100 * math.pi))           # 314.1592712402344: the reference's wrap period
HALF_PI32 = float(np.float32(0.5 * math.pi))
CONTRACT, NO_INT, CYL = 1, 2, 4
SWITCH = (2048.0 - HALF_PI32) / 512.0            # lane encoder: big branch from max|x| >= 3.99693...
ALPHAS = (0.0, 2.5, 4.5, 6.5, 10.0)
REL_GAP = 1e-4                                   # no in-domain sample within this (relative) of a discontinuity


def _lin(t0, t1):
    return np.linspace(t0, t1, N + 1, dtype=np.float64)


def _sweep(axis, a0, a1, rest=(0.3, -1.2, 0.7), t=(1.0, 2.0)):
    """a ray whose coordinate `axis` runs from a0 to a1 while t runs over `t`; the other coordinates stay at `rest`"""
    o, d = list(rest), [0.0, 0.0, 0.0]
    d[axis] = (a1 - a0) / (t[1] - t[0])
    o[axis] = a0 - d[axis] * t[0]
    return o, d, 1e-3, _lin(*t)


def _rays():
    out = []                                      # (label, o, d, radius, t_vals, hit row)
    add = lambda label, o, d, r, tv, hit=(0, 0, 0): out.append((label, o, d, r, tv, hit))
    # branch switch of the lane encoder: both sides and both signs, interleaved ray by ray (N = 32: two rays share a wave)
    for axis, sign in ((0, 1), (1, -1), (2, 1), (0, -1)):
        add('switch_lo', *_sweep(axis, sign * 3.9935, sign * 3.9955))
        add('switch_hi', *_sweep(axis, sign * 3.9985, sign * 4.0005))
    # wrap at 100 pi: 2^deg x (sine) and 2^deg x + pi/2 (cosine) just below / above +-T32
    for deg, sign, shift in itertools.product((0, 4, 9), (1, -1), (0.0, HALF_PI32)):
        for lo, hi in ((1 - 3e-3, 1 - 4e-4), (1 + 4e-4, 1 + 3e-3)):
            a0, a1 = ((sign * T32 * lo - shift) / 2 ** deg, (sign * T32 * hi - shift) / 2 ** deg)
            add('wrap', *_sweep(deg % 3, a0, a1, rest=(0.11, -0.23, 0.05)))
    # |y| up to 1e5 (undamped in the no-integration groups).  d = 0: x = o exactly, so the twin's dx is 0 and the sine half is
    # gated at 1e-5; 512 x = q T32 + 0.05, a small sine, where one bf16 ulp is small too (the exact-period control needs both)
    for axis, q in ((0, 318), (1, -250), (2, 200)):
        o = [0.25, -0.5, 0.125]
        o[axis] = float(np.float32((q * T32 + 0.05) / 512))
        add('huge', o, [0, 0, 0], 1e-3, _lin(1, 2))
    # contraction: norms below 1e-6, the zero vector, either side of the switch at 0.1, 1, 2, 1e3, 1e6
    u = np.array([0.6, -0.64, 0.48])
    add('tiny', [0, 0, 0], list(u * 5e-7), 1e-3, _lin(0.5, 1.5))
    add('zero', [0, 0, 0], [0, 0, 0], 1e-3, _lin(1, 2))
    add('n01_lo', list(u * 0.1 * (1 - 1e-3)), list(u * 1e-6), 1e-3, _lin(1, 2))
    add('n01_hi', list(u * 0.1 * (1 + 1e-3)), list(u * 1e-6), 1e-3, _lin(1, 2))
    add('n01_lo', [0, -0.1 * (1 - 1e-3), 0], [1e-6, 0, 0], 1e-3, _lin(1, 2))
    add('n01_hi', [0, 0, 0.1 * (1 + 1e-3)], [0, 1e-6, 0], 1e-3, _lin(1, 2))
    for label, n in (('n1', 1.0), ('n2', 2.0), ('n1e3', 1e3), ('n1e6', 1e6)):
        add(label, list(u * n), list(np.array([0.48, 0.6, 0.64]) * n * 1e-3), 1e-3, _lin(1, 2))
        add(label, [0, 0, -n], [n * 1e-3, 0, 0], 1e-3, _lin(1, 2))
    # hit masks: an ordinary ray, one box hit (mask 0), two boxes hit (mask -1: out of domain) between ordinary neighbours
    plain = ([0.3, 0.2, -0.5], [0.36, 0.48, -0.8], 2e-3, _lin(0.5, 3.0))       # (no coordinate crosses 0)
    add('plain', *plain)
    add('hit1', *plain, hit=(0, 1, 0))
    add('plain', *plain)
    add('hit2', *plain, hit=(1, 0, 1))
    add('plain', *plain)
    # frustum
    add('t_equal', plain[0], plain[1], 1e-2, np.full(N + 1, 1.5))
    add('thin', plain[0], plain[1], 1e-2, 1.5 * (1 + np.arange(N + 1) * 2.0 ** -21))
    add('thick', plain[0], plain[1], 1e-3, np.geomspace(0.05, 2000.0, N + 1))
    add('radius0', plain[0], plain[1], 0.0, _lin(0.5, 3.0))
    for axis in range(3):
        e = [0.0, 0.0, 0.0]
        e[axis] = 1.0
        add('axis', plain[0], e, 5e-3, _lin(0.5, 3.0))
        e[axis] = -2.5
        add('axis', plain[0], list(e), 5e-3, _lin(0.5, 3.0))
    add('dzero', plain[0], [0, 0, 0], 5e-3, _lin(0.5, 3.0))
    add('nonunit', plain[0], [0.3, 0.4, -1.2], 5e-3, _lin(0.5, 3.0))
    add('nonunit', plain[0], [30.0, 40.0, -120.0], 1e-4, _lin(0.05, 0.3))
    # damping: var = 0; degree 0 already underflows; 0.5 var 4^deg crosses the underflow of exp (88 .. 104) at degree 1 .. 5
    add('var0', plain[0], plain[1], 0.0, np.full(N + 1, 1.5))
    add('var_big', plain[0], plain[1], 60.0, _lin(1, 2))
    for r in (9.2, 4.6, 2.3, 1.15, 0.575):
        add('var_cross', plain[0], plain[1], r, _lin(1, 2))
    # object frame: coordinates up to 40
    add('obj40', [-38.0, 25.0, 12.0], [0.5, -0.3, 0.2], 2e-3, _lin(0.5, 4.0))
    return out


_R = _rays()
LABELS = [r[0] for r in _R]
B = len(_R)
ORIGINS = torch.tensor(np.array([r[1] for r in _R], dtype=np.float32))
DIRS = torch.tensor(np.array([r[2] for r in _R], dtype=np.float32))
RADII = torch.tensor(np.array([r[3] for r in _R], dtype=np.float32))
T_VALS = torch.tensor(np.array([r[4] for r in _R], dtype=np.float32))
HIT = torch.tensor(np.array([r[5] for r in _R], dtype=np.int32))
assert (T_VALS > 0).all(), 'near > 0: t0 = t1 = 0 is 0/0 in the reference too'

# every launch configuration: (kind, flags, hit columns, alpha)
GROUPS = ([('bkgd', f, k, None) for f in range(8) for k in (3, 0)] +
          [('obj', f, 0, a) for f in (0, NO_INT, CYL, NO_INT | CYL) for a in ALPHAS])


def contracted(group):
    return group[0] == 'bkgd' and bool(group[1] & CONTRACT)


def rays_of(label):
    return [i for i, l in enumerate(LABELS) if l == label]


def _reference_sin(x):
    """safe_sin as the reference means it, whatever the tensor's type: period and threshold T32, and the cosine half (the
    second half of the last axis: sin(y + pi/2), internal/mip.py:273-282) at the float32 sum fl32(y + fl32(pi/2)) the reference
    forms -- at |y| = 1e5 that rounding is 3.9e-3 rad, and it is the reference's, like the rounded period"""
    if x.dtype == torch.float64:
        h = x.shape[-1] // 2
        x = torch.cat([x[..., :h], (x[..., :h] + HALF_PI32).float().double()], -1)
    return R.safe_trig_helper(x, torch.sin, t=T32)


@contextlib.contextmanager
def _reference_wrap():
    keep = R.safe_sin
    R.safe_sin = _reference_sin
    try:
        yield
    finally:
        R.safe_sin = keep


def gaussian(group, dt):
    """(x_pre, x, var) [B, N, 3]: the Gaussian before the contraction (masked) and as the encoder sees it (diag of cov)"""
    kind, flags, k, _ = group
    tv, o, d, r = T_VALS.to(dt), ORIGINS.to(dt), DIRS.to(dt), RADII.to(dt)[:, None]
    mean, cov = R.cast_rays(tv, o, d, r, 'cylinder' if flags & CYL else 'cone')
    if flags & NO_INT:
        cov = torch.zeros_like(cov)
    if kind == 'bkgd' and k:
        bm = (1 - HIT.to(dt).sum(-1))[:, None, None]
        mean, cov = bm * mean, bm[..., None] * cov
    pre = mean
    if kind == 'bkgd' and flags & CONTRACT:
        mean, cov = R.new_space((mean, cov))
    return pre, mean, cov


def encode(group, dt=torch.float64):
    """dict: x_pre, x, var [B, N, 3]; enc [B, N, 60 | 63]: the oracle's features of `group` in `dt`"""
    pre, mean, cov = gaussian(group, dt)
    with _reference_wrap():
        if group[0] == 'obj':
            enc = R.weighted_ipe((mean, cov), 0, 10, group[3])
        else:
            enc = R.integrated_pos_enc((mean, cov), 0, 10)
    return dict(x_pre=pre, x=mean, var=torch.diagonal(cov, dim1=-2, dim2=-1), enc=enc)


def conditioning(x, var):
    """(e, cond_x, cond_v, y) [..., 30] in the feature order deg * 3 + axis of one half of the encoding"""
    sc = torch.tensor([2.0 ** g for g in range(10)], dtype=x.dtype)
    y = (x[..., None, :] * sc[:, None]).reshape(*x.shape[:-1], 30)
    yv = (var[..., None, :] * sc[:, None] ** 2).reshape(*x.shape[:-1], 30)
    e = torch.exp(-0.5 * yv)
    s = sc[:, None].expand(10, 3).reshape(30)
    return e, s * e, 0.5 * yv * e, y


def in_domain(group):
    """[B] bool: False for the rays whose rows are declared out of domain in this group"""
    ok = torch.ones(B, dtype=torch.bool)
    if group[0] == 'bkgd' and group[2]:
        ok &= HIT.sum(-1) <= 1
    return ok


def _norm(x):
    return x.norm(dim=-1)


# label -> (groups it is about, property of the float64 Gaussian every sample of its rays has there)
_unc = lambda g: not (g[0] == 'bkgd' and (g[1] & CONTRACT or g[2]))
_con = lambda g: g[0] == 'bkgd' and g[1] & CONTRACT and not g[2]
_int = lambda g: not g[1] & NO_INT
_any = lambda g: True
_amax = lambda t: t['x'].abs().amax(-1)
PROPS = {
    'switch_lo': (_unc, lambda t: (_amax(t) > 3.99) & (_amax(t) < 3.9969)),
    'switch_hi': (_unc, lambda t: (_amax(t) > 3.9970) & (_amax(t) < 4.01)),
    'wrap': (_unc, lambda t: _near_wrap(t)),
    'huge': (_unc, lambda t: (_amax(t) * 512 > 5e4) & (_amax(t) * 512 <= 1e5)),
    'tiny': (_con, lambda t: (_norm(t['x_pre']) < 1e-6) & (_norm(t['x_pre']) > 0)),
    'zero': (_con, lambda t: _norm(t['x_pre']) == 0),
    'n01_lo': (_con, lambda t: (_norm(t['x_pre']) / 0.1 - (1 - 1e-3)).abs() < 1e-4),
    'n01_hi': (_con, lambda t: ((_norm(t['x_pre']) / 0.1 - (1 + 1e-3)).abs() < 1e-4) & (_amax(t) > 4)),
    'n1': (_con, lambda t: (_norm(t['x_pre']) - 1).abs() < 5e-3),
    'n2': (_con, lambda t: (_norm(t['x_pre']) / 2 - 1).abs() < 5e-3),
    'n1e3': (_con, lambda t: (_norm(t['x_pre']) / 1e3 - 1).abs() < 5e-3),
    'n1e6': (_con, lambda t: (_norm(t['x_pre']) / 1e6 - 1).abs() < 5e-3),
    'plain': (_any, lambda t: _amax(t) > 0),
    'hit1': (lambda g: g[0] == 'bkgd' and g[2], lambda t: (_amax(t) == 0) & (t['var'].abs().amax(-1) == 0)),
    't_equal': (lambda g: _int(g) and not g[1] & CONTRACT,
                lambda t: (t['t1'] == t['t0']) & (t['var'].amin(-1) > 0)),
    'thin': (_int, lambda t: ((t['t1'] - t['t0']) / t['t0'] < 1e-6) & (t['t1'] > t['t0'])),
    'thick': (_int, lambda t: t['t1'] / t['t0'] > 1.3),
    'radius0': (_any, lambda t: t['radius'] == 0),
    'axis': (_any, lambda t: ((t['d'] != 0).sum(-1) == 1)),
    'dzero': (_any, lambda t: (t['d'] == 0).all(-1)),
    'nonunit': (_any, lambda t: (_norm(t['d']) - 1).abs() > 0.25),
    'var0': (lambda g: not (g[0] == 'bkgd' and g[1] & CONTRACT), lambda t: (t['var'] == 0).all(-1)),
    'var_big': (lambda g: _unc(g) and _int(g), lambda t: 0.5 * t['var'].amax(-1) > 104),
    'var_cross': (lambda g: _unc(g) and _int(g), lambda t: _crosses(t)),
    'obj40': (lambda g: g[0] == 'obj', lambda t: (_amax(t) > 30) & (_amax(t) <= 40)),
}
CLASSES = sorted(PROPS)


def _near_wrap(t):
    """some sine or cosine argument of the sample lies within 4e-3 (relative) of +-T32, and none within REL_GAP"""
    _, _, _, y = conditioning(t['x'], t['var'])
    a = torch.cat([y, y + HALF_PI32], -1).abs() / T32
    return ((a - 1).abs() < 4e-3).any(-1) & ~((a - 1).abs() < 2 * REL_GAP).any(-1)


def _crosses(t):
    """0.5 var 4^deg passes through the underflow band of float32 exp (88 .. 104) between degree 0 and degree 6"""
    a = 0.5 * t['var'].amax(-1)
    return (a < 104) & (a * 4.0 ** 6 > 88)


def _info(group):
    t = encode(group)
    exp = lambda v: v[:, None].expand(B, N)
    t.update(t0=T_VALS[:, :-1].double(), t1=T_VALS[:, 1:].double(), radius=exp(RADII.double()),
             d=DIRS.double()[:, None, :].expand(B, N, 3))
    return t


def classify():
    """{label: number of samples that populate the class}, and the checks: every sample of a label's rays has the label's
    property in every group the label is about; no in-domain sample of any group is within REL_GAP of a discontinuity (the
    contraction switch at norm 0.1, the safe_norm floor at norm 1e-6).  Returns (population, excluded share)."""
    pop = {c: 0 for c in CLASSES}
    excluded = total = 0
    for g in GROUPS:
        t = _info(g)
        dom = in_domain(g)
        total += int(dom.sum()) * N
        if g[0] == 'bkgd' and g[1] & CONTRACT:
            n = _norm(t['x_pre'])[dom]
            close = ((n / 0.1 - 1).abs() < REL_GAP) | ((n / 1e-6 - 1).abs() < REL_GAP)
            excluded += int(close.sum())
        for c in CLASSES:
            about, prop = PROPS[c]
            if not about(g):
                continue
            rows = rays_of(c)
            ok = prop(t)[rows]
            assert bool(ok.all()), 'label %s, group %s: %d of %d samples miss the property' % (c, g, int((~ok).sum()), ok.numel())
            pop[c] += ok.numel()
    return pop, excluded / total


def _ulp32(v):
    """spacing of float32 at |v| (float64 in, float64 out; the smallest normal's spacing below it)"""
    a = v.abs().clamp(min=2.0 ** -126)
    return torch.exp2(torch.floor(torch.log2(a)) - 23)


def twin_distance():
    """{(label, contracted): (dx in ulps of x, relative dvar)}: the float32 oracle's Gaussian against the float64 one, the
    largest over the in-domain samples of the label's rays in all groups with / without the contraction.  var = 0 in
    float64 must be 0 in the twin."""
    out = {(c, k): [0.0, 0.0] for c in CLASSES for k in (False, True)}
    for g in GROUPS:
        _, x64, c64 = gaussian(g, torch.float64)
        _, x32, c32 = gaussian(g, torch.float32)
        v64 = torch.diagonal(c64, dim1=-2, dim2=-1)
        v32 = torch.diagonal(c32, dim1=-2, dim2=-1).double()
        x32 = x32.double()
        dx = (x32 - x64).abs() / _ulp32(torch.maximum(x64.abs(), x32.abs()))
        dx = torch.where(x32 == x64, torch.zeros_like(dx), dx)
        assert bool((v32[v64 == 0] == 0).all()), g
        dv = torch.where(v64 != 0, (v32 - v64).abs() / v64.abs().clamp(min=1e-300), torch.zeros_like(v64))
        dom = in_domain(g)
        for c in CLASSES:
            rows = [i for i in rays_of(c) if dom[i]]
            k = (c, contracted(g))
            out[k][0] = max(out[k][0], float(dx[rows].max()))
            out[k][1] = max(out[k][1], float(dv[rows].max()))
    return {c: tuple(v) for c, v in out.items()}


# the float32 twin's figures (see the module docstring), rounded UP to the digits shown
YARDSTICK = {
    ('axis', False): (2.08, 1.2e-07),
    ('axis', True): (2.06, 6.4e-06),
    ('dzero', False): (0.00, 9.8e-08),
    ('dzero', True): (4.68, 6.4e-07),
    ('hit1', False): (0.98, 2.1e-07),
    ('hit1', True): (2.51, 5.6e-07),
    ('huge', False): (0.00, 8.5e-08),
    ('huge', True): (1.09, 4.0e-05),
    ('n01_hi', False): (0.73, 1.4e-07),
    ('n01_hi', True): (2.72, 6.6e-07),
    ('n01_lo', False): (0.73, 1.4e-07),
    ('n01_lo', True): (0.73, 1.4e-07),
    ('n1', False): (0.78, 1.7e-07),
    ('n1', True): (1.89, 6.9e-07),
    ('n1e3', False): (0.50, 1.8e-07),
    ('n1e3', True): (1.78, 1.4e-04),
    ('n1e6', False): (0.80, 1.2e-07),
    ('n1e6', True): (1.43, 2.3e-04),
    ('n2', False): (0.78, 1.6e-07),
    ('n2', True): (2.22, 3.9e-07),
    ('nonunit', False): (1.35, 2.1e-07),
    ('nonunit', True): (2.67, 4.7e-07),
    ('obj40', False): (0.50, 1.6e-07),
    ('obj40', True): (1.92, 4.7e-07),
    ('plain', False): (0.98, 2.1e-07),
    ('plain', True): (2.51, 5.6e-07),
    ('radius0', False): (0.98, 2.0e-07),
    ('radius0', True): (2.51, 5.8e-07),
    ('switch_hi', False): (0.49, 1.1e-07),
    ('switch_hi', True): (1.90, 3.2e-06),
    ('switch_lo', False): (0.49, 1.1e-07),
    ('switch_lo', True): (1.94, 4.3e-06),
    ('t_equal', False): (0.50, 1.1e-07),
    ('t_equal', True): (0.83, 1.9e-07),
    ('thick', False): (1.51, 1.8e-07),
    ('thick', True): (1.97, 4.5e-07),
    ('thin', False): (0.74, 1.7e-07),
    ('thin', True): (1.45, 4.5e-07),
    ('tiny', False): (1.14, 1.5e-07),
    ('tiny', True): (1.14, 1.5e-07),
    ('var0', False): (0.50, 0.0e+00),
    ('var0', True): (0.83, 0.0e+00),
    ('var_big', False): (1.00, 1.5e-07),
    ('var_big', True): (1.63, 4.0e-07),
    ('var_cross', False): (1.00, 2.3e-07),
    ('var_cross', True): (1.63, 4.8e-07),
    ('wrap', False): (0.50, 9.9e-08),
    ('wrap', True): (5.18, 1.6e-04),
    ('zero', False): (0.00, 8.5e-08),
    ('zero', True): (0.00, 8.5e-08),
}


def bounds(group, t=None):
    """Per-feature error budgets of `group` against the float64 truth, [B, N, 60] each (the object form's weights applied):
      cond   4 x (twin dx ulp32(x) 2^deg e + twin dvar 0.5 4^deg var e), the label's YARDSTICK figures;
      small  the v_fract branch of enc_lane.h: (2e-4 |y| / 2048 + 16e-6 + 5.9e-6 [wraps ignored]) e + 2e-6 e, and on the
             cosine half 0.5 ulp32(y + pi/2) e: cos(y) stands in for sin(fl32(y + fl32(pi/2))) (3e-5 rad at |y| = 1000);
      big    the exact-wrap branch: (1e-4 |m| / 300 + 2e-6) e + 2e-6 e, m the wrapped argument;
      is_big the branch the lane encoder takes, from the float64 x against SWITCH in doubles; near: within 1e-4 (relative)
             of the switch, where the kernel's float32 expression max|x| * 512 + pi/2 < 2048 may decide either way."""
    t = t or encode(group)
    x, var = t['x'], t['var']
    e, cx, cv, y = conditioning(x, var)
    key = lambda l: ('plain' if l == 'hit2' else l, contracted(group))       # (hit2 without hit columns: the plain ray)
    dxu = torch.tensor([YARDSTICK[key(l)][0] for l in LABELS], dtype=torch.float64)[:, None, None]
    dvr = torch.tensor([YARDSTICK[key(l)][1] for l in LABELS], dtype=torch.float64)[:, None, None]
    ux = _ulp32(x)[..., None, :].expand(*x.shape[:-1], 10, 3).reshape(*x.shape[:-1], 30)
    cond = 4 * (dxu * ux * cx + dvr * cv)
    yc = y + HALF_PI32
    ssum = torch.cat([torch.zeros_like(y), 0.5 * _ulp32(yc) * e], -1)
    yy, ee = torch.cat([y, yc], -1), torch.cat([e, e], -1)
    wraps = torch.where(yy.abs() < T32, torch.zeros_like(yy), torch.floor(yy / T32).abs())
    m = torch.where(yy.abs() < T32, yy, torch.remainder(yy, T32))
    small = (2e-4 * yy.abs() / 2048 + 16e-6 + 5.9e-6 * wraps) * ee + 2e-6 * ee + ssum
    big = (1e-4 * m.abs() / 300 + 2e-6) * ee + 2e-6 * ee
    amax = x.abs().amax(-1)
    w = torch.ones(60, dtype=torch.float64)
    if group[0] == 'obj':
        w = R.barf_weights(group[3], 10, torch.float64)[:, None].expand(10, 6).reshape(60)
    return dict(cond=torch.cat([cond, cond], -1) * w, small=small * w, big=big * w, e=ee, w=w,
                is_big=amax >= SWITCH, near=(amax / SWITCH - 1).abs() < 1e-4)


if __name__ == '__main__':
    pop, share = classify()
    print('excluded share', share)
    for (c, k), (a, b) in sorted(twin_distance().items()):
        print("    (%r, %r): (%.2f, %.1e)," % (c, k, math.ceil(a * 100) / 100, float('%.1e' % (b * 1.05))))
    print(pop)
