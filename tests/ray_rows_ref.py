"""TEST INFRASTRUCTURE: the per-ray float64 oracle of the ray prologue (csrc/rays.hip: k_ray_setup, k_sample_t, k_view_enc,
k_compact_hits / k_compact_all, k_density_noise, k_ray_prologue) and the inputs tests/test_gpu_ray_edges.py aims at its edges.

Every function takes the float32 INPUT values and evaluates the reference's formulas (box_helpers.aa2matrix :148-167,
world2object_rpy :286-341, ray_box_intersection :59-106, the model's sums obbpose_model.py:112-131, mip.sample_along_rays
:330-370, mip.pos_enc :36-45) in the dtype it is handed: np.float64 is the oracle, np.float32 its TWIN -- the same expressions in
the kernels' operation order, every product and sum rounded on its own as a build without contraction rounds them.  numpy's
minimum / maximum propagate NaN as jnp's do.  The file stands on its own; tests/test_ray_rows_ref.py cross-checks it against
oracle/durf_ref.py.  (linspace(0, 1, N + 1) is a float32 tensor in the reference, so the grid s = float32(i) / float32(N) is an
input of both dtypes; so is the uniform draw.)

UNDECIDED entries.  For a (ray, box) pair m = min(|tf - tn|, |tf|) / ((|po|_inf + |e|_inf) / min_i |pd_i|) (finite axes, float64).
A pair with m < TAU is undecided: a rounding may turn its hit, so neither its hit nor its ray's origins_s / dirs_s / zo / dyn are
compared.  TAU is 4 x the largest distance, in that same unit, between the twin's and the oracle's tn / tf over the generic cases
below (`measure_tau`; tests/test_ray_rows_ref.py holds TAU to a fresh measurement).  The hand-aimed TABLE is outside this rule
by construction: every box has rotation vector exactly 0 (R is exactly the identity: a * 0 + b * 0 stays 0), centres, extents and
origins are dyadic and directions are +-e_i, so tn and tf are the SAME numbers (or the same inf / NaN) in both dtypes; the two
diagonal rays graze an edge and a corner through products of one shared 1 / pd with +-1, +-2, +-3, so tf == tn holds in any
precision.  The CPU test asserts that bit-equality of twin and oracle on the whole table, which is what makes m = 0 decided."""
import numpy as np

MAX_OBJ = 16
F32, F64 = np.float32, np.float64
TAU = 1.9e-5          # 4 x 4.6e-06, the figure `measure_tau()` gives over GENERIC_CASES (rounded up)
VIEW_DIM = 32


def _in(x, dt):
    return np.ascontiguousarray(np.asarray(x, dtype=F32)).astype(dt)


# ---------------------------------------------------------------------------
# ray setup
# ---------------------------------------------------------------------------
def aa2matrix(rot, dt=F64):
    """rotation vectors [K,3] (float32 values) -> world->object matrices [K,3,3] in dtype dt"""
    r = _in(rot, dt).reshape(-1, 3)
    rx, ry, rz = r[:, 0], r[:, 1], r[:, 2]
    floor = dt(1e-12)
    s = rx * rx + ry * ry + rz * rz
    s = np.where(s < floor, floor, s)                        # math.safe_norm
    th = np.sqrt(s) + floor
    a = np.sin(th) / th
    b = (dt(1) - np.cos(th)) / (th * th)
    z = np.zeros_like(rx)
    S = np.stack([np.stack([z, -rz, ry], -1), np.stack([rz, z, -rx], -1), np.stack([-ry, rx, z], -1)], -2)
    R = np.empty_like(S)
    for i in range(3):
        for j in range(3):
            s2 = S[:, i, 0] * S[:, 0, j] + S[:, i, 1] * S[:, 1, j] + S[:, i, 2] * S[:, 2, j]
            R[:, i, j] = (dt(1 if i == j else 0) + a * S[:, i, j]) + b * s2
    return R


def _rot3(Rk, v):
    """rows of Rk against the vectors v [B,3] -> ([B,3] products summed left to right, [B,3] sum of their absolute values)"""
    p0, p1, p2 = Rk[:, 0] * v[:, 0:1], Rk[:, 1] * v[:, 1:2], Rk[:, 2] * v[:, 2:3]
    return (p0 + p1) + p2, np.abs(p0) + np.abs(p1) + np.abs(p2)


def ray_setup(o, d, pose, ext, enable=None, dt=F64):
    """the ray side of MipNerfModel.__call__ :99-131 for every ray on its own.  o, d [B,3], pose [K,6], ext [K,3], enable [K] or None
    -> dict(hit [B,K] int32, o_s, d_s [B,3], zo [B], dyn [B], tn, tf, m [B,K], s_o, s_d [B,3], s_z [B]): s_* are the SCALES, the
    sums of the absolute terms each output is made of"""
    o, d, pose, ext = _in(o, dt).reshape(-1, 3), _in(d, dt).reshape(-1, 3), _in(pose, dt).reshape(-1, 6), _in(ext, dt).reshape(-1, 3)
    B, K = o.shape[0], pose.shape[0]
    assert K <= MAX_OBJ
    R = aa2matrix(pose[:, 3:], dt)
    c = -pose[:, :3]
    zB = np.zeros(B, dt)
    out = dict(hit=np.zeros((B, K), np.int32), tn=np.full((B, K), np.nan, dt), tf=np.full((B, K), np.nan, dt),
               m=np.full((B, K), np.inf, dt), unit=np.ones((B, K), dt))
    so, sd, s_o, s_d = (np.zeros((B, 3), dt) for _ in range(4))
    zsum, s_z = zB.copy(), zB.copy()
    with np.errstate(all='ignore'):
        for k in range(K):
            if enable is not None and int(enable[k]) == 0:
                continue
            Rk = R[k]
            sT, aT = _rot3(Rk, c[k:k + 1])
            po, apo = _rot3(Rk, o)
            po, apo = po + sT, apo + aT
            pd, apd = _rot3(Rk, d)
            nrm = np.sqrt((pd[:, 0] * pd[:, 0] + pd[:, 1] * pd[:, 1]) + pd[:, 2] * pd[:, 2])
            pd, apd = pd / nrm[:, None], apd / nrm[:, None]
            inv = dt(1) / pd
            tmin, tmax = (-ext[k] - po) * inv, (ext[k] - po) * inv
            t0, t1 = np.minimum(tmin, tmax), np.maximum(tmin, tmax)
            tn = np.maximum(np.maximum(t0[:, 0], t0[:, 1]), t0[:, 2])
            tf = np.minimum(np.minimum(t1[:, 0], t1[:, 1]), t1[:, 2])
            h = tf > tn
            h = h & (tf * h.astype(dt) > 0)
            hf = h.astype(dt)
            zsum = zsum + hf * (tf * hf)
            so, sd = so + po * hf[:, None], sd + pd * hf[:, None]
            s_o, s_d = s_o + apo * hf[:, None], s_d + apd * hf[:, None]
            # zo: tf = (+-e_i - po_i) / pd_i on the axis that ends the overlap
            ax = np.argmin(np.where(np.isnan(t1), np.inf, t1), axis=1)
            rows = np.arange(B)
            s_z = s_z + np.where(h, (apo[rows, ax] + ext[k][ax]) / np.abs(pd[rows, ax]), 0)
            unit = (np.abs(po).max(1) + np.abs(ext[k]).max()) / np.where(pd == 0, np.inf, np.abs(pd)).min(1)
            m = np.minimum(np.abs(tf - tn), np.abs(tf)) / unit
            out['hit'][:, k], out['tn'][:, k], out['tf'][:, k] = h, tn, tf
            out['m'][:, k] = np.where(np.isnan(m), 0, m)
            out['unit'][:, k] = unit
    nhit = out['hit'].sum(1)
    bk = (nhit == 0).astype(dt)
    out.update(o_s=so + bk[:, None] * o, d_s=sd + bk[:, None] * d, zo=zsum, dyn=nhit.astype(np.int32),
               s_o=s_o + bk[:, None] * np.abs(o), s_d=s_d + bk[:, None] * np.abs(d), s_z=np.where(nhit == 0, 1, s_z))
    return out


def decided(ref):
    """(pairs [B,K], rays [B]) bool: what a comparison may look at (see the module docstring)"""
    pairs = ref['m'] >= TAU
    return pairs, pairs.all(1)


def setup_errors(o_s, d_s, zo, ref, rays):
    """largest error of each output over the rays `rays` against the oracle's scale: (origins_s, dirs_s, zo)"""
    e = lambda got, want, scale: float((np.abs(np.asarray(got, F64) - want).reshape(len(rays), -1).max(1)
                                        / scale.reshape(len(rays), -1).max(1))[rays].max())
    return e(o_s, ref['o_s'], ref['s_o']), e(d_s, ref['d_s'], ref['s_d']), e(zo, ref['zo'], ref['s_z'])


def same_bits(got, want64):
    """got (float32 array) is the float64 `want64` rounded to float32, bit for bit, NaN for NaN"""
    got, want = np.asarray(got, F32), np.asarray(want64, F64).astype(F32)
    nan = np.isnan(want)
    return bool(np.array_equal(np.isnan(got), nan) and np.array_equal(got[~nan].view(np.int32), want[~nan].view(np.int32)))


# ---------------------------------------------------------------------------
# the hand-aimed table: K = 16 boxes, all of rotation exactly 0, dyadic everywhere
# ---------------------------------------------------------------------------
def table_scene():
    """-> pose [16,6], ext [16,3], enable [16] int32 (box 5 switched off)"""
    pose, ext = np.zeros((16, 6), F32), np.ones((16, 3), F32)
    for k in range(16):                                      # out of every table ray's way unless placed below
        pose[k, :3] = (-64.0, 8.0 * k, 64.0)
        ext[k] = (0.5, 1.0, 2.0) if k % 2 else (1.0, 1.0, 1.0)
    pose[0, :3], ext[0] = (0, 0, 0), (1.0, 0.5, 2.0)
    pose[1, :3], ext[1] = (4, 0, 0), (1.0, 1.0, 1.0)
    pose[2, :3], ext[2] = (8, 0, 0), (1.0, 1.0, 2.0)
    pose[5, :3], ext[5] = (0, 0, -8), (1.0, 1.0, 1.0)
    pose[15, :3], ext[15] = (0, 0, 16), (1.0, 1.0, 1.0)
    enable = np.ones(16, np.int32)
    enable[5] = 0
    return pose, ext, enable


X, Y, Z = (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0)
_neg = lambda v: tuple(-x + 0.0 for x in v)
# (name, origin, direction, boxes hit with box 5 off, boxes hit with every box on [None: the same])
TABLE_RAYS = [
    ('through the centre', (0, -4, 0), Y, (0,), None),
    ('through the centre, heading -y', (0, 4, 0), _neg(Y), (0,), None),
    ('origin inside the box', (0.25, 0.125, -0.5), Y, (0,), None),
    ('box wholly behind the origin', (0, 4, 0), Y, (), None),
    ('origin on a face heading out: tf == 0', (0, 0.5, 0), Y, (), None),
    ('origin on a face heading in', (0, -0.5, 0), Y, (0,), None),
    ('parallel to the x and z slabs, outside x', (2, -4, 0), Y, (), None),
    ('parallel to the x and z slabs, inside both', (0.5, -4, 1.5), Y, (0,), None),
    ('parallel and exactly in the face plane x = +e: NaN', (1, -4, 0), Y, (), None),
    ('parallel and exactly in the face plane z = -e: NaN', (0, -4, -2), Y, (), None),
    ('grazing the edge (1, 0.5, .): tf == tn', (0, 1.5, 0), (1.0, -1.0, 0.0), (), None),
    ('grazing the corner (1, 0.5, 2): tf == tn', (-1, 2.5, 0), (1.0, -1.0, 1.0), (), None),
    ('through two boxes', (-4, 0, 1.5), X, (0, 2), None),
    ('through three boxes', (-4, 0, 0), X, (0, 1, 2), None),
    ('through three boxes, heading -x', (12, 0, 0.5), _neg(X), (0, 1, 2), None),
    ('box 0 and box 15 only', (0, 0, -4), Z, (0, 15), None),
    ('a box that would be hit but is switched off', (0.5, 0, -12), Z, (0, 15), (0, 5, 15)),
]
# zo of a few of them by hand, against the first K boxes of the scene: (K, the sum of the exit distances).  It is NaN where the
# reference's own t_far * intersection is -inf * 0 or NaN * 0 -- a ray parallel to a slab of ANY box and outside it, which among
# 16 boxes is every axis-parallel ray: hence the sub-scenes K = 1 and K = 3, launched like the whole table
TABLE_ZO = {'through the centre': (1, 4.5), 'origin inside the box': (1, 0.375), 'origin on a face heading out: tf == 0': (1, 0.0),
            'origin on a face heading in': (1, 1.0), 'parallel to the x and z slabs, outside x': (1, float('nan')),
            'parallel and exactly in the face plane x = +e: NaN': (1, float('nan')), 'grazing the edge (1, 0.5, .): tf == tn': (1, 0.0),
            'through three boxes': (3, 5.0 + 9.0 + 13.0), 'through two boxes': (3, float('nan')), 'box 0 and box 15 only': (1, 6.0)}
TABLE_KS = (16, 3, 1)


def table():
    """-> dict(o, d [R,3] float32, names, want [R,16] int32 with box 5 off, want_all [R,16] with every box on): TABLE_RAYS, then
    the axis-parallel ones again with -0.0 in place of every +0.0 direction component (same literals)"""
    rows = [r + (False,) for r in TABLE_RAYS] + [r + (True,) for r in TABLE_RAYS if sum(x != 0 for x in r[2]) == 1]
    o = np.array([r[1] for r in rows], F32)
    d = np.array([r[2] for r in rows], F32)
    for i, r in enumerate(rows):
        if r[5]:
            d[i] = np.where(d[i] == 0, F32(-0.0), d[i])
    want, want_all = np.zeros((len(rows), 16), np.int32), np.zeros((len(rows), 16), np.int32)
    for i, r in enumerate(rows):
        want[i, list(r[3])] = 1
        want_all[i, list(r[3] if r[4] is None else r[4])] = 1
    return dict(o=o, d=d, names=[r[0] + (' (-0.0)' if r[5] else '') for r in rows], want=want, want_all=want_all)


# ---------------------------------------------------------------------------
# generic cases: K in {1, 3, 16}, every rotation class, rays aimed at points within 1.3 x a box's extents
# ---------------------------------------------------------------------------
ROTATIONS = {                       # rotation vector = axis * angle
    'zero': 0.0, 'below': 5e-7, 'one': 1.0, 'near_pi': 3.140592653589793, 'above_pi': 4.0}
GENERIC_CASES = {
    'K1-zero': ('zero',), 'K1-below': ('below',), 'K1-one': ('one',), 'K1-near_pi': ('near_pi',), 'K1-above_pi': ('above_pi',),
    'K3-a': ('zero', 'one', 'near_pi'), 'K3-b': ('below', 'above_pi', 'one'),
    'K16': tuple(['zero', 'below', 'one', 'near_pi', 'above_pi'][k % 5] for k in range(16)),
}
RAYS = 256
INSIDE = 8                          # the first rays of a case start inside a box
_CACHE = {}


def generic(name):
    """-> dict(o, d [256,3], pose [K,6], ext [K,3], enable [K] (every third box off; K = 1: on), classes)"""
    if name in _CACHE:
        return _CACHE[name]
    classes = GENERIC_CASES[name]
    K = len(classes)
    g = np.random.default_rng(2012 + sorted(GENERIC_CASES).index(name))
    spread = {1: 0.0, 3: 1.0, 16: 1.5}[K]             # overlapping boxes: hits and misses both common at every K
    pose, ext = np.zeros((K, 6), F64), g.uniform(0.75, 2.0, (K, 3))
    pose[:, :3] = g.uniform(-spread, spread, (K, 3)) + g.uniform(-4, 4, 3)
    for k, cl in enumerate(classes):
        ax = g.normal(size=3)
        pose[k, 3:] = ax / np.linalg.norm(ax) * ROTATIONS[cl]
    pose, ext = pose.astype(F32), ext.astype(F32)
    R = aa2matrix(pose[:, 3:], F64)
    k_of = np.arange(RAYS) % K
    u = g.uniform(-1.3, 1.3, (RAYS, 3))
    if K == 1:      # a lone box: three rays of four aim at the shell 1 <= |u|_inf <= 1.3 around it, or four of five would hit
        shell = u / np.abs(u).max(1, keepdims=True) * g.uniform(1.0, 1.3, (RAYS, 1))
        u = np.where((np.arange(RAYS) % 4 != 0)[:, None], shell, u)
    target = pose[k_of, :3] + np.einsum('bji,bj->bi', R[k_of], u * ext[k_of])          # R^T (u e) + c
    away = g.normal(size=(RAYS, 3))
    o = target + away / np.linalg.norm(away, axis=1, keepdims=True) * g.uniform(5, 10, (RAYS, 1))
    ins = np.arange(INSIDE)
    o[ins] = pose[k_of[ins], :3] + np.einsum('bji,bj->bi', R[k_of[ins]], g.uniform(-0.5, 0.5, (INSIDE, 3)) * ext[k_of[ins]])
    target[ins] = o[ins] + g.normal(size=(INSIDE, 3))
    d = target - o
    d = d / np.linalg.norm(d, axis=1, keepdims=True)
    enable = np.ones(K, np.int32)
    if K > 1:
        enable[2::3] = 0
    _CACHE[name] = dict(o=o.astype(F32), d=d.astype(F32), pose=pose, ext=ext, enable=enable, classes=classes)
    return _CACHE[name]


def measure_tau():
    """the largest distance between the twin's and the oracle's tn / tf over the generic cases, in the unit of m"""
    worst = 0.0
    for name in GENERIC_CASES:
        c = generic(name)
        a, b = ray_setup(c['o'], c['d'], c['pose'], c['ext'], None, F64), ray_setup(c['o'], c['d'], c['pose'], c['ext'], None, F32)
        for key in ('tn', 'tf'):
            worst = max(worst, float((np.abs(b[key].astype(F64) - a[key]) / a['unit']).max()))
    return worst


def setup_floor(name, masked):
    """the twin's distance from the oracle on the decided rays of a generic case: (origins_s, dirs_s, zo)"""
    c = generic(name)
    en = c['enable'] if masked else None
    ref, twin = ray_setup(c['o'], c['d'], c['pose'], c['ext'], en, F64), ray_setup(c['o'], c['d'], c['pose'], c['ext'], en, F32)
    return setup_errors(twin['o_s'], twin['d_s'], twin['zo'], ref, decided(ref)[1])


def shuffled_copies(n, base, seed):
    """n indices into `base` rays in shuffled order, every base ray present when n >= base"""
    g = np.random.default_rng(seed)
    return g.permutation(np.resize(np.arange(base), n) if n >= base else g.permutation(base)[:n])


# ---------------------------------------------------------------------------
# compaction (integers)
# ---------------------------------------------------------------------------
PATTERNS = ('zeros', 'ones', 'first', 'last', 'round_edge', 'alternating', 'random_0.5', 'random_0.01')


def hit_pattern(pattern, B, K, value=1, seed=0):
    g = np.random.default_rng(seed + 7 * B + K)
    h = np.zeros((B, K), np.int32)
    if pattern == 'ones':
        h[:] = 1
    elif pattern == 'first':
        h[0] = 1
    elif pattern == 'last':
        h[B - 1] = 1
    elif pattern == 'round_edge':                       # rays 1023 and 1024: the last lane of a round and the first of the next
        h[[b for b in (1023, 1024) if b < B]] = 1
    elif pattern == 'alternating':
        h[(np.arange(B)[:, None] + np.arange(K)[None]) % 2 == 0] = 1
    elif pattern.startswith('random'):
        h[g.random((B, K)) < float(pattern.split('_')[1])] = 1
    else:
        assert pattern == 'zeros'
    return h * np.int32(value)


def compact_ref(hit, N):
    """-> dict(count [K], idx (list of K arrays), slot [B,K], dyn [B], ccount [5], cidx (2 arrays), cslot [B,2])"""
    on = np.asarray(hit) != 0
    B, K = on.shape

    def lists(cols):
        idx = [np.nonzero(cols[:, k])[0].astype(np.int32) for k in range(cols.shape[1])]
        slot = np.where(cols, np.cumsum(cols, 0) - 1, -1).astype(np.int32)
        return idx, np.array([len(i) for i in idx], np.int32), slot
    idx, count, slot = lists(on)
    dyn = on.sum(1).astype(np.int32)
    cidx, cc, cslot = lists(np.stack([dyn != 1, dyn == 1], 1))
    multi = dyn > 1
    bits = 0
    for k in range(K):
        if (on[:, k] & multi).any():
            bits |= 1 << k
    ccount = np.array([cc[0], cc[1], int(cc[0]) * N + int(cc[1]), int(multi.sum()), bits], np.int32)
    return dict(count=count, idx=idx, slot=slot, dyn=dyn, ccount=ccount, cidx=cidx, cslot=cslot)


# ---------------------------------------------------------------------------
# level-0 sample positions (mip.sample_along_rays)
# ---------------------------------------------------------------------------
NEAR_FAR = ((2.0, 6.0), (0.05, 1e4), (3.0, 3.0), (1e-6, 1.0))
NEAR_FAR_INF = (0.0, 1.0)           # lindisp only: 1 / 0, compared as a pattern
T_RANDS = ('none', 'zero', 'one', 'random')
T_NS, T_BS = (1, 2, 31, 128, 255), (1, 3, 257)


def t_rand_of(kind, B, N):
    if kind == 'none':
        return None
    if kind == 'random':
        r = np.random.default_rng(B * 1000 + N).random((B, N + 1), dtype=F32)
        return np.minimum(r, F32(1 - 2.0 ** -24))
    return np.full((B, N + 1), 0.0 if kind == 'zero' else 1 - 2.0 ** -24, F32)


def sample_t(near, far, N, t_rand, lindisp, dt=F64):
    """near, far [B], t_rand [B,N+1] or None -> t_vals [B,N+1]"""
    s = (np.arange(N + 1, dtype=F32) / F32(N)).astype(dt)
    s[N] = 1
    nr, fr = _in(near, dt)[:, None], _in(far, dt)[:, None]
    with np.errstate(all='ignore'):
        t = nr * (dt(1) - s) + fr * s
        if lindisp:
            t = dt(1) / t
        if t_rand is not None:
            mids = dt(0.5) * (t[:, 1:] + t[:, :-1])
            upper, lower = np.concatenate([mids, t[:, -1:]], 1), np.concatenate([t[:, :1], mids], 1)
            t = lower + (upper - lower) * _in(t_rand, dt)
    return t


def t_unit(near, far, N, lindisp):
    """[B,N+1]: the float32 ulp of the largest |t| of each position's interval [t(n-1), t(n+1)] (finite entries)"""
    t = np.abs(sample_t(near, far, N, None, lindisp, F64))
    t = np.where(np.isfinite(t), t, 0)
    pad = np.concatenate([t[:, :1], t, t[:, -1:]], 1)
    big = np.maximum(np.maximum(pad[:, :-2], pad[:, 1:-1]), pad[:, 2:])
    return np.spacing(np.maximum(big, np.finfo(F32).tiny).astype(F32)).astype(F64)


def t_errors(got, near, far, N, t_rand, lindisp):
    """largest |got - oracle| over the finite oracle entries in ulps of t_unit; the inf / NaN pattern must be the oracle's"""
    ref = sample_t(near, far, N, t_rand, lindisp, F64)
    got = np.asarray(got, F32)
    fin = np.isfinite(ref.astype(F32))
    same = np.array_equal(np.isnan(got), np.isnan(ref)) and np.array_equal(got[np.isinf(ref)], ref[np.isinf(ref)].astype(F32))
    assert same and np.array_equal(np.isfinite(got), fin), 'inf / NaN pattern'
    if not fin.any():
        return 0.0
    with np.errstate(all='ignore'):
        return float((np.abs(got.astype(F64) - ref) / t_unit(near, far, N, lindisp))[fin].max())


def t_floor(pair, lindisp, kind):
    """the twin's t_errors over every N of T_NS at B = 3"""
    worst = 0.0
    for N in T_NS:
        near, far = np.full(3, pair[0], F32), np.full(3, pair[1], F32)
        tr = t_rand_of(kind, 3, N)
        worst = max(worst, t_errors(sample_t(near, far, N, tr, lindisp, F32), near, far, N, tr, lindisp))
    return worst


# ---------------------------------------------------------------------------
# view-direction encoding (mip.pos_enc(view, 0, 4))
# ---------------------------------------------------------------------------
HALF_PI_F32 = F32(1.5707963705062866)


def view_inputs(B):
    g = np.random.default_rng(77)
    fixed = np.array([X, Y, Z, _neg(X), _neg(Y), _neg(Z), (1, 1, 1), (-1, -1, -1), (0, 0, 0), (-0.0, -0.0, -0.0),
                      (1e-40, -1e-40, 0.0)], F32)
    r = g.normal(size=(max(B, 16), 3))
    v = np.concatenate([fixed, (r / np.linalg.norm(r, axis=1, keepdims=True)).astype(F32)])
    return np.ascontiguousarray(v[np.arange(B) % len(v)] if B < len(fixed) else v[:B])


def pos_enc(v, dt=F64):
    """[B,3] -> [B,27]: v, sin(2^i v_j), sin(2^i v_j + pi/2), degree-major; the twin adds float32(pi/2) as the kernel does"""
    v = _in(v, dt)
    xb = np.concatenate([v * dt(2 ** i) for i in range(4)], 1)
    shift = HALF_PI_F32 if dt is F32 else F64(0.5 * np.pi)
    return np.concatenate([v, np.sin(xb), np.sin(xb + shift)], 1)


VIEW_SHIFT = 2.0 ** -21             # y + float32(pi/2), |y| <= 8: the sum is rounded once, half an ulp of 9.6


def view_floor():
    v = view_inputs(257)
    return float(np.abs(pos_enc(v, F32).astype(F64) - pos_enc(v, F64)).max())


def bf16_rne(x):
    """float32 array -> the int16 bit patterns of its round-to-nearest-even bfloat16 (no NaN among the inputs)"""
    u = np.asarray(x, F32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16).view(np.int16)
