"""CPU side of tests/test_gpu_pose_edges.py: the base rays of the box-pose gradient kernels (csrc/pose.hip: k_encode_obj_bwd,
k_pose_reduce, k_pose_finish; csrc/pose_bkgd.h: k_encode_bkgd_bwd) and their per-ray float64 oracle.

A hit ray's 21 pose rows depend on that ray alone, so a launch of any size can be filled with copies of a few base rays and
held to the base launch bit for bit; only the base rays need a reference.  The reference is built from oracle.durf_ref
functions only: L = sum(encoding(cast_rays(t_vals, o', d')) * d_enc) with the object-frame (o', d') as leaves, one backward()
for every ray's g_o = dL/do', g_d = dL/dd' (rays are independent), and the 21 rows
    g_o | g_o (x) o_w | g_u (x) d_w,     u = R d_w, d^ = u / |u|, g_u = (g_d - d^ (d^ . g_d)) / |u|, R = aa2matrix(pose[3:]).
`dtype=torch.float32` runs the same code in fp32: the twin whose distance from float64 is the yardstick of the GPU gates.

The pose gradient is a sum over rays that cancels to ~1 % of its summed magnitudes, and a ray's g_o, g_d cancel over samples
and features in the same way.  Errors are therefore measured against a SCALE, never against the cancelled value: the sum over
samples and features of |d_enc[n,f] * d enc[n,f] / d o'_i| (forward mode, one tangent per input), pushed through the same
outer products.  No ray is left out of any comparison.

Base: K = 2 boxes well apart (half-extents >= 2), RAYS = 12 hand-aimed rays per box: an origin 8 units from a target point
inside the box, samples 3.2 units either side of it, so every ray hits its own box only and object-frame coordinates pass
0.62 (the safe_sin wrap at degree 9) on both signs.  The last two rays of each box aim within 0.02 of the box centre: their
samples fall on both sides of the 0.1 threshold of mip360.contract.  The world directions are not normalised."""
import math

import torch
import torch.nn.functional as F

from oracle import durf_ref as R

K = 2
RAYS = 12                                   # per box
NEAR_ORIGIN = (10, 11)                      # rays of each box aimed at its centre
ENC_CONTRACT, ENC_NO_INTEGRATION, ENC_CYLINDER = 1, 2, 4         # include/durf_hip.h DURF_ENC_*
N_LIST = (1, 64, 65, 128, 129, 256)         # P = 1 | 1 full | 2 partial | 2 full | 4 partial | 4 full
DENSITY_BIAS = -1.0
SEED = 5
REGIONS = ((0, 3), (3, 12), (12, 21))       # g_o | g_o (x) o_w | g_u (x) d_w
WRAP = 314.15927124023438 / 512             # |x| beyond which degree 9 wraps


def make_base(zero_rot=False):
    """world rays [K*RAYS, 3] (ray r of box k is row k*RAYS + r), radii, pose [K,6], ext [K,3] (half-extents): float32.
    zero_rot: box 1 with a zero rotation vector (aa2matrix's safe_norm branch), its rays aimed accordingly"""
    g = torch.Generator().manual_seed(SEED)
    pose = torch.tensor([[-8.0, 0.5, 0.3, 0.3, -0.2, 0.5], [9.0, -0.4, 0.2, -0.4, 0.6, 0.1]], dtype=torch.float64)
    if zero_rot:
        pose[1, 3:] = 0.0
    ext = torch.tensor([[2.0, 2.2, 2.5], [2.4, 2.0, 2.1]], dtype=torch.float64)
    rot = R.aa2matrix(pose[:, 3:])
    o_w, d_w, obj, mid = [], [], [], []
    for k in range(K):
        for r in range(RAYS):
            p = (torch.rand(3, generator=g, dtype=torch.float64) * 2 - 1) * (0.02 / math.sqrt(3) if r in NEAR_ORIGIN else 1.2)
            u = torch.randn(3, generator=g, dtype=torch.float64)
            u = u / u.norm()
            s = 0.8 + 0.5 * float(torch.rand((), generator=g, dtype=torch.float64))
            o_obj = p - 8.0 * u
            o_w.append(rot[k].T @ o_obj + pose[k, :3])
            d_w.append(rot[k].T @ u * s)
            obj.append(k)
            mid.append(8.0)
    radii = 1e-3 + 2e-3 * torch.rand(K * RAYS, generator=g, dtype=torch.float64)
    return dict(o_w=torch.stack(o_w).float(), d_w=torch.stack(d_w).float(), radii=radii.float(), pose=pose.float(),
                ext=ext.float(), obj=torch.tensor(obj), mid=torch.tensor(mid, dtype=torch.float64))


def make_t_vals(base, N, level=0):
    """[K*RAYS, N+1] float32, increasing: 3.2 units either side of each ray's target, jittered (another draw per level)"""
    g = torch.Generator().manual_seed(SEED * 1000 + N * 10 + level)
    n = base['mid'].shape[0]
    u = torch.linspace(0, 1, N + 1, dtype=torch.float64).expand(n, N + 1)
    u = u + (torch.rand(n, N + 1, generator=g, dtype=torch.float64) - 0.5) * (0.6 / N)
    near = base['mid'] - 3.2 + 0.1 * torch.rand(n, generator=g, dtype=torch.float64)
    far = base['mid'] + 3.2 - 0.1 * torch.rand(n, generator=g, dtype=torch.float64)
    return (near[:, None] + (far - near)[:, None] * u).float()


def make_d_enc(nrays, N, level=0):
    """[nrays*N, 64] float32.  Every column is filled: the kernels must not read column 63 (object) / 60..63 (background)."""
    g = torch.Generator().manual_seed(SEED * 2000 + N * 10 + level)
    return (torch.randn(nrays * N, 64, generator=g, dtype=torch.float64) * 0.1).float()


def make_raw_draw(nrays, N):
    """raw, draw [nrays*N, 4] float32; raw[:, 3] + DENSITY_BIAS covers x < -15, x > 20 and between on every ray with N >= 3"""
    g = torch.Generator().manual_seed(SEED * 3000 + N)
    raw = torch.randn(nrays * N, 4, generator=g, dtype=torch.float64) * 2
    draw = torch.randn(nrays * N, 4, generator=g, dtype=torch.float64) * 0.1
    raw[0::3, 3] -= 18.0 if N >= 3 else 0.0
    raw[1::3, 3] += 25.0 if N >= 3 else 0.0
    return raw.float(), draw.float()


def object_frame(o_w, d_w, pose, hit):
    """oracle.durf_ref's world2object_rpy, summed over the boxes a ray hits (hit [B,K] 0/1): what ray_setup hands the encoders"""
    B, Kb = o_w.shape[0], pose.shape[0]
    rot = R.aa2matrix(pose[:, 3:])
    oo, do = R.world2object_rpy(o_w, d_w, pose[:, :3].expand(B, Kb, 3), rot.expand(B, Kb, 3, 3))
    f = hit.to(o_w.dtype)[..., None]
    return (oo * f).sum(-2), (do * f).sum(-2)


def base_hits(base, pose=None, ext=None):
    """[B,K] from the oracle's ray_box_intersection in float64"""
    pose = base['pose'] if pose is None else pose
    ext = base['ext'] if ext is None else ext
    B, Kb = base['o_w'].shape[0], pose.shape[0]
    p64 = pose.double()
    rot = R.aa2matrix(p64[:, 3:])
    oo, do = R.world2object_rpy(base['o_w'].double(), base['d_w'].double(), p64[:, :3].expand(B, Kb, 3), rot.expand(B, Kb, 3, 3))
    dims = ext.double().expand(B, Kb, 3)
    return R.ray_box_intersection(oo, do, -dims, dims)[2]


# ---------------------------------------------------------------------------
# encodings
# ---------------------------------------------------------------------------
def _shape(flags):
    return 'cylinder' if flags & ENC_CYLINDER else 'cone'


def _samples(o, d, radii, t_vals, flags):
    means, covs = R.cast_rays(t_vals, o, d, radii[:, None], _shape(flags))
    if flags & ENC_NO_INTEGRATION:
        covs = torch.zeros_like(covs)
    return means, covs


def enc_obj(o, d, radii, t_vals, alpha, flags, wdiv=6):
    """[rays, N, 63]; wdiv = 6 is the model's BARF weight index (feature // 6: oracle.durf_ref.weighted_ipe itself); any other
    value restates it with feature // wdiv -- a WRONG encoding, the negative control of the GPU test"""
    s = _samples(o, d, radii, t_vals, flags)
    if wdiv == 6:
        return R.weighted_ipe(s, 0, 10, alpha)
    w = R.barf_weights(alpha, 10, o.dtype)
    return torch.cat([s[0], w[torch.clamp(torch.arange(60) // wdiv, max=9)] * R._ipe_core(s[0], s[1], 0, 10)], dim=-1)


def enc_bkgd(o, d, radii, t_vals, flags):
    """[rays, N, 60]"""
    s = _samples(o, d, radii, t_vals, flags)
    if flags & ENC_CONTRACT:
        s = R.new_space(s)
    return R.integrated_pos_enc(s, 0, 10)


def norm_term(raw, draw, nrays, dtype):
    """per ray: sum_n draw[n,3] softplus(x_n) / sigmoid(x_n) and the sum of its absolute terms, x = raw[n,3] + DENSITY_BIAS
    (mip.py:305: delta = t_dists |d_s|, so d(loss)/d|d_s| = sum_n density_n d(loss)/d(density_n) / |d_s|)"""
    x = raw[:, 3].to(dtype).reshape(nrays, -1) + DENSITY_BIAS
    t = draw[:, 3].to(dtype).reshape(nrays, -1) * (F.softplus(x) / torch.sigmoid(x))
    return t.sum(-1), t.abs().sum(-1)


def _ray_grads(enc_fn, o_s, d_s, d_enc, nfeat, dtype):
    o = o_s.to(dtype).clone().requires_grad_(True)
    d = d_s.to(dtype).clone().requires_grad_(True)
    enc = enc_fn(o, d)
    (enc * d_enc.to(dtype).reshape(enc.shape[0], enc.shape[1], 64)[..., :nfeat]).sum().backward()
    return o.grad, d.grad


def _abs_sums(enc_fn, o_s, d_s, d_enc, nfeat):
    """float64 [rays, 3] each: sum over samples and features of |d_enc * d enc / d o'_i|, and the same for d'_i; also the
    signed sums (= the backward's g_o, g_d: tests/test_pose_rows_ref.py holds them equal)"""
    o, d = o_s.double(), d_s.double()
    ge = d_enc.double().reshape(o.shape[0], -1, 64)[..., :nfeat]
    out = [torch.zeros(o.shape[0], 3, dtype=torch.float64) for _ in range(4)]
    for i in range(3):
        e = torch.zeros_like(o)
        e[:, i] = 1.0
        for which, (to, td) in enumerate(((e, torch.zeros_like(e)), (torch.zeros_like(e), e))):
            _, j = torch.func.jvp(enc_fn, (o, d), (to, td))
            t = ge * j
            out[which][:, i] = t.abs().sum((1, 2))
            out[2 + which][:, i] = t.sum((1, 2))
    return out


def _rows(g_o, g_d, o_w, d_w, pose, dtype, swap=False):
    """[rays, 21] from per-ray g_o, g_d [rays, 3], world rays and the per-ray pose [rays, 6] of the box the column belongs to.
    swap: o_w and d_w exchanged in the outer products -- a WRONG row layout, a negative control of the GPU test"""
    rot = R.aa2matrix(pose[:, 3:].to(dtype))
    ow, dw = o_w.to(dtype), d_w.to(dtype)
    u = torch.matmul(rot, dw[:, :, None])[:, :, 0]
    nrm = torch.sqrt((u * u).sum(-1, keepdim=True))
    dh = u / nrm
    g_u = (g_d - dh * (dh * g_d).sum(-1, keepdim=True)) / nrm
    a, b = (dw, ow) if swap else (ow, dw)
    return torch.cat([g_o, (g_o[:, :, None] * a[:, None, :]).reshape(-1, 9), (g_u[:, :, None] * b[:, None, :]).reshape(-1, 9)], -1)


def _scale(a_o, a_d, o_w, d_w, pose):
    """float64 [rays, 21]: the absolute sums through the same maps, every factor by its absolute value"""
    rot = R.aa2matrix(pose[:, 3:].double())
    ow, dw = o_w.double(), d_w.double()
    u = torch.matmul(rot, dw[:, :, None])[:, :, 0]
    nrm = torch.sqrt((u * u).sum(-1, keepdim=True))
    dh = u / nrm
    proj = (torch.eye(3, dtype=torch.float64) - dh[:, :, None] * dh[:, None, :]).abs()
    a_u = torch.matmul(proj, a_d[:, :, None])[:, :, 0] / nrm
    return torch.cat([a_o, (a_o[:, :, None] * ow.abs()[:, None, :]).reshape(-1, 9),
                      (a_u[:, :, None] * dw.abs()[:, None, :]).reshape(-1, 9)], -1)


def rows_obj(o_s, d_s, radii, t_vals, d_enc, alpha, flags, o_w, d_w, pose, dtype=torch.float64, wdiv=6, swap=False,
             want_scale=True):
    """k_encode_obj_bwd's columns: rows [rays, 21] in `dtype` and the float64 scale [rays, 21] (None unless want_scale).
    o_s, d_s: the object-frame rays as the kernel reads them; d_enc [rays*N, 64] ray-major; pose [rays, 6] per ray."""
    def fn(o, d):
        return enc_obj(o, d, radii.to(o.dtype), t_vals.to(o.dtype), alpha, flags, wdiv)
    g_o, g_d = _ray_grads(fn, o_s, d_s, d_enc, 63, dtype)
    rows = _rows(g_o, g_d, o_w, d_w, pose, dtype, swap)
    if not want_scale:
        return rows, None
    a_o, a_d, _, _ = _abs_sums(fn, o_s, d_s, d_enc, 63)
    return rows, _scale(a_o, a_d, o_w, d_w, pose)


def rows_bkgd(o_s, d_s, radii, t_vals, d_enc, flags, o_w, d_w, pose, raw=None, draw=None, dtype=torch.float64, want_scale=True):
    """k_encode_bkgd_bwd's columns; d_enc [rays*N, 64] ray-major (60 features, no identity, no BARF weights); raw / draw
    [rays*N, 4] add the |d_s| term to g_d"""
    def fn(o, d):
        return enc_bkgd(o, d, radii.to(o.dtype), t_vals.to(o.dtype), flags)
    g_o, g_d = _ray_grads(fn, o_s, d_s, d_enc, 60, dtype)
    dd = d_s.to(dtype)
    dsq = (dd * dd).sum(-1, keepdim=True)
    if raw is not None:
        gn, _ = norm_term(raw, draw, o_s.shape[0], dtype)
        g_d = g_d + gn[:, None] * dd / dsq
    rows = _rows(g_o, g_d, o_w, d_w, pose, dtype)
    if not want_scale:
        return rows, None
    a_o, a_d, _, _ = _abs_sums(fn, o_s, d_s, d_enc, 60)
    if raw is not None:
        _, gabs = norm_term(raw, draw, o_s.shape[0], torch.float64)
        a_d = a_d + gabs[:, None] * d_s.double().abs() / (d_s.double() ** 2).sum(-1, keepdim=True)
    return rows, _scale(a_o, a_d, o_w, d_w, pose)


def region_errors(got, want, scale):
    """the largest |got - want| / scale over the rays and rows of each of the three row regions"""
    e = (got.double() - want.double()).abs() / scale
    return tuple(float(e[:, a:b].max()) for a, b in REGIONS)


# ---------------------------------------------------------------------------
# sums [K,21] -> d(loss)/d(pose) [K,6]
# ---------------------------------------------------------------------------
def pose_finish_ref(pose, sums, want_pos=True, want_rot=True):
    """k_pose_finish's map in the dtype of `pose` (float64: the reference; float32: its twin): dL/dc = -R^T sum g_o,
    dL/dr_i = <G, dR/dr_i> with G = sum g_o (x) (o_w - c) + sum g_u (x) d_w and R = aa2matrix(r) (box_helpers.py:148-167,
    whose safe_norm makes theta a constant below |r|^2 = 1e-12)"""
    dt = pose.dtype
    sums = sums.to(dt)
    c, r = pose[:, :3], pose[:, 3:]
    rot = R.aa2matrix(r)
    s0 = (r * r).sum(-1)
    tiny = s0 < 1e-12
    rt = torch.sqrt(torch.where(tiny, torch.full_like(s0, 1e-12), s0))
    th = rt + 1e-12
    sn, cs = torch.sin(th), torch.cos(th)
    a, b = sn / th, (1 - cs) / th ** 2
    da = (th * cs - sn) / th ** 2
    db = (th * sn - 2 * (1 - cs)) / th ** 3
    z = torch.zeros_like(s0)
    km = torch.stack([torch.stack([z, -r[:, 2], r[:, 1]], -1), torch.stack([r[:, 2], z, -r[:, 0]], -1),
                      torch.stack([-r[:, 1], r[:, 0], z], -1)], -2)
    k2 = torch.matmul(km, km)
    G = sums[:, 3:12].reshape(-1, 3, 3) - sums[:, :3, None] * c[:, None, :] + sums[:, 12:21].reshape(-1, 3, 3)
    out = torch.zeros(pose.shape[0], 6, dtype=dt)
    if want_pos:
        out[:, :3] = -torch.matmul(rot.transpose(-1, -2), sums[:, :3, None])[:, :, 0]
    if want_rot:
        for i in range(3):
            E = torch.zeros(3, 3, dtype=dt)
            j, l = (i + 1) % 3, (i + 2) % 3
            E[l, j], E[j, l] = 1.0, -1.0                      # skew(e_i)
            dth = torch.where(tiny, z, r[:, i] / rt)
            dR = ((da * dth)[:, None, None] * km + a[:, None, None] * E + (db * dth)[:, None, None] * k2 +
                  b[:, None, None] * (torch.matmul(E.expand_as(km), km) + torch.matmul(km, E.expand_as(km))))
            out[:, 3 + i] = (G * dR).sum((-1, -2))
    return out


def pose_finish_autograd(pose, sums):
    """float64 autograd of the function whose gradient the sums stand for: L(c, r) = sum g_o . R (o_w - c) + sum g_u . R d_w"""
    p = pose.double().clone().requires_grad_(True)
    s = sums.double()
    rot = R.aa2matrix(p[:, 3:])
    L = ((s[:, 3:12] + s[:, 12:21]).reshape(-1, 3, 3) * rot).sum() - (s[:, :3] * torch.matmul(rot, p[:, :3, None])[:, :, 0]).sum()
    L.backward()
    return p.grad


ROTATIONS = (('zero', 0.0), ('below', 5e-7), ('above', 2e-6), ('one', 1.0), ('near_pi', math.pi - 1e-3))


def make_finish_case(Kf, seed, first=0):
    """pose [Kf,6] whose rotations walk ROTATIONS from `first` (object k: class (first + k) % 5), random sums [Kf,21] and a
    non-zero grad6 [Kf,6] to add into: float32.  -> pose, sums, grad6, class names"""
    g = torch.Generator().manual_seed(SEED * 4000 + seed)
    pose = torch.randn(Kf, 6, generator=g, dtype=torch.float64)
    names = []
    for k in range(Kf):
        name, mag = ROTATIONS[(first + k) % len(ROTATIONS)]
        v = pose[k, 3:] / pose[k, 3:].norm()
        pose[k, 3:] = v * mag
        names.append(name)
    sums = torch.randn(Kf, 21, generator=g, dtype=torch.float64)
    grad6 = torch.randn(Kf, 6, generator=g, dtype=torch.float64)
    return pose.float(), sums.float(), grad6.float(), names


# ---------------------------------------------------------------------------
# the base cases of tests/test_gpu_pose_edges.py and the float32 twin's floors
# ---------------------------------------------------------------------------
C, NI, CY = ENC_CONTRACT, ENC_NO_INTEGRATION, ENC_CYLINDER
ALPHA = 3.3
# object kernel: (N, flags, alpha); N = 8 is the base of the copy-filled launches
OBJ_CASES = tuple((n, 0, ALPHA) for n in (8,) + N_LIST) + ((65, CY, ALPHA), (65, NI, ALPHA), (65, CY | NI, ALPHA),
                                                          (64, 0, 0.0), (64, 0, 10.0))
# background kernel: (N, flags, variant); 'raw': with the |d_s| term; 'two': two coincident boxes (rays in both), with the term
BKGD_CASES = (tuple((n, C, 'plain') for n in N_LIST) + ((65, 0, 'plain'), (65, C | NI, 'plain'), (65, C | CY, 'plain'),
                                                       (65, C, 'raw'), (65, 0, 'raw'), (65, C, 'two'), (8, C, 'raw')))


def variant_base(variant):
    """the base of a case: 'two' keeps box 0's rays and doubles the box (same pose, same extents: every ray is in both)"""
    b = make_base()
    if variant == 'two':
        b = dict(b, o_w=b['o_w'][:RAYS], d_w=b['d_w'][:RAYS], radii=b['radii'][:RAYS], obj=b['obj'][:RAYS], mid=b['mid'][:RAYS],
                 pose=b['pose'][[0, 0]].contiguous(), ext=b['ext'][[0, 0]].contiguous())
    return b


def cpu_object_frame(b):
    """float32 (o_s, d_s) of a base from the float64 oracle (the GPU test takes them from the device's own ray_setup)"""
    o, d = object_frame(b['o_w'].double(), b['d_w'].double(), b['pose'].double(), base_hits(b, b['pose'], b['ext']))
    return o.float(), d.float()


def case_rows(kind, case, b, o_s, d_s, dtype=torch.float64, want_scale=True, **kw):
    """the oracle's (rows, scale) of one base case on the object-frame rays given"""
    n = b['o_w'].shape[0]
    pose = b['pose'][b['obj']]
    N = case[0]
    t, de = make_t_vals(b, N), make_d_enc(n, N)
    if kind == 'obj':
        return rows_obj(o_s, d_s, b['radii'], t, de, case[2], case[1], b['o_w'], b['d_w'], pose, dtype, want_scale=want_scale, **kw)
    raw, draw = make_raw_draw(n, N) if case[2] in ('raw', 'two') else (None, None)
    return rows_bkgd(o_s, d_s, b['radii'], t, de, case[1], b['o_w'], b['d_w'], pose, raw, draw, dtype, want_scale)


def twin_floor(kind, case):
    """max_j |rows of the float32 twin - rows in float64| / scale_j for the three row regions, on the CPU"""
    b = variant_base(case[2] if kind == 'bkgd' else 'plain')
    o_s, d_s = cpu_object_frame(b)
    r64, sc = case_rows(kind, case, b, o_s, d_s)
    r32, _ = case_rows(kind, case, b, o_s, d_s, torch.float32, False)
    return region_errors(r32, r64, sc)


# durf_pose_finish: (K, class of object 0); every rotation class appears at K = 1 and inside a larger call
FINISH_CASES = tuple((1, f) for f in range(len(ROTATIONS))) + ((3, 0), (3, 2), (16, 0))
HALVES = (('pos', slice(0, 3)), ('rot', slice(3, 6)))


def finish_errors(got, pose, sums, grad6, names, want_pos, want_rot):
    """{(rotation class, half): the largest norm-wise distance of an object's half of `got` from grad6 + float64 autograd,
    relative to the autograd's half} over the objects of one call; only the halves that were asked for"""
    want = pose_finish_autograd(pose, sums)
    out = {}
    for k, name in enumerate(names):
        for (half, sl), on in zip(HALVES, (want_pos, want_rot)):
            if on:
                e = float((got[k, sl].double() - (grad6[k, sl].double() + want[k, sl])).norm() / want[k, sl].norm())
                out[(name, half)] = max(out.get((name, half), 0.0), e)
    return out


def finish_floors():
    """the float32 twin (pose_finish_ref in float32, added into the float32 grad6) over FINISH_CASES with both halves wanted"""
    out = {}
    for Kf, first in FINISH_CASES:
        pose, sums, grad6, names = make_finish_case(Kf, Kf * 10 + first, first)
        twin = grad6 + pose_finish_ref(pose, sums)
        for key, e in finish_errors(twin, pose, sums, grad6, names, True, True).items():
            out[key] = max(out.get(key, 0.0), e)
    return out
