"""The sample encoders (csrc/rays.hip k_encode<false|true>, k_encode_lane<false|true>; csrc/enc_lane.h; csrc/gauss.h) held to
a per-sample float64 oracle at their edges.  Rays, truth, classes and budgets: tests/enc_rows_ref.py (E below); every output
buffer starts as 0xFF bytes; comparisons run on the device.

(a) test_base_launch_against_the_float64_oracle: all E.GROUPS (8 flag sets x hit columns 3 | 0 for the background form, 4 flag
    sets x alpha 0 / 2.5 / 4.5 / 6.5 / 10 for the object form), E.B rays x 32 samples.  Gates per feature, against
    E.encode(group) in float64 (the reference's meaning: wrap by the float32 100 pi, cosine half at fl32(y + fl32(pi/2)));
    b = E.bounds(group):
      fp32 path   |got - truth| <= 1e-5 + b.cond               (b.cond: 4 x the float32 twin's conditioning terms)
      lane path   |got - bf16(truth)| <= ulp_bf16(max(|.|, |.|)) + floor + b.cond, floor = b.small (v_fract branch) or b.big
                  (exact-wrap branch), the larger within 1e-4 of the switch; where |truth| < 2^-126 the gate has 2^-126 more:
                  the kernel's float32 product may be flushed to 0 there while bf16(truth) is a denormal (labels thick,
                  var_big, var_cross, n01_hi; the values concerned are <= 1.2e-38);
                  mean |got - truth| < 1.5e-3 per label and launch, over all 60 features; left out by name: label n1e6 in
                  the groups without the contraction (MEAN_EXEMPT: measured 0.10, the conditioning of x = 1e6).
    The tile of the fp32 call is bf16(its fp32 output) exactly; object slots 0-2 of the lane tile are bf16(g.x of the fp32 path)
    exactly; the pad slots are exactly 0; features with BARF weight 0 are exactly 0.  The two-hit ray (out of domain): the fp32
    path is NaN / inf or within rtol 1e-2, atol 1e-3 of the truth; the lane path writes every row of it (pad slots 0, no
    fill) with whatever value its absolute error times e ~ 1e16 gives; on both paths its two neighbours carry the bits of the
    same plain ray elsewhere in the launch.
(b) Position invariance (seed 20240 + a case number for every permutation): launches filled with permuted copies of the base
    rays must give the base launch's bits at every valid row and leave the 0xFF fill everywhere else.
      k_encode_lane<false>   1 ray (one 32-row tile); 9 rays (288 rows: a partial 256-thread block); 3 x E.B rays; K = 3 / 0
      N = 96                 1 ray (96 rows), 9 rays (864 rows: three blocks and a partial one), K = 3 / 1 / 0 hit columns:
                             row / N and row % N are no shifts; lane and fp32 background encoders, lane object encoder
      idx / count (lane)     count 0 (nothing written), 5, = capacity; idx a permutation, rays beyond the list
      k_encode<false> + idx  count > rays: the min(count, rays) clamp; rows beyond keep the fill
      durf_encode_obj        count 0, 1, max_rays; fp32 with 4100 rays x 32 = 131 200 rows > 4096 x 256 / 8: the capped grid
                             strides
      ..._obj_f32_batch      K = 3, counts (0, 5, 600): 600 x 32 x 8 / 256 = 600 blocks > 512, so that object strides and the
                             others do not; idx_stride / f32_stride per object; the zero-count slab keeps the fill
      durf_obj_fwd_batch     K = 3, counts (0, 5, all), training and inference slabs (ops.ObjSlabs): every object's enc slab
                             is ops.encode_obj(..., f32=False) bit for bit, the rest of the slab keeps the fill
    Surplus rows of a partial last tile: not reachable for the background encoder (durf_encode_bkgd requires B * N % 32 == 0
    for tiles, so count * N is a multiple of 32 as well) and not reached for the object encoders here (N = 32 and 96 give
    whole tiles); no statement about them is made.
(c) ops.mlp_fwd_enc on the base rays (fixed weights, seed 7), contraction on and off, K = 3 / 0: the encoding tile it returns
    is bit-identical to ops.encode_bkgd(..., f32=False) -- on lanes in the big branch, at the wrap, at the contraction switch.
    The object forward likewise: the durf_obj_fwd_batch case of (b).
(d) Negative controls: the EXPECTED side corrupted, the gates of (a) / (b) must reject exactly the rows concerned (cosine half
    one degree up; BARF index f // 3; contraction switch at 0.11; exact-period wrap; one ray's rows swapped).  For the first
    two the failing set of the fp32 gate is derived from the corruption (_exact_set): more than two gates from the truth
    must fail, unchanged must pass.

Worst figures per label and branch over all 36 groups, on an MI355X (test_report_of_the_base_launches prints this table):
fp32 and lane error as a fraction of their gates; what the lane path adds beyond half a bf16 ulp and b.cond as a fraction of
its documented floor (huge / big: the 1e-4 __sinf figure at |m| ~ 300 is used to 0.18); mean |lane - truth|.
  label      branch  fp32 err/gate  lane err/gate  lane excess/floor  mean |lane - truth|
  axis       big             0.22           0.98               0.00              8.3e-04
  axis       small           0.24           1.00               0.00              8.3e-04
  dzero      small           0.22           0.99               0.05              8.6e-04
  hit1       small           0.25           0.98               0.00              7.7e-04
  hit2       small           0.25           0.98               0.00              7.7e-04
  huge       big             0.01           0.99               0.18              7.7e-04
  huge       small           0.15           0.00               0.00              6.1e-04
  n01_hi     big             0.27           1.00               0.00              5.5e-04
  n01_hi     small           0.15           0.00               0.00              5.0e-04
  n01_lo     small           0.17           1.00               0.01              6.0e-04
  n1         small           0.26           0.97               0.00              6.3e-04
  n1e3       big             0.50           0.95               0.00              9.9e-04
  n1e3       small           0.26           1.00               0.00              5.9e-04
  n1e6       big             0.31           0.55               0.00              1.0e-01
  n1e6       small           0.30           0.99               0.00              5.9e-04
  n2         small           0.26           0.99               0.00              6.4e-04
  nonunit    big             0.30           0.93               0.00              7.5e-04
  nonunit    small           0.23           0.99               0.00              7.7e-04
  obj40      big             0.50           0.97               0.00              7.5e-04
  obj40      small           0.25           0.96               0.00              7.5e-04
  plain      small           0.25           0.98               0.00              7.7e-04
  radius0    small           0.25           0.99               0.00              7.7e-04
  switch_hi  big             0.84           0.98               0.00              8.0e-04
  switch_hi  small           0.26           0.98               0.00              7.5e-04
  switch_lo  small           0.94           0.98               0.00              8.0e-04
  t_equal    small           0.30           0.99               0.00              7.5e-04
  thick      big             0.32           0.99               0.00              1.3e-03
  thick      small           0.27           0.98               0.00              7.7e-04
  thin       small           0.27           1.00               0.00              7.3e-04
  tiny       small           0.01           0.19               0.19              1.9e-04
  var0       small           0.30           0.00               0.00              7.5e-04
  var_big    small           0.29           0.98               0.00              7.8e-04
  var_cross  small           0.29           0.98               0.00              7.8e-04
  wrap       big             0.50           0.99               0.00              8.3e-04
  wrap       small           0.43           1.00               0.10              8.0e-04
  zero       small           0.00           0.00               0.00              2.2e-04
(lane err/gate near 1: the bf16 ulp term, a re-rounding flip is a whole ulp.  hit2: the groups without hit columns.)
Every comparison passed on the kernels as they stand: nothing had to be fixed.
"""
import ctypes as C
import functools

import pytest
import torch

from durf_amd import _lib, ops
from tests import enc_rows_ref as E

pytestmark = pytest.mark.gpu
N = E.N
SEED = 20240
I32 = torch.int32


def _ff(n, dtype, dev):
    """n elements of `dtype`, every byte 0xFF (NaN in fp32 and bf16)"""
    return torch.full((n * torch.empty(0, dtype=dtype).element_size(),), 0xFF, dtype=torch.uint8, device=dev).view(dtype)


def _is_fill(t):
    return bool((t.contiguous().view(torch.uint8) == 0xFF).all())


def _rows16(tile, rows):
    """bf16 tile buffer -> [rows, 64] int16 bit patterns in natural feature order (rows a multiple of 32)"""
    t = tile.reshape(-1)[:rows * 64].view(torch.int16).reshape(rows // 32, 4, 2, 32, 8)
    return t.permute(0, 3, 1, 2, 4).reshape(rows, 64)


def _bf(rows16):
    return rows16.contiguous().view(torch.bfloat16).double()


def _inputs(cuda, pick=None, k=3):
    """the base rays (or the copies `pick`) on the device: (t_vals, origins, dirs, radii, hit | None)"""
    sel = (lambda t: t) if pick is None else (lambda t: t[pick])
    g = lambda t: sel(t).contiguous().to(cuda)
    return g(E.T_VALS), g(E.ORIGINS), g(E.DIRS), g(E.RADII), (g(E.HIT[:, :k]) if k else None)


SLACK = 64            # rows of fill behind every output
FLUSH = 2.0 ** -126   # the smallest normal float32 (bf16 shares the exponent range)


def _bkgd(inp, flags, f32, idx=None, count=None):
    """durf_encode_bkgd into 0xFF buffers -> (tile buffer [(rows + SLACK) * 64] bf16, fp32 [(rows + SLACK), 60] | None)"""
    tv, o, d, r, hit = inp
    B, dev, n = tv.shape[0], tv.device, tv.shape[1] - 1
    tile = None if (f32 and idx is not None) else _ff((ops.tile_rows(B * n) + SLACK) * 64, torch.bfloat16, dev)
    of = _ff((B * n + SLACK) * 60, torch.float32, dev).reshape(-1, 60) if f32 else None
    _lib.check(_lib.lib().durf_encode_bkgd(ops._stream(), B, n, ops._p(tv), ops._p(o), ops._p(d), ops._p(r), ops._p(hit),
                                           0 if hit is None else hit.shape[1], flags, ops._p(tile), ops._p(of), ops._p(idx),
                                           ops._p(count)), 'durf_encode_bkgd')
    return tile, of


def _barf(alpha):
    return (C.c_float * 10)(*[float(x) for x in ops.barf_weights(alpha)])


def _obj(inp, flags, alpha, f32, idx, count, max_rays):
    tv, o, d, r, _ = inp
    dev, n = tv.device, tv.shape[1] - 1
    tile = _ff((ops.tile_rows(max_rays * n) + SLACK) * 64, torch.bfloat16, dev)
    of = _ff((max_rays * n + SLACK) * 63, torch.float32, dev).reshape(-1, 63) if f32 else None
    _lib.check(_lib.lib().durf_encode_obj(ops._stream(), max_rays, n, ops._p(idx), ops._p(count), ops._p(tv), ops._p(o),
                                          ops._p(d), ops._p(r), _barf(alpha), flags, ops._p(tile), ops._p(of)), 'durf_encode_obj')
    return tile, of


def _iota(n, dev):
    return torch.arange(n, dtype=I32, device=dev), torch.tensor([n], dtype=I32, device=dev)


@functools.lru_cache(maxsize=None)
def _truth(group):
    t = E.encode(group)
    return t, E.bounds(group, t)


def _ulp_bf16(v):
    a = v.abs()
    return torch.where(a > 0, torch.exp2(torch.floor(torch.log2(a.clamp(min=2.0 ** -126))) - 7), torch.zeros_like(a))


def _run_base(cuda, group):
    """both paths of `group` on the base rays -> (fp32 rows [B*N, dim] float32, fp32 call's tile rows, lane tile rows)"""
    kind, flags, k, alpha = group
    inp = _inputs(cuda, k=k)
    rows = E.B * N
    if kind == 'bkgd':
        t1, of = _bkgd(inp, flags, True)
        t2, _ = _bkgd(inp, flags, False)
    else:
        idx, count = _iota(E.B, cuda)
        t1, of = _obj(inp, flags, alpha, True, idx, count, E.B)
        t2, _ = _obj(inp, flags, alpha, False, idx, count, E.B)
    for t in (t1, t2):
        assert _is_fill(t[rows * 64:]), 'fill behind the last tile'
    assert _is_fill(of[rows:]), 'fill behind the last fp32 row'
    return of[:rows], _rows16(t1, rows), _rows16(t2, rows)


def _gate(group, of, lane16, expected=None):
    """-> (fail_f32 [B, N] bool, fail_lane [B, N] bool, stats): the per-feature gates of (a), a sample fails with any feature.
    expected: a corrupted float64 encoding in place of the truth (negative controls); the budgets stay the truth's."""
    t, b = _truth(group)
    dev = of.device
    off = 3 if group[0] == 'obj' else 0
    enc = (t['enc'] if expected is None else expected)[..., off:].to(dev)
    bd = {k: v.to(dev) for k, v in b.items()}
    got = of.double().reshape(E.B, N, -1)[..., off:]
    err32 = (got - enc).abs()
    gate32 = 1e-5 + bd['cond']
    lane = _bf(lane16).reshape(E.B, N, 64)[..., off:off + 60]
    ref16 = enc.to(torch.bfloat16).double()
    big, near = bd['is_big'][..., None], bd['near'][..., None]
    floor = torch.where(near, torch.maximum(bd['small'], bd['big']), torch.where(big, bd['big'], bd['small']))
    errl = (lane - ref16).abs()
    # (FLUSH: only where the truth itself is below the smallest normal float32 -- there the kernel's product may be flushed
    # to 0 while bf16(truth) is a denormal; labels thick, var_big, var_cross, n01_hi, values <= 1.2e-38)
    gatel = _ulp_bf16(torch.maximum(lane.abs(), ref16.abs())) + floor + bd['cond'] + FLUSH * (enc.abs() < FLUSH)
    # what the kernel adds beyond the re-rounding flip, against its documented floor (the figure recorded in the docstring)
    excess = ((lane - enc).abs() - 0.5 * _ulp_bf16(lane) - bd['cond']).clamp(min=0) / floor.clamp(min=1e-30)
    stats = dict(r32=torch.nan_to_num(err32 / gate32), rl=torch.nan_to_num(errl / gatel), excess=excess, big=bd['is_big'],
                 mean_l=(lane - enc).abs(), gate32=gate32)
    return ~(err32 <= gate32).all(-1), ~(errl <= gatel).all(-1), stats


WORST = {}            # (label, branch) -> [fp32 err/gate, lane err/gate, lane excess/floor, mean |lane - truth|], over the groups run
GROUPS_RUN = set()
# Labels left out of the 1.5e-3 mean ceiling, by name, in the groups WITHOUT the contraction (object form included): their
# coordinates are 1e6, so at the upper degrees 2^deg ulp32(x) is radians and the mean measures the inputs' conditioning.
# Their features stay under the per-feature gates like all others.
MEAN_EXEMPT = ('n1e6',)    # ulp32(1e6) = 0.0625: from degree 5 the float32 argument is a radian off; measured mean 0.10


@pytest.mark.parametrize('group', E.GROUPS, ids=lambda g: '%s-f%d-k%d-a%s' % g)
def test_base_launch_against_the_float64_oracle(cuda, group):
    kind, flags, k, alpha = group
    of, t1, lane16 = _run_base(cuda, group)
    t, b = _truth(group)
    dom = E.in_domain(group).to(cuda)
    dim = 63 if kind == 'obj' else 60
    # exact statements
    assert torch.equal(t1[:, :dim], of.to(torch.bfloat16).view(torch.int16)), 'tile of the fp32 call == bf16(its fp32 output)'
    assert bool((_bf(t1)[:, dim:] == 0).all()) and bool((_bf(lane16)[:, dim:] == 0).all()), 'pad slots'
    if kind == 'obj':
        assert torch.equal(lane16[:, :3], of[:, :3].to(torch.bfloat16).view(torch.int16)), 'lane slots 0-2 == bf16(g.x)'
        zero_w = (b['w'] == 0).nonzero().flatten().to(cuda) + 3
        assert bool((of[:, zero_w] == 0).all()) and bool((_bf(lane16)[:, zero_w] == 0).all()), 'weight 0 -> exactly 0'
        x = t['x'].to(cuda).reshape(-1, 3)
        dxu = torch.tensor([E.YARDSTICK[('plain' if l == 'hit2' else l, False)][0] for l in E.LABELS], device=cuda)
        okx = (of[:, :3].double() - x).abs() <= 4 * dxu.repeat_interleave(N)[:, None] * E._ulp32(x)
        assert bool(okx.all()), 'coordinates (slots 0-2 of the fp32 path)'
    f32_bad, lane_bad, st = _gate(group, of, lane16)
    # the declared out-of-domain rows: the fp32 path NaN / inf or close (test_encode_bkgd's tolerance for such rows); the lane
    # path, whose absolute error is multiplied by e ~ 1e16 there: every row written (pad slots 0, no fill left), any value
    for i in (~dom).nonzero().flatten().tolist():
        want = t['enc'][i].to(cuda)
        got = of.double().reshape(E.B, N, -1)[i]
        ok = ~torch.isfinite(got) | torch.isclose(got, want, rtol=1e-2, atol=1e-3, equal_nan=True)
        assert bool(ok.all()), 'out-of-domain ray %d' % i
        lrow = lane16.reshape(E.B, N, 64)[i]
        assert bool((lrow[:, dim:] == 0).all()) and not bool((lrow == -1).all(-1).any()), 'lane rows of ray %d written' % i
        # its neighbours (the same plain ray before and after it) carry the bits of a plain ray far from it
        first = E.rays_of('plain')[0]
        for tl in (t1, lane16):
            r = tl.reshape(E.B, N, 64)
            assert torch.equal(r[i - 1], r[first]) and torch.equal(r[i + 1], r[first]), 'neighbours of ray %d' % i
    # figures before the assertions
    over = []
    for lab in sorted(set(E.LABELS)):
        rows = torch.tensor(E.rays_of(lab), device=cuda)
        rows = rows[dom[rows]]
        if rows.numel() == 0:
            continue
        mean = float(st['mean_l'][rows].mean())
        if mean >= 1.5e-3 and not (lab in MEAN_EXEMPT and not E.contracted(group)):
            over.append((lab, mean))
        bigm = st['big'][rows]
        for name, m in (('small', ~bigm), ('big', bigm)):
            if not bool(m.any()):
                continue
            vals = [float(st['r32'][rows][m].max()), float(st['rl'][rows][m].max()), float(st['excess'][rows][m].max()),
                    float(st['mean_l'][rows][m].mean())]
            w = WORST.setdefault((lab, name), [0.0] * 4)
            WORST[(lab, name)] = [max(a, c) for a, c in zip(w, vals)]
    GROUPS_RUN.add(group)
    assert bool(torch.isfinite(of[dom.repeat_interleave(N)]).all())
    bad = lambda m: [(E.LABELS[i], i) for i in (m & dom[:, None]).any(-1).nonzero().flatten().tolist()]
    assert not bad(f32_bad), 'fp32 path outside its gate: %s' % bad(f32_bad)
    assert not bad(lane_bad), 'lane path outside its gate: %s' % bad(lane_bad)
    assert not over, 'mean |lane - truth| per label: %s' % over
    # consistency across the branch switch: both sides were held to their own oracle values above, and both branches ran
    if E._unc(group):
        lo, hi = E.rays_of('switch_lo'), E.rays_of('switch_hi')
        assert not bool(st['big'][lo].any()) and bool(st['big'][hi].all())


def test_report_of_the_base_launches():
    """prints the table of the module docstring (worst figures per label and branch over the groups run so far); after a
    whole run of (a) it also holds that table to the gates"""
    print('label      branch  fp32 err/gate  lane err/gate  lane excess/floor  mean |lane - truth|   (%d groups)' % len(GROUPS_RUN))
    for (lab, name), v in sorted(WORST.items()):
        print('  %-10s %-6s %13.2f  %13.2f  %17.2f  %19.1e' % ((lab, name) + tuple(v)))
    if len(GROUPS_RUN) == len(E.GROUPS):
        assert all(v[0] <= 1 and v[1] <= 1 for v in WORST.values())


# ---------------------------------------------------------------------------------------------------------------- (b)
def _pick(n, seed=SEED):
    """n ray numbers: whole shuffled copies of the base set (seeded), so every base ray is there when n >= E.B"""
    g = torch.Generator().manual_seed(seed)
    return torch.cat([torch.randperm(E.B, generator=g) for _ in range((n + E.B - 1) // E.B)])[:n]


def _same_rows(got16, base16, pick, what):
    """got16 [len(pick) * N, 64] must be base16's rows of rays `pick`, bit for bit -> the rays that differ"""
    want = base16.reshape(E.B, N, 64)[pick.to(base16.device)]
    diff = (got16.reshape(-1, N, 64) != want).any(-1).any(-1)
    return diff.nonzero().flatten().tolist()


@pytest.mark.parametrize('k', [3, 0])
@pytest.mark.parametrize('flags', [1, 0])
def test_lane_bkgd_rows_do_not_depend_on_the_launch(cuda, flags, k):
    base, _ = _bkgd(_inputs(cuda, k=k), flags, False)
    base16 = _rows16(base, E.B * N)
    for n in (1, 9, 3 * E.B):                   # one tile; 288 rows: a partial 256-thread block; more than one block
        pick = _pick(n, SEED + n)
        tile, _ = _bkgd(_inputs(cuda, pick, k), flags, False)
        assert _same_rows(_rows16(tile, n * N), base16, pick, n) == [], n
        assert _is_fill(tile[n * N * 64:]), n
    # the negative control of this comparison: one ray's rows swapped on the expected side
    pick = _pick(9, SEED + 9)
    tile, _ = _bkgd(_inputs(cuda, pick, k), flags, False)
    wrong = pick.clone()
    wrong[4] = pick[5]
    assert pick[4] != pick[5] and _same_rows(_rows16(tile, 9 * N), base16, wrong, 'control') == [4]


@pytest.mark.parametrize('count', [0, 5, 'capacity'])
def test_lane_bkgd_compacted_list(cuda, count):
    n = E.B + 7                                  # rays in the arrays; the list names `count` of them, in shuffled order
    pick = _pick(n, SEED + 1)
    inp = _inputs(cuda, pick, 3)
    c = n if count == 'capacity' else count
    g = torch.Generator().manual_seed(SEED + 2)
    idx = torch.randperm(n, generator=g).to(I32).to(cuda)
    cnt = torch.tensor([c], dtype=I32, device=cuda)
    base16 = _rows16(_bkgd(_inputs(cuda, k=3), 1, False)[0], E.B * N)
    tile, _ = _bkgd(inp, 1, False, idx, cnt)
    rows = c * N                                 # (whole tiles: durf_encode_bkgd requires B * N % 32 == 0)
    assert _is_fill(tile[rows * 64:])
    if c:
        assert _same_rows(_rows16(tile, rows), base16, pick[idx[:c].cpu().long()], count) == []


def test_f32_bkgd_compacted_list_clamps_the_count(cuda):
    n = 11
    pick = _pick(n, SEED + 3)
    inp = _inputs(cuda, pick, 3)
    idx = torch.randperm(n, generator=torch.Generator().manual_seed(SEED + 4)).to(I32).to(cuda)
    _, base = _bkgd(_inputs(cuda, k=3), 1, True)
    base = base[:E.B * N].view(I32).reshape(E.B, N, 60)
    for c in (n + 1000, n, 3, 0):                # count > rays: min(count, rays)
        _, of = _bkgd(inp, 1, True, idx, torch.tensor([c], dtype=I32, device=cuda))
        m = min(c, n)
        assert _is_fill(of[m * N:]), c
        want = base[pick[idx[:m].cpu().long()].to(cuda)]
        assert torch.equal(of[:m * N].view(I32).reshape(m, N, 60), want), c


@pytest.mark.parametrize('f32', [False, True])
def test_obj_counts_and_the_capped_grid(cuda, f32):
    alpha, flags = 4.5, 0
    idx0, cnt0 = _iota(E.B, cuda)
    bt, bf = _obj(_inputs(cuda), flags, alpha, True, idx0, cnt0, E.B)
    lane = _rows16(_obj(_inputs(cuda), flags, alpha, False, idx0, cnt0, E.B)[0], E.B * N)
    base32 = bf[:E.B * N].view(I32).reshape(E.B, N, 63)
    base16 = _rows16(bt, E.B * N) if f32 else lane
    max_rays = 4100 if f32 else 3 * E.B          # fp32: 4100 x 32 = 131 200 rows > 131 072: the 4096-block grid strides
    pick = _pick(max_rays, SEED + 5)
    inp = _inputs(cuda, pick)
    idx = torch.randperm(max_rays, generator=torch.Generator().manual_seed(SEED + 6)).to(I32).to(cuda)
    for c in (0, 1, max_rays):
        tile, of = _obj(inp, flags, alpha, f32, idx, torch.tensor([c], dtype=I32, device=cuda), max_rays)
        src = pick[idx[:c].cpu().long()]
        whole = c * N                            # (N = 32: whole tiles)
        assert _is_fill(tile[whole * 64:]), c
        if c:
            assert _same_rows(_rows16(tile, whole), base16, src, c) == [], c
        if f32:
            assert _is_fill(of[c * N:]), c
            assert torch.equal(of[:c * N].view(I32).reshape(c, N, 63), base32[src.to(cuda)]), c


def test_obj_f32_batch_strides_per_object(cuda):
    K, Bn, alpha = 3, 640, 6.5
    counts = (0, 5, 600)                         # 600 x 32 x 8 / 256 = 600 blocks > the 512-block cap; 5 -> 5 blocks
    pick = _pick(Bn, SEED + 7)
    tv, o, d, r, _ = _inputs(cuda, pick)
    g = torch.Generator().manual_seed(SEED + 8)
    idx = torch.stack([torch.randperm(Bn, generator=g) for _ in range(K)]).to(I32).to(cuda)
    cnt = torch.tensor(counts, dtype=I32, device=cuda)
    enc = _ff((K * Bn * N + SLACK) * 63, torch.float32, cuda)
    _lib.check(_lib.lib().durf_encode_obj_f32_batch(ops._stream(), K, Bn, N, ops._p(idx), ops._p(cnt), ops._p(tv), ops._p(o),
                                                    ops._p(d), ops._p(r), _barf(alpha), 0, ops._p(enc)),
               'durf_encode_obj_f32_batch')
    idx0, cnt0 = _iota(E.B, cuda)
    base32 = _obj(_inputs(cuda), 0, alpha, True, idx0, cnt0, E.B)[1][:E.B * N].view(I32).reshape(E.B, N, 63)
    assert _is_fill(enc[K * Bn * N * 63:])
    slabs = enc[:K * Bn * N * 63].reshape(K, Bn * N, 63)
    for kk, c in enumerate(counts):
        assert _is_fill(slabs[kk, c * N:]), kk
        src = pick[idx[kk, :c].cpu().long()].to(cuda)
        assert torch.equal(slabs[kk, :c * N].view(I32).reshape(c, N, 63), base32[src]), kk


@pytest.mark.parametrize('k', [3, 1, 0])
def test_n96_rows_are_the_n32_rows(cuda, k):
    """N = 96: row / N and row % N are no shifts, t_vals rows are 97 floats apart.  A ray's 97 t_vals are its 33 followed twice
    by its last 32, so samples 0 .. 31, 33 .. 63 and 65 .. 95 are the base samples 0 .. 31, 1 .. 31, 1 .. 31 (samples 32 and 64
    pair the last t with the second: written, not compared).  1 ray = 96 rows; 9 rays = 864 rows: three 256-thread blocks and
    a partial one; B * 96 is always a multiple of 32."""
    wide = lambda inp: (torch.cat([inp[0], inp[0][:, 1:], inp[0][:, 1:]], 1).contiguous(),) + inp[1:]
    keep = torch.tensor(list(range(32)) + list(range(33, 64)) + list(range(65, 96)), device=cuda)
    src = torch.tensor(list(range(32)) + list(range(1, 32)) * 2, device=cuda)
    base_l, _ = _bkgd(_inputs(cuda, k=k), 1, False)
    _, base_f = _bkgd(_inputs(cuda, k=k), 1, True)
    idx0, cnt0 = _iota(E.B, cuda)
    base_o, _ = _obj(_inputs(cuda), 0, 4.5, False, idx0, cnt0, E.B)
    b16 = lambda t: _rows16(t, E.B * N).reshape(E.B, N, 64)
    for n in (1, 9):
        pick = _pick(n, SEED + 96 + n)
        inp = wide(_inputs(cuda, pick, k))
        rows = n * 96
        tile, _ = _bkgd(inp, 1, False)
        assert _is_fill(tile[rows * 64:])
        got = _rows16(tile, rows).reshape(n, 96, 64)
        assert torch.equal(got[:, keep], b16(base_l)[pick.to(cuda)][:, src]), ('lane', n)
        assert not bool((got == -1).all(-1).any()), 'every row written'
        _, of = _bkgd(inp, 1, True)
        assert _is_fill(of[rows:])
        want = base_f[:E.B * N].view(I32).reshape(E.B, N, 60)[pick.to(cuda)][:, src]
        assert torch.equal(of[:rows].view(I32).reshape(n, 96, 60)[:, keep], want), ('fp32', n)
        if k == 0:                              # the object form does not read hit columns: once
            idx, cnt = _iota(n, cuda)
            tile, _ = _obj(inp, 0, 4.5, False, idx, cnt, n)
            assert _is_fill(tile[rows * 64:])
            assert torch.equal(_rows16(tile, rows).reshape(n, 96, 64)[:, keep], b16(base_o)[pick.to(cuda)][:, src]), ('obj', n)


def test_object_forward_encodes_the_same_bits_per_object(cuda):
    """durf_obj_fwd_batch (the object forward that encodes its own tiles: the copy of k_encode_lane<true>'s body in
    csrc/mlp_fwd.hip, one enc slab per object, durf_obj_enc_stride apart) on the base rays: K = 3 objects with counts
    (0, 5, all) and a shuffled list each.  Every object's slab is ops.encode_obj(..., f32=False) of its list bit for bit on the
    count * N rows; the zero-count slab and everything behind an object's last row keep the 0xFF fill."""
    K, alpha = 3, 4.5
    tv, o, d, r, _ = _inputs(cuda)
    g = torch.Generator().manual_seed(SEED + 11)
    idx = torch.stack([torch.randperm(E.B, generator=g) for _ in range(K)]).to(I32).to(cuda)
    counts = (0, 5, E.B)
    cnt = torch.tensor(counts, dtype=I32, device=cuda)
    no = ops.mlp_param_count(ops.W_OBJ_, ops.IN_OBJ_)
    po = ((torch.rand(K * no, generator=g) - 0.5) * 0.1).to(cuda)
    wf, _ = ops.pack_weights_batch(K, po, no)
    view = torch.zeros(E.B, ops.VIEW_DIM)
    view[:, :27] = torch.rand(E.B, 27, generator=g) - 0.5
    view = view.to(torch.bfloat16).to(cuda)
    for train in (True, False):
        slabs = ops.ObjSlabs(K, E.B, N, cuda, train)
        slabs.enc.fill_(0xFF)
        vt = ops.obj_view_tiles(K, E.B, N, cuda) if train else None
        ops.obj_fwd_batch(slabs, idx, cnt, tv, o, d, r, alpha, view, wf, view_tile=vt)
        per = slabs.enc.view(torch.bfloat16).reshape(K, -1)
        for kk, c in enumerate(counts):
            assert _is_fill(per[kk, c * N * 64:]), (train, kk)
            if c:
                sep, _ = ops.encode_obj(E.B, idx[kk].contiguous(), cnt[kk:kk + 1], tv, o, d, r, alpha, tile=True, f32=False)
                assert torch.equal(_rows16(per[kk], c * N), _rows16(sep, c * N)), (train, kk)


# ---------------------------------------------------------------------------------------------------------------- (c)
@pytest.mark.parametrize('k', [3, 0])
@pytest.mark.parametrize('contraction', [True, False])
def test_fused_forward_encodes_the_same_bits(cuda, contraction, k):
    tv, o, d, r, hit = _inputs(cuda, k=k)
    g = torch.Generator().manual_seed(7)
    params = ((torch.rand(ops.mlp_param_count(256, 60), generator=g) - 0.5) * 0.1).to(cuda)
    wf = ops.pack_weights(256, 60, params)
    view = torch.zeros(E.B, ops.VIEW_DIM)
    view[:, :27] = torch.rand(E.B, 27, generator=g) - 0.5
    view = view.to(torch.bfloat16).to(cuda)
    rows = E.B * N
    _, fused = ops.mlp_fwd_enc(rows, N, tv, o, d, r, hit, view, wf, contraction=contraction)
    sep, _ = ops.encode_bkgd(tv, o, d, r, hit, contraction, tile=True, f32=False)
    assert torch.equal(_rows16(fused, rows), _rows16(sep, rows))
    # the lanes concerned are there: the big branch, the wrap, the contraction switch
    t, b = _truth(('bkgd', 1 if contraction else 0, k, None))
    assert bool(b['is_big'].any()) and not bool(b['is_big'].all())


# ---------------------------------------------------------------------------------------------------------------- (d)
def _failing_labels(group, m):
    dom = E.in_domain(group)
    return {E.LABELS[i] for i in (m.cpu() & dom[:, None]).any(-1).nonzero().flatten().tolist()}


def _all_fail(group, m, labels):
    """every ray of `labels` has a failing sample"""
    m = m.cpu().any(-1)
    return all(bool(m[E.rays_of(l)].all()) for l in labels)


def _exact_set(group, f32_fail, st, corrupt):
    """The failing set of the fp32 gate, derived from the corruption itself: with |got - truth| <= gate (test (a)), a sample
    whose corrupted expectation is more than 2 gates from the truth in some feature MUST fail, and one whose expectation is
    unchanged MUST pass.  Holds both, sample by sample, over the in-domain rays -> (must-fail labels, untouched labels)."""
    off = 3 if group[0] == 'obj' else 0
    truth = _truth(group)[0]['enc']
    diff = (corrupt - truth).abs()[..., off:]
    dom = E.in_domain(group)[:, None]
    must = (diff > 2 * st['gate32'].cpu()).any(-1) & dom
    same = (diff == 0).all(-1) & dom
    f = f32_fail.cpu()
    assert bool(f[must].all()), 'a corrupted sample passed'
    assert not bool(f[same].any()), 'an untouched sample failed'
    lab = lambda m: {E.LABELS[i] for i in m.any(-1).nonzero().flatten().tolist()}
    return lab(must), {l for l in set(E.LABELS) if all(bool(same[i].all()) for i in E.rays_of(l))}


def test_control_cosine_half_one_degree_up(cuda):
    group = ('bkgd', 0, 3, None)
    of, _, lane16 = _run_base(cuda, group)
    enc = _truth(group)[0]['enc'].clone()
    cosh = enc[..., 30:].reshape(E.B, N, 10, 3)
    enc[..., 30:] = torch.roll(cosh, -1, dims=2).reshape(E.B, N, 30)
    f, l, st = _gate(group, of, lane16, enc)
    must, same = _exact_set(group, f, st, enc)
    # hit1: cos = 1 at every degree, nothing changes; var_big: every feature underflows to 0, the change is below the gate
    assert same == {'hit1'} and must == set(E.LABELS) - {'hit1', 'hit2', 'var_big'}, (must, same)
    for m in (f, l):
        assert _all_fail(group, m, ['plain', 'switch_lo', 'switch_hi', 'wrap', 'n1', 'thick', 'axis'])
        assert 'hit1' not in _failing_labels(group, m)


def test_control_barf_index(cuda):
    for alpha, rejects in ((4.5, True), (2.5, True), (10.0, False), (0.0, False)):
        group = ('obj', 0, 0, alpha)
        of, _, lane16 = _run_base(cuda, group)
        t = _truth(group)[0]
        w6 = E.R.barf_weights(alpha, 10, torch.float64)[:, None].expand(10, 6).reshape(60)
        w3 = torch.cat([E.R.barf_weights(alpha, 10, torch.float64)[:, None].expand(10, 3).reshape(30)] * 2)
        plain = E.encode(('obj', 0, 0, 10.0))['enc'][..., 3:]                    # weights all 1
        enc = torch.cat([t['enc'][..., :3], plain * w3], -1)
        f, l, st = _gate(group, of, lane16, enc)
        must, same = _exact_set(group, f, st, enc)
        assert (len(must) > 20 and not same) if rejects else (not must and same == set(E.LABELS)), (alpha, must, same)
        for m in (f, l):
            if rejects:
                assert _all_fail(group, m, ['plain', 'n1', 'obj40', 'switch_lo'])
            else:
                assert _failing_labels(group, m) == set()       # all 0 / all 1: f // 3 and f // 6 agree, nothing to reject


def test_control_contraction_switch_moved(cuda):
    group = ('bkgd', 1, 0, None)
    of, _, lane16 = _run_base(cuda, group)
    enc = _truth(group)[0]['enc'].clone()
    rows = E.rays_of('n01_hi')                   # norms in (0.1, 0.11]: a switch at 0.11 leaves them uncontracted
    enc[rows] = _truth(('bkgd', 0, 0, None))[0]['enc'][rows]
    f, l, _ = _gate(group, of, lane16, enc)
    for m in (f, l):
        assert _failing_labels(group, m) == {'n01_hi'} and _all_fail(group, m, ['n01_hi'])


def test_control_exact_period_wrap(cuda):
    group = ('bkgd', E.NO_INT, 0, None)
    of, _, lane16 = _run_base(cuda, group)
    t = _truth(group)[0]
    _, _, _, y = E.conditioning(t['x'], t['var'])
    enc = torch.sin(torch.cat([y, y + 0.5 * torch.pi], -1))       # no integration: e = 1; period 2 pi exactly, no wrap
    f, l, _ = _gate(group, of, lane16, enc)
    below = (torch.cat([y, y + E.HALF_PI32], -1).abs() < E.T32).all(-1)
    assert bool(below.any())
    for m in (f, l):
        assert _all_fail(group, m, ['huge'])                      # 318 wraps x 5.9e-6 rad = 1.9e-3
        assert not bool((m.cpu() & below).any())                  # accepted below 100 pi
