"""The box-pose gradient kernels (csrc/pose.hip: k_encode_obj_bwd, k_pose_reduce, k_pose_finish; csrc/pose_bkgd.h:
k_encode_bkgd_bwd) held to a per-ray float64 oracle at the edges of their launches.

The instrument is tests/test_gpu_mlp_edges.py's: a hit ray's 21 pose rows (one column of rows_out[21][B]) depend on that ray
alone, so a launch of any size is filled with copies of a few hand-aimed base rays (tests/pose_rows_ref.py: K = 2 boxes, 12
rays each) in shuffled order and must reproduce the base launch's columns BIT FOR BIT: a workgroup's second ray (more than 256
hit rays per box), the reduction's second stride (more than 1024), every device count from 0 to past B, the batched call
against one call per box, one launch over several levels against one launch per level, the same launch twice.  Only the base
launches need the float64 reference.  idx / count / slot come from the project's own ray_setup and compact_hits.  Every
scratch buffer starts as 0xFF bytes (NaN in fp32) with 64 floats of slack behind it: the columns j >= count and the slack
must still hold the fill after a launch, every column j < count must be finite.  The K x 21 sums are held to the float64 sum
of the device's own columns within (ceil(count / 1024) + 6 + 15) 2^-24 sum_j |column_j|: k_pose_reduce's strided adds, the
six levels of a 64-lane wave_sum and the in-order adds of the 16 waves.

Errors of the base launches are measured per row against the oracle's SCALE (the sum over samples and features of the
absolute terms, through the same outer products), never against the cancelled row value, and no ray is left out.  The
yardstick is FLOOR: the distance of the oracle's float32 twin from float64 on the CPU, per kernel, case and row region
(g_o | g_o (x) o_w | g_u (x) d_w).  Gates: 4 x FLOOR for the libm paths (precise = 1, the background kernel) -- the margin for
the kernels' other summation order (4 waves x 64 lanes x P) and the device's libm; 4 x FLOOR + 4e-5 for precise = 0: the
hardware sine below the wrap loses at most |z| 2^-24 <= 1.9e-5 rad (csrc/pose.hip), which enters every term at most linearly,
doubled for __expf.  durf_pose_finish: 4 x the twin's norm-wise distance from float64 autograd, per rotation class and half.
MEASURED / FINISH_MEASURED are an MI355X's figures; a case without one is an error in this file.

FLOOR -> MEASURED per region (obj: precise = 1, then precise = 0; cases are (N, flags, alpha | variant), flags 1 = CONTRACT,
2 = NO_INTEGRATION, 4 = CYLINDER):
  obj  (8, 0, 3.3)      3.1e-06 3.1e-06 3.2e-06 -> 2.5e-06 2.5e-06 2.5e-06 | 2.3e-06 2.3e-06 2.5e-06
  obj  (1, 0, 3.3)      1.8e-06 1.9e-06 5.1e-07 -> 1.7e-06 1.8e-06 5.9e-07 | 2.1e-06 2.1e-06 4.9e-07
  obj  (64, 0, 3.3)     1.8e-06 1.8e-06 1.1e-06 -> 1.8e-06 1.8e-06 9.5e-07 | 1.9e-06 1.9e-06 1.1e-06
  obj  (65, 0, 3.3)     2.8e-06 2.8e-06 1.2e-06 -> 2.8e-06 2.8e-06 9.7e-07 | 3.3e-06 3.3e-06 1.0e-06
  obj  (128, 0, 3.3)    1.2e-06 1.2e-06 8.0e-07 -> 1.2e-06 1.2e-06 1.0e-06 | 1.1e-06 1.1e-06 9.6e-07
  obj  (129, 0, 3.3)    1.7e-06 1.7e-06 1.1e-06 -> 2.4e-06 2.4e-06 1.1e-06 | 2.7e-06 2.7e-06 1.0e-06
  obj  (256, 0, 3.3)    1.7e-06 1.7e-06 7.4e-07 -> 1.7e-06 1.7e-06 7.0e-07 | 1.7e-06 1.7e-06 7.1e-07
  obj  (65, 4, 3.3)     1.4e-06 1.4e-06 8.8e-07 -> 1.5e-06 1.5e-06 1.0e-06 | 2.0e-06 2.0e-06 1.3e-06
  obj  (65, 2, 3.3)     3.7e-06 3.7e-06 2.8e-06 -> 4.5e-06 4.5e-06 2.8e-06 | 5.0e-06 5.0e-06 2.7e-06
  obj  (65, 6, 3.3)     3.6e-06 3.6e-06 2.0e-06 -> 3.6e-06 3.6e-06 2.0e-06 | 4.1e-06 4.1e-06 2.1e-06
  obj  (64, 0, 0.0)     3.0e-08 3.6e-08 5.8e-08 -> 2.7e-08 3.9e-08 7.7e-08 | 2.7e-08 3.9e-08 7.7e-08
  obj  (64, 0, 10.0)    2.6e-06 2.6e-06 1.9e-06 -> 2.3e-06 2.3e-06 1.6e-06 | 2.1e-06 2.1e-06 1.7e-06
  bkgd (1, 1, 'plain')  1.9e-05 1.9e-05 1.3e-05 -> 1.8e-05 1.8e-05 1.2e-05
  bkgd (64, 1, 'plain') 9.8e-04 9.8e-04 7.9e-04 -> 6.4e-04 6.4e-04 2.4e-04
  bkgd (65, 1, 'plain') 4.1e-05 4.1e-05 2.6e-05 -> 4.2e-05 4.2e-05 2.7e-05
  bkgd (128, 1, 'plain') 3.7e-05 3.7e-05 1.9e-05 -> 3.0e-05 3.0e-05 1.5e-05
  bkgd (129, 1, 'plain') 3.4e-05 3.4e-05 9.1e-06 -> 3.4e-05 3.4e-05 9.6e-06
  bkgd (256, 1, 'plain') 5.7e-04 5.7e-04 3.1e-04 -> 5.8e-04 5.8e-04 3.1e-04
  bkgd (65, 0, 'plain') 2.4e-06 2.4e-06 2.1e-06 -> 2.6e-06 2.6e-06 2.0e-06
  bkgd (65, 3, 'plain') 8.6e-03 8.6e-03 3.9e-03 -> 8.6e-03 8.6e-03 3.9e-03
  bkgd (65, 5, 'plain') 1.6e-05 1.6e-05 1.1e-05 -> 1.6e-05 1.6e-05 1.1e-05
  bkgd (65, 1, 'raw')   4.1e-05 4.1e-05 2.6e-05 -> 4.2e-05 4.2e-05 2.7e-05
  bkgd (65, 0, 'raw')   2.4e-06 2.4e-06 2.1e-06 -> 2.6e-06 2.6e-06 2.0e-06
  bkgd (65, 1, 'two')   5.9e-05 5.9e-05 1.5e-05 -> 6.1e-05 6.1e-05 1.5e-05
  bkgd (8, 1, 'raw')    1.4e-05 1.4e-05 6.9e-06 -> 1.4e-05 1.4e-05 8.0e-06
durf_pose_finish, (rotation class, half) floor -> measured:
  above pos 5.3e-08 -> 5.3e-08; above rot 1.0e-06 -> 1.0e-06; below pos 1.2e-07 -> 1.2e-07; below rot 1.9e-06 -> 1.9e-06;
  near_pi pos 2.4e-07 -> 2.4e-07; near_pi rot 4.0e-07 -> 4.1e-07; one pos 9.9e-08 -> 1.2e-07; one rot 1.5e-07 -> 1.0e-07;
  zero pos 4.1e-08 -> 4.1e-08; zero rot 9.2e-08 -> 9.2e-08;

Every comparison passed on the kernels as they stand: nothing had to be fixed.
"""
import math

import pytest
import torch

from durf_amd import ops
from tests import pose_rows_ref as PR

pytestmark = pytest.mark.gpu
I32 = torch.int32
SLACK = 64                       # floats of poisoned slack behind every scratch buffer
FAST_MATH = 4e-5                 # precise = 0: 2 x 1.9e-5 (see above)
NB = PR.K * PR.RAYS

# the float32 twin's floors (tests/scripts/pose_rows_floors.py; tests/test_pose_rows_ref.py holds them to a fresh run)
FLOOR = {
    ('obj', 8, 0, 3.3): (3.1e-06, 3.1e-06, 3.2e-06),
    ('obj', 1, 0, 3.3): (1.8e-06, 1.9e-06, 5.1e-07),
    ('obj', 64, 0, 3.3): (1.8e-06, 1.8e-06, 1.1e-06),
    ('obj', 65, 0, 3.3): (2.8e-06, 2.8e-06, 1.2e-06),
    ('obj', 128, 0, 3.3): (1.2e-06, 1.2e-06, 8.0e-07),
    ('obj', 129, 0, 3.3): (1.7e-06, 1.7e-06, 1.1e-06),
    ('obj', 256, 0, 3.3): (1.7e-06, 1.7e-06, 7.4e-07),
    ('obj', 65, 4, 3.3): (1.4e-06, 1.4e-06, 8.8e-07),
    ('obj', 65, 2, 3.3): (3.7e-06, 3.7e-06, 2.8e-06),
    ('obj', 65, 6, 3.3): (3.6e-06, 3.6e-06, 2.0e-06),
    ('obj', 64, 0, 0.0): (3.0e-08, 3.6e-08, 5.8e-08),
    ('obj', 64, 0, 10.0): (2.6e-06, 2.6e-06, 1.9e-06),
    ('bkgd', 1, 1, 'plain'): (1.9e-05, 1.9e-05, 1.3e-05),
    ('bkgd', 64, 1, 'plain'): (9.8e-04, 9.8e-04, 7.9e-04),
    ('bkgd', 65, 1, 'plain'): (4.1e-05, 4.1e-05, 2.6e-05),
    ('bkgd', 128, 1, 'plain'): (3.7e-05, 3.7e-05, 1.9e-05),
    ('bkgd', 129, 1, 'plain'): (3.4e-05, 3.4e-05, 9.1e-06),
    ('bkgd', 256, 1, 'plain'): (5.7e-04, 5.7e-04, 3.1e-04),
    ('bkgd', 65, 0, 'plain'): (2.4e-06, 2.4e-06, 2.1e-06),
    ('bkgd', 65, 3, 'plain'): (8.6e-03, 8.6e-03, 3.9e-03),
    ('bkgd', 65, 5, 'plain'): (1.6e-05, 1.6e-05, 1.1e-05),
    ('bkgd', 65, 1, 'raw'): (4.1e-05, 4.1e-05, 2.6e-05),
    ('bkgd', 65, 0, 'raw'): (2.4e-06, 2.4e-06, 2.1e-06),
    ('bkgd', 65, 1, 'two'): (5.9e-05, 5.9e-05, 1.5e-05),
    ('bkgd', 8, 1, 'raw'): (1.4e-05, 1.4e-05, 6.9e-06),
}
FINISH_FLOOR = {
    ('above', 'pos'): 5.3e-08,
    ('above', 'rot'): 1.0e-06,
    ('below', 'pos'): 1.2e-07,
    ('below', 'rot'): 1.9e-06,
    ('near_pi', 'pos'): 2.4e-07,
    ('near_pi', 'rot'): 4.0e-07,
    ('one', 'pos'): 9.9e-08,
    ('one', 'rot'): 1.5e-07,
    ('zero', 'pos'): 4.1e-08,
    ('zero', 'rot'): 9.2e-08,
}
# measured on an MI355X: object cases carry `precise` as their last entry
MEASURED = {
    ('obj', 8, 0, 3.3, 1): (2.5e-06, 2.5e-06, 2.5e-06),
    ('obj', 8, 0, 3.3, 0): (2.3e-06, 2.3e-06, 2.5e-06),
    ('obj', 1, 0, 3.3, 1): (1.7e-06, 1.8e-06, 5.9e-07),
    ('obj', 1, 0, 3.3, 0): (2.1e-06, 2.1e-06, 4.9e-07),
    ('obj', 64, 0, 3.3, 1): (1.8e-06, 1.8e-06, 9.5e-07),
    ('obj', 64, 0, 3.3, 0): (1.9e-06, 1.9e-06, 1.1e-06),
    ('obj', 65, 0, 3.3, 1): (2.8e-06, 2.8e-06, 9.7e-07),
    ('obj', 65, 0, 3.3, 0): (3.3e-06, 3.3e-06, 1.0e-06),
    ('obj', 128, 0, 3.3, 1): (1.2e-06, 1.2e-06, 1.0e-06),
    ('obj', 128, 0, 3.3, 0): (1.1e-06, 1.1e-06, 9.6e-07),
    ('obj', 129, 0, 3.3, 1): (2.4e-06, 2.4e-06, 1.1e-06),
    ('obj', 129, 0, 3.3, 0): (2.7e-06, 2.7e-06, 1.0e-06),
    ('obj', 256, 0, 3.3, 1): (1.7e-06, 1.7e-06, 7.0e-07),
    ('obj', 256, 0, 3.3, 0): (1.7e-06, 1.7e-06, 7.1e-07),
    ('obj', 65, 4, 3.3, 1): (1.5e-06, 1.5e-06, 1.0e-06),
    ('obj', 65, 4, 3.3, 0): (2.0e-06, 2.0e-06, 1.3e-06),
    ('obj', 65, 2, 3.3, 1): (4.5e-06, 4.5e-06, 2.8e-06),
    ('obj', 65, 2, 3.3, 0): (5.0e-06, 5.0e-06, 2.7e-06),
    ('obj', 65, 6, 3.3, 1): (3.6e-06, 3.6e-06, 2.0e-06),
    ('obj', 65, 6, 3.3, 0): (4.1e-06, 4.1e-06, 2.1e-06),
    ('obj', 64, 0, 0.0, 1): (2.7e-08, 3.9e-08, 7.7e-08),
    ('obj', 64, 0, 0.0, 0): (2.7e-08, 3.9e-08, 7.7e-08),
    ('obj', 64, 0, 10.0, 1): (2.3e-06, 2.3e-06, 1.6e-06),
    ('obj', 64, 0, 10.0, 0): (2.1e-06, 2.1e-06, 1.7e-06),
    ('bkgd', 1, 1, 'plain'): (1.8e-05, 1.8e-05, 1.2e-05),
    ('bkgd', 64, 1, 'plain'): (6.4e-04, 6.4e-04, 2.4e-04),
    ('bkgd', 65, 1, 'plain'): (4.2e-05, 4.2e-05, 2.7e-05),
    ('bkgd', 128, 1, 'plain'): (3.0e-05, 3.0e-05, 1.5e-05),
    ('bkgd', 129, 1, 'plain'): (3.4e-05, 3.4e-05, 9.6e-06),
    ('bkgd', 256, 1, 'plain'): (5.8e-04, 5.8e-04, 3.1e-04),
    ('bkgd', 65, 0, 'plain'): (2.6e-06, 2.6e-06, 2.0e-06),
    ('bkgd', 65, 3, 'plain'): (8.6e-03, 8.6e-03, 3.9e-03),
    ('bkgd', 65, 5, 'plain'): (1.6e-05, 1.6e-05, 1.1e-05),
    ('bkgd', 65, 1, 'raw'): (4.2e-05, 4.2e-05, 2.7e-05),
    ('bkgd', 65, 0, 'raw'): (2.6e-06, 2.6e-06, 2.0e-06),
    ('bkgd', 65, 1, 'two'): (6.1e-05, 6.1e-05, 1.5e-05),
    ('bkgd', 8, 1, 'raw'): (1.4e-05, 1.4e-05, 8.0e-06),
}
FINISH_MEASURED = {
    ('above', 'pos'): 5.3e-08,
    ('above', 'rot'): 1.0e-06,
    ('below', 'pos'): 1.2e-07,
    ('below', 'rot'): 1.9e-06,
    ('near_pi', 'pos'): 2.4e-07,
    ('near_pi', 'rot'): 4.1e-07,
    ('one', 'pos'): 1.2e-07,
    ('one', 'rot'): 1.0e-07,
    ('zero', 'pos'): 4.1e-08,
    ('zero', 'rot'): 9.2e-08,
}


def _gates(kind, case, precise):
    return tuple(4 * f + (FAST_MATH if kind == 'obj' and not precise else 0.0) for f in FLOOR[(kind,) + case])


# ---------------------------------------------------------------------------
# launches
# ---------------------------------------------------------------------------
def _poison(n, dev):
    return torch.full((n,), -1, dtype=I32, device=dev).view(torch.float32)


def _setup(cuda, b, src=None, box=None):
    """the device side of a launch filled with the base rays `src` (all of them in order when None) against every box of the
    base, or box `box` alone: the project's own ray_setup and compact_hits"""
    src = torch.arange(b['o_w'].shape[0]) if src is None else torch.as_tensor(src)
    ks = slice(None) if box is None else slice(box, box + 1)
    S = dict(b=b, src=src, B=src.numel(), o_w=b['o_w'][src].contiguous().to(cuda), d_w=b['d_w'][src].contiguous().to(cuda),
             radii=b['radii'][src].contiguous().to(cuda), pose=b['pose'][ks].contiguous().to(cuda),
             ext=b['ext'][ks].contiguous().to(cuda), K=b['pose'][ks].shape[0], dev=cuda)
    S['o_s'], S['d_s'], hit, _ = ops.ray_setup(S['o_w'], S['d_w'], S['pose'], S['ext'])
    S['idx'], S['count'], S['slot'] = ops.compact_hits(hit)
    S['idx_c'], S['count_c'], S['slot_c'] = S['idx'].cpu(), S['count'].cpu(), S['slot'].cpu()
    return S


def _t_vals(S, N, level=0):
    return PR.make_t_vals(S['b'], N, level)[S['src']].contiguous().to(S['dev'])


def _by_ray(S, rows, N):
    """[base rays * N, c] -> the launch's [B * N, c]: ray b of the launch carries the rows of base ray src[b]"""
    return rows.view(-1, N, rows.shape[-1])[S['src']].reshape(-1, rows.shape[-1]).contiguous().to(S['dev'])


def _slab(S, N, level=0):
    """the object kernels' d_enc [K, B*N, 64]: rows j*N + n of box k belong to its j-th hit ray; NaN beyond the hit rays"""
    de = PR.make_d_enc(S['b']['o_w'].shape[0], N, level).view(-1, N, 64)
    slab = torch.full((S['K'], S['B'] * N, 64), float('nan'))
    for k in range(S['K']):
        c = int(S['count_c'][k])
        slab[k, :c * N] = de[S['src'][S['idx_c'][k, :c].long()]].reshape(-1, 64)
    return slab.to(S['dev'])


def _read(S, scratch, counts, nblocks=1, K=None):
    """the launch's columns as int32 [nblocks, K, 21, B] on the host, after checking the fill: columns j >= count and the slack
    still 0xFF, columns j < count finite"""
    K, B = S['K'] if K is None else K, S['B']
    raw = scratch.view(I32).cpu()
    n = nblocks * K * 21 * B
    assert raw.numel() == n + SLACK and bool((raw[n:] == -1).all()), 'the slack behind the rows was written'
    cols = raw[:n].view(nblocks, K, 21, B)
    for k in range(K):
        c = min(int(counts[k]), B)
        assert bool((cols[:, k, :, c:] == -1).all()), 'box %d: a column beyond the count was written' % k
        assert bool(torch.isfinite(cols[:, k, :, :c].view(torch.float32)).all()), 'box %d: a column below the count is not finite' % k
    return cols


def _check_sums(S, cols, sums, counts):
    """each of the K x 21 sums against the float64 sum of the device's own columns: k_pose_reduce's order bounds the distance"""
    for k in range(cols.shape[0]):
        c = min(int(counts[k]), S['B'])
        col = cols[k, :, :c].view(torch.float32).double()
        bound = (math.ceil(c / 1024) + 6 + 15) * 2.0 ** -24 * col.abs().sum(-1)
        err = (sums[k].double() - col.sum(-1)).abs()
        assert bool((err <= bound).all()), (k, c, err, bound)


def _run_obj(S, N, flags, alpha, precise, count=None, how='batch', check=True):
    """-> columns int32 [K,21,B], sums [K,21] (host)"""
    cnt = S['count'] if count is None else count
    counts = cnt.cpu()
    args = (_t_vals(S, N), S['o_s'], S['d_s'], S['radii'], S['o_w'], S['d_w'], S['pose'], alpha)
    slab = _slab(S, N)
    sums = torch.zeros(S['K'], 21, device=S['dev'])
    if how == 'batch':
        scratch = _poison(S['K'] * 21 * S['B'] + SLACK, S['dev'])
        ops.encode_obj_bwd_batch(S['K'], S['idx'], cnt, slab, *args, sums, precise=precise, enc_flags=flags, scratch=scratch)
        cols = _read(S, scratch, counts)[0]
    else:
        per = []
        for k in range(S['K']):
            scratch = _poison(21 * S['B'] + SLACK, S['dev'])
            ops.encode_obj_bwd(k, S['idx'][k], cnt[k:k + 1], slab[k], *args, sums, scratch=scratch, precise=precise, enc_flags=flags)
            per.append(_read(S, scratch, counts[k:k + 1], K=1)[0, 0])
        cols = torch.stack(per)
    sums = sums.cpu()
    if check:
        _check_sums(S, cols, sums, counts)
    return cols, sums


def _run_bkgd(S, N, flags, variant, count=None, slot=False):
    cnt = S['count'] if count is None else count
    counts = cnt.cpu()
    nb = S['b']['o_w'].shape[0]
    d_enc = _by_ray(S, PR.make_d_enc(nb, N), N)
    raw, draw = (_by_ray(S, x, N) for x in PR.make_raw_draw(nb, N)) if variant in ('raw', 'two') else (None, None)
    denc_slot = None
    if slot:                                       # the rows of ray b live at denc_slot[b]: a permutation of the rays
        perm = torch.randperm(S['B'], generator=torch.Generator().manual_seed(9))
        moved = torch.empty_like(d_enc).view(S['B'], N, 64)
        moved[perm.to(S['dev'])] = d_enc.view(S['B'], N, 64)
        d_enc, denc_slot = moved.view(-1, 64), perm.to(I32).to(S['dev'])
    sums = torch.zeros(S['K'], 21, device=S['dev'])
    scratch = _poison(S['K'] * 21 * S['B'] + SLACK, S['dev'])
    ops.encode_bkgd_bwd_batch(S['K'], S['idx'], cnt, d_enc, _t_vals(S, N), S['o_s'], S['d_s'], S['radii'], S['o_w'], S['d_w'],
                              S['pose'], sums, raw=raw, draw=draw, density_bias=PR.DENSITY_BIAS, denc_slot=denc_slot,
                              enc_flags=flags, scratch=scratch)
    cols = _read(S, scratch, counts)[0]
    sums = sums.cpu()
    _check_sums(S, cols, sums, counts)
    return cols, sums


_BASE = {}


def _base(cuda, kind, case, precise=1):
    """the base launch of a case, once per session: (S, columns int32 [K,21,NB], per-ray columns int32 [rays, K, 21])"""
    key = (kind,) + case + (precise,)
    if key not in _BASE:
        b = PR.variant_base(case[2] if kind == 'bkgd' else 'plain')
        S = _setup(cuda, b)
        assert S['count_c'].tolist() == [PR.RAYS] * S['K'], S['count_c']        # every base ray hits (its own box | both)
        if kind == 'obj':
            cols, _ = _run_obj(S, case[0], case[1], case[2], precise)
        else:
            cols, _ = _run_bkgd(S, case[0], case[1], case[2])
        n = b['o_w'].shape[0]
        ray_cols = torch.full((n, S['K'], 21), -1, dtype=I32)
        for k in range(S['K']):
            ids = S['idx_c'][k, :int(S['count_c'][k])].long()
            ray_cols[ids, k] = cols[k, :, :ids.numel()].T
        _BASE[key] = (S, cols, ray_cols)
    return _BASE[key]


def _own(b, ray_cols):
    """[rays, 21] float32: every base ray's column in its own box"""
    return ray_cols[torch.arange(ray_cols.shape[0]), b['obj']].view(torch.float32)


def _hold(kind, case, precise, errs, gates):
    key = (kind,) + case + ((precise,) if kind == 'obj' else ())
    print('MEASURED %r: (%s),   # gates %s' % (key, ', '.join('%.1e' % e for e in errs), ', '.join('%.1e' % g for g in gates)))
    for region, (e, g) in enumerate(zip(errs, gates)):
        assert e <= g, 'rows %s of %r: %.3g of the scale, gate %.3g' % (PR.REGIONS[region], key, e, g)
    assert key in MEASURED, 'no recorded figure for %r' % (key,)


# ---------------------------------------------------------------------------
# the base launches against the float64 oracle
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('precise', [1, 0])
@pytest.mark.parametrize('case', PR.OBJ_CASES, ids=lambda c: 'N%d-f%d-a%g' % c)
def test_object_rows_against_the_oracle(cuda, case, precise):
    assert (ops.ENC_CONTRACT, ops.ENC_NO_INTEGRATION, ops.ENC_CYLINDER) == (PR.C, PR.NI, PR.CY)
    S, _, ray_cols = _base(cuda, 'obj', case, precise)
    b = S['b']
    rows, scale = PR.case_rows('obj', case, b, S['o_s'].cpu(), S['d_s'].cpu())
    _hold('obj', case, precise, PR.region_errors(_own(b, ray_cols), rows, scale), _gates('obj', case, precise))


@pytest.mark.parametrize('case', PR.BKGD_CASES, ids=lambda c: 'N%d-f%d-%s' % c)
def test_background_rows_against_the_oracle(cuda, case):
    S, _, ray_cols = _base(cuda, 'bkgd', case)
    b = S['b']
    rows, scale = PR.case_rows('bkgd', case, b, S['o_s'].cpu(), S['d_s'].cpu())
    if case[2] == 'two':          # both boxes take the whole d(o_s), d(d_s): with one pose, the same column twice
        assert torch.equal(ray_cols[:, 0], ray_cols[:, 1])
        assert float((S['d_s'].cpu().norm(dim=-1) - 2).abs().max()) < 1e-5
    _hold('bkgd', case, 1, PR.region_errors(_own(b, ray_cols), rows, scale), _gates('bkgd', case, 1))


def test_background_rows_through_a_slot_permutation(cuda):
    """denc_slot: the d_enc rows of ray b at denc_slot[b] -- the same columns as the rows in place"""
    S, cols, _ = _base(cuda, 'bkgd', (65, PR.C, 'plain'))
    moved, sums = _run_bkgd(S, 65, PR.C, 'plain', slot=True)
    assert torch.equal(moved, cols)


# ---------------------------------------------------------------------------
# copy-filled launches against the base launch, bit for bit
# ---------------------------------------------------------------------------
def _src(n, lo, hi, seed):
    """n base rays drawn from [lo, hi) in shuffled order, every one of them present"""
    g = torch.Generator().manual_seed(seed)
    reps = torch.arange(lo, hi).repeat(n // (hi - lo) + 1)[:n]
    return reps[torch.randperm(n, generator=g)]


def _want(S, ray_cols, k, box, c):
    """the columns the base launch holds for the first c hit rays of box k of a copy-filled launch: int32 [21, c]"""
    return ray_cols[S['src'][S['idx_c'][k, :c].long()], box].T


N8 = 8
KINDS = [('obj', 1), ('obj', 0), ('bkgd', 1)]


def _dup(cuda, kind, precise, B, seed, box=0, count=None, **kw):
    """a launch of B copies of box `box`'s base rays against that box alone (K = 1): every one hits"""
    case = (N8, 0, PR.ALPHA) if kind == 'obj' else (N8, PR.C, 'raw')
    bS, _, ray_cols = _base(cuda, kind, case, precise)
    S = _setup(cuda, bS['b'], _src(B, box * PR.RAYS, (box + 1) * PR.RAYS, seed), box=box)
    assert S['count_c'].tolist() == [B]
    cnt = None if count is None else torch.tensor([count], dtype=I32, device=cuda)
    if kind == 'obj':
        cols, sums = _run_obj(S, N8, case[1], case[2], precise, count=cnt, **kw)
    else:
        cols, sums = _run_bkgd(S, N8, case[1], case[2], count=cnt)
    return S, cols, sums, ray_cols


@pytest.mark.parametrize('kind,precise', KINDS)
def test_a_workgroups_second_ray(cuda, kind, precise):
    """B = 300 > 256 hit rays: workgroups 0..43 take a second ray (j += gridDim.x) behind the barrier that frees part[][]"""
    S, cols, _, ray_cols = _dup(cuda, kind, precise, 300, 1, box=1)
    assert torch.equal(cols[0], _want(S, ray_cols, 0, 1, 300))


def test_two_strides_of_the_reduction(cuda):
    """B = 1100 > 1024 hit rays through the single-object call and a 21 B scratch: threads 0..75 of k_pose_reduce add two
    columns, every workgroup of k_encode_obj_bwd walks 4 or 5 rays"""
    S, cols, sums, ray_cols = _dup(cuda, 'obj', 1, 1100, 2, how='single')
    assert torch.equal(cols[0], _want(S, ray_cols, 0, 0, 1100))
    assert float(sums.abs().min()) > 0


@pytest.mark.parametrize('count', [0, 1, 256, 257, 300, 307])
@pytest.mark.parametrize('kind,precise', KINDS)
def test_device_counts(cuda, kind, precise, count):
    """the count lives on the device: 0 (nothing written, sums stay 0), 1, the grid's 256 and one more, B, and B + 7, which
    the kernels clamp to B (every read stays inside [K,B])"""
    S, cols, sums, ray_cols = _dup(cuda, kind, precise, 300, 3, count=count)
    c = min(count, 300)
    assert torch.equal(cols[0, :, :c], _want(S, ray_cols, 0, 0, c))
    if count == 0:
        assert bool((sums.view(I32) == 0).all())
    if count > 300:
        full = _dup(cuda, kind, precise, 300, 3, count=300)
        assert torch.equal(full[1], cols) and torch.equal(full[2].view(I32), sums.view(I32))


@pytest.mark.parametrize('precise', [1, 0])
def test_batched_call_is_one_call_per_object(cuda, precise):
    """K = 2, B = 300 rays of both boxes: blockIdx.y strides idx, count, d_enc and the rows; ops.encode_obj_bwd per object
    gives the same columns and the same sums"""
    case = (N8, 0, PR.ALPHA)
    bS, _, ray_cols = _base(cuda, 'obj', case, precise)
    S = _setup(cuda, bS['b'], _src(300, 0, NB, 4))
    counts = S['count_c'].tolist()
    assert sum(counts) == 300 and min(counts) >= 100
    cols, sums = _run_obj(S, N8, case[1], case[2], precise)
    for k in range(PR.K):
        assert torch.equal(cols[k, :, :counts[k]], _want(S, ray_cols, k, k, counts[k]))
    cols1, sums1 = _run_obj(S, N8, case[1], case[2], precise, how='single')
    assert torch.equal(cols1, cols) and torch.equal(sums1.view(I32), sums.view(I32))
    again = _run_obj(S, N8, case[1], case[2], precise)                       # the same launch twice: the same bits
    assert torch.equal(again[0], cols) and torch.equal(again[1].view(I32), sums.view(I32))


def test_background_launch_twice(cuda):
    case = (N8, PR.C, 'raw')
    bS, _, ray_cols = _base(cuda, 'bkgd', case)
    S = _setup(cuda, bS['b'], _src(300, 0, NB, 5))
    counts = S['count_c'].tolist()
    cols, sums = _run_bkgd(S, N8, case[1], case[2])
    for k in range(PR.K):
        assert torch.equal(cols[k, :, :counts[k]], _want(S, ray_cols, k, k, counts[k]))
    again = _run_bkgd(S, N8, case[1], case[2])
    assert torch.equal(again[0], cols) and torch.equal(again[1].view(I32), sums.view(I32))


@pytest.mark.parametrize('nlev', [2, 3])
def test_levels_launch_is_one_launch_per_level(cuda, nlev):
    """durf_encode_obj_bwd_levels (blockIdx.z = level; the one-call step's form): another d_enc and t_vals per level, K = 2,
    B = 300 -- the columns of every level and the accumulated sums are those of one single-level call per level, in order,
    into the same sums"""
    case = (N8, 0, PR.ALPHA)
    bS, _, ray_cols = _base(cuda, 'obj', case, 1)
    S = _setup(cuda, bS['b'], _src(300, 0, NB, 6))
    K, B, counts = S['K'], S['B'], S['count_c']
    slabs = [_slab(S, N8, l) for l in range(nlev)]
    tvs = [_t_vals(S, N8, l) for l in range(nlev)]
    rest = (S['o_s'], S['d_s'], S['radii'], S['o_w'], S['d_w'], S['pose'], PR.ALPHA)
    sums = torch.zeros(K, 21, device=cuda)
    scratch = _poison(nlev * K * 21 * B + SLACK, cuda)
    ops.encode_obj_bwd_levels(K, S['idx'], S['count'], slabs, tvs, *rest, sums, scratch=scratch, precise=True)
    cols = _read(S, scratch, counts, nblocks=nlev)
    seq = torch.zeros(K, 21, device=cuda)
    for l in range(nlev):
        one = _poison(K * 21 * B + SLACK, cuda)
        ops.encode_obj_bwd_batch(K, S['idx'], S['count'], slabs[l], tvs[l], *rest, seq, precise=True, scratch=one)
        assert torch.equal(_read(S, one, counts)[0], cols[l]), 'level %d' % l
    assert torch.equal(seq.view(I32), sums.view(I32))
    for k in range(K):                               # level 0 draws the base's d_enc and t_vals
        assert torch.equal(cols[0, k, :, :int(counts[k])], _want(S, ray_cols, k, k, int(counts[k])))
    assert not torch.equal(cols[0], cols[1])
    without = torch.zeros(K, 21, device=cuda)        # the wrapper's own scratch
    ops.encode_obj_bwd_levels(K, S['idx'], S['count'], slabs, tvs, *rest, without, precise=True)
    assert torch.equal(without.view(I32), sums.view(I32))


# ---------------------------------------------------------------------------
# durf_pose_finish
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('want_pos,want_rot', [(1, 1), (1, 0), (0, 1), (0, 0)])
@pytest.mark.parametrize('Kf,first', PR.FINISH_CASES)
def test_pose_finish(cuda, Kf, first, want_pos, want_rot):
    """sums [K,21] -> d(loss)/d(pose) ADDED into a non-zero grad6, against float64 autograd (and pose_finish_ref) per rotation
    class: 0 and |r| = 5e-7 (the `tiny` branch: d theta = 0), 2e-6 just above it, 1, pi - 1e-3; K = 1, 3, DURF_MAX_OBJ = 16;
    a half that is not asked for keeps its bits"""
    pose, sums, grad6, names = PR.make_finish_case(Kf, Kf * 10 + first, first)
    buf = _poison(Kf * 6 + SLACK, cuda)
    buf[:Kf * 6] = grad6.reshape(-1).to(cuda)
    ops.pose_finish(pose.to(cuda), sums.to(cuda), want_pos, want_rot, buf[:Kf * 6].view(Kf, 6))
    out = buf.cpu()
    assert bool((out[Kf * 6:].view(I32) == -1).all())
    got = out[:Kf * 6].view(Kf, 6)
    for (half, sl), on in zip(PR.HALVES, (want_pos, want_rot)):
        if not on:
            assert torch.equal(got[:, sl].contiguous().view(I32), grad6[:, sl].contiguous().view(I32)), half
    ref = grad6.double() + PR.pose_finish_ref(pose.double(), sums.double(), bool(want_pos), bool(want_rot))
    for key, e in sorted(PR.finish_errors(got, pose, sums, grad6, names, want_pos, want_rot).items()):
        gate = 4 * FINISH_FLOOR[key]
        print('FINISH_MEASURED %r: %.1e,   # gate %.1e (K = %d)' % (key, e, gate, Kf))
        assert e <= gate, (key, e, gate)
        assert key in FINISH_MEASURED, 'no recorded figure for %r' % (key,)
    for k in range(Kf):
        for (half, sl), on in zip(PR.HALVES, (want_pos, want_rot)):
            if on:
                d = float((got[k, sl].double() - ref[k, sl]).norm() / (ref[k, sl] - grad6[k, sl].double()).norm())
                assert d <= 4 * FINISH_FLOOR[(names[k], half)], (names[k], half, d)


# ---------------------------------------------------------------------------
# negative controls: a wrong oracle, a wrong column -- each must FAIL the gate that the right one passes
# ---------------------------------------------------------------------------
CONTROL = (65, 0, PR.ALPHA)


def _control_errors(cuda, **wrong):
    S, _, ray_cols = _base(cuda, 'obj', CONTROL, 1)
    b = S['b']
    _, scale = PR.case_rows('obj', CONTROL, b, S['o_s'].cpu(), S['d_s'].cpu())
    rows, _ = PR.case_rows('obj', CONTROL, b, S['o_s'].cpu(), S['d_s'].cpu(), want_scale=False, **wrong)
    return PR.region_errors(_own(b, ray_cols), rows, scale), _gates('obj', CONTROL, 0)      # (the wider of the two gates)


def test_control_barf_weight_index(cuda):
    """the oracle with the BARF weight of feature f taken at f // 3 instead of f // 6: every region fails"""
    errs, gates = _control_errors(cuda, wdiv=3)
    assert all(e > g for e, g in zip(errs, gates)), (errs, gates)


def test_control_swapped_world_rays(cuda):
    """the oracle with o_w and d_w exchanged in the outer products: rows 3..20 fail, rows 0..2 (g_o alone) still pass"""
    errs, gates = _control_errors(cuda, swap=True)
    assert errs[0] <= gates[0] and errs[1] > gates[1] and errs[2] > gates[2], (errs, gates)


def test_control_neighbouring_column(cuda):
    """a copy-filled launch held to the base column of the NEXT base ray: no column agrees"""
    S, cols, _, ray_cols = _dup(cuda, 'obj', 1, 300, 1, box=1)
    shifted = ray_cols.roll(-1, 0)
    wrong = shifted[S['src'][S['idx_c'][0, :300].long()], 1].T
    assert not bool((cols[0] == wrong).all(0).any())
