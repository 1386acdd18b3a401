"""The ray prologue and the hit compaction (csrc/rays.hip: k_ray_setup, k_compact_hits<false / true>, k_compact_all, k_sample_t,
k_view_enc, k_density_noise and the fused k_ray_prologue) held to the per-ray float64 oracle of tests/ray_rows_ref.py at the
edges of their launches and of their arithmetic.

The instrument is tests/test_gpu_pose_edges.py's.  Every entry point is called through the C ABI on the test's own buffers; every
output buffer starts as 0xFF bytes with 64 elements of slack behind it, and after each launch the slack and everything the
contract leaves unwritten (idx[k, count[k]:] above all) must still hold the fill, everything it writes must not.  A ray's outputs
depend on that ray alone, so launches of B = 1 ... 3000 are filled with shuffled copies of 256 base rays and must reproduce the
base launch BIT FOR BIT: through k_ray_setup and through k_ray_prologue, with and without `enable`, and twice over.

Ray setup.  The hand-aimed table (K = 16 boxes of rotation exactly 0, dyadic numbers, rays +-e_i and two grazing diagonals; also
against its first 3 and its first box) is exact in fp32 and fp64 alike: hit is a literal written next to each ray, origins_s,
dirs_s and zo are the oracle's bits after rounding -- including zo = NaN where the reference's own t_far * 0 is -inf * 0 (a ray
parallel to a slab and outside it) or NaN * 0 (a ray in a face plane), the one place where a written value is not finite.
Generic cases (K = 1, 3, 16; rotation classes zero, below safe_norm's floor, 1 rad, near pi, |r| = 4): hit equals the oracle on
every decided pair (ray_rows_ref.TAU), and the errors of origins_s / dirs_s / zo on decided rays are measured against the
oracle's SCALE (the sum of the absolute terms), gate 4 x FLOOR with FLOOR the float32 twin's own distance from float64 on the
CPU -- the margin for the device's sinf / cosf / sqrtf.  Sample positions: the error against the float64 oracle in ulps of the
largest |t| of the position's interval, gate 4 x the twin's floor, the inf / NaN pattern of lindisp at near = 0 as a pattern.
View encoding: 4 x the twin's floor + 2^-21 (y + float32(pi / 2) is rounded once, half an ulp of 9.6), bf16 = the round-to-
nearest-even of the device's own fp32.  Compaction, the prologue's chores and the injected density noise are exact.

FLOOR -> MEASURED (an MI355X's figures; a case without one is an error in this file), as (origins_s dirs_s zo) of the scale,
per (generic case, masked):
  ('K1-zero', 0)     5.5e-08 7.9e-08 1.5e-07 -> 5.5e-08 7.9e-08 1.5e-07
  ('K1-zero', 1)     5.5e-08 7.9e-08 1.5e-07 -> 5.5e-08 7.9e-08 1.5e-07
  ('K1-below', 0)    7.9e-08 1.1e-07 1.8e-07 -> 7.9e-08 1.1e-07 1.8e-07
  ('K1-below', 1)    7.9e-08 1.1e-07 1.8e-07 -> 7.9e-08 1.1e-07 1.8e-07
  ('K1-one', 0)      1.2e-07 1.4e-07 1.4e-07 -> 1.4e-07 1.2e-07 1.5e-07
  ('K1-one', 1)      1.2e-07 1.4e-07 1.4e-07 -> 1.4e-07 1.2e-07 1.5e-07
  ('K1-near_pi', 0)  2.6e-07 2.5e-07 2.6e-07 -> 2.6e-07 2.5e-07 2.6e-07
  ('K1-near_pi', 1)  2.6e-07 2.5e-07 2.6e-07 -> 2.6e-07 2.5e-07 2.6e-07
  ('K1-above_pi', 0) 1.4e-07 1.7e-07 1.3e-07 -> 1.4e-07 1.7e-07 1.3e-07
  ('K1-above_pi', 1) 1.4e-07 1.7e-07 1.3e-07 -> 1.4e-07 1.7e-07 1.3e-07
  ('K3-a', 0)        3.4e-07 2.2e-07 3.1e-07 -> 3.4e-07 2.2e-07 3.1e-07
  ('K3-a', 1)        1.0e-07 1.3e-07 1.8e-07 -> 1.0e-07 1.3e-07 1.8e-07
  ('K3-b', 0)        1.1e-07 1.1e-07 1.2e-07 -> 1.1e-07 1.1e-07 1.2e-07
  ('K3-b', 1)        9.1e-08 1.1e-07 1.3e-07 -> 9.1e-08 1.1e-07 1.3e-07
  ('K16', 0)         1.8e-07 3.2e-07 1.7e-07 -> 1.8e-07 3.2e-07 1.7e-07
  ('K16', 1)         2.4e-07 3.2e-07 1.7e-07 -> 2.4e-07 3.2e-07 1.7e-07
sample positions, ulps of the interval's largest |t|, floor -> measured per ((near, far) pair | 'inf', lindisp), t_rand none /
zero / one / random:
  (0, 0)     1.00 -> 1.00  1.25 -> 1.25  1.25 -> 1.25  1.66 -> 1.73
  (0, 1)     1.81 -> 1.81  1.55 -> 1.55  1.55 -> 1.55  1.87 -> 2.02
  (1, 0)     0.92 -> 0.92  1.25 -> 1.25  1.24 -> 1.24  1.50 -> 1.71
  (1, 1)     2.14 -> 2.14  1.58 -> 1.58  1.59 -> 1.59  1.91 -> 2.02
  (2, 0)     1.00 -> 1.00  0.00 -> 0.00  0.00 -> 0.00  0.00 -> 0.00
  (2, 1)     1.33 -> 1.33  1.33 -> 1.33  1.33 -> 1.33  1.33 -> 1.33
  (3, 0)     0.50 -> 0.50  0.97 -> 0.97  0.97 -> 0.97  1.35 -> 1.42
  (3, 1)     1.12 -> 1.12  1.40 -> 1.40  1.41 -> 1.41  1.54 -> 1.80
  ('inf', 1) 0.49 -> 0.49  0.93 -> 0.93  0.94 -> 0.94  1.25 -> 1.39
view encoding (absolute): 3.2e-07 -> 3.2e-07

Every comparison passed on the kernels as they stand: nothing had to be fixed.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from durf_amd import _lib, ops
from oracle import philox_ref
from tests import ray_rows_ref as RR

pytestmark = pytest.mark.gpu
SLACK = 64
F32, F64 = np.float32, np.float64

# the float32 twin's floors (tests/scripts/ray_rows_floors.py; tests/test_ray_rows_ref.py holds them to a fresh run)
FLOOR = {
    ('K1-zero', 0): (5.5e-08, 7.9e-08, 1.5e-07), ('K1-zero', 1): (5.5e-08, 7.9e-08, 1.5e-07),
    ('K1-below', 0): (7.9e-08, 1.1e-07, 1.8e-07), ('K1-below', 1): (7.9e-08, 1.1e-07, 1.8e-07),
    ('K1-one', 0): (1.2e-07, 1.4e-07, 1.4e-07), ('K1-one', 1): (1.2e-07, 1.4e-07, 1.4e-07),
    ('K1-near_pi', 0): (2.6e-07, 2.5e-07, 2.6e-07), ('K1-near_pi', 1): (2.6e-07, 2.5e-07, 2.6e-07),
    ('K1-above_pi', 0): (1.4e-07, 1.7e-07, 1.3e-07), ('K1-above_pi', 1): (1.4e-07, 1.7e-07, 1.3e-07),
    ('K3-a', 0): (3.4e-07, 2.2e-07, 3.1e-07), ('K3-a', 1): (1.0e-07, 1.3e-07, 1.8e-07),
    ('K3-b', 0): (1.1e-07, 1.1e-07, 1.2e-07), ('K3-b', 1): (9.1e-08, 1.1e-07, 1.3e-07),
    ('K16', 0): (1.8e-07, 3.2e-07, 1.7e-07), ('K16', 1): (2.4e-07, 3.2e-07, 1.7e-07),
}
MEASURED = {
    ('K1-zero', 0): (5.5e-08, 7.9e-08, 1.5e-07), ('K1-zero', 1): (5.5e-08, 7.9e-08, 1.5e-07),
    ('K1-below', 0): (7.9e-08, 1.1e-07, 1.8e-07), ('K1-below', 1): (7.9e-08, 1.1e-07, 1.8e-07),
    ('K1-one', 0): (1.4e-07, 1.2e-07, 1.5e-07), ('K1-one', 1): (1.4e-07, 1.2e-07, 1.5e-07),
    ('K1-near_pi', 0): (2.6e-07, 2.5e-07, 2.6e-07), ('K1-near_pi', 1): (2.6e-07, 2.5e-07, 2.6e-07),
    ('K1-above_pi', 0): (1.4e-07, 1.7e-07, 1.3e-07), ('K1-above_pi', 1): (1.4e-07, 1.7e-07, 1.3e-07),
    ('K3-a', 0): (3.4e-07, 2.2e-07, 3.1e-07), ('K3-a', 1): (1.0e-07, 1.3e-07, 1.8e-07),
    ('K3-b', 0): (1.1e-07, 1.1e-07, 1.2e-07), ('K3-b', 1): (9.1e-08, 1.1e-07, 1.3e-07),
    ('K16', 0): (1.8e-07, 3.2e-07, 1.7e-07), ('K16', 1): (2.4e-07, 3.2e-07, 1.7e-07),
}
T_FLOOR = {
    (0, 0, 'none'): 1.00, (0, 0, 'zero'): 1.25, (0, 0, 'one'): 1.25, (0, 0, 'random'): 1.66,
    (0, 1, 'none'): 1.81, (0, 1, 'zero'): 1.55, (0, 1, 'one'): 1.55, (0, 1, 'random'): 1.87,
    (1, 0, 'none'): 0.92, (1, 0, 'zero'): 1.25, (1, 0, 'one'): 1.24, (1, 0, 'random'): 1.50,
    (1, 1, 'none'): 2.14, (1, 1, 'zero'): 1.58, (1, 1, 'one'): 1.59, (1, 1, 'random'): 1.91,
    (2, 0, 'none'): 1.00, (2, 0, 'zero'): 0.00, (2, 0, 'one'): 0.00, (2, 0, 'random'): 0.00,
    (2, 1, 'none'): 1.33, (2, 1, 'zero'): 1.33, (2, 1, 'one'): 1.33, (2, 1, 'random'): 1.33,
    (3, 0, 'none'): 0.50, (3, 0, 'zero'): 0.97, (3, 0, 'one'): 0.97, (3, 0, 'random'): 1.35,
    (3, 1, 'none'): 1.12, (3, 1, 'zero'): 1.40, (3, 1, 'one'): 1.41, (3, 1, 'random'): 1.54,
    ('inf', 1, 'none'): 0.49, ('inf', 1, 'zero'): 0.93, ('inf', 1, 'one'): 0.94, ('inf', 1, 'random'): 1.25,
}
T_MEASURED = {
    ('inf', 1, 'none'): 0.49, ('inf', 1, 'one'): 0.94, ('inf', 1, 'random'): 1.39, ('inf', 1, 'zero'): 0.93,
    (0, 0, 'none'): 1.00, (0, 0, 'one'): 1.25, (0, 0, 'random'): 1.73, (0, 0, 'zero'): 1.25,
    (0, 1, 'none'): 1.81, (0, 1, 'one'): 1.55, (0, 1, 'random'): 2.02, (0, 1, 'zero'): 1.55,
    (1, 0, 'none'): 0.92, (1, 0, 'one'): 1.24, (1, 0, 'random'): 1.71, (1, 0, 'zero'): 1.25,
    (1, 1, 'none'): 2.14, (1, 1, 'one'): 1.59, (1, 1, 'random'): 2.02, (1, 1, 'zero'): 1.58,
    (2, 0, 'none'): 1.00, (2, 0, 'one'): 0.00, (2, 0, 'random'): 0.00, (2, 0, 'zero'): 0.00,
    (2, 1, 'none'): 1.33, (2, 1, 'one'): 1.33, (2, 1, 'random'): 1.33, (2, 1, 'zero'): 1.33,
    (3, 0, 'none'): 0.50, (3, 0, 'one'): 0.97, (3, 0, 'random'): 1.42, (3, 0, 'zero'): 0.97,
    (3, 1, 'none'): 1.12, (3, 1, 'one'): 1.41, (3, 1, 'random'): 1.80, (3, 1, 'zero'): 1.40,
}
VIEW_FLOOR = 3.2e-07
VIEW_MEASURED = 3.2e-07


# ---------------------------------------------------------------------------
# buffers and launches
# ---------------------------------------------------------------------------
class Buf:
    """n elements of `dtype` + SLACK, all 0xFF bytes"""

    def __init__(self, n, dtype, dev):
        self.n, self.dtype = n, dtype
        self.size = torch.empty(0, dtype=dtype).element_size()
        self.raw = torch.full(((n + SLACK) * self.size,), 0xFF, dtype=torch.uint8, device=dev)
        self.t = self.raw.view(dtype)

    @property
    def p(self):
        return self.raw.data_ptr()

    def ints(self, what, written=True):
        """the n elements as an integer numpy array after checking the slack; written: none of them is the fill any more"""
        v = self.raw.view(torch.int32 if self.size == 4 else torch.int16).cpu().numpy()
        assert (v[self.n:] == -1).all(), 'the slack behind %s was written' % what
        if written:
            assert (v[:self.n] != -1).all(), '%s: an element was left unwritten' % what
        return v[:self.n].copy()

    def f32(self, what):
        return self.ints(what).view(F32)


def _dev(x, dev, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(x))
    return (t if dtype is None else t.to(dtype)).to(dev)


def _p(t):
    return None if t is None else t.data_ptr()


def _call(name, *args):
    _lib.check(getattr(_lib.lib(), name)(torch.cuda.current_stream().cuda_stream, *args), name)


def _ray_setup(dev, o, d, pose, ext, enable=None, masked_entry=False):
    """durf_ray_setup (or _masked) -> dict of numpy: hit [B,K] int32, o_s, d_s [B,3], zo [B] as int32 bit patterns"""
    B, K = len(o), len(pose)
    bo, bd, bh, bz = Buf(3 * B, torch.float32, dev), Buf(3 * B, torch.float32, dev), Buf(B * K, torch.int32, dev), Buf(B, torch.float32, dev)
    ins = [_dev(x, dev) for x in (o, d, pose, ext)]
    en = None if enable is None else _dev(np.asarray(enable, np.int32), dev)
    if enable is not None or masked_entry:
        _call('durf_ray_setup_masked', B, K, *[_p(x) for x in ins], _p(en), bo.p, bd.p, bh.p, bz.p)
    else:
        _call('durf_ray_setup', B, K, *[_p(x) for x in ins], bo.p, bd.p, bh.p, bz.p)
    return dict(o_s=bo.ints('origins_s').reshape(B, 3), d_s=bd.ints('dirs_s').reshape(B, 3), hit=bh.ints('hit').reshape(B, K),
                zo=bz.ints('zo'))


def _prologue(dev, o, d, pose, ext, N, view=None, near=None, far=None, t_rand=None, lindisp=0, enable=None, seed=None,
              zero_count=None, zero_count2=None, pose_copy=False, pack=None, zero_start=None):
    """durf_ray_prologue, or _pack / _pack_masked where an argument needs them -> dict of Buf (and 'packed': 4 Buf or None)"""
    B, K = len(o), len(pose)
    view = d if view is None else view
    near = np.full(B, 2.0, F32) if near is None else near
    far = np.full(B, 6.0, F32) if far is None else far
    f32 = torch.float32
    out = dict(o_s=Buf(3 * B, f32, dev), d_s=Buf(3 * B, f32, dev), hit=Buf(B * K, torch.int32, dev), zo=Buf(B, f32, dev),
               view=Buf(B * RR.VIEW_DIM, torch.bfloat16, dev), t=Buf(B * (N + 1), f32, dev),
               u=Buf(3 * B * (N + 1) if seed is not None else 0, f32, dev), pose_copy=Buf(K * 6 if pose_copy else 0, f32, dev),
               zero=Buf(zero_count or 0, f32, dev), zero2=Buf(zero_count2 or 0, f32, dev))
    if zero_start is not None:
        out['zero'].t[:zero_count or 0] = zero_start
        out['zero2'].t[:zero_count2 or 0] = zero_start
    ins = [_dev(x, dev) for x in (o, d, pose, ext)]
    vw, nr, fr = _dev(view, dev), _dev(near, dev), _dev(far, dev)
    tr = None if t_rand is None else _dev(t_rand, dev)
    en = None if enable is None else _dev(np.asarray(enable, np.int32), dev)
    lo, hi = (0, 0) if seed is None else ops.split_seed(seed)
    common = (B, K, N, *[_p(x) for x in ins], out['o_s'].p, out['d_s'].p, out['hit'].p, out['zo'].p, _p(vw), out['view'].p, _p(nr),
              _p(fr), _p(tr), int(lindisp), out['t'].p, out['pose_copy'].p if pose_copy else None,
              out['zero'].p if zero_count is not None else None, zero_count or 0, lo, hi, out['u'].p if seed is not None else None)
    out['packed'] = None
    if pack is None and zero_count2 is None and enable is None:
        _call('durf_ray_prologue', *common)
        return out
    L = _lib.lib()
    pack_args = (None, 0, None, None, 0, None, 0, 0, None, None)
    if pack is not None:
        pb, Kp, po, stride = pack
        bf, bb = Buf(int(L.durf_wpack_fwd_bytes(256)) // 2, torch.int16, dev), Buf(int(L.durf_wpack_bwd_bytes(256)) // 2, torch.int16, dev)
        of, ob = (Buf(Kp * int(L.durf_wpack_fwd_bytes(128)) // 2, torch.int16, dev),
                  Buf(Kp * int(L.durf_wpack_bwd_bytes(128)) // 2, torch.int16, dev))
        out['packed'] = (bf, bb, of, ob)
        pack_args = (_p(pb), ops.IN_BKGD, bf.p, bb.p, Kp, _p(po) if Kp else None, stride, ops.IN_OBJ_, of.p if Kp else None,
                     ob.p if Kp else None)
    z2 = (out['zero2'].p if zero_count2 is not None else None, zero_count2 or 0)
    if enable is not None:
        _call('durf_ray_prologue_pack_masked', *common, *pack_args, *z2, _p(en))
    else:
        _call('durf_ray_prologue_pack', *common, *pack_args, *z2)
    return out


def _setup_of(out, B, K):
    return dict(o_s=out['o_s'].ints('origins_s').reshape(B, 3), d_s=out['d_s'].ints('dirs_s').reshape(B, 3),
                hit=out['hit'].ints('hit').reshape(B, K), zo=out['zo'].ints('zo'))


def _same(a, b, what=''):
    for key in ('hit', 'o_s', 'd_s', 'zo'):
        assert np.array_equal(a[key], b[key]), (what, key)


# ---------------------------------------------------------------------------
# ray setup: the hand-aimed table
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('K', RR.TABLE_KS)
@pytest.mark.parametrize('how', ['setup', 'masked', 'prologue', 'prologue_masked'])
def test_table_is_the_oracle_bit_for_bit(cuda, how, K):
    pose, ext, enable = RR.table_scene()
    pose, ext, enable = pose[:K], ext[:K], enable[:K]
    T = RR.table()
    masked = 'masked' in how
    en = enable if masked else None
    got = (_ray_setup(cuda, T['o'], T['d'], pose, ext, en) if 'prologue' not in how
           else _setup_of(_prologue(cuda, T['o'], T['d'], pose, ext, 2, enable=en), len(T['o']), K))
    ref = RR.ray_setup(T['o'], T['d'], pose, ext, en)
    want = (T['want'] if masked else T['want_all'])[:, :K]
    for i, name in enumerate(T['names']):
        assert got['hit'][i].tolist() == want[i].tolist(), name
        for key in ('o_s', 'd_s', 'zo'):
            assert RR.same_bits(got[key][i].view(F32), ref[key][i]), (name, key, got[key][i].view(F32), ref[key][i])
        zo = RR.TABLE_ZO.get(name.replace(' (-0.0)', ''))
        if zo is not None and zo[0] == K:
            assert RR.same_bits(got['zo'][i:i + 1].view(F32), [zo[1]]), name


# ---------------------------------------------------------------------------
# ray setup: generic cases against the oracle
# ---------------------------------------------------------------------------
_BASE = {}


def _base(cuda, name, masked):
    key = (name, masked)
    if key not in _BASE:
        c = RR.generic(name)
        en = c['enable'] if masked else None
        _BASE[key] = (_ray_setup(cuda, c['o'], c['d'], c['pose'], c['ext'], en), RR.ray_setup(c['o'], c['d'], c['pose'], c['ext'], en))
    return _BASE[key]


@pytest.mark.parametrize('masked', [0, 1])
@pytest.mark.parametrize('name', list(RR.GENERIC_CASES))
def test_generic_rays_against_the_oracle(cuda, name, masked):
    got, ref = _base(cuda, name, masked)
    pairs, rays = RR.decided(ref)
    assert np.array_equal(got['hit'][pairs], ref['hit'][pairs]), 'hit on a decided pair'
    assert set(np.unique(got['hit'])) <= {0, 1}
    o_s, d_s, zo = (got[k].view(F32) for k in ('o_s', 'd_s', 'zo'))
    assert np.isfinite(o_s).all() and np.isfinite(d_s).all() and np.isfinite(zo).all()
    errs = RR.setup_errors(o_s, d_s, zo, ref, rays)
    gates = tuple(4 * f for f in FLOOR[(name, masked)])
    print('MEASURED %r: (%s),   # gates %s' % ((name, masked), ', '.join('%.1e' % e for e in errs), ', '.join('%.1e' % g for g in gates)))
    for what, e, g in zip(('origins_s', 'dirs_s', 'zo'), errs, gates):
        assert e <= g, '%s of %r: %.3g of the scale, gate %.3g' % (what, (name, masked), e, g)
    # the same rays through the fused launch: the same bits
    c = RR.generic(name)
    pro = _prologue(cuda, c['o'], c['d'], c['pose'], c['ext'], 5, enable=c['enable'] if masked else None)
    _same(_setup_of(pro, RR.RAYS, len(c['pose'])), got, 'k_ray_prologue')
    assert (name, masked) in MEASURED, 'no recorded figure for %r' % ((name, masked),)


# ---------------------------------------------------------------------------
# ray setup: copy-filled launches against the base launch, bit for bit
# ---------------------------------------------------------------------------
def _take(base, src):
    return {k: v[src] for k, v in base.items()}


@pytest.mark.parametrize('B', [1, 63, 64, 65, 255, 256, 257, 1025, 3000])
@pytest.mark.parametrize('scene', ['K16', 'K3-a', 'table'])
def test_copies_reproduce_their_base_ray(cuda, scene, B):
    if scene == 'table':
        pose, ext, enable = RR.table_scene()
        T = RR.table()
        o, d = T['o'], T['d']
        base = {m: _ray_setup(cuda, o, d, pose, ext, enable if m else None) for m in (0, 1)}
    else:
        c = RR.generic(scene)
        o, d, pose, ext, enable = c['o'], c['d'], c['pose'], c['ext'], c['enable']
        base = {m: _base(cuda, scene, m)[0] for m in (0, 1)}
    K = len(pose)
    src = RR.shuffled_copies(B, len(o), B)
    oc, dc = o[src], d[src]
    plain = _ray_setup(cuda, oc, dc, pose, ext)
    _same(plain, _take(base[0], src), 'k_ray_setup')
    _same(_ray_setup(cuda, oc, dc, pose, ext), plain, 'the same launch twice')
    masked = _ray_setup(cuda, oc, dc, pose, ext, enable)
    _same(masked, _take(base[1], src), 'k_ray_setup with enable')
    assert not masked['hit'][:, enable == 0].any()
    _same(_ray_setup(cuda, oc, dc, pose, ext, np.ones(K, np.int32)), plain, 'enable all ones is the unmasked launch')
    _same(_ray_setup(cuda, oc, dc, pose, ext, None, masked_entry=True), plain, 'enable NULL is the unmasked launch')
    off = _ray_setup(cuda, oc, dc, pose, ext, np.zeros(K, np.int32))
    assert not off['hit'].any() and not off['zo'].any(), 'enable all zeros: no hit, zo == +0'
    # (so + 1 * o: a -0.0 component comes out as +0.0, as 0 + (-0) does in the reference's own sum)
    assert np.array_equal(off['o_s'], (oc + F32(0)).view(np.int32)) and np.array_equal(off['d_s'], (dc + F32(0)).view(np.int32))
    for en, want in ((None, plain), (enable, masked)):
        for N in (2, 40):                  # N + 1 < 32: the grid is sized by the view space; N + 1 > 32: by the sample positions
            pro = _prologue(cuda, oc, dc, pose, ext, N, enable=en)
            _same(_setup_of(pro, B, K), want, 'k_ray_prologue')
    again = _prologue(cuda, oc, dc, pose, ext, 2, enable=enable)
    _same(_setup_of(again, B, K), masked, 'k_ray_prologue twice')


# ---------------------------------------------------------------------------
# compaction
# ---------------------------------------------------------------------------
def _compact(dev, hit, N, how):
    """how: 'hits' | 'classes' | 'all' -> dict of int numpy arrays (idx WITH the poison behind count)"""
    B, K = hit.shape
    h = _dev(hit, dev)
    i32 = torch.int32
    out = {}
    if how in ('hits', 'all'):
        idx, count, slot = Buf(K * B, i32, dev), Buf(K, i32, dev), Buf(B * K, i32, dev)
    if how in ('classes', 'all'):
        cidx, ccount, cslot, dyn = Buf(2 * B, i32, dev), Buf(5, i32, dev), Buf(B * 2, i32, dev), Buf(B, i32, dev)
    if how == 'hits':
        _call('durf_compact_hits', B, K, _p(h), idx.p, count.p, slot.p)
    elif how == 'classes':
        _call('durf_compact_classes', B, K, N, _p(h), cidx.p, ccount.p, cslot.p, dyn.p)
    else:
        _call('durf_compact_all', B, K, N, _p(h), idx.p, count.p, slot.p, cidx.p, ccount.p, cslot.p, dyn.p)
    if how in ('hits', 'all'):
        out.update(idx=idx.ints('idx', written=False).reshape(K, B), count=count.ints('count'), slot=slot.ints('slot', written=False).reshape(B, K))
    if how in ('classes', 'all'):
        out.update(cidx=cidx.ints('class idx', written=False).reshape(2, B), ccount=ccount.ints('class count', written=False),
                   cslot=cslot.ints('class slot', written=False).reshape(B, 2), dyn=dyn.ints('dyn'))
    return out


def _check_lists(idx, count, slot, want_idx, want_count, want_slot, what):
    assert count.tolist() == want_count.tolist(), what
    assert np.array_equal(slot, want_slot), what
    for k, w in enumerate(want_idx):
        assert np.array_equal(idx[k, :len(w)], w), (what, k)
        assert (idx[k, len(w):] == -1).all(), '%s: the poison behind idx[%d, count:] was written' % (what, k)


@pytest.mark.parametrize('N', [1, 128])
@pytest.mark.parametrize('K', [1, 2, 16])
@pytest.mark.parametrize('B', [1, 63, 64, 65, 1023, 1024, 1025, 2049, 3000])
def test_compaction_is_nonzero_and_cumsum(cuda, B, K, N):
    for pattern in RR.PATTERNS:
        for value in (1, 7, -1):
            hit = RR.hit_pattern(pattern, B, K, value)
            what = (pattern, value)
            ref = RR.compact_ref(hit, N)
            a = _compact(cuda, hit, N, 'hits')
            _check_lists(a['idx'], a['count'], a['slot'], ref['idx'], ref['count'], ref['slot'], what)
            c = _compact(cuda, hit, N, 'classes')
            _check_lists(c['cidx'], c['ccount'][:2], c['cslot'], ref['cidx'], ref['ccount'][:2], ref['cslot'], what)
            assert np.array_equal(c['dyn'], ref['dyn']), what
            assert c['ccount'].tolist() == ref['ccount'].tolist(), (what, c['ccount'], ref['ccount'])
            assert int(c['ccount'][2]) == int(c['ccount'][0]) * N + int(c['ccount'][1])
            both = _compact(cuda, hit, N, 'all')
            for key, v in {**a, **c}.items():
                assert np.array_equal(both[key], v), (what, key, 'durf_compact_all')
    if K == 16:          # bit 15 of count[4]: the last ray hits box 15 and one other box, every other ray none
        hit = np.zeros((B, K), np.int32)
        hit[B - 1, [3, 15]] = 1
        assert _compact(cuda, hit, N, 'classes')['ccount'].tolist() == [B, 0, B * N, 1, (1 << 15) | (1 << 3)]


# ---------------------------------------------------------------------------
# sample positions
# ---------------------------------------------------------------------------
def _sample_t(dev, near, far, N, t_rand, lindisp):
    B = len(near)
    out = Buf(B * (N + 1), torch.float32, dev)
    nr, fr, tr = _dev(near, dev), _dev(far, dev), None if t_rand is None else _dev(t_rand, dev)
    _call('durf_sample_t', B, N, _p(nr), _p(fr), _p(tr), int(lindisp), out.p)
    return out.ints('t_vals').reshape(B, N + 1)


def _rays_for(B):
    c = RR.generic('K1-one')
    src = RR.shuffled_copies(B, RR.RAYS, 5)
    return c['o'][src], c['d'][src], c['pose'], c['ext']


T_KEYS = [(i, l, k) for i in list(range(len(RR.NEAR_FAR))) + ['inf'] for l in (0, 1) for k in RR.T_RANDS if i != 'inf' or l]


@pytest.mark.parametrize('pair,lindisp,kind', T_KEYS)
def test_sample_positions_against_the_oracle(cuda, pair, lindisp, kind):
    nf = RR.NEAR_FAR_INF if pair == 'inf' else RR.NEAR_FAR[pair]
    worst = 0.0
    for B in RR.T_BS:
        o, d, pose, ext = _rays_for(B)
        near, far = np.full(B, nf[0], F32), np.full(B, nf[1], F32)
        for N in RR.T_NS:
            tr = RR.t_rand_of(kind, B, N)
            bits = _sample_t(cuda, near, far, N, tr, lindisp)
            got = bits.view(F32)
            worst = max(worst, RR.t_errors(got, near, far, N, tr, lindisp))
            twin = RR.sample_t(near, far, N, tr, lindisp, F32)
            with np.errstate(all='ignore'):
                up = twin[:, 1:] >= twin[:, :-1]
                assert (got[:, 1:] >= got[:, :-1])[up].all(), 'a row decreases where the twin does not'
            pro = _prologue(cuda, o, d, pose, ext, N, near=near, far=far, t_rand=tr, lindisp=lindisp)
            assert np.array_equal(pro['t'].ints('t_vals').reshape(B, N + 1), bits), ('k_ray_prologue', B, N)
            assert pro['u'].ints('u_rand').size == 0
    key = (pair, lindisp, kind)
    gate = 4 * T_FLOOR[key]
    print('T_MEASURED %r: %.2f,   # gate %.2f' % (key, worst, gate))
    assert worst <= gate, (key, worst, gate)
    assert key in T_MEASURED, 'no recorded figure for %r' % (key,)


@pytest.mark.parametrize('B,N', [(1, 1), (3, 2), (257, 31)])
@pytest.mark.parametrize('seed', [0, (1 << 40) + 12345])
def test_in_kernel_draws_at_small_totals(cuda, B, N, seed):
    """totals B (N + 1) that are no multiple of 256, N + 1 < 32: the trailing workgroups of the view space draw nothing"""
    o, d, pose, ext = _rays_for(B)
    t_ref, u_ref = philox_ref.step_draws_planes(seed, B, N)
    for lindisp in (0, 1):
        own = _prologue(cuda, o, d, pose, ext, N, seed=seed, lindisp=lindisp)
        fed = _prologue(cuda, o, d, pose, ext, N, t_rand=t_ref, lindisp=lindisp)
        assert np.array_equal(own['t'].ints('t_vals'), fed['t'].ints('t_vals'))
        assert np.array_equal(own['u'].f32('u_rand').reshape(3, B, N + 1), u_ref)
        _same(_setup_of(own, B, 1), _setup_of(fed, B, 1))


# ---------------------------------------------------------------------------
# view encoding
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('B', [1, 7, 8, 9, 257])
def test_view_encoding(cuda, B):
    v = RR.view_inputs(B)
    b16, b32 = Buf(B * RR.VIEW_DIM, torch.bfloat16, cuda), Buf(B * 27, torch.float32, cuda)
    vd = _dev(v, cuda)
    _call('durf_view_enc', B, _p(vd), b16.p, b32.p)
    f = b32.f32('view fp32').reshape(B, 27)
    h = b16.ints('view bf16').reshape(B, RR.VIEW_DIM)
    assert np.isfinite(f).all()
    err = float(np.abs(f.astype(F64) - RR.pos_enc(v)).max())
    gate = 4 * VIEW_FLOOR + RR.VIEW_SHIFT
    print('VIEW_MEASURED (B = %d) %.1e   # gate %.1e' % (B, err, gate))
    assert err <= gate, (err, gate)
    assert np.array_equal(f[:, :3].view(np.int32), v.view(np.int32)), 'the identity columns are the input bits'
    assert np.array_equal(h[:, :27], RR.bf16_rne(f)), 'bf16 is the round-to-nearest-even of the fp32 output'
    assert not h[:, 27:].any(), 'columns 27..31 are +0'
    only16 = Buf(B * RR.VIEW_DIM, torch.bfloat16, cuda)
    _call('durf_view_enc', B, _p(vd), only16.p, None)
    assert np.array_equal(only16.ints('view bf16').reshape(B, RR.VIEW_DIM), h)
    o, d, pose, ext = _rays_for(B)
    for N in (1, 40):
        pro = _prologue(cuda, o, d, pose, ext, N, view=v)
        assert np.array_equal(pro['view'].ints('view').reshape(B, RR.VIEW_DIM), h), 'k_ray_prologue'
    assert VIEW_MEASURED > 0, 'no recorded figure'


# ---------------------------------------------------------------------------
# the prologue's chores
# ---------------------------------------------------------------------------
def _check_chores(out, B, K, N, zc, zc2, want=None):
    z = out['zero'].ints('zero_buf', written=False)
    z2 = out['zero2'].ints('zero_buf2', written=False)
    assert z.size == (zc or 0) and not z.any() and z2.size == (zc2 or 0) and not z2.any(), (zc, zc2)
    if want is not None:
        _same(_setup_of(out, B, K), want['setup'])
        assert np.array_equal(out['t'].ints('t_vals'), want['t']) and np.array_equal(out['view'].ints('view'), want['view'])


@pytest.mark.parametrize('B,N', [(5, 3), (300, 32)])
def test_zero_fill_and_pose_copy(cuda, B, N):
    c = RR.generic('K16')
    src = RR.shuffled_copies(B, RR.RAYS, 3)
    o, d, pose, ext = c['o'][src], c['d'][src], c['pose'], c['ext']
    plain = _prologue(cuda, o, d, pose, ext, N)
    want = dict(setup=_setup_of(plain, B, 16), t=plain['t'].ints('t_vals'), view=plain['view'].ints('view'))
    assert plain['pose_copy'].ints('pose_copy').size == 0
    for zc in (0, 1, 3, 4, 5, 1023, 4099):
        for zc2 in (None, 0, 1, 97):
            out = _prologue(cuda, o, d, pose, ext, N, zero_count=zc, zero_count2=zc2, pose_copy=True, zero_start=1.5)
            _check_chores(out, B, 16, N, zc, zc2, want)
            assert np.array_equal(out['pose_copy'].ints('pose_copy').view(F32).reshape(16, 6), pose), 'pose_copy == pose at K = 16'


def _mlp_params(dev, K):
    g = torch.Generator().manual_seed(5)
    nb, no = ops.mlp_param_count(256, 60), ops.mlp_param_count(128, 63)
    return (torch.rand(nb, generator=g) - 0.5).to(dev), (torch.rand(max(K, 1) * no, generator=g) - 0.5).to(dev), no


def _check_packed(packed, pb, Kp, po, no):
    (bf, bb), objs = ops.pack_weights_all(pb, Kp, po if Kp else None, no, want_bwd=True)
    got = [b.ints('packed stream', written=False) for b in packed]
    assert np.array_equal(got[0], bf.view(torch.int16).cpu().numpy()) and np.array_equal(got[1], bb.view(torch.int16).cpu().numpy())
    if Kp:
        assert np.array_equal(got[2], objs[0].view(torch.int16).cpu().numpy()) and np.array_equal(got[3], objs[1].view(torch.int16).cpu().numpy())
    else:
        assert got[2].size == 0 and got[3].size == 0


@pytest.mark.parametrize('B,N', [(1, 1), (300, 32)])
@pytest.mark.parametrize('Kp', [0, 2])
def test_weight_packing_rides_in_the_prologue(cuda, Kp, B, N):
    c = RR.generic('K3-a')
    src = RR.shuffled_copies(B, RR.RAYS, 4)
    o, d, pose, ext = c['o'][src], c['d'][src], c['pose'], c['ext']
    pb, po, no = _mlp_params(cuda, Kp)
    plain = _prologue(cuda, o, d, pose, ext, N)
    want = dict(setup=_setup_of(plain, B, 3), t=plain['t'].ints('t_vals'), view=plain['view'].ints('view'))
    out = _prologue(cuda, o, d, pose, ext, N, zero_count=5, zero_count2=97, pack=(pb, Kp, po, no), zero_start=1.5)
    _check_chores(out, B, 3, N, 5, 97, want)
    _check_packed(out['packed'], pb, Kp, po, no)


@pytest.mark.parametrize('Kp', [None, 0, 2])
def test_an_empty_batch(cuda, Kp):
    """B = 0: both regions are zeroed, nothing else is written; with a pack list the streams are still packed (nb_pro = 0)"""
    c = RR.generic('K3-a')
    empty = np.zeros((0, 3), F32)
    pack = None
    if Kp is not None:
        pb, po, no = _mlp_params(cuda, Kp)
        pack = (pb, Kp, po, no)
    for zc, zc2 in ((0, 0), (5, 97), (4099, 1)):
        out = _prologue(cuda, empty, empty, c['pose'], c['ext'], 4, zero_count=zc, zero_count2=zc2, pose_copy=True, pack=pack,
                        zero_start=1.5)
        _check_chores(out, 0, 3, 4, zc, zc2)
        assert (out['pose_copy'].ints('pose_copy', written=False) == -1).all(), 'an empty batch snapshots no pose'
        for key in ('o_s', 'd_s', 'hit', 'zo', 'view', 't'):
            assert out[key].ints(key).size == 0
        if pack is not None:
            _check_packed(out['packed'], pb, Kp, po, no)
    if Kp is None:
        out = _prologue(cuda, empty, empty, c['pose'], c['ext'], 4, zero_count=5, zero_start=1.5)          # durf_ray_prologue itself
        _check_chores(out, 0, 3, 4, 5, None)


# ---------------------------------------------------------------------------
# density noise
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('rows', [1, 255, 256, 257])
def test_density_noise_at_block_edges(cuda, rows):
    g = np.random.default_rng(rows)
    raw = g.normal(size=(rows, 4)).astype(F32) * 3
    z = g.normal(size=rows).astype(F32)
    scale = F32(0.1)

    def run(scale, normal, seed=0):
        buf = Buf(rows * 4, torch.float32, cuda)
        buf.t[:rows * 4] = _dev(raw.reshape(-1), cuda)
        lo, hi = ops.split_seed(seed)
        nz = None if normal is None else _dev(normal, cuda)
        _call('durf_density_noise', rows, buf.p, C.c_float(float(scale)), _p(nz), lo, hi, 1)
        return buf.ints('raw').reshape(rows, 4)
    got = run(scale, z)
    assert np.array_equal(got[:, :3], raw.view(np.int32)[:, :3]), 'the colour channels keep their bits'
    want = raw[:, 3] + scale * z                      # float32 numpy: one multiply, one add, each rounded
    assert np.array_equal(got[:, 3], want.view(np.int32))
    assert np.array_equal(run(0.0, z), raw.view(np.int32)), 'scale == 0 leaves the buffer untouched'
    assert np.array_equal(run(0.0, None), raw.view(np.int32))
    # the seeded path at the same row counts, as tests/test_gpu_sampling_noise.py holds it: 4 ulp of the largest |z| (5.77) and
    # half an ulp of the sum (|raw| + |z| < 32)
    seeded = run(1.0, None, seed=20200823)
    assert np.array_equal(seeded[:, :3], raw.view(np.int32)[:, :3])
    dz = seeded[:, 3].view(F32).astype(F64) - raw[:, 3].astype(F64)
    assert float(np.abs(dz - philox_ref.density_draws(20200823, rows, 1).astype(F64)).max()) <= 4 * 2.0 ** -21 + 2.0 ** -20
