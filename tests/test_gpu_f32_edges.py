"""The exact-fp32 hit-ray MLP kernels (csrc/mlp_f32.hip: k_mlp_fwd_f32, k_mlp_bwd_f32, both weight-gradient kernels, the bf16x3
variants, durf_bkgd_hit_rays_f32) held to a row-wise float64 oracle at every edge of their tile walk.

The instrument is tests/test_gpu_mlp_edges.py's: an MLP row depends on no other row, so a launch of any size is filled with
copies of a few base rows (tests/mlp_rows_ref.py) and must reproduce the base launch BIT FOR BIT wherever the walk placed a copy:
a whole or a partial 32-row tile, tiles that straddle rays (N = 24), the first or a later tile of a workgroup (the grid is capped
at 512 workgroups, 128 per object in a batched call), a compacted list with a device count, a constant-encoding row.  Only the
base rows need the float64 reference (records64: every Dense's input = the act record, every pre-activation gradient = the dz
record, d_enc).  Every output buffer starts as 0xFF bytes (NaN in fp32) and carries slack behind its last row, so a tile that
the walk skipped, a row written past the count, or a record written into the neighbouring object's slab shows.

Bases (seeds W = 256: 11, W = 128: 12; N = 24 base: seed + 1000; objects of the batched calls: weights 12, 112, 212, ray data 7):
  main 16 rays x 32 samples; n24 21 rays x 24 samples = 504 rows = 15.75 tiles; tail (W = 256) 16 constant-encoding rows, N = 1.
Delicate rows (a ReLU pre-activation within 2e-6 of zero in float64: the kernel's own mask `h > 0` may differ there), left out
of the BACKWARD oracle comparison of the base launches only, and given a zero head gradient in the weight-gradient cases:
  W = 256: main 4 of 512, n24 5 of 504, tail 0;  W = 128: main 5, n24 3 (tests/test_mlp_rows_ref.py holds the 2 % cap).

Measured on an MI355X against the float64 oracle (MEASURED below: the largest over a variant's bases); every region gate is
4 x that figure rounded up to one digit (_gate), 0 where the figure is 0 (values a kernel only copies).  The exact kernels' raw
stays at the project's rtol = atol = 2e-6 and their d_enc at 1e-5 norm-wise; act regions are max-abs over every row, dz regions
norm-wise over the non-delicate rows.  Regions are named by their Dense: act l = its input, dz l = its pre-activation gradient.
  exact, W = 256 (main / n24 / tail): raw 4.6e-7 4.4e-7 2.3e-7; d_enc 4.6e-7 4.6e-7 4.5e-7; d_enc[:, 60:] 0;
           act 0-8, 10, 11: 0 9.3e-7 1.1e-6 5.8e-7 7.6e-7 4.7e-7 8.0e-7 1.0e-6 6.2e-7, 6.0e-7 7.7e-7
           -> gates 0 4e-6 5e-6 3e-6 4e-6 2e-6 4e-6 4e-6 3e-6, 3e-6 4e-6;
           dz 0-11: 6.4e-7 5.9e-7 5.7e-7 5.4e-7 4.6e-7 3.9e-7 3.4e-7 2.7e-7 0 1.5e-7 3.8e-8 0
           -> gates 3e-6 3e-6 3e-6 3e-6 2e-6 2e-6 2e-6 2e-6 0 6e-7 2e-7 0.
  exact, W = 128 (main / n24): raw 3.9e-7 4.2e-7; d_enc 3.2e-7 3.3e-7; d_enc[:, 63:] 0;
           act: 0 1.4e-6 9.0e-7 7.2e-7 4.4e-7 4.2e-7 1.0e-6 8.4e-7 5.9e-7, 4.0e-7 7.9e-7
           -> gates 0 6e-6 4e-6 3e-6 2e-6 2e-6 4e-6 4e-6 3e-6, 2e-6 4e-6;
           dz: 4.3e-7 4.1e-7 3.8e-7 3.5e-7 3.1e-7 2.8e-7 2.5e-7 2.0e-7 0 1.5e-7 3.5e-8 0
           -> gates 2e-6 2e-6 2e-6 2e-6 2e-6 2e-6 1e-6 8e-7 0 6e-7 2e-7 0.
  batched object calls, exact (three objects, 3 / 1 / 5 delicate rows of 512; fused encoding == separate launch, bitwise):
           raw 2.5e-7; d_enc 3.2e-7; act: 0 3.8e-7 3.9e-7 3.1e-7 2.5e-7 1.9e-7 3.7e-7 3.4e-7 3.7e-7, 1.8e-7 4.6e-7
           -> gates 0 2e-6 2e-6 2e-6 1e-6 8e-7 2e-6 2e-6 2e-6, 8e-7 2e-6;
           dz: 4.3e-7 4.0e-7 3.7e-7 3.4e-7 3.1e-7 2.8e-7 2.4e-7 2.0e-7 0 1.5e-7 3.7e-8 0 -> gates as W = 128 above.
  batched object calls, bf16x3 (same rows; three launches bitwise equal; every object's raw differs from the exact kernel's):
           raw 7.7e-6 (max-abs) -> gate 4e-5: 250 x below the bf16 kernels' 1.9e-3 (tests/test_gpu_mlp_edges.py);
           d_enc 9.7e-6 -> 4e-5; act: 7.4e-6 7.0e-6 7.4e-6 6.6e-6 6.6e-6 7.4e-6 5.9e-6 7.5e-6 6.1e-6, 4.8e-6 7.5e-6
           -> gates 3e-5 each, act 10 2e-5 (act 0, the encoding, is recorded as hi + lo of the split: 2^-17 of it);
           dz: 1.3e-5 1.2e-5 1.2e-5 1.0e-5 9.2e-6 8.2e-6 6.9e-6 5.1e-6 0 4.6e-6 3.7e-8 0
           -> gates 6e-5 5e-5 5e-5 4e-5 4e-5 4e-5 3e-5 3e-5 0 2e-5 2e-7 0.  (dz 0-3 sit above the EXACT kernels' class gate of
           1e-5: 16-17-bit operands through 20 matrix products, not held to that gate.)
  weight gradients against float64 X^T dZ / sum dZ of the oracle's records (gate 1e-5 norm-wise per Dense, kernel and bias):
           32 and 504 rows 4.2e-7 .. 6.9e-7 at every nsplit; 16416 rows 4.5e-7 .. 7.0e-7 at nsplit 7 and 64, and at nsplit 1
           (one split: every lane adds 2052 terms in one fp32 chain) 9.4e-6 at W = 256 and 2.5e-6 at W = 128; batched, two
           levels: 4.5e-7 .. 5.7e-7, 3.9e-6 for the 133-ray object at nsplit 1.  The three nsplit = 1 figures are all the bias
           of the density head, db Dense_8 = the cancelling sum of every row's d density; every kernel gradient stays below 1e-6.
  durf_bkgd_hit_rays_f32 against the tail rows' oracle at rtol = atol = 2e-6, counts 0, 1, 3, 4, 5, 19 of 19.

Dispatch bits seen (asserted): W = 128 weight gradients F32_DW_TILE (single and batched), W = 256 F32_DW_B2.  The forward and
backward launches record no bit (a bit for bf16x3 needs the library's header): that the variant ran is shown by its bits.

Every comparison passed on the kernels as they stand: nothing had to be fixed.
"""
import math
import os
import re

import pytest
import torch

from durf_amd import ops
from tests import mlp_rows_ref as MR

pytestmark = pytest.mark.gpu
N, RAYS, ROWS = MR.N, MR.RAYS, MR.ROWS
I32 = torch.int32
ROW_MAJOR = ('raw', 'raw_infer', 'd_enc')          # written row by row; the records in whole 32-row tiles
SLACK = 32                                         # rows of poisoned slack behind every buffer
CLASS_GATE = 1e-5                                  # what the project holds these kernels to; no region gate may exceed it

# measured on an MI355X against the float64 oracle: (variant, width) -> quantity -> figure.  'f32': the single-MLP calls on the
# main / n24 / tail bases; 'obj': the batched object calls (fused encoding), exact kernels; 'x3': the same on the bf16x3 kernels
def _table(act, dz, **kw):
    t = dict(kw)
    t.update({'act%d' % l: v for l, v in zip((0, 1, 2, 3, 4, 5, 6, 7, 8, 10, 11), act)})
    t.update({'dz%d' % l: v for l, v in enumerate(dz)})
    return t


MEASURED = {          # act regions 0-8, 10, 11 (max-abs); dz regions 0-11 (norm-wise)
    ('f32', 256): _table((0, 9.3e-7, 1.1e-6, 5.8e-7, 7.6e-7, 4.7e-7, 8.0e-7, 1.0e-6, 6.2e-7, 6.0e-7, 7.7e-7),
                         (6.4e-7, 5.9e-7, 5.7e-7, 5.4e-7, 4.6e-7, 3.9e-7, 3.4e-7, 2.7e-7, 0, 1.5e-7, 3.8e-8, 0)),
    ('f32', 128): _table((0, 1.4e-6, 9.0e-7, 7.2e-7, 4.4e-7, 4.2e-7, 1.0e-6, 8.4e-7, 5.9e-7, 4.0e-7, 7.9e-7),
                         (4.3e-7, 4.1e-7, 3.8e-7, 3.5e-7, 3.1e-7, 2.8e-7, 2.5e-7, 2.0e-7, 0, 1.5e-7, 3.5e-8, 0)),
    ('obj', 128): _table((0, 3.8e-7, 3.9e-7, 3.1e-7, 2.5e-7, 1.9e-7, 3.7e-7, 3.4e-7, 3.7e-7, 1.8e-7, 4.6e-7),
                         (4.3e-7, 4.0e-7, 3.7e-7, 3.4e-7, 3.1e-7, 2.8e-7, 2.4e-7, 2.0e-7, 0, 1.5e-7, 3.7e-8, 0)),
    ('x3', 128): _table((7.4e-6, 7.0e-6, 7.4e-6, 6.6e-6, 6.6e-6, 7.4e-6, 5.9e-6, 7.5e-6, 6.1e-6, 4.8e-6, 7.5e-6),
                        (1.3e-5, 1.2e-5, 1.2e-5, 1.0e-5, 9.2e-6, 8.2e-6, 6.9e-6, 5.1e-6, 0, 4.6e-6, 3.7e-8, 0),
                        raw=7.7e-6, d_enc=9.7e-6),
}


def _gate(measured):
    """4 x the measured figure, rounded up to one digit"""
    if measured == 0:
        return 0.0
    g = 4 * measured
    e = math.floor(math.log10(g))
    return math.ceil(g / 10 ** e - 1e-9) * 10 ** e


# ---------------------------------------------------------------------------
# buffers and their row views
# ---------------------------------------------------------------------------
def _poison(shape, dev):
    return torch.full(shape, -1, dtype=I32, device=dev).view(torch.float32)


def _rec_rows(buf, nfloat):
    """a record buffer [tile][float index][32 samples] -> int32 [tiles * 32, nfloat]: one row per sample"""
    nt = buf.numel() // (32 * nfloat)
    return buf.view(I32)[:nt * 32 * nfloat].view(nt, nfloat, 32).permute(0, 2, 1).reshape(nt * 32, nfloat)


def _views(S, out):
    """every output of a launch as (name, int32 tensor with one row per sample)"""
    v = {}
    for k in ROW_MAJOR:
        if k in out:
            v[k] = out[k].view(I32).reshape(-1, out[k].shape[-1])
    if 'act' in out:
        v['act'] = _rec_rows(out['act'], S['act'])
    if 'dz' in out:
        v['dz'] = _rec_rows(out['dz'], S['dz'])
    return v


def _mismatch(got, want):
    if got.shape == want.shape and torch.equal(got, want):
        return None
    bad = (got != want).reshape(got.shape[0], -1).any(1).nonzero().flatten()
    return '%d of %d rows differ, first row %d (tile %d)' % (bad.numel(), got.shape[0], int(bad[0]), int(bad[0]) // 32)


def _check(views, base, src_rows, nvalid):
    """valid row i of every output == row src_rows[i] of the base launch, bit for bit; beyond the valid rows (beyond their last
    tile for the records) the 0xFF fill is intact; the surplus rows of a partial last tile hold finite inputs and zero dz (what
    the weight-gradient kernels read under their `ok` mask)"""
    hi = (nvalid + 31) // 32 * 32
    for name, got in views.items():
        msg = _mismatch(got[:nvalid], base[name][src_rows[:nvalid]])
        assert msg is None, '%s: %s' % (name, msg)
        rest = got[nvalid:] if name in ROW_MAJOR else got[hi:]
        assert rest.shape[0] >= SLACK and bool((rest == -1).all()), '%s: written beyond the valid rows' % name
        if name == 'act':
            assert bool(torch.isfinite(got[nvalid:hi].view(torch.float32)).all()), 'act: surplus rows of the last tile not finite'
        if name == 'dz':
            assert bool((got[nvalid:hi].view(torch.float32) == 0).all()), 'dz: surplus rows of the last tile not zero'
    return sorted(views)


def _launch(B, rows, n, enc, view, draw, ray_idx=None, count=None, flat=None, ws=None):
    """training forward, inference forward, backward with d_enc, all into poisoned buffers with slack"""
    W, IN, S = B['width'], B['in_dim'], B['S']
    dev = view.device
    flat = B['flat'] if flat is None else flat
    kw = dict(ray_idx=ray_idx, count=count, wstream=B['ws'] if ws is None else ws)
    tr = ops.tile_rows(rows) + SLACK
    out = dict(raw=_poison((rows + SLACK, 4), dev), raw_infer=_poison((rows + SLACK, 4), dev), act=_poison((tr * S['act'],), dev),
               dz=_poison((tr * S['dz'],), dev), d_enc=_poison((rows + SLACK, 64), dev))
    ops.mlp_fwd_f32(W, IN, rows, n, enc, view, flat, raw=out['raw'], act=out['act'], **kw)
    ops.mlp_fwd_f32(W, IN, rows, n, enc, view, flat, raw=out['raw_infer'], **kw)
    ops.mlp_bwd_f32(W, IN, rows, n, draw, flat, out['act'], dz=out['dz'], d_enc=out['d_enc'], **kw)
    return out


# ---------------------------------------------------------------------------
# the base launches (once per width)
# ---------------------------------------------------------------------------
_BASE = {}


def _base(width, cuda):
    if width not in _BASE:
        o = MR.oracle_f32(width)
        b, b24 = o['base'], o['base24']
        in_dim = b['in_dim']
        S = MR.f32_spec(width, in_dim)
        L = ops._lib.lib()
        assert S['act'] == int(L.durf_mlp_f32_act_floats(width, in_dim)) and S['dz'] == int(L.durf_mlp_f32_dz_floats(width, in_dim))
        flat = b['flat'].to(cuda)
        assert flat.numel() == ops.mlp_param_count(width, in_dim)
        B = dict(width=width, in_dim=in_dim, S=S, flat=flat, ws=ops.mlp_f32_pack(width, in_dim, flat))
        B['in'] = dict(main=dict(n=N, enc=b['x'].reshape(ROWS, -1).to(cuda), view=b['cond'].to(cuda), draw=b['draw'].to(cuda)),
                       n24=dict(n=MR.N24, enc=b24['x'].reshape(MR.ROWS24, -1).to(cuda), view=b24['cond'].to(cuda).contiguous(),
                                draw=b24['draw'].to(cuda)))
        if width == 256:
            B['in']['tail'] = dict(n=1, enc=None, view=b['cond'].to(cuda), draw=b['draw_tail'].to(cuda))
        B['out'], B['views'] = {}, {}
        for name, i in B['in'].items():
            rows = i['view'].shape[0] * i['n']
            B['out'][name] = _launch(B, rows, i['n'], i['enc'], i['view'], i['draw'])
            B['views'][name] = {k: v[:rows].clone() for k, v in _views(S, B['out'][name]).items()}
        _BASE[width] = B
    return _BASE[width]


def _host(S, views, sel=slice(None)):
    """rows `sel` of a launch's views -> host float64"""
    return {k: v[sel].contiguous().view(torch.float32).double().cpu() for k, v in views.items()}


# ---------------------------------------------------------------------------
# the gates against the float64 oracle
# ---------------------------------------------------------------------------
def _errors(vals, rec, S, in_dim, keep, table, exact=True):
    """quantity -> (measured, bound, within).  raw rtol = atol = 2e-6 (test_mlp_f32_forward_backward's gate); d_enc 1e-5
    norm-wise on the rows `keep` (the non-delicate ones) and exactly zero beyond in_dim; act region l (the input of Dense_l)
    max-abs on every row and dz region l norm-wise on the rows `keep`, each at 4 x MEASURED (a region without a figure
    in `table` is a KeyError, never a wider gate).  exact=False (the bf16x3 variant,
    which is measured, not held to the exact kernels' class gates): raw max-abs and d_enc norm-wise at 4 x MEASURED too"""
    def rel(a, b):
        return float((a - b).norm() / b.norm()) if float(b.norm()) > 0 else float((a - b).abs().max())
    e = {}
    if 'raw' in vals:
        d = (vals['raw'] - rec['raw']).abs()
        e['raw'] = (float(d.max()), 2e-6, bool((d <= 2e-6 + 2e-6 * rec['raw'].abs()).all()))
        if not exact:
            e['raw'] = (float(d.max()), _gate(table['raw']), float(d.max()) <= _gate(table['raw']))
    if 'raw_infer' in vals:
        e['raw_infer'] = (0.0, 0.0, torch.equal(vals['raw_infer'], vals['raw']))
    if 'd_enc' in vals:
        r = rel(vals['d_enc'][keep], rec['d_enc'][keep])
        g = CLASS_GATE if exact else _gate(table['d_enc'])
        e['d_enc'] = (r, g, r < g)
        z = float(vals['d_enc'][:, in_dim:].abs().max())
        e['d_enc_pad'] = (z, 0.0, z == 0)
    for l, Ly in enumerate(S['L']):
        if 'act' in vals and l != 9:
            m = float((vals['act'][:, Ly['x_off']:Ly['x_off'] + Ly['fi']] - rec['X'][l]).abs().max())
            g = _gate(table['act%d' % l])
            e['act%d' % l] = (m, g, m <= g)
        if 'dz' in vals:
            m = rel(vals['dz'][keep, Ly['dz_off']:Ly['dz_off'] + Ly['fo']], rec['dz'][l][keep])
            g = _gate(table['dz%d' % l])
            e['dz%d' % l] = (m, g, m <= g)
    return e


def _gates(what, e):
    print('%s: ' % what + ', '.join('%s %.2g' % (k, v[0]) for k, v in e.items()))
    over = {k: v[:2] for k, v in e.items() if v[1] > CLASS_GATE}
    assert not over, '%s: a gate above the class gate 1e-5 is a finding, not a gate: %s' % (what, over)
    failed = {k: v[:2] for k, v in e.items() if not v[2]}
    assert not failed, '%s: (measured, bound) %s' % (what, failed)


@pytest.mark.parametrize('width', [256, 128])
def test_base_launches_against_the_float64_oracle(cuda, width):
    vals, bad = MR.conditions_f32(width)
    assert not bad, bad
    print('width %d seed %d: %s' % (width, MR.SEEDS[width], vals))
    o, B = MR.oracle_f32(width), _base(width, cuda)
    for name in B['in']:
        rec = o[name]
        keep = ~MR.delicate_rows(rec)[0]
        e = _errors(_host(B['S'], B['views'][name]), rec, B['S'], B['in_dim'], keep, MEASURED[('f32', width)])
        assert len(e) == 4 + 11 + 12
        _gates('W = %d %s (%d rows, %d delicate)' % (width, name, keep.numel(), int((~keep).sum())), e)
        # the launch's own untouched-memory check: the base rows as copies of themselves
        rows = keep.numel()
        _check(_views(B['S'], B['out'][name]), B['views'][name], torch.arange(rows, device=cuda), rows)


# ---------------------------------------------------------------------------
# position invariance at the walk's edges
# ---------------------------------------------------------------------------
def _case(B, name, nray, use_idx, seed, cuda):
    """a launch of nray rays, each a copy of a base ray of base `name` -> rows, src_rows, and the launch's arguments"""
    i = B['in'][name]
    n, nb = i['n'], i['view'].shape[0]
    src = torch.randint(0, nb, (nray,), generator=torch.Generator().manual_seed(seed)).to(cuda)
    src_rows = (src[:, None] * n + torch.arange(n, device=cuda)).reshape(-1)
    enc = None if i['enc'] is None else i['enc'][src_rows].contiguous()
    if use_idx:
        return nray * n, src_rows, dict(n=n, enc=enc, view=i['view'], draw=i['draw'], ray_idx=src.to(I32))
    return nray * n, src_rows, dict(n=n, enc=enc, view=i['view'][src].contiguous(), draw=i['draw'][src_rows].contiguous())


# (base, rays): what the size reaches
EDGES = [
    ('main', 1),        # 32 rows: one tile
    ('main', 512),      # 16384 rows: exactly the cap, one round
    ('main', 513),      # 16416 rows: workgroup 0 walks a second tile
    ('main', 1031),     # 32992 rows: three rounds, the last partial over the workgroups
    ('n24', 700),       # 16800 rows = 525 tiles: tiles straddle rays, a second round, no partial tile
    ('n24', 701),       # 16824 rows = 525.75 tiles: ... and the last valid tile is partial in rows
]


@pytest.mark.parametrize('use_idx', [False, True])
@pytest.mark.parametrize('name,nray', EDGES)
@pytest.mark.parametrize('width', [256, 128])
def test_position_invariance_at_the_walks_edges(cuda, width, name, nray, use_idx):
    B = _base(width, cuda)
    rows, src_rows, a = _case(B, name, nray, use_idx, 1000 + nray, cuda)
    out = _launch(B, rows, a['n'], a['enc'], a['view'], a['draw'], ray_idx=a.get('ray_idx'))
    names = _check(_views(B['S'], out), B['views'][name], src_rows, rows)
    print('W = %d, %s, %d rows, ray_idx %s: compared %s' % (width, name, rows, use_idx, ' '.join(names)))


@pytest.mark.parametrize('use_idx', [False, True])
@pytest.mark.parametrize('count', [16389, 41])
def test_constant_encoding_rows_at_the_walks_edges(cuda, count, use_idx):
    """W = 256, enc = None, N = 1: 16389 rows = 512 tiles and 5 rows, with every row valid and with 41"""
    B = _base(256, cuda)
    rows, src_rows, a = _case(B, 'tail', 16389, use_idx, 2000 + count, cuda)
    cnt = torch.tensor([count], dtype=I32, device=cuda)
    out = _launch(B, rows, 1, None, a['view'], a['draw'], ray_idx=a.get('ray_idx'), count=cnt)
    _check(_views(B['S'], out), B['views']['tail'], src_rows, count)


@pytest.mark.parametrize('count', [0, 1, 5, 75])
@pytest.mark.parametrize('width', [256, 128])
def test_device_counts_on_a_list_of_70_rays(cuda, width, count):
    """count 0: an object without hits, nothing is written; capacity + 5: f32_rows clamps, exactly `rows` rows are written"""
    B = _base(width, cuda)
    rows, src_rows, a = _case(B, 'main', 70, True, 3000 + count, cuda)
    cnt = torch.tensor([count], dtype=I32, device=cuda)
    out = _launch(B, rows, N, a['enc'], a['view'], a['draw'], ray_idx=a['ray_idx'], count=cnt)
    _check(_views(B['S'], out), B['views']['main'], src_rows, min(count * N, rows))


# ---------------------------------------------------------------------------
# the batched object calls, exact and bf16x3
# ---------------------------------------------------------------------------
K_OBJ, ALPHA = 3, 4.5
OBJ_SEEDS = (12, 112, 212)
_OBJ = {}


def _obj_rays(B, cuda):
    """B rays, ray r a copy of base ray r % 16: seeded ray data in front of the object encoding, the W = 128 base's view
    directions and head gradients"""
    b = MR.oracle_f32(128)['base']
    g = torch.Generator().manual_seed(7)
    o = torch.randn(RAYS, 3, generator=g) * 0.3
    d = torch.randn(RAYS, 3, generator=g)
    d = d / d.norm(dim=-1, keepdim=True)
    t = 0.2 + torch.cumsum(torch.rand(RAYS, N + 1, generator=g) * 0.05, -1)
    radii = torch.rand(RAYS, generator=g) * 2e-3 + 1e-3
    r = torch.arange(B) % RAYS
    dv = lambda x: x.to(cuda).contiguous()
    return dict(B=B, t_vals=dv(t[r]), o_s=dv(o[r]), d_s=dv(d[r]), radii=dv(radii[r]), view=dv(b['cond'][r]),
                draw=dv(b['draw'].reshape(RAYS, N * 4)[r].reshape(B * N, 4)))


def _obj_run(P, rays, idx, count, x3, fused=True, draw=None):
    """forward (training and inference) and backward of all objects into poisoned slabs with slack behind the last one"""
    B, dev, S = rays['B'], rays['view'].device, P['S']
    L = ops._lib.lib()
    a_st, z_st = int(L.durf_objf32_act_stride(B, N)), int(L.durf_objf32_dz_stride(B, N))
    assert a_st == ops.tile_rows(B * N) * S['act'] and z_st == ops.tile_rows(B * N) * S['dz']
    # row-major slabs: the [K, B * N, c] the calls ask for, viewed out of a backing buffer with SLACK poisoned rows behind it
    back = {name: _poison((K_OBJ * B * N + SLACK, c), dev) for name, c in (('raw', 4), ('raw_infer', 4), ('d_enc', 64))}
    slab = lambda name: back[name][:K_OBJ * B * N].view(K_OBJ, B * N, -1)
    sl = ops.ObjSlabsF32(K_OBJ, B, N, dev, True, raw=slab('raw'), act=_poison((K_OBJ * a_st + SLACK * S['act'],), dev))
    inf = ops.ObjSlabsF32(K_OBJ, B, N, dev, False, raw=slab('raw_infer'))
    ws = P['ws_x3'] if x3 else P['ws']
    args = (idx, count, rays['t_vals'], rays['o_s'], rays['d_s'], rays['radii'], ALPHA, rays['view'], P['flat'], P['sz'], ws)
    ops.objf32_fwd_batch(sl, *args, fused_encode=fused, x3=x3)
    ops.objf32_fwd_batch(inf, *args, fused_encode=fused, x3=x3)
    ops.objf32_bwd_batch(sl, idx, count, rays['draw'] if draw is None else draw, P['flat'], P['sz'], ws, x3=x3,
                         dz=_poison((K_OBJ * z_st + SLACK * S['dz'],), dev), d_enc=slab('d_enc'))
    assert sl.raw.data_ptr() == back['raw'].data_ptr() and sl.d_enc.data_ptr() == back['d_enc'].data_ptr()
    return dict(slabs=sl, raw=sl.raw, raw_infer=inf.raw, act=sl.act, dz=sl.dz, d_enc=sl.d_enc, a_st=a_st, z_st=z_st, back=back)


def _obj_views(S, out, k, last):
    """object k's slabs as row views; the slack behind the last object's records belongs to it"""
    a0, z0 = k * out['a_st'], k * out['z_st']
    a1 = out['act'].numel() if last else a0 + out['a_st']
    z1 = out['dz'].numel() if last else z0 + out['z_st']
    return dict(raw=out['raw'][k].view(I32), raw_infer=out['raw_infer'][k].view(I32), d_enc=out['d_enc'][k].view(I32),
                act=_rec_rows(out['act'][a0:a1], S['act']), dz=_rec_rows(out['dz'][z0:z1], S['dz']))


def _obj_check(S, out, base_views, idx, counts):
    """every object's valid rows are its base rows; its slabs are 0xFF from its last tile to the next object's first row"""
    B = idx.shape[1]
    for k in range(K_OBJ):
        nvalid = counts[k] * N
        src = ((idx[k, :counts[k]].long() % RAYS)[:, None] * N + torch.arange(N, device=idx.device)).reshape(-1)
        hi = (nvalid + 31) // 32 * 32
        for name, got in _obj_views(S, out, k, k == K_OBJ - 1).items():
            msg = _mismatch(got[:nvalid], base_views[k][name][src])
            assert msg is None, 'object %d %s: %s' % (k, name, msg)
            rest = got[nvalid:] if name in ROW_MAJOR else got[hi:]
            assert rest.shape[0] >= (B * N - hi) and bool((rest == -1).all()), 'object %d %s: written beyond its valid rows' % (k, name)
    for name, buf in out['back'].items():
        rest = buf.view(I32)[K_OBJ * B * N:]
        assert rest.shape[0] == SLACK and bool((rest == -1).all()), '%s: written beyond the last object\'s slab' % name


def _obj(cuda):
    if not _OBJ:
        S = MR.f32_spec(128, 63)
        pf = [MR.make_params(128, s) for s in OBJ_SEEDS]
        flat = torch.cat([f for _, f in pf]).to(cuda)
        sz = ops.mlp_param_count(128, 63)
        assert flat.numel() == K_OBJ * sz
        P = dict(S=S, params=[p for p, _ in pf], flat=flat, sz=sz, ws=ops.mlp_f32_pack(128, 63, flat, K=K_OBJ, param_stride=sz),
                 ws_x3=ops.mlp_f32_pack(128, 63, flat, K=K_OBJ, param_stride=sz, x3=True))
        rays = _obj_rays(RAYS, cuda)
        idx = torch.arange(RAYS, dtype=I32, device=cuda).repeat(K_OBJ, 1).contiguous()
        count = torch.full((K_OBJ,), RAYS, dtype=I32, device=cuda)
        sep = _obj_run(P, rays, idx, count, False, fused=False)
        base = {False: _obj_run(P, rays, idx, count, False), True: _obj_run(P, rays, idx, count, True)}
        for name in ('raw', 'act', 'd_enc', 'dz'):       # fused == separate, bitwise, before anything rests on it
            assert torch.equal(sep[name].view(I32), base[False][name].view(I32)), 'fused encoding: ' + name
        enc = sep['slabs'].enc.cpu()                      # what durf_encode_obj_f32_batch wrote (test_encode_obj holds it to the oracle)
        b = MR.oracle_f32(128)['base']
        cond_rows = b['cond'][:, None, :].expand(RAYS, N, 27).reshape(ROWS, 27)
        P['rec'] = [MR.records64(P['params'][k], enc[k], cond_rows, b['draw']) for k in range(K_OBJ)]
        P['enc'] = enc
        P['views'] = {x3: [{n_: v[:ROWS].clone() for n_, v in _obj_views(S, base[x3], k, k == K_OBJ - 1).items()}
                           for k in range(K_OBJ)] for x3 in (False, True)}
        P['base_out'] = base
        _OBJ.update(P)
    return _OBJ


def _obj_lists(counts, B, seed, cuda):
    g = torch.Generator().manual_seed(seed)
    idx = torch.stack([torch.randperm(B, generator=g) for _ in range(K_OBJ)]).to(I32).to(cuda)      # distinct rays per list
    return idx, torch.tensor(counts, dtype=I32, device=cuda)


@pytest.mark.parametrize('x3', [False, True])
def test_object_base_rows_against_the_float64_oracle(cuda, x3):
    P = _obj(cuda)
    worst, failed = {}, {}
    for k in range(K_OBJ):
        rec = P['rec'][k]
        dl = MR.delicate_rows(rec)
        assert int(dl[0].sum()) <= int(MR.DELICATE_CAP * ROWS), 'object %d: %d delicate rows' % (k, int(dl[0].sum()))
        active = [float((rec['Z'][l] > 0).double().mean()) for l in MR.RELU_LAYERS]
        assert all(0.1 <= a <= 0.9 for a in active), active
        e = _errors(_host(P['S'], P['views'][x3][k]), rec, P['S'], 63, ~dl[0], MEASURED[('x3' if x3 else 'obj', 128)], exact=not x3)
        print('object %d, x3 %s, %d delicate rows, smallest |z| %.2g: ' % (k, x3, int(dl[0].sum()), dl[1])
              + ', '.join('%s %.2g' % (q, v[0]) for q, v in e.items()))
        for q, v in e.items():
            worst[q] = max(worst.get(q, (0, 0, True)), v, key=lambda t: t[0])
        failed.update({(k, q): v[:2] for q, v in e.items() if not v[2] or (not x3 and v[1] > CLASS_GATE)})
    print('worst over the objects, x3 %s: ' % x3 + ', '.join('%s %.2g' % (q, v[0]) for q, v in worst.items()))
    assert not failed, 'x3 %s: (object, quantity) -> (measured, bound) %s' % (x3, failed)
    if x3:
        differ = [k for k in range(K_OBJ) if _mismatch(P['views'][True][k]['raw'], P['views'][False][k]['raw']) is not None]
        assert differ, 'the bf16x3 launch gave the exact kernels bits: the variant did not run'


@pytest.mark.parametrize('x3', [False, True])
@pytest.mark.parametrize('counts', [(0, 5, 133), (133, 0, 5)])
def test_batched_object_calls_at_the_cap_of_128_workgroups(cuda, counts, x3):
    """B = 160 rays: the object with 133 rays has 133 tiles, five workgroups walk a second one; the object without hits writes
    nothing; the object with 5 exits early in most workgroups"""
    P = _obj(cuda)
    B = 160
    rays = _obj_rays(B, cuda)
    idx, count = _obj_lists(counts, B, 5000 + counts[0], cuda)
    out = _obj_run(P, rays, idx, count, x3)
    _obj_check(P['S'], out, P['views'][x3], idx, counts)
    if x3:          # run to run: the first build of chunk_mma_x3 was not reproducible
        for _ in range(2):
            again = _obj_run(P, rays, idx, count, x3)
            for name in ('raw', 'raw_infer', 'act', 'dz', 'd_enc'):
                assert torch.equal(again[name].view(I32), out[name].view(I32)), 'bf16x3, repeated launch: %s differs' % name


# ---------------------------------------------------------------------------
# weight gradients
# ---------------------------------------------------------------------------
def _layer_slices(S):
    off = 0
    for Ly in S['L']:
        yield slice(off, off + Ly['fi'] * Ly['fo']), slice(off + Ly['fi'] * Ly['fo'], off + Ly['fi'] * Ly['fo'] + Ly['fo']), Ly
        off += Ly['fi'] * Ly['fo'] + Ly['fo']


def _dw_compare(what, S, grad, X, dZ, mult):
    """grad (flax layout, float64 on the host) against X^T (mult * dZ) and sum(mult * dZ) per Dense at 1e-5 norm-wise"""
    rel = lambda a, b: float((a - b).norm() / b.norm())
    worst = (0.0, '')
    for l, (sk, sb, Ly) in enumerate(_layer_slices(S)):
        wz = dZ[l] * mult[:, None]
        rk, rb = rel(grad[sk].reshape(Ly['fi'], Ly['fo']), X[l].T @ wz), rel(grad[sb], wz.sum(0))
        worst = max(worst, (rk, 'dK Dense_%d' % l), (rb, 'db Dense_%d' % l))
        assert rk < CLASS_GATE, '%s: dK Dense_%d rel %.3g' % (what, l, rk)
        assert rb < CLASS_GATE, '%s: db Dense_%d rel %.3g' % (what, l, rb)
    return worst


_NODELICATE = {}


def _quiet(width, name):
    """base `name` with a zero head gradient on its delicate rows -> (draw, records64 of it): dz is zero there whatever the mask"""
    if (width, name) not in _NODELICATE:
        o = MR.oracle_f32(width)
        b = o['base'] if name == 'main' else o['base24']
        n, nr = (N, RAYS) if name == 'main' else (MR.N24, MR.RAYS24)
        draw = b['draw'].clone()
        draw[MR.delicate_rows(o[name])[0]] = 0
        cond_rows = b['cond'][:, None, :].expand(nr, n, 27).reshape(nr * n, 27)
        _NODELICATE[(width, name)] = (draw, MR.records64(o['base']['params'], b['x'].reshape(nr * n, -1), cond_rows, draw))
    return _NODELICATE[(width, name)]


# (base, rays): 32 rows (one tile: with nsplit = 7 most (split, wave) pairs are empty and still write zero partials), 504 rows
# (N = 24, a partial last tile), 16416 rows (513 tiles)
@pytest.mark.parametrize('name,nray', [('main', 1), ('n24', 21), ('main', 513)])
@pytest.mark.parametrize('width', [256, 128])
def test_weight_gradients_against_float64_products_of_the_oracles_records(cuda, width, name, nray):
    B = _base(width, cuda)
    S, IN = B['S'], B['in_dim']
    draw_q, rec = _quiet(width, name)
    i = B['in'][name]
    n = i['n']
    if nray == i['view'].shape[0]:
        src = torch.arange(nray, device=cuda)                      # the base itself, in order
    else:
        src = torch.randint(0, RAYS, (nray,), generator=torch.Generator().manual_seed(6000 + nray)).to(cuda)
    src_rows = (src[:, None] * n + torch.arange(n, device=cuda)).reshape(-1)
    rows = nray * n
    out = _launch(B, rows, n, i['enc'][src_rows].contiguous(), i['view'][src].contiguous(), draw_q.to(cuda)[src_rows].contiguous())
    mult = torch.bincount(src_rows.cpu(), minlength=rec['raw'].shape[0]).double()
    for nsplit in (1, 7, 64):
        g0, g0b = torch.zeros_like(B['flat']), torch.zeros_like(B['flat'])
        g1 = torch.full_like(B['flat'], 0.5)                       # the call ADDS: a known value stays under the sum
        ops.dispatch_reset()
        ops.mlp_dw_f32(width, IN, rows, n, out['act'], out['dz'], g0, nsplit=nsplit)
        assert ops.dispatch_seen() == {'F32_DW_B2' if width == 256 else 'F32_DW_TILE'}, ops.dispatch_seen()
        ops.mlp_dw_f32(width, IN, rows, n, out['act'], out['dz'], g0b, nsplit=nsplit)
        assert torch.equal(g0.view(I32), g0b.view(I32)), 'nsplit %d: the same launch twice differs in bits' % nsplit
        ops.mlp_dw_f32(width, IN, rows, n, out['act'], out['dz'], g1, nsplit=nsplit)
        assert torch.equal(g1, g0 + 0.5), 'nsplit %d: added to 0.5, the gradient is not the one added to 0' % nsplit
        w = _dw_compare('W = %d, %d rows, nsplit %d' % (width, rows, nsplit), S, g0.double().cpu(), rec['X'], rec['dz'], mult)
        print('W = %d, %s, %d rows, nsplit %d: worst rel %.2g (%s)' % ((width, name, rows, nsplit) + w))


def test_batched_weight_gradients_over_two_levels(cuda):
    """durf_objf32_dw_batch with nlevels = 2 (two segments per object) at counts (0, 5, 133): object 0's gradient is exactly zero,
    the others are X^T dZ of the oracle's records over both levels' valid rows; grad starts as 0xFF: the call overwrites"""
    P = _obj(cuda)
    S, B, counts = P['S'], 160, (0, 5, 133)
    rays = _obj_rays(B, cuda)
    b = MR.oracle_f32(128)['base']
    delicate = torch.stack([MR.delicate_rows(r)[0] for r in P['rec']]).any(0)         # one draw buffer serves every object
    draw = b['draw'].clone()
    draw[delicate] = 0
    cond_rows = b['cond'][:, None, :].expand(RAYS, N, 27).reshape(ROWS, 27)
    rec = [MR.records64(P['params'][k], P['enc'][k], cond_rows, draw) for k in range(K_OBJ)]
    draw_d = draw.reshape(RAYS, N * 4)[torch.arange(B) % RAYS].reshape(B * N, 4).to(cuda).contiguous()
    levels, mult = [], [torch.zeros(ROWS, dtype=torch.float64) for _ in range(K_OBJ)]
    count = None
    for lvl in range(2):
        idx, count = _obj_lists(counts, B, 7000 + lvl, cuda)
        levels.append(_obj_run(P, rays, idx, count, False, draw=draw_d))
        for k in range(K_OBJ):
            src = ((idx[k, :counts[k]].long() % RAYS)[:, None] * N + torch.arange(N, device=cuda)).reshape(-1)
            mult[k] += torch.bincount(src.cpu(), minlength=ROWS).double()
    for nsplit in (1, 7, 64):
        grads = []
        for _ in range(2):
            grad = _poison((K_OBJ * P['sz'] + SLACK,), cuda)
            ops.dispatch_reset()
            ops.objf32_dw_batch([l_['slabs'] for l_ in levels], count, grad, P['sz'], nsplit=nsplit)
            assert ops.dispatch_seen() == {'F32_DW_TILE'}, ops.dispatch_seen()
            grads.append(grad)
        assert torch.equal(grads[0].view(I32), grads[1].view(I32)), 'nsplit %d twice' % nsplit
        assert bool((grads[0][K_OBJ * P['sz']:].view(I32) == -1).all()), 'written beyond the last object\'s gradient'
        g = grads[0][:K_OBJ * P['sz']].view(K_OBJ, P['sz'])
        assert bool((g[0] == 0).all()), 'an object without hits has a zero gradient'
        for k in (1, 2):
            w = _dw_compare('object %d, nsplit %d' % (k, nsplit), S, g[k].double().cpu(), rec[k]['X'], rec[k]['dz'], mult[k])
            print('object %d, nsplit %d: worst rel %.2g (%s)' % ((k, nsplit) + w))


# ---------------------------------------------------------------------------
# durf_bkgd_hit_rays_f32
# ---------------------------------------------------------------------------
def _hitrays_per_wg():
    src = open(os.path.join(os.path.dirname(ops.__file__), 'csrc', 'mlp_f32.hip')).read()
    return int(re.search(r'#define\s+HITRAYS_PER_WG\s+(\d+)', src).group(1))


def test_background_hit_rays_around_the_workgroups_share(cuda):
    per = _hitrays_per_wg()
    Bn = 4 * per + 3
    o, B = MR.oracle_f32(256), _base(256, cuda)
    g = torch.Generator().manual_seed(8000)
    ray_of = torch.randint(0, RAYS, (Bn,), generator=g)               # ray r of the batch looks along base view ray_of[r]
    idx1 = torch.randperm(Bn, generator=g)
    view = B['in']['tail']['view'][ray_of.to(cuda)].contiguous()
    trunk = ops.bkgd_const_trunk_f32(B['flat'])
    for cnt in (0, 1, per - 1, per, per + 1, Bn):
        out = _poison((Bn + SLACK, 4), cuda)
        ops.bkgd_hit_rays_f32(Bn, view, B['flat'], idx1.to(I32).to(cuda), torch.tensor([cnt], dtype=I32, device=cuda), trunk=trunk,
                              raw_tail=out)
        assert bool((out[cnt:].view(I32) == -1).all()), 'count %d: rows past the count written' % cnt
        want = o['tail']['raw'][ray_of[idx1[:cnt]]]
        torch.testing.assert_close(out[:cnt].double().cpu(), want, rtol=2e-6, atol=2e-6)


# ---------------------------------------------------------------------------
# the comparisons reject what they are there to reject
# ---------------------------------------------------------------------------
def test_negative_controls(cuda):
    width = 256
    o, B = MR.oracle_f32(width), _base(width, cuda)
    S, IN, rec = B['S'], B['in_dim'], o['main']
    keep = ~MR.delicate_rows(rec)[0]
    table = MEASURED[('f32', width)]
    i = B['in']['main']
    every = torch.arange(ROWS, device=cuda)
    good = _errors(_host(S, B['views']['main']), rec, S, IN, keep, table)
    assert all(v[2] for v in good.values()), 'the uncorrupted comparison passes'

    def rejected(out, spec=S):
        vals = _host(S, {k: v[:ROWS] for k, v in _views(S, out).items()})
        return {k for k, v in _errors(vals, rec, spec, IN, keep, table).items() if not v[2]}

    # (a) one kernel entry of Dense_3 changed by 1e-3 relative, on the device side only
    off3 = sum(Ly['fi'] * Ly['fo'] + Ly['fo'] for Ly in S['L'][:3])
    k3 = B['flat'][off3:off3 + width * width]
    flat2 = B['flat'].clone()
    flat2[off3 + int(k3.abs().argmax())] *= 1 + 1e-3
    out = _launch(B, ROWS, N, i['enc'], i['view'], i['draw'], flat=flat2, ws=ops.mlp_f32_pack(width, IN, flat2))
    r = rejected(out)
    assert 'act4' in r and not r & {'act0', 'act1', 'act2', 'act3'}, 'a changed Dense_3 entry: %s rejected' % sorted(r)
    with pytest.raises(AssertionError, match='raw|act'):
        _check(_views(S, out), B['views']['main'], every, ROWS)

    # (b) two rays' view rows swapped in ray_idx (the encodings stay where they are)
    rows, src_rows, a = _case(B, 'main', 5, True, 1005, cuda)
    swapped = a['ray_idx'].clone()
    j = int((a['ray_idx'] != a['ray_idx'][0]).nonzero()[0])
    swapped[0], swapped[j] = a['ray_idx'][j], a['ray_idx'][0]
    ok = _launch(B, rows, N, a['enc'], a['view'], a['draw'], ray_idx=a['ray_idx'])
    _check(_views(S, ok), B['views']['main'], src_rows, rows)
    bad = _launch(B, rows, N, a['enc'], a['view'], a['draw'], ray_idx=swapped)
    with pytest.raises(AssertionError, match='raw: 64 of 160 rows differ, first row 0'):
        _check(_views(S, bad), B['views']['main'], src_rows, rows)

    # (c) count one ray short: the oracle has 32 rows more than the launch wrote
    short = _launch(B, ROWS, N, i['enc'], i['view'], i['draw'], ray_idx=every[:RAYS].to(I32),
                    count=torch.tensor([RAYS - 1], dtype=I32, device=cuda))
    _check(_views(S, short), B['views']['main'], every, ROWS - N)
    r = rejected(short)
    assert {'raw', 'd_enc', 'act0', 'act11', 'dz0', 'dz11'} <= r, 'a count one ray short: only %s rejected' % sorted(r)
    with pytest.raises(AssertionError):
        _check(_views(S, short), B['views']['main'], every, ROWS)

    # (d) a base-row copy taken from the wrong source row
    wrong = src_rows.clone()
    wrong[77] = src_rows[77] + 1 if int(src_rows[77]) % N < N - 1 else src_rows[77] - 1
    for name in ('raw', 'act', 'dz', 'd_enc'):
        with pytest.raises(AssertionError, match='%s: 1 of 160 rows differ, first row 77' % name):
            _check({name: _views(S, ok)[name]}, B['views']['main'], wrong, rows)

    # (e) one dz region compared at the wrong Dense offset
    spec = dict(S, L=[dict(Ly) for Ly in S['L']])
    spec['L'][3]['dz_off'] = S['L'][4]['dz_off']
    r = rejected(B['out']['main'], spec)
    assert r == {'dz3'}, 'dz3 read at Dense_4\'s offset: %s rejected' % sorted(r)
    spec = dict(S, L=[dict(Ly) for Ly in S['L']])
    spec['L'][6]['x_off'] = S['L'][7]['x_off']
    r = rejected(B['out']['main'], spec)
    assert r == {'act6'}, 'act6 read at Dense_7\'s offset: %s rejected' % sorted(r)
