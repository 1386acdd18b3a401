"""The fused MLP launches (k_mlp_fwd / k_mlp_bwd and the M-split object kernels) held to a row-wise float64 oracle at every
edge of their block walk.

An MLP row depends on no other row, so a launch of any size is filled with copies of 16 base rays x 32 samples
(tests/mlp_rows_ref.py) and must reproduce the base launch BIT FOR BIT wherever the persistent walk placed a copy: 4-wave
or 8-wave blocks, the first or a later round of a workgroup, a whole or a partial block, a compacted list with a device
count, a tail row.  Only the base rows (and the 16 base tail rows) need the float64 reference.  Every output buffer
starts as 0xFF bytes (NaN in bf16 and fp32), so a row that a launch skipped, or wrote where it should not, shows.

Seeds (tests/mlp_rows_ref.py SEEDS, the first tried): W = 256: 11, W = 128: 12; the copies' permutations: 1000 + rows
(scheduling edges), 4000 + capacity + 64 count + tail_count (compacted lists), 5 (the W = 128 compacted base list).

Conditions of the base rows, from the CPU oracle alone (tests/test_mlp_rows_ref.py holds them without a GPU):
  W = 256: ReLUs active per stashed layer 0.503 0.495 0.506 0.498 0.501 0.502 0.530 0.541, view layer 0.461; smallest
           max-abs distance between two of the 528 raw rows 8.6e-3, between two rays at one sample index 4.3e-2;
  W = 128: 0.499 0.498 0.475 0.537 0.481 0.495 0.497 0.482, view layer 0.492; 2.5e-2 and 3.2e-2.

Measured on an MI355X against the float64 oracle (gates: raw rtol = atol = 5e-3; stash regions 1e-2; dz per region and
d_enc 3e-2 norm-wise; dz_out slots 0-3 exactly bf16(d raw)).  The stash figures are whole bf16 quanta: a re-rounding flip.
  W = 256, 512 base rows: raw 2.4e-3; stash regions 0-7, 9 (max abs) 3.8e-6 3.9e-3 2.0e-3 2.0e-3 3.9e-3 3.9e-3 3.9e-3
           3.9e-3, 7.8e-3; dz regions 0-7, 9 (norm-wise) 7.2e-3 7.1e-3 7.4e-3 6.8e-3 6.0e-3 4.9e-3 4.7e-3 4.5e-3, 1.4e-3;
           d_enc 5.0e-3; dz_out 0.
  W = 128, 512 base rows (alone, and on the compacted list under either object kernel: the same bits): raw 1.9e-3; stash
           0 3.1e-5 4.8e-7 3.8e-6 4.9e-4 9.8e-4 3.9e-3 3.9e-3, 3.9e-3; dz 2.7e-3 2.5e-3 2.4e-3 2.8e-3 2.8e-3 2.4e-3 2.6e-3
           2.9e-3, 0; d_enc 2.0e-3; dz_out 0.
  tail rows (both widths; the 16 base ones and the 37 of every list below): raw 2.6e-8 .. 3.8e-8, d_enc 5.1e-8 .. 6.7e-8,
           every stash and dz region and dz_out 0 (no re-rounding flip in so few rows).
  weight gradients of the four lists against float64 X^T dZ of the valid rows: 2.9e-8 .. 4.9e-7 direct (gate 1e-5),
           6.0e-4 .. 1.6e-3 through the bottleneck (gate 5e-3).

Variants dispatch_seen() reported (each asserted): fwd_train / fwd_infer, bwd, bwd_d_enc
  W = 256, 32 / 160 / 32768 rows:           FWD256_4W, BWD256_4W, BWD256_8W + BWD_POSE
  W = 256, 32800 / 65568 / 131936 rows:     FWD256_8W, BWD256_8W, BWD256_8W + BWD_POSE
  W = 128, 32 / 288 / 65568 rows, no count: FWD128_SAMPLE, BWD128_SAMPLE, BWD128_SAMPLE + BWD_POSE
  W = 128 compacted, 512 rows:              FWD128_MSPLIT, BWD128_MSPLIT; with DURF_OBJ_MSPLIT=0 FWD128_SAMPLE, BWD128_SAMPLE
  capacity 70016, count 2050, tail 37:      FWD256_8W + FWD_TAIL, BWD256_8W, BWD256_8W + BWD_POSE
  capacity 1024, (5, 37) / (0, 37) / (5, 0): FWD256_4W + FWD_TAIL, BWD256_4W, BWD256_8W + BWD_POSE

Every comparison passed on the kernels as they stand: nothing had to be fixed.  Region 8 of stash and dz (the linear
bottleneck, docs/history.md 4.1e) is never written and stays 0xFF; the weight-gradient launch reads none of it.
"""
import pytest
import torch

from durf_amd import ops
from tests import helpers as H
from tests import mlp_rows_ref as MR

pytestmark = pytest.mark.gpu
N, RAYS, ROWS, STASHED = MR.N, MR.RAYS, MR.ROWS, MR.STASHED
BF, I16, I32 = torch.bfloat16, torch.int16, torch.int32


# ---------------------------------------------------------------------------
# buffers and their row views
# ---------------------------------------------------------------------------
def _poison(shape, dtype, dev):
    it = {torch.float32: I32, BF: I16, torch.uint8: torch.uint8}[dtype]
    return torch.full(shape, 255 if it == torch.uint8 else -1, dtype=it, device=dev).view(dtype)


def _region(buf, width, nt, j):
    """region j of a stash / dz buffer of nt 32-row tiles (csrc/mlp_spec.h) -> int16 [nt, k-steps, 2, 32, 8]"""
    KW = width // 16
    nks = 8 if j == 9 else KW
    o = j * KW * nt * 512
    return buf.view(I16)[o:o + nks * nt * 512].view(nt, nks, 2, 32, 8)


def _rows_of(tiles):
    """[nt, k-steps, 2, 32, 8] -> [nt * 32, k-steps * 16]: one row per sample, fragment order"""
    nt, nks = tiles.shape[:2]
    return tiles.permute(0, 3, 1, 2, 4).reshape(nt * 32, nks * 16)


def _views(width, nt, out):
    """every output of a launch as (name, integer tensor with one row per sample), one at a time"""
    if 'raw' in out:
        yield 'raw', out['raw'].view(I32)
    if 'stash' in out:
        for j in STASHED:
            yield 'stash%d' % j, _rows_of(_region(out['stash'], width, nt, j))
        m = out['mask'].view(I32).view(9, nt, 2, 32, 4)           # one uint4 per lane; lanes n and n + 32 hold sample n
        for j in range(9):
            yield 'mask%d' % j, m[j].permute(0, 2, 1, 3).reshape(nt * 32, 8)
    if 'dz' in out:
        for j in STASHED:
            yield 'dz%d' % j, _rows_of(_region(out['dz'], width, nt, j))
        yield 'dz_out', _rows_of(out['dz_out'].view(I16).view(nt, 1, 2, 32, 8))
    if 'd_enc' in out:
        yield 'd_enc', out['d_enc'].view(I32)


ROW_MAJOR = ('raw', 'd_enc')          # written row by row; the others in whole 32-row tiles


def _mismatch(got, want):
    """bitwise comparison on the device -> None, or what differs"""
    if got.shape == want.shape and torch.equal(got, want):
        return None
    bad = (got != want).reshape(got.shape[0], -1).any(1).nonzero().flatten()
    return '%d of %d rows differ, first row %d (tile %d)' % (bad.numel(), got.shape[0], int(bad[0]), int(bad[0]) // 32)


def _check(views, base, src_rows, nvalid):
    """valid row i of every output == row src_rows[i] of the base launch, bit for bit; beyond the valid rows (beyond their
    last tile for the tiled outputs) the 0xFF fill is intact"""
    names = []
    for name, got in views:
        msg = _mismatch(got[:nvalid], base[name][src_rows])
        assert msg is None, '%s: %s' % (name, msg)
        rest = got[nvalid:] if name in ROW_MAJOR else got[(nvalid + 31) // 32 * 32:]
        assert bool((rest == -1).all()), '%s: written beyond the valid rows' % name
        names.append(name)
    return names


def _fwd(width, rows, n, enc, view, wf, train, **kw):
    dev = enc.device
    out = dict(raw=_poison((rows + 32, 4), torch.float32, dev))             # 32 rows of slack behind the launch's rows
    if train:
        out['stash'] = _poison((ops.mlp_stash_bytes(width, rows),), torch.uint8, dev)
        out['mask'] = _poison((ops.mlp_mask_bytes(rows),), torch.uint8, dev)
    ops.dispatch_reset()
    ops.mlp_fwd(width, rows, n, enc, view, wf, stash=out.get('stash'), raw=out['raw'], relu_mask=out.get('mask'), **kw)
    out['seen'] = ops.dispatch_seen()
    return out


def _bwd(width, rows, n, draw, wb, mask, want_d_enc, **kw):
    dev = draw.device
    out = dict(dz=_poison((ops.mlp_stash_bytes(width, rows),), torch.uint8, dev),
               dz_out=_poison((ops.tile_rows(rows), 16), BF, dev))
    if want_d_enc:
        out['d_enc'] = _poison((rows + 32, 64), torch.float32, dev)
    ops.dispatch_reset()
    ops.mlp_bwd(width, rows, n, draw, wb, mask, want_d_enc=want_d_enc, dz=out['dz'], dz_out=out['dz_out'],
                d_enc=out.get('d_enc'), **kw)
    out['seen'] = ops.dispatch_seen()
    return out


def _expect_seen(width, variant, mode, tail=False):
    if mode.startswith('fwd'):
        return {'FWD%d_%s' % (width, variant)} | ({'FWD_TAIL'} if tail else set())
    if mode == 'bwd':
        return {'BWD%d_%s' % (width, variant)}
    return {'BWD256_8W' if width == 256 else 'BWD128_' + variant, 'BWD_POSE'}      # d(enc): never the 4-wave / M-split kernels


# ---------------------------------------------------------------------------
# the base launches (once per width)
# ---------------------------------------------------------------------------
_BASE = {}


def _enc_tile(x, dev):
    xp = torch.zeros(x.shape[0], 64)
    xp[:, :x.shape[1]] = x
    return H.tile(xp, 4).to(dev)


def _launch_all(width, rows, n, enc, view, draw, wf, wb):
    tr = _fwd(width, rows, n, enc, view, wf, True)
    inf = _fwd(width, rows, n, enc, view, wf, False)
    bw = _bwd(width, rows, n, draw, wb, tr['mask'], False)
    bp = _bwd(width, rows, n, draw, wb, tr['mask'], True)
    views = dict(_views(width, rows // 32, dict(raw=tr['raw'], stash=tr['stash'], mask=tr['mask'], dz=bw['dz'],
                                                 dz_out=bw['dz_out'], d_enc=bp['d_enc'])))
    return dict(train=tr, infer=inf, bwd=bw, pose=bp, views={k: v.clone() for k, v in views.items()})


def _base(width, cuda):
    if width not in _BASE:
        b = MR.oracle(width)['base']
        flat = b['flat'].to(cuda)
        assert flat.numel() == ops.mlp_param_count(width, b['in_dim'])
        wf, wb = ops.pack_weights(width, b['in_dim'], flat, want_bwd=True)
        view = torch.zeros(RAYS, 32)
        view[:, :27] = b['cond']
        view = view.to(BF).to(cuda)
        B = dict(width=width, flat=flat, wf=wf, wb=wb, view=view, enc=_enc_tile(b['x'].reshape(ROWS, -1), cuda),
                 draw=b['draw'].to(cuda), draw_tail=b['draw_tail'].to(cuda))
        B['main'] = _launch_all(width, ROWS, N, B['enc'], view, B['draw'], wf, wb)
        # the tail rows through the ORDINARY path: the constant encoding spelled out in an encoding tile, one "ray" per row
        # (N = 1); rows 16..31 of the tile repeat rows 0..15
        B['enc_tail'] = _enc_tile(b['x_tail'].reshape(RAYS, -1).repeat(2, 1), cuda)
        B['tail'] = _launch_all(width, 32, 1, B['enc_tail'], view.repeat(2, 1).contiguous(),
                                B['draw_tail'].repeat(2, 1).contiguous(), wf, wb)
        # rows 0..511: the base rows; 512 + i: the tail row of base ray i
        B['views'] = {k: torch.cat([v[:ROWS], B['tail']['views'][k][:RAYS]]) for k, v in B['main']['views'].items()}
        _BASE[width] = B
    return _BASE[width]


def _values(width, views, sel):
    """rows `sel` of a launch's views -> host float64, natural feature order (what the oracle returns)"""
    out = {}
    for name, v in views.items():
        if name.startswith('mask'):
            continue
        v = v[sel]
        if name in ROW_MAJOR:
            out[name] = v.view(torch.float32).double().cpu()
        elif name == 'dz_out':
            out[name] = v.view(BF).double().cpu()[:, :4]
        else:
            x = v.view(BF).double().cpu()
            out[name] = x[:, H.cperm_cols(x.shape[1] // 16)]
    return out


# ---------------------------------------------------------------------------
# part 2: the gates against the float64 oracle
# ---------------------------------------------------------------------------
def _errors(vals, fo, bo):
    """name -> (measured, bound, within): raw rtol = atol = 5e-3 (the project's gate against this oracle), stash regions 1e-2
    (as test_mlp_fwd holds region 0), dz per region and d_enc 3e-2 norm-wise (the kernel-level gradient gate), dz_out slots
    0-3 exactly bf16(d raw)"""
    def close(a, b, tol):
        d = (a - b).abs()
        return float(d.max()), tol, bool((d <= tol + tol * b.abs()).all())

    def rel(a, b):
        r = float((a - b).norm() / b.norm())
        return r, 3e-2, r < 3e-2
    e = {}
    if 'raw' in vals:
        e['raw'] = close(vals['raw'], fo['raw'], 5e-3)
    for j in STASHED:
        if 'stash%d' % j in vals:
            e['stash%d' % j] = close(vals['stash%d' % j], fo['hc'] if j == 9 else fo['h'][j], 1e-2)
        if 'dz%d' % j in vals:
            e['dz%d' % j] = rel(vals['dz%d' % j], bo['dz'][j])
    if 'd_enc' in vals:
        e['d_enc'] = rel(vals['d_enc'], bo['d_enc'])
    if 'dz_out' in vals:
        e['dz_out'] = (float((vals['dz_out'] - bo['dz_out']).abs().max()), 0.0, torch.equal(vals['dz_out'], bo['dz_out']))
    return e


def _gates(what, vals, fo, bo):
    e = _errors(vals, fo, bo)
    print('%s: ' % what + ', '.join('%s %.3g' % (k, v[0]) for k, v in e.items()))
    failed = {k: v[:2] for k, v in e.items() if not v[2]}
    assert not failed, '%s: (measured, bound) %s' % (what, failed)
    return e


@pytest.mark.parametrize('width', [256, 128])
def test_base_launch_against_the_float64_oracle(cuda, width):
    vals, bad = MR.conditions(width)
    assert not bad, bad
    print('width %d seed %d: %s' % (width, MR.SEEDS[width], vals))
    o, B = MR.oracle(width), _base(width, cuda)
    for part, n, fo, bo in (('main', ROWS, o['fwd'], o['bwd']), ('tail', RAYS, o['fwd_tail'], o['bwd_tail'])):
        L = B[part]
        small = width == 256
        assert L['train']['seen'] == _expect_seen(width, '4W' if small else 'SAMPLE', 'fwd_train')
        assert L['infer']['seen'] == _expect_seen(width, '4W' if small else 'SAMPLE', 'fwd_infer')
        assert L['bwd']['seen'] == _expect_seen(width, '4W' if small else 'SAMPLE', 'bwd')
        assert L['pose']['seen'] == _expect_seen(width, 'SAMPLE', 'bwd_d_enc')
        assert torch.equal(L['train']['raw'].view(I32), L['infer']['raw'].view(I32)), \
            'training and inference instantiations must agree bitwise'
        for k in ('dz', 'dz_out'):
            assert torch.equal(L['bwd'][k].view(I16), L['pose'][k].view(I16)), '%s with and without want_d_enc' % k
        e = _gates('W = %d %s rows' % (width, part), _values(width, L['views'], slice(0, n)), fo, bo)
        assert set(e) == {'raw', 'd_enc', 'dz_out'} | {'stash%d' % j for j in STASHED} | {'dz%d' % j for j in STASHED}


@pytest.mark.parametrize('msplit', ['unset', '0'])
def test_base_rows_on_a_compacted_list_run_both_object_kernels(cuda, monkeypatch, msplit):
    """W = 128 with ray_idx and a device count: the M-split kernels by default, the sample-split ones with DURF_OBJ_MSPLIT=0;
    either way the base rows, permuted: bit-identical to the base launch and within the gates of the oracle"""
    if msplit == 'unset':
        monkeypatch.delenv('DURF_OBJ_MSPLIT', raising=False)
    else:
        monkeypatch.setenv('DURF_OBJ_MSPLIT', msplit)
    variant = 'MSPLIT' if msplit == 'unset' else 'SAMPLE'
    width = 128
    o, B = MR.oracle(width), _base(width, cuda)
    perm = torch.randperm(RAYS, generator=torch.Generator().manual_seed(5)).to(cuda)       # list position j = base ray perm[j]
    kw = dict(ray_idx=perm.int(), count=torch.tensor([RAYS], dtype=I32, device=cuda))
    enc = B['enc'].view(I16).view(RAYS, 2048)[perm].view(BF).view(ROWS, 64)
    tr = _fwd(width, ROWS, N, enc, B['view'], B['wf'], True, **kw)
    inf = _fwd(width, ROWS, N, enc, B['view'], B['wf'], False, **kw)
    bw = _bwd(width, ROWS, N, B['draw'], B['wb'], tr['mask'], False, **kw)          # draw: the full layout, gathered by ray
    assert tr['seen'] == {'FWD128_' + variant} and inf['seen'] == {'FWD128_' + variant}, (tr['seen'], inf['seen'])
    assert bw['seen'] == {'BWD128_' + variant}, bw['seen']
    src_rows = (perm[:, None] * 32 + torch.arange(32, device=cuda)).reshape(-1)
    out = dict(raw=tr['raw'], stash=tr['stash'], mask=tr['mask'], dz=bw['dz'], dz_out=bw['dz_out'])
    _check(_views(width, RAYS, out), B['views'], src_rows, ROWS)
    _check(_views(width, RAYS, dict(raw=inf['raw'])), B['views'], src_rows, ROWS)
    vals = _values(width, dict(_views(width, RAYS, out)), torch.argsort(src_rows))
    _gates('W = 128 compacted, %s' % variant, vals, o['fwd'], o['bwd'])


# ---------------------------------------------------------------------------
# part 3: position invariance at the scheduling edges
# ---------------------------------------------------------------------------
# (width, rows, the variant the launchers choose): what the size reaches
EDGES = [
    (256, 32, '4W'),          # one tile: three waves of the block have none
    (256, 160, '4W'),         # a whole block and a one-tile block
    (256, 32768, '4W'),       # 256 blocks: the largest launch of the 4-wave variant
    (256, 32800, '8W'),       # the smallest 8-wave launch: 129 blocks, the last holds one tile
    (256, 65568, '8W'),       # 257 blocks: workgroup 0 alone takes a second block (has_next), the last block is partial
    (256, 131936, '8W'),      # 515 blocks + 3 tiles: two whole rounds, a partial third round, a partial last block
    (128, 32, 'SAMPLE'),      # k_mlp_fwd<128> / k_mlp_bwd<128> (no count; always 8 waves): one tile
    (128, 288, 'SAMPLE'),     # a partial block
    (128, 65568, 'SAMPLE'),   # the second round
]
MODES = ['fwd_train', 'fwd_infer', 'bwd', 'bwd_d_enc']


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('width,rows,variant', EDGES)
def test_position_invariance_at_the_scheduling_edges(cuda, width, rows, variant, mode):
    B = _base(width, cuda)
    nray = rows // N
    src = (torch.randperm(nray, generator=torch.Generator().manual_seed(1000 + rows)) % RAYS).to(cuda)    # ray j = base ray perm[j] % 16
    src_rows = (src[:, None] * 32 + torch.arange(32, device=cuda)).reshape(-1)
    if mode.startswith('fwd'):
        enc = B['enc'].view(I16).view(RAYS, 2048)[src].view(BF).view(rows, 64)
        out = _fwd(width, rows, N, enc, B['view'][src].contiguous(), B['wf'], mode == 'fwd_train')
    else:
        draw = B['draw'].view(RAYS, N * 4)[src].view(rows, 4)
        # the ReLU masks the forward must have written (what the forward cases above hold it to), tile for tile
        mask = B['main']['train']['mask'].view(I32).view(9, RAYS, 256)[:, src].contiguous().view(-1).view(torch.uint8)
        out = _bwd(width, rows, N, draw, B['wb'], mask, mode == 'bwd_d_enc')
    assert out['seen'] == _expect_seen(width, variant, mode), out['seen']
    names = _check(_views(width, nray, out), B['views'], src_rows, rows)
    print('W = %d, %d rows, %s: %s; compared %s' % (width, rows, mode, sorted(out['seen']), ' '.join(names)))


# ---------------------------------------------------------------------------
# part 4: compacted lists, device counts, tail rows
# ---------------------------------------------------------------------------
# (capacity in rows, count, tail_count, variant)
LISTS = [
    (70016, 2050, 37, '8W'),     # 8 waves; the tail tiles sit in the one block of the second round; the last tile holds 5 rows
    (1024, 5, 37, '4W'),         # 4 waves; two blocks
    (1024, 0, 37, '4W'),         # a count of zero with a tail
    (1024, 5, 0, '4W'),          # a tail count of zero
]
NTAIL = 37


def _list_case(B, cap, count, tail, cuda):
    ncap = cap // N
    VA = ncap + 100                                            # the view array: more rays than the list holds
    g = torch.Generator().manual_seed(4000 + cap + 64 * count + tail)
    ray_of = torch.randint(0, RAYS, (VA,), generator=g)       # ray r of the batch is base ray ray_of[r]
    perm = torch.randperm(VA, generator=g)
    ray_idx, tail_idx = perm[:ncap], perm[ncap:ncap + NTAIL]   # distinct rays
    src_c, src_t = ray_of[ray_idx[:count]], ray_of[tail_idx[:tail]]
    src_rows = torch.cat([(src_c[:, None] * 32 + torch.arange(32)).reshape(-1), ROWS + src_t]).to(cuda)
    ray_of = ray_of.to(cuda)
    enc = _poison((cap, 64), BF, cuda)                         # rows beyond the count: NaN, never to be read
    enc.view(I16).view(ncap, 2048)[:count] = B['enc'].view(I16).view(RAYS, 2048)[src_c.to(cuda)]
    i32 = lambda t: t.to(I32).to(cuda)
    return dict(V=count * N + tail, src_rows=src_rows, enc=enc, view=B['view'][ray_of].contiguous(),
                draw=B['draw'].view(RAYS, N * 4)[ray_of].reshape(VA * N, 4).contiguous(),         # full layout [VA * N, 4]
                ray_sum=B['draw_tail'][ray_of].contiguous(),
                kw=dict(ray_idx=i32(ray_idx), count=i32(torch.tensor([count])), tail_idx=i32(tail_idx),
                        tail_count=i32(torch.tensor([tail]))))


def _surplus(views, V, want_zero):
    """rows V .. the end of their 32-row tile: what the weight-gradient launch reads beside the valid rows (docs/history.md 4.1c)"""
    hi = (V + 31) // 32 * 32
    for name, got in views:
        x = got[V:hi]
        if name.startswith('stash') and not want_zero:
            assert bool(torch.isfinite(x.view(BF).float()).all()), '%s: surplus rows of the last tile not finite' % name
        if name.startswith('dz') and want_zero:
            assert bool((x.view(BF).float() == 0).all()), '%s: surplus rows of the last tile not zero' % name


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('cap,count,tail,variant', LISTS)
def test_compacted_list_with_device_counts_and_tail_rows(cuda, cap, count, tail, variant, mode):
    width = 256
    B = _base(width, cuda)
    c = _list_case(B, cap, count, tail, cuda)
    V, nt = c['V'], cap // 32
    tr = None
    if mode != 'fwd_infer':
        tr = _fwd(width, cap, N, c['enc'], c['view'], B['wf'], True, **c['kw'])
    if mode == 'fwd_train':
        out = tr
    elif mode == 'fwd_infer':
        out = _fwd(width, cap, N, c['enc'], c['view'], B['wf'], False, **c['kw'])
    else:
        out = _bwd(width, cap, N, c['draw'], B['wb'], tr['mask'], mode == 'bwd_d_enc', draw_ray_sum=c['ray_sum'], **c['kw'])
    assert out['seen'] == _expect_seen(width, variant, mode, tail=True), out['seen']
    names = _check(_views(width, nt, out), B['views'], c['src_rows'], V)
    _surplus(_views(width, nt, out), V, want_zero=mode.startswith('bwd'))
    if mode == 'fwd_train':
        # the encoding tile: the training forward spells the constant encoding out for the weight-gradient launch
        e = _rows_of(c['enc'].view(I16).view(nt, 4, 2, 32, 8))
        hi = (V + 31) // 32 * 32
        const = torch.zeros(64, device=cuda)
        const[30:60] = 1.0
        assert bool((e[count * N:V].view(BF).float() == const).all()), 'encoding of the tail rows'
        assert bool(torch.isfinite(e[V:hi].view(BF).float()).all()), 'encoding tile: surplus rows of the last tile not finite'
        assert bool((e[hi:] == -1).all()), 'encoding tile written beyond the valid rows'
    if tail and mode != 'fwd_infer':
        # the tail rows against the float64 oracle on the constant encoding with tail_idx[i]'s view direction
        o = MR.oracle(width)
        sel = (c['src_rows'][count * N:] - ROWS).cpu()
        fo = dict(raw=o['fwd_tail']['raw'][sel], h=[a[sel] for a in o['fwd_tail']['h']], hc=o['fwd_tail']['hc'][sel])
        bo = dict(dz={j: a[sel] for j, a in o['bwd_tail']['dz'].items()}, d_enc=o['bwd_tail']['d_enc'][sel],
                  dz_out=o['bwd_tail']['dz_out'][sel])
        _gates('tail rows of (%d, %d, %d), %s' % (cap, count, tail, mode),
               _values(width, dict(_views(width, nt, out)), slice(count * N, V)), fo, bo)
    print('capacity %d, count %d, tail %d, %s: %s; compared %s' % (cap, count, tail, mode, sorted(out['seen']), ' '.join(names)))


LAYERS = [(60, 256), (256, 256), (256, 256), (256, 256), (256, 256), (316, 256), (256, 256), (256, 256), (256, 1), (256, 256),
          (283, 128), (128, 3)]                       # flax Dense_l (fan_in, fan_out) of the 8x256 MLP


@pytest.mark.parametrize('cap,count,tail,variant', LISTS)
def test_weight_gradients_of_a_deduplicated_list(cuda, cap, count, tail, variant):
    """mlp_dw_levels + mlp_dw_finalize_levels with the geometry a de-duplicated step passes (train_boxpose.py: one segment of
    count * N + tail_count valid rows, 1 row per "ray") against float64 X^T dZ products of the UNTILED VALID rows.  The launch
    reads whole 32-row tiles, and every buffer started as NaN: the 27 surplus rows of the last tile must be finite operands
    with zero dz.  Tolerances: test_weight_gradients_of_both_split_plans_against_untiled_matmuls' (1e-5 direct, 5e-3 where
    the linear bottleneck's gradients are derived through its weights)."""
    W, IN, KW = 256, 60, 16
    B = _base(W, cuda)
    c = _list_case(B, cap, count, tail, cuda)
    V, nt, flat = c['V'], cap // 32, B['flat']
    tr = _fwd(W, cap, N, c['enc'], c['view'], B['wf'], True, **c['kw'])
    bw = _bwd(W, cap, N, c['draw'], B['wb'], tr['mask'], False, draw_ray_sum=c['ray_sum'], **c['kw'])
    view_tile = ops.expand_view(cap, N, c['view'], out=_poison((cap, 32), BF, cuda), **c['kw'])
    vt = _rows_of(view_tile.view(I16).view(nt, 2, 2, 32, 8))
    hi = (V + 31) // 32 * 32
    assert bool(torch.isfinite(vt[:hi].view(BF).float()).all()), 'view tile: valid and surplus rows finite'
    assert bool((vt[hi:] == -1).all()), 'view tile written beyond the valid rows'
    nrows = torch.tensor([V], dtype=I32, device=cuda)
    part, bpart = ops.dw_buffers(W, cuda)
    part.fill_(float('nan'))
    bpart.fill_(float('nan'))
    geo = ([cap], [1], [nrows])
    ops.mlp_dw_levels(W, *geo, [c['enc']], [view_tile], [tr['stash']], [bw['dz']], [bw['dz_out']], part, bpart)
    grad = torch.zeros_like(flat)
    ops.mlp_dw_finalize_levels(W, IN, *geo, part, bpart, grad, flat)
    assert bool(torch.isfinite(grad).all()), 'gradients finite'

    def nat(rows, perm):
        x = rows[:V].view(BF).double()
        return x[:, H.cperm_cols(x.shape[1] // 16).to(cuda)] if perm else x

    def par(layer):
        fi, fo = LAYERS[layer]
        return ops.mlp_layer_offset(W, IN, layer, False), ops.mlp_layer_offset(W, IN, layer, True), fi, fo
    enc60 = nat(_rows_of(c['enc'].view(I16).view(nt, 4, 2, 32, 8)), False)[:, :60]
    view27 = nat(vt, False)[:, :27]
    h = [nat(_rows_of(_region(tr['stash'], W, nt, j)), True) for j in range(8)]
    hv = nat(_rows_of(_region(tr['stash'], W, nt, 9)), True)
    o9, ob9, _, _ = par(9)
    K9, b9 = flat[o9:o9 + 256 * 256].reshape(256, 256).double(), flat[ob9:ob9 + 256].double()
    K10 = flat[par(10)[0]:par(10)[0] + 283 * 128].reshape(283, 128).double()
    X = {0: enc60, 5: torch.cat([h[4], enc60], 1), 8: h[7], 9: h[7], 10: torch.cat([h[7] @ K9 + b9, view27], 1), 11: hv}
    for layer in (1, 2, 3, 4, 6, 7):
        X[layer] = h[layer - 1]
    dZ = {j: nat(_rows_of(_region(bw['dz'], W, nt, j)), True) for j in range(8)}
    dZ[10] = nat(_rows_of(_region(bw['dz'], W, nt, 9)), True)
    head = nat(_rows_of(bw['dz_out'].view(I16).view(nt, 1, 2, 32, 8)), False)
    dZ[8], dZ[11] = head[:, 3:4], head[:, :3]
    dZ[9] = dZ[10] @ K10[:256].T                                      # through the view layer's bottleneck rows
    rel = lambda a, b: float((a - b).norm() / b.norm())
    worst = {}
    for layer in range(12):
        o, ob, fi, fo = par(layer)
        gk, gb = grad[o:o + fi * fo].reshape(fi, fo).double(), grad[ob:ob + fo].double()
        wk, wb_ = X[layer].T @ dZ[layer], dZ[layer].sum(0)
        worst[layer] = (rel(gk, wk), rel(gb, wb_))
        assert worst[layer][0] < (5e-3 if layer in (9, 10) else 1e-5), 'dK Dense_%d: rel %.3g' % (layer, worst[layer][0])
        assert worst[layer][1] < (5e-3 if layer == 9 else 1e-5), 'db Dense_%d: rel %.3g' % (layer, worst[layer][1])
    g10 = grad[par(10)[0]:par(10)[0] + 283 * 128].reshape(283, 128)[256:].double()
    assert rel(g10, (X[10].T @ dZ[10])[256:]) < 1e-5                  # the view layer's view rows: direct
    print('capacity %d, count %d, tail %d: dK / db rel %s' % (cap, count, tail, {k: '%.2g / %.2g' % v for k, v in worst.items()}))


# ---------------------------------------------------------------------------
# part 5: the comparisons reject what they are there to reject
# ---------------------------------------------------------------------------
def test_negative_controls(cuda):
    width = 256
    o, B = MR.oracle(width), _base(width, cuda)
    b, fo, bo = o['base'], o['fwd'], o['bwd']
    vals = _values(width, B['main']['views'], slice(0, ROWS))
    assert all(v[2] for v in _errors(vals, fo, bo).values()), 'the uncorrupted comparison passes'
    every = set(_errors(vals, fo, bo))

    def rejected(fo2, bo2):
        return {k for k, v in _errors(vals, fo2, bo2).items() if not v[2]}

    # (a) one 32-row tile of the expected tensor taken from the neighbouring ray
    def swap(t):
        t = t.clone()
        t[3 * N:4 * N] = t[4 * N:5 * N]
        return t
    fo_a = dict(raw=swap(fo['raw']), h=[swap(a) for a in fo['h']], hc=swap(fo['hc']))
    bo_a = dict(dz={j: swap(a) for j, a in bo['dz'].items()}, d_enc=swap(bo['d_enc']), dz_out=swap(bo['dz_out']))
    assert rejected(fo_a, bo_a) == every, 'oracle gates, neighbouring tile: only %s rejected' % rejected(fo_a, bo_a)
    rows = 160
    src = (torch.randperm(rows // N, generator=torch.Generator().manual_seed(1000 + rows)) % RAYS).to(cuda)
    enc = B['enc'].view(I16).view(RAYS, 2048)[src].view(BF).view(rows, 64)
    mask = B['main']['train']['mask'].view(I32).view(9, RAYS, 256)[:, src].contiguous().view(-1).view(torch.uint8)
    out = _fwd(width, rows, N, enc, B['view'][src].contiguous(), B['wf'], True)
    out.update(_bwd(width, rows, N, B['draw'].view(RAYS, N * 4)[src].view(rows, 4), B['wb'], mask, True))
    src_bad = src.clone()
    src_bad[2] = (src[2] + 1) % RAYS
    good = (src[:, None] * 32 + torch.arange(32, device=cuda)).reshape(-1)
    bad = (src_bad[:, None] * 32 + torch.arange(32, device=cuda)).reshape(-1)
    for name, got in _views(width, rows // N, out):
        assert _mismatch(got[:rows], B['views'][name][good]) is None, name
        msg = _mismatch(got[:rows], B['views'][name][bad])
        assert msg is not None and 'first row 64 (tile 2)' in msg, 'bitwise, neighbouring tile: %s not rejected (%s)' % (name, msg)
    with pytest.raises(AssertionError):
        _check(_views(width, rows // N, out), B['views'], bad, rows)

    # (b) the expected view directions shifted by one ray: everything behind the view layer, forward and backward, must go
    cond_rows = b['cond'].roll(1, 0)[:, None, :].expand(RAYS, N, 27).reshape(ROWS, 27)
    fo_b = MR.forward64(b['params'], b['x'].reshape(ROWS, -1), cond_rows)
    bo_b = MR.backward64(b['params'], fo_b, b['draw'])
    behind_view = {'raw', 'stash9', 'd_enc'} | {'dz%d' % j for j in STASHED}
    assert rejected(fo_b, bo_b) == behind_view, 'oracle gates, shifted view directions: %s rejected' % rejected(fo_b, bo_b)
    sh = _fwd(width, ROWS, N, B['enc'], B['view'].roll(1, 0).contiguous(), B['wf'], True)
    differ = {name for name, got in _views(width, RAYS, sh) if _mismatch(got[:ROWS], B['views'][name][:ROWS]) is not None}
    assert differ == {'raw', 'stash9', 'mask8'}, 'bitwise, shifted view directions: %s differ' % differ

    # (c) one stash region swapped with the next
    h2, dz2 = list(fo['h']), dict(bo['dz'])
    h2[3], h2[4] = h2[4], h2[3]
    dz2[3], dz2[4] = dz2[4], dz2[3]
    got_r = rejected(dict(raw=fo['raw'], h=h2, hc=fo['hc']), dict(dz=dz2, d_enc=bo['d_enc'], dz_out=bo['dz_out']))
    assert got_r == {'stash3', 'stash4', 'dz3', 'dz4'}, 'oracle gates, swapped regions: %s rejected' % got_r
    for q in ('stash', 'dz'):
        assert _mismatch(B['views'][q + '3'], B['views'][q + '4']) is not None, 'bitwise, swapped regions: ' + q
    # a launch whose regions 3 and 4 changed places in memory does not pass the tile comparison
    nt = ROWS // 32
    st = B['main']['train']['stash'].clone()
    r3, r4 = _region(st, width, nt, 3).clone(), _region(st, width, nt, 4).clone()
    _region(st, width, nt, 3).copy_(r4)
    _region(st, width, nt, 4).copy_(r3)
    with pytest.raises(AssertionError, match='stash3'):
        _check(_views(width, nt, dict(stash=st, mask=B['main']['train']['mask'])), B['views'],
               torch.arange(ROWS, device=cuda), ROWS)
