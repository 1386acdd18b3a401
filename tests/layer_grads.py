"""Per-piece gradient comparison: the flat gradient of one training step, split into the pieces that different kernels write,
each held to the oracle on its own.

A whole-MLP norm-wise gate cannot see a layer that carries a few per cent of its MLP's gradient norm: zeroing MLP_0's
Dense_9..11 (bottleneck, view layer, rgb head), flipping the sign of its Dense_0 kernel or zeroing a BoxMLP's view rows all
pass a 5e-2 whole-MLP gate.  Here every Dense kernel and bias of every MLP is a piece of its own, and so is every row block
that another code path writes: Dense_5's rows from h4 and from the skip input (the encoding tile), Dense_10's bottleneck rows
(k_bottleneck_grads) and its 27 view rows, the BARF-masked encoding rows of the object MLPs, and the box-pose rows.

The flat layout is R.params_leaves order (box_centers [T, K, 6], MLP_0, BoxMLP_0..K-1; each Dense kernel [in, out] then its
bias), the order of the product's flat parameter buffer (durf_amd/obbpose_model.py ParamLayout).
"""
import collections
import math

import torch

from oracle import durf_ref as R

IN_BKGD, IN_OBJ, VIEW = 60, 63, 27

# A piece whose oracle norm is below FLOOR x its group's (MLP's, or box_centers[ts]'s) oracle norm is measured against that
# floor instead: its error is then a share of the group's gradient, not of its own (near-)zero.
FLOOR = 1e-3

# Per-piece gates, per comparison and piece kind (MLP_0 / BoxMLP, kernel / bias): about 3x the worst value measured on the
# MI355X over every case of the suite that carries them (tests/test_gpu_layer_grads.py and the end-to-end tests of
# test_gpu_train.py, test_gpu_fullsize.py, test_gpu_dedup.py, test_gpu_x3.py, test_gpu_noview.py, test_gpu_f32_exact.py,
# test_gpu_dispatch_matrix.py), and never above the comparison's ceiling.
#   'bf16':        the bf16 production path against the oracle with bf16-rounded GEMM operands (R.mlp_apply_bf16); ceiling 0.1.
#                  Measured: MLP_0 kernels 2.4e-3..3.2e-2, biases 1.0e-3..2.3e-2; BoxMLP kernels 4.6e-3..4.8e-2, biases
#                  4.0e-3..5.7e-2.  The worst pieces are the first layers (Dense_0..2) of sparsely hit objects on two-level
#                  steps (train_step K=3, an object of 4 rays: Dense_0 bias 5.7e-2, Dense_1 4.9e-2, Dense_2 4.1e-2, ...,
#                  Dense_11 < 1e-2; one level, test_train_step_with_other_level_counts L=1: <= 6.6e-3).  Not the MLP
#                  arithmetic: the emulation rounds what the kernels round (autograd casts each activation gradient to bf16
#                  through _bf.  On the CPU, on that batch: rounding the heads' d(raw) to bf16 as the kernels do, which the
#                  emulation does not, moves these pieces by 5e-3; fp64 instead of fp32 accumulation by 3e-3).  It is the
#                  resampled level's conditioning: its sample positions follow the level-0 weights, which product and
#                  emulation compute with different bf16 rounding flips, and the emulation's own gradient moves by 2.6e-2 on
#                  the same pieces when its sampling noise moves by 1e-6 (5.7e-2 for another draw of that shift;
#                  test_layer_grads_gate.py::test_bf16_object_layers_are_conditioned_by_the_sample_positions).
#   'f32':         the exact-fp32 path (mlp_precision = 'f32', or the fp32 object branch) against the fp32 oracle; ceiling 1e-2.
#                  Measured: MLP_0 kernels 1.5e-5..3.4e-3, biases 8.9e-6..2.0e-3; BoxMLP kernels 1.0e-6..7.3e-3 (the
#                  split-operand bf16x3 objects at 512 x 128 samples), biases 7.6e-7..4.1e-3 (every ray inside one box:
#                  object-frame coordinates up to 40 through the 2^9 encoding).
#   'bf16_vs_f32': the bf16 production path against the plain fp32 oracle or the product's exact-fp32 path; ceiling 0.25.
#                  Measured: MLP_0 kernels 5.0e-2..1.4e-1, biases 3.3e-2..1.2e-1; BoxMLP 2.9e-3..1.1e-1 -- bf16 rounding
#                  itself, with the same depth profile: the bf16-rounded CPU oracle is 0.14 away from the fp32 one on
#                  BoxMLP Dense_0/1 and 0.095 on MLP_0's Dense_0 (tests/test_layer_grads_gate.py).
GATES = {
    'bf16': {'MLP_0.kernel': 0.1, 'MLP_0.bias': 0.07, 'BoxMLP.kernel': 0.1, 'BoxMLP.bias': 0.1},
    'f32': {'MLP_0.kernel': 1e-2, 'MLP_0.bias': 6e-3, 'BoxMLP.kernel': 1e-2, 'BoxMLP.bias': 1e-2},
    'bf16_vs_f32': {'MLP_0.kernel': 0.25, 'MLP_0.bias': 0.25, 'BoxMLP.kernel': 0.25, 'BoxMLP.bias': 0.25},
}

Piece = collections.namedtuple('Piece', 'name group kind idx')


def barf_masked_features(alpha):
    """indices f (of the 60 encoding features after the identity x) whose BARF weight is exactly zero at `alpha`.  Feature f
    is weighted by barf_weights(alpha, 10)[f // 6] (R.weighted_ipe, the reference's f//6 quirk): monotone in f, so the masked
    features are a tail."""
    w = R.barf_weights(alpha, 10, torch.float64)
    return [f for f in range(60) if float(w[f // 6]) == 0.0]


def pieces(T, K, ts, use_viewdirs=True, barf_alpha=None, check_offsets=True):
    """-> [Piece(name, group, kind, idx)] covering the flat gradient exactly once; idx is a slice or an index tensor.
    use_viewdirs=False: MLP_0 is the 10-Dense tree (no bottleneck, no view layer).  barf_alpha: split the object MLPs' encoding
    rows (Dense_0 rows 3.., Dense_5 rows 128+3..) into the live ones and the ones BARF masks to exactly zero at that alpha."""
    out = []
    nb = T * K * 6
    row = K * 6
    for k in range(K):
        o = ts * row + 6 * k
        out.append(Piece('box_centers[ts].%d.position' % k, 'box_centers', 'position', slice(o, o + 3)))
        out.append(Piece('box_centers[ts].%d.rotation' % k, 'box_centers', 'rotation', slice(o + 3, o + 6)))
    if T > 1 and K > 0:
        other = torch.cat([torch.arange(0, ts * row), torch.arange((ts + 1) * row, nb)])
        out.append(Piece('box_centers[other ts]', 'box_centers', 'other_ts', other))
    off = nb
    masked = barf_masked_features(barf_alpha) if barf_alpha is not None else []
    cut = masked[0] if masked else None
    mlps = [('MLP_0', IN_BKGD, R.MLP_BKGD, VIEW if use_viewdirs else None)] + \
           [('BoxMLP_%d' % k, IN_OBJ, R.MLP_BOX, VIEW) for k in range(K)]
    for name, in_dim, cfg, view_dim in mlps:
        W = cfg['net_width']
        shapes = R.mlp_layer_shapes(in_dim, view_dim, cfg)
        base = off
        if check_offsets and len(shapes) == 12:
            from durf_amd import ops
            o = 0
            for i, (fi, fo) in enumerate(shapes):
                assert ops.mlp_layer_offset(W, in_dim, i, False) == o, (name, i, 'kernel')
                assert ops.mlp_layer_offset(W, in_dim, i, True) == o + fi * fo, (name, i, 'bias')
                o += fi * fo + fo
        for i, (fi, fo) in enumerate(shapes):
            pre = '%s.Dense_%d' % (name, i)
            blocks = [('kernel', 0, fi)]
            if i == 0 and name != 'MLP_0' and cut is not None:
                blocks = [('kernel[live]', 0, 3 + cut), ('kernel[masked]', 3 + cut, fi)]
            elif i == 5:
                blocks = [('kernel[h4]', 0, W), ('kernel[skip]', W, fi)]
                if name != 'MLP_0' and cut is not None:
                    blocks = [('kernel[h4]', 0, W), ('kernel[skip live]', W, W + 3 + cut),
                              ('kernel[skip masked]', W + 3 + cut, fi)]
            elif i == 10 and len(shapes) == 12:
                blocks = [('kernel[bottleneck]', 0, W), ('kernel[view]', W, fi)]
            for label, r0, r1 in blocks:
                out.append(Piece('%s.%s' % (pre, label), name, 'kernel', slice(off + r0 * fo, off + r1 * fo)))
            off += fi * fo
            out.append(Piece(pre + '.bias', name, 'bias', slice(off, off + fo)))
            off += fo
        assert off - base == sum(a * b + b for a, b in shapes)
    return out


def pieces_for(layout, ts, barf_alpha=None):
    """pieces() of a product's ParamLayout (durf_amd/obbpose_model.py)"""
    pcs = pieces(layout.T, layout.K, ts, layout.use_viewdirs, barf_alpha)
    last = pcs[-1].idx
    assert last.stop == layout.total, (last.stop, layout.total)
    for name in layout.mlp_names():
        first = [p for p in pcs if p.group == name][0]
        assert first.idx.start == layout.mlp_off[name], name
    return pcs


def structural_zeros(pcs, frozen_pose=True, unhit=(), masked=True):
    """names of the pieces that are exactly zero in the oracle for a structural reason -- valid with weight_decay_mult = 0 only:
    box_centers rows of the other timesteps, the pose of frozen boxes, the whole MLP of an object no ray hits, and the
    encoding rows BARF weights by exactly 0 (pieces(barf_alpha=...))"""
    out = []
    for p in pcs:
        if p.kind == 'other_ts' or (frozen_pose and p.kind in ('position', 'rotation')) or p.group in unhit or \
                (masked and p.name.endswith('masked]')):
            out.append(p.name)
    return out


def flat_oracle(ograds):
    """the oracle's per-leaf gradients (R.params_leaves order) -> one flat float64 tensor"""
    return torch.cat([g.reshape(-1) for g in ograds]).double()


def compare(grad, ograd, pcs, gates, zeros=(), title=''):
    """Hold every piece of `grad` (the product's flat gradient) to `ograd` (the oracle's): |g - o| / |o| in float64, with
    |o| floored at FLOOR x the group's oracle norm (marked 'floor').  `gates`: {kind: gate}; a piece whose kind has no gate is
    reported, not gated.  `zeros`: names of structural zeros -- the oracle's piece must be exactly zero and the product's too.
    -> the table (worst piece first) as a string; AssertionError with the whole table if a piece fails."""
    g = grad.detach().reshape(-1).cpu().double()
    o = ograd.detach().reshape(-1).cpu().double()
    assert g.numel() == o.numel() == pcs[-1].idx.stop, (g.numel(), o.numel(), pcs[-1].idx.stop)
    zeros = set(zeros)
    unknown = zeros - {p.name for p in pcs}
    assert not unknown, 'structural zeros that are no piece: %s' % sorted(unknown)
    gnorm = collections.defaultdict(float)
    for p in pcs:
        gnorm[p.group] += float((o[p.idx] ** 2).sum())
    rows, bad = [], []
    for p in pcs:
        gp, op = g[p.idx], o[p.idx]
        if p.name in zeros:
            assert int(torch.count_nonzero(op)) == 0, '%s is declared a structural zero but the oracle has %d nonzeros' % (
                p.name, int(torch.count_nonzero(op)))
            nz = int(torch.count_nonzero(gp))
            rows.append((math.inf if nz else 0.0, p.name, 'nonzero %d of %d' % (nz, gp.numel()), '== 0', ''))
            if nz:
                bad.append(p.name)
            continue
        on = float(op.norm())
        fl = FLOOR * math.sqrt(gnorm[p.group])
        den, note = (on, '') if on >= fl else (fl, 'floor')
        d = float((gp - op).norm())
        err = d / den if den > 0 else (0.0 if d == 0 else math.inf)
        gate = _gate(gates, p)
        rows.append((err / gate if gate else -1.0, p.name, '%.3e' % err, '%.2g' % gate if gate else '-', note))
        if gate is not None and not err < gate:
            bad.append(p.name)
    rows.sort(key=lambda r: -r[0])
    w = max(len(r[1]) for r in rows)
    worst = worst_by_kind(grad, ograd, pcs, zeros)
    lines = ['%s%s' % (title + ': ' if title else '', 'per-piece gradient error vs the oracle (%d pieces, %d failing); worst %s'
                       % (len(rows), len(bad), ', '.join('%s %.2e' % kv for kv in sorted(worst.items()))))]
    lines += ['  %-*s  %-18s  %-6s %s' % (w, r[1], r[2], r[3], r[4]) for r in rows]
    table = '\n'.join(lines)
    if bad:
        raise AssertionError('pieces over their gate: %s\n%s' % (', '.join(bad), table))
    return table


def _kind(p):
    return ('MLP_0.' if p.group == 'MLP_0' else 'BoxMLP.' if p.group.startswith('BoxMLP') else '') + p.kind


def _gate(gates, p):
    """gates[kind], or gates['MLP_0.' + kind] / gates['BoxMLP.' + kind] where one MLP runs at another precision"""
    return gates.get(_kind(p), gates.get(p.kind))


def mixed_gates(bkgd, obj):
    """gates for a step whose background MLP and object MLPs run at different precisions (e.g. pose optimisation: the
    box-hit rays in fp32)"""
    out = {k: v for k, v in GATES[bkgd].items() if k.startswith('MLP_0.')}
    out.update({k: v for k, v in GATES[obj].items() if k.startswith('BoxMLP.')})
    return out


def hit_counts(ob, ts):
    """rays of the oracle batch `ob` that hit each box at init[ts] (the oracle's own hit test, R.model_apply)"""
    rays, init, ext = ob['rays'], ob['init'], ob['ext']
    K, B = init.shape[1], rays.origins.shape[0]
    if K == 0:
        return []
    oo, do = R.world2object_rpy(rays.origins, rays.directions, init[ts, :, :3].expand(B, K, 3),
                                R.aa2matrix(init[ts, :, 3:]).expand(B, K, 3, 3))
    _, _, hit = R.ray_box_intersection(oo, do, -ext.expand(B, K, 3), ext.expand(B, K, 3))
    return [int(n) for n in hit.sum(0)]


def unhit_objects(ob, ts):
    """the object MLPs no ray of the oracle batch `ob` hits: their gradients are structural zeros"""
    return ['BoxMLP_%d' % k for k, n in enumerate(hit_counts(ob, ts)) if n == 0]


def worst_by_kind(grad, ograd, pcs, zeros=()):
    """{kind: worst error} over the non-zero pieces (for measuring gates)"""
    g = grad.detach().reshape(-1).cpu().double()
    o = ograd.detach().reshape(-1).cpu().double()
    gnorm = collections.defaultdict(float)
    for p in pcs:
        gnorm[p.group] += float((o[p.idx] ** 2).sum())
    out = {}
    for p in pcs:
        if p.name in zeros:
            continue
        on = max(float(o[p.idx].norm()), FLOOR * math.sqrt(gnorm[p.group]))
        if on > 0:
            out[_kind(p)] = max(out.get(_kind(p), 0.0), float((g[p.idx] - o[p.idx]).norm()) / on)
    return out


# ---- tampers: what a subtly wrong kernel would leave, each a few per cent of its MLP's gradient norm ----
def _by_name(pcs, name):
    return [p for p in pcs if p.name == name][0]


def _by_prefix(pcs, prefix):
    return [p for p in pcs if p.name.startswith(prefix)]


def tamper(grad, pcs, how, obj='BoxMLP_0'):
    """a copy of `grad` with one kernel's output spoilt:
      'zero_head':        MLP_0's Dense_9, Dense_10 and Dense_11 zeroed (bottleneck, view layer, rgb head)
      'flip_dense0':      MLP_0's Dense_0 kernel sign-flipped
      'zero_view_rows':   the 27 view rows of `obj`'s Dense_10 zeroed
      'scale_bias':       MLP_0's Dense_3 bias scaled by 0.8"""
    t = grad.detach().clone().reshape(-1)
    if how == 'zero_head':
        for i in (9, 10, 11):
            for p in _by_prefix(pcs, 'MLP_0.Dense_%d.' % i):
                t[p.idx] = 0
    elif how == 'flip_dense0':
        p = _by_name(pcs, 'MLP_0.Dense_0.kernel')
        t[p.idx] = -t[p.idx]
    elif how == 'zero_view_rows':
        p = _by_name(pcs, '%s.Dense_10.kernel[view]' % obj)
        t[p.idx] = 0
    elif how == 'scale_bias':
        p = _by_name(pcs, 'MLP_0.Dense_3.bias')
        t[p.idx] = 0.8 * t[p.idx]
    else:
        raise ValueError(how)
    return t


TAMPERS = ('zero_head', 'flip_dense0', 'zero_view_rows', 'scale_bias')


def whole_mlp_rel(grad, ograd, pcs, group):
    """the existing whole-MLP gate's measure: |g - o| / |o| over one MLP's flat gradient"""
    idx = [p.idx for p in pcs if p.group == group]
    sl = slice(idx[0].start, idx[-1].stop)
    g, o = grad.reshape(-1)[sl].double(), ograd.reshape(-1)[sl].double()
    return float((g - o).norm() / o.norm())
