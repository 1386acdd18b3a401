"""CPU self-test of the per-piece gradient gate (tests/layer_grads.py): its pieces tile the flat layout the product uses, an
oracle gradient with 1 % noise in every piece passes, and each spoilt kernel output the whole-MLP gate lets through fails."""
import pytest
import torch

from durf_amd import obbpose_model, synthetic
from oracle import durf_ref as R
from tests import helpers as H
from tests import layer_grads as LG

B, K, N = 256, 3, 32


@pytest.fixture(scope='module')
def oracle_grads():
    """test_train_step's setup (B = 256, K = 3, N = 32, batch seed 34, random biases): the oracle's gradient with bf16-rounded
    GEMM operands and with plain fp32 ones"""
    b = synthetic.make_batch(B, K, seed=34)
    ob = H.oracle_batch(b)
    params = R.init_params(1, ob['init'], K)
    g = torch.Generator().manual_seed(4)
    for name in ['MLP_0'] + ['BoxMLP_%d' % k for k in range(K)]:
        for layer in params[name]:
            layer[1] = (torch.rand(layer[1].shape, generator=g) - 0.5) * 0.1
    noise = dict(t_rand=torch.rand(B, N + 1, generator=g), u_rand=torch.rand(B, N + 1, generator=g))
    ocfg = dict(R.CONFIG_DEFAULTS, randomized=True, tv_loss_mult=0.0)
    out = {}
    # the last: the bf16 emulation with its sampling noise moved by 1e-6
    shifted = dict(noise, t_rand=noise['t_rand'] + 1e-6 * torch.randn(B, N + 1, generator=torch.Generator().manual_seed(12)))
    for nm, hook, nz in (('bf16', R.mlp_apply_bf16, noise), ('f32', None, noise), ('bf16 shifted', R.mlp_apply_bf16, shifted)):
        _, _, st, ograds = R.train_step(params, R.new_opt_state(params), ob, ocfg, dict(num_samples=N), 5e-4, 3.0, 10.0,
                                        ob['init'][0:1], noise=nz, mlp_hook=hook)
        assert not (st['losses'] != st['losses']).any()
        out[nm] = LG.flat_oracle(ograds)
    return b, out


def _noisy(o, pcs, seed):
    """o plus seeded noise of 1 % of each piece's norm in every piece"""
    g = torch.Generator().manual_seed(seed)
    t = o.clone()
    for p in pcs:
        n = torch.randn(o[p.idx].shape, generator=g, dtype=torch.float64)
        t[p.idx] = o[p.idx] + 0.01 * float(o[p.idx].norm()) * n / n.norm()
    return t


def test_pieces_tile_the_flat_layout_of_both_trees():
    for T, K_, ts, view in ((5, 3, 2, True), (5, 0, 0, False), (1, 1, 0, True), (4, 8, 3, True)):
        lay = obbpose_model.ParamLayout(T, K_, view)
        pcs = LG.pieces_for(lay, ts)                    # (12-Dense MLPs: offsets checked against ops.mlp_layer_offset)
        cover = torch.zeros(lay.total, dtype=torch.int64)
        for p in pcs:
            cover[p.idx] += 1
        assert bool((cover == 1).all()), 'every flat entry in exactly one piece'
        assert len({p.name for p in pcs}) == len(pcs)
        n_mlp0 = len([p for p in pcs if p.group == 'MLP_0'])
        # 12 Dense: 12 biases + 12 kernels + Dense_5's and Dense_10's second row block; 10 Dense: no bottleneck / view layer
        assert n_mlp0 == (26 if view else 21)
        for k in range(K_):
            assert len([p for p in pcs if p.group == 'BoxMLP_%d' % k]) == 26
        assert len([p for p in pcs if p.group == 'box_centers']) == 2 * K_ + (1 if T > 1 and K_ else 0)
    # the named row blocks sit where the kernels write them
    lay = obbpose_model.ParamLayout(5, 1)
    pcs = {p.name: p for p in LG.pieces_for(lay, 1)}
    o10 = lay.mlp_off['MLP_0'] + sum(a * b + b for a, b in R.mlp_layer_shapes(60, 27, R.MLP_BKGD)[:10])
    assert pcs['MLP_0.Dense_10.kernel[bottleneck]'].idx == slice(o10, o10 + 256 * 128)
    assert pcs['MLP_0.Dense_10.kernel[view]'].idx == slice(o10 + 256 * 128, o10 + 283 * 128)
    assert pcs['box_centers[ts].0.rotation'].idx == slice(1 * 6 + 3, 1 * 6 + 6)


@pytest.mark.parametrize('alpha,cut', [(4.5, 30), (2.5, 18), (10.0, None), (8.5, 54), (9.5, None)])
def test_barf_masked_rows(alpha, cut):
    """feature f of the 60 is weighted by barf_weights(alpha, 10)[f // 6]: at 4.5 every cosine feature (30..59) is masked"""
    assert LG.barf_masked_features(alpha) == ([] if cut is None else list(range(cut, 60)))
    pcs = {p.name: p for p in LG.pieces(5, 2, 0, barf_alpha=alpha, check_offsets=False)}
    if cut is None:
        assert 'BoxMLP_1.Dense_0.kernel[masked]' not in pcs and 'BoxMLP_1.Dense_0.kernel' in pcs
        return
    o = pcs['BoxMLP_1.Dense_0.kernel[live]'].idx.start
    assert pcs['BoxMLP_1.Dense_0.kernel[masked]'].idx == slice(o + (3 + cut) * 128, o + 63 * 128)
    o5 = pcs['BoxMLP_1.Dense_5.kernel[h4]'].idx.start
    assert pcs['BoxMLP_1.Dense_5.kernel[skip masked]'].idx == slice(o5 + (128 + 3 + cut) * 128, o5 + 191 * 128)
    assert 'MLP_0.Dense_0.kernel' in pcs and 'MLP_0.Dense_5.kernel[skip]' in pcs      # the background is not BARF-weighted


def test_the_gate_passes_noise_and_rejects_what_the_whole_mlp_gate_lets_through(oracle_grads):
    b, og = oracle_grads
    o = og['bf16']
    pcs = LG.pieces(5, K, b['ts'], check_offsets=False)
    zeros = LG.structural_zeros(pcs)
    gates = LG.GATES['bf16']
    product = _noisy(o, pcs, 0)
    print(LG.compare(product, o, pcs, gates, zeros, title='oracle + 1 % noise'))
    cases = [(how, LG.tamper(product, pcs, how)) for how in LG.TAMPERS]
    cases.append(('zero_view_rows of MLP_0', LG.tamper(product, pcs, 'zero_view_rows', obj='MLP_0')))
    for how, bad in cases:
        # MLP_0's zeroed head, its sign-flipped Dense_0 and its zeroed view rows pass the whole-MLP gate of the end-to-end
        # tests (5e-2): only the per-piece gate sees them (a BoxMLP's view rows carry more of its norm)
        if how in ('zero_head', 'flip_dense0', 'zero_view_rows of MLP_0'):
            assert LG.whole_mlp_rel(bad, o, pcs, 'MLP_0') < 5e-2, how
        with pytest.raises(AssertionError, match='pieces over their gate'):
            LG.compare(bad, o, pcs, gates, zeros, title=how)
    # a structural zero that is not zero in the product fails, however small
    p = [q for q in pcs if q.name == 'box_centers[other ts]'][0]
    bad = product.clone()
    bad[p.idx[0]] = 1e-30
    with pytest.raises(AssertionError, match='box_centers'):
        LG.compare(bad, o, pcs, gates, zeros)
    # and one declared where the oracle is not zero is a mistake of the test, not a pass
    with pytest.raises(AssertionError, match='declared a structural zero'):
        LG.compare(product, o, pcs, gates, zeros + ['MLP_0.Dense_0.bias'])


def test_bf16_rounding_alone_stays_inside_the_bf16_vs_fp32_ceiling(oracle_grads):
    """the bf16-rounded oracle against the plain one: what the 'bf16_vs_f32' comparisons have to leave room for"""
    b, og = oracle_grads
    pcs = LG.pieces(5, K, b['ts'], check_offsets=False)
    table = LG.compare(og['bf16'], og['f32'], pcs, LG.GATES['bf16_vs_f32'], LG.structural_zeros(pcs),
                       title='bf16-rounded oracle vs fp32 oracle')
    print(table)
    worst = LG.worst_by_kind(og['bf16'], og['f32'], pcs, LG.structural_zeros(pcs))
    assert worst['MLP_0.kernel'] > 1e-2, 'bf16 rounding must show (else this is no comparison): %s' % worst


def test_bf16_object_layers_are_conditioned_by_the_sample_positions(oracle_grads):
    """why the bf16 gates of the first object layers need room (layer_grads.GATES): the bf16 emulation against ITSELF, with its
    stratified-sampling noise moved by 1e-6, moves by several per cent on the first layers of the sparsely hit objects (the
    batch's objects are hit by 1, 19 and 4 rays) -- the resampled level's sample positions follow the level-0 weights, and the
    product computes those with other bf16 rounding flips than the emulation does"""
    b, og = oracle_grads
    pcs = LG.pieces(5, K, b['ts'], check_offsets=False)
    assert LG.hit_counts(H.oracle_batch(b), b['ts']) == [1, 19, 4]
    print(LG.compare(og['bf16 shifted'], og['bf16'], pcs, LG.GATES['bf16'], LG.structural_zeros(pcs),
                     title='bf16 emulation, sampling noise moved by 1e-6'))
    worst = LG.worst_by_kind(og['bf16 shifted'], og['bf16'], pcs, LG.structural_zeros(pcs))
    assert worst['BoxMLP.bias'] > 2e-2 and worst['MLP_0.kernel'] < 5e-2, worst
