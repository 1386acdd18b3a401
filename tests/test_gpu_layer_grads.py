"""Every Dense layer's gradient -- each kernel, each bias and the row blocks other code writes -- of every MLP against the oracle
(tests/layer_grads.py), on the production path (train_boxpose.loss_and_grad) at the sizes and edges that select its variants:
engineered per-object hit counts on both sides of the 128- / 256-sample blocks under all three object-MLP dispatches, BARF-masked
encoding rows, the two hit extremes, and tampered product gradients the whole-MLP gate lets through.  The bf16 path is held to the
oracle with bf16-rounded GEMM operands (R.mlp_apply_bf16), the fp32 path (mlp_precision = 'f32') to the plain fp32 oracle;
no_pose_opt, so that every MLP really runs in bf16 on the bf16 path.  N = 32 and B <= 512: ~1 s of CPU oracle per case.
Gates: layer_grads.GATES.  Measured here, worst piece per case: bf16 4.6e-3..1.9e-2 (every ray inside the box: BoxMLP Dense_0
1.8e-2; no ray in any box: MLP_0 1.9e-2), fp32 4.0e-5..4.6e-3 (every ray inside the box: object-frame coordinates up to 40
through the 2^9 encoding); the three object dispatches give the same table."""
import numpy as np
import pytest
import torch

from durf_amd import obbpose_model, ops, synthetic, train_boxpose, utils
from oracle import durf_ref as R
from tests import helpers as H
from tests import layer_grads as LG
from tests.test_gpu_dispatch_matrix import _env

pytestmark = pytest.mark.gpu

N = 32


def _gin(precision):
    utils.clear_gin()
    utils.parse_gin('MipNerfModel.num_samples = %d\nMipNerfModel.density_noise = 0.0\nMipNerfModel.mlp_precision = %r\n'
                    'MipNerfModel.no_pose_opt = True\nMipNerfModel.no_yaw_opt = True\n'
                    'Config.randomized = True\nConfig.rand_bkgd = False\nConfig.grad_max_norm = 1.0\n'
                    'Config.grad_max_val = 0.1\nConfig.tv_loss_mult = 0.0\n' % (N, precision))
    return utils.configured(utils.Config)


def _step(cuda, b, precision, alpha, seed, env=None, bias_seed=None):
    """the product's gradient of one step on batch `b` (random biases, as test_train_step) -> (grad on the CPU, the oracle's
    params, the sampling noise, layout, the variants dispatched)"""
    config = _gin(precision)
    db = H.device_batch(b, cuda)
    B = db['rays'].origins.shape[0]
    model, variables = obbpose_model.construct_mipnerf(seed, db, device=cuda)
    assert model.mlp_precision == precision
    g = torch.Generator().manual_seed(seed if bias_seed is None else bias_seed)
    for name in variables.layout.mlp_names():
        for i in range(12):
            bias = variables['params'][name]['Dense_%d' % i]['bias']
            bias.copy_(((torch.rand(bias.shape, generator=g) - 0.5) * 0.1).to(cuda))
    noise = dict(t_rand=torch.rand(B, N + 1, generator=g), u_rand=torch.rand(B, N + 1, generator=g))
    params = H.oracle_params_from_variables(variables)
    ops.dispatch_reset()
    with _env(**(env or {})):
        grad, _, _ = train_boxpose.loss_and_grad(model, config, 0, variables, db, 3.0, alpha, db['init'][0:1],
                                                 noise={k: v.to(cuda) for k, v in noise.items()})
        torch.cuda.synchronize()
    return grad.cpu(), params, noise, variables.layout, ops.dispatch_seen()


def _oracle(b, params, noise, precision, alpha):
    ob = H.oracle_batch(b)
    ocfg = dict(R.CONFIG_DEFAULTS, randomized=True, tv_loss_mult=0.0)
    _, _, st, ograds = R.train_step(params, R.new_opt_state(params), ob, ocfg, dict(num_samples=N), 5e-4, 3.0, alpha,
                                    ob['init'][0:1], noise=noise, mlp_hook=R.mlp_apply_bf16 if precision == 'bf16' else None)
    assert not (st['losses'] != st['losses']).any(), 'a multi-hit ray in the batch'
    return LG.flat_oracle(ograds)


GATES = {'bf16': LG.GATES['bf16'], 'f32': LG.GATES['f32']}


# ---- engineered hit counts ----
HITS = (0, 1, 5, 9, 120)          # rays per object: 0, 32, 160, 288 and 3840 sample rows per level at N = 32
MISSES = 310                      # B = 445: not a multiple of 32


def engineered_batch():
    """K = 5 objects hit by exactly HITS rays each, plus MISSES rays that hit none, drawn from a large pool classified against
    init[ts] (float64 slab test, synthetic._hits): a hit is a ray inside a box shrunk by 3 % and outside every other box grown
    by 3 %, a miss one outside every grown box -- so the fp32 hit tests of the oracle and the product agree with the count"""
    b = synthetic.make_batch(3000, 5, seed=57, hit_range=(0.35, 0.5))
    ts = b['ts']
    c, e = b['init'][ts].astype(np.float64), b['ext'].astype(np.float64)
    o, d = b['rays']['origins'].astype(np.float64), b['rays']['directions'].astype(np.float64)
    core = synthetic._hits(o, d, c[:, :3], c[:, 3:], e * 0.97)
    hull = synthetic._hits(o, d, c[:, :3], c[:, 3:], e * 1.03)
    single = hull.sum(-1) == 1
    idx = [np.nonzero(core[:, k] & single)[0][:n] for k, n in enumerate(HITS)]
    idx.append(np.nonzero(hull.sum(-1) == 0)[0][:MISSES])
    assert [len(i) for i in idx] == list(HITS) + [MISSES], [len(i) for i in idx]
    idx = np.random.default_rng(3).permutation(np.concatenate(idx))
    return H.subset_batch(b, idx)


def _hit_counts(b):
    return LG.hit_counts(H.oracle_batch(b), b['ts'])


# the object MLPs' three dispatches at this size (bit-identical A/B switches, ops.obj_mix / mlp_fwd.hip obj_msplit):
# items of the background MLP's persistent launches, M-split launches of their own, sample-split launches
WAYS = [('mixed', {}, {'FWD_MIX', 'BWD_MIX', 'FWD_ENC'}),
        ('M-split', dict(DURF_OBJ_MIX=0), {'FWD128_MSPLIT', 'BWD128_MSPLIT'}),
        ('sample-split', dict(DURF_OBJ_MSPLIT=0), {'FWD128_SAMPLE', 'BWD128_SAMPLE'})]


@pytest.fixture(scope='module')
def engineered(cuda):
    b = engineered_batch()
    assert _hit_counts(b) == list(HITS), 'the oracle classifies the rays as the pool did'
    grad, params, noise, lay, seen = _step(cuda, b, 'bf16', 10.0, 8)
    return dict(b=b, grad=grad, params=params, noise=noise, lay=lay, seen=seen, ograd=_oracle(b, params, noise, 'bf16', 10.0))


@pytest.mark.parametrize('way', [w[0] for w in WAYS])
def test_engineered_hit_counts_bf16(cuda, engineered, way):
    """per-object hit counts 0 / 1 / 5 / 9 / 120 rays (0, 32, 160, 288, 3840 rows) plus misses, B = 445 (ragged), through each
    object-MLP dispatch; the count-0 object's gradient is exactly zero"""
    E = engineered
    _, env, variants = [w for w in WAYS if w[0] == way][0]
    if env:
        grad, _, _, _, seen = _step(cuda, E['b'], 'bf16', 10.0, 8, env=env)
    else:
        grad, seen = E['grad'], E['seen']
    assert variants <= seen, '%s: expected %s, dispatched %s' % (way, sorted(variants - seen), sorted(seen))
    pcs = LG.pieces_for(E['lay'], E['b']['ts'])
    zeros = LG.structural_zeros(pcs, unhit=['BoxMLP_0'])
    print(LG.compare(grad, E['ograd'], pcs, GATES['bf16'], zeros, title='engineered hits, bf16, %s' % way))


def test_engineered_hit_counts_f32(cuda):
    b = engineered_batch()
    grad, params, noise, lay, seen = _step(cuda, b, 'f32', 10.0, 8)
    pcs = LG.pieces_for(lay, b['ts'])
    zeros = LG.structural_zeros(pcs, unhit=['BoxMLP_0'])
    print(LG.compare(grad, _oracle(b, params, noise, 'f32', 10.0), pcs, GATES['f32'], zeros, title='engineered hits, f32'))


# ---- BARF masking ----
@pytest.mark.parametrize('precision', ['bf16', 'f32'])
@pytest.mark.parametrize('alpha', [4.5, 2.5])
def test_barf_masked_encoding_rows(cuda, alpha, precision):
    """alpha below the full window: feature f of the 60 is weighted by barf_weights(alpha, 10)[f // 6] (the reference's f//6
    quirk, enc_lane.h); where that weight is exactly 0 (alpha 4.5: every cosine feature; 2.5: features 18..59) the rows
    3 + f of every BoxMLP's Dense_0 kernel and 128 + 3 + f of its Dense_5 kernel must be exactly zero, as in the oracle; the
    rows weighted 0.5 are held by the gate"""
    b = synthetic.make_batch(300, 2, seed=66, hit_range=(0.3, 0.45))
    grad, params, noise, lay, _ = _step(cuda, b, precision, alpha, 6)
    pcs = LG.pieces_for(lay, b['ts'], barf_alpha=alpha)
    zeros = LG.structural_zeros(pcs, unhit=LG.unhit_objects(H.oracle_batch(b), b['ts']))
    assert len([z for z in zeros if z.endswith('masked]')]) == 2 * 2
    print(LG.compare(grad, _oracle(b, params, noise, precision, alpha), pcs, GATES[precision], zeros,
                     title='BARF alpha %g, %s' % (alpha, precision)))


# ---- hit extremes ----
@pytest.mark.parametrize('precision', ['bf16', 'f32'])
@pytest.mark.parametrize('case', ['all_rays_hit', 'no_ray_hits'])
def test_hit_extremes_against_the_oracle(cuda, case, precision):
    """every ray hits the one box (the background MLP sees only de-duplicated once-per-ray rows), or no ray hits any of K = 3
    boxes (every BoxMLP gradient exactly zero) -- test_gpu_dedup.py::test_extreme_hit_fractions holds these to the
    sample-by-sample path only"""
    if case == 'all_rays_hit':
        b = synthetic.make_batch(200, 1, seed=5)
        b['ext'] = b['ext'] * 0 + 1.0e3                  # a box that contains every camera
    else:
        b = synthetic.make_batch(200, 3, seed=5)
        b['init'] = b['init'].copy()
        b['init'][:, :, 2] = 1.0e4                       # far behind every camera
    K = b['init'].shape[1]
    assert _hit_counts(b) == ([200] if case == 'all_rays_hit' else [0] * K)
    grad, params, noise, lay, _ = _step(cuda, b, precision, 10.0, 5)
    pcs = LG.pieces_for(lay, b['ts'])
    zeros = LG.structural_zeros(pcs, unhit=['BoxMLP_%d' % k for k in range(K)] if case == 'no_ray_hits' else ())
    print(LG.compare(grad, _oracle(b, params, noise, precision, 10.0), pcs, GATES[precision], zeros,
                     title='%s, %s' % (case, precision)))


# ---- tampered product gradients ----
def test_tampered_product_gradients_fail_the_per_piece_gate(cuda):
    """test_train_step's scenario (B = 256, K = 3, batch seed 34, random biases): the product's own bf16 gradient passes; each
    spoilt kernel output fails the per-piece gate.  The whole-MLP gate of the end-to-end tests (5e-2) passes MLP_0's Dense_9..11
    zeroed (0.043 on the CPU oracle), its Dense_0 kernel sign-flipped (0.038) and its 27 view rows zeroed (0.029); a BoxMLP's
    view rows carry more of its norm (~0.5), and a hidden bias scaled by 0.8 moves MLP_0's gradient by < 1e-2."""
    b = synthetic.make_batch(256, 3, seed=34)
    grad, params, noise, lay, _ = _step(cuda, b, 'bf16', 10.0, 1, bias_seed=4)
    ograd = _oracle(b, params, noise, 'bf16', 10.0)
    pcs = LG.pieces_for(lay, b['ts'])
    zeros = LG.structural_zeros(pcs, unhit=LG.unhit_objects(H.oracle_batch(b), b['ts']))
    LG.compare(grad, ograd, pcs, GATES['bf16'], zeros)
    cases = [(how, LG.tamper(grad, pcs, how)) for how in LG.TAMPERS]
    cases.append(('zero_view_rows of MLP_0', LG.tamper(grad, pcs, 'zero_view_rows', obj='MLP_0')))
    report = []
    for how, bad in cases:
        group = 'BoxMLP_0' if how == 'zero_view_rows' else 'MLP_0'
        report.append('%s: whole-MLP %.3f' % (how, LG.whole_mlp_rel(bad, ograd, pcs, group)))
        with pytest.raises(AssertionError, match='pieces over their gate'):
            LG.compare(bad, ograd, pcs, GATES['bf16'], zeros, title=how)
    print('tampers rejected by the per-piece gate; ' + ', '.join(report))
    for how, bad in cases:
        if how in ('zero_head', 'flip_dense0', 'zero_view_rows of MLP_0'):
            assert LG.whole_mlp_rel(bad, ograd, pcs, 'MLP_0') < 5e-2, how
