"""BASELINE.json's full sizes (cfg2: 4096 rays x 128 samples x K=1; cfg3: K=3) through size-independent
properties -- the oracle needs minutes per step at these sizes, so parity at full size is pinned by:
  * invariants of volumetric rendering recomputed from the outputs (mip.py:285-327),
  * chunk invariance: rays are independent, so apply(all) == concat(apply(halves)) BIT-exactly
    (deterministic kernels; this is also what data-parallel sharding relies on),
  * the reported losses recomputed from the rendered colours (train_boxpose.py:123-131),
  * a checksum of the weight-gradient path: db of the rgb head == column sums of bf16(d raw),
  * determinism of a whole training step (no atomics anywhere)."""
import pytest
import torch

from durf_amd import obbpose_model, ops, synthetic, train_boxpose, utils
from tests import helpers as H
from tests import layer_grads as LG

pytestmark = pytest.mark.gpu
B, N = 4096, 128


def _setup(cuda, K, randomized):
    utils.clear_gin()
    utils.parse_gin('MipNerfModel.num_samples = %d\nMipNerfModel.density_noise = 0.0\n'
                    'MipNerfModel.no_pose_opt = True\nMipNerfModel.no_yaw_opt = True\n'
                    'Config.randomized = %s\nConfig.rand_bkgd = False\nConfig.grad_max_norm = 1.0\n'
                    'Config.grad_max_val = 0.1\nConfig.tv_loss_mult = 0.0\n' % (N, randomized))
    config = utils.configured(utils.Config)
    b = synthetic.make_batch(B, K, seed=77 + K, far=40.0)
    db = H.device_batch(b, cuda)
    model, variables = obbpose_model.construct_mipnerf(3, db, device=cuda)
    return config, b, db, model, variables


def _slice(db, sl):
    out = dict(db)
    out['rays'] = utils.namedtuple_map(lambda r: r[sl].contiguous(), db['rays'])
    for k in ('pixels', 'depth', 'sky'):
        out[k] = db[k][sl].contiguous()
    return out


@pytest.mark.parametrize('K', [1, 3])
def test_rendering_invariants_and_chunk_invariance(cuda, K):
    config, b, db, model, variables = _setup(cuda, K, False)
    run = lambda d: model.apply(variables, 0, d['rays'], d['init'], d['ext'], b['ts'], randomized=False,
                                rand_bkgd=False, white_bkgd=False, alpha=10.0)
    full = run(db)
    again = run(db)
    lo, hi = run(_slice(db, slice(0, B // 2))), run(_slice(db, slice(B // 2, B)))
    for lvl in range(2):
        rgb, depth, acc, w, t_vals, t_mids, t_dists = full[lvl][:7]
        assert torch.isfinite(rgb).all() and torch.isfinite(w).all()
        assert float(w.min()) >= 0.0 and float(acc.max()) <= 1.0 + 1e-5
        torch.testing.assert_close(acc, w.sum(-1), rtol=1e-5, atol=1e-6)                      # mip.py:318
        torch.testing.assert_close(depth, (w * t_mids).sum(-1), rtol=1e-4, atol=1e-4)         # :319
        assert bool((t_vals[:, 1:] >= t_vals[:, :-1]).all())                                   # sorted samples
        assert float(t_vals.min()) >= 0.0 and float(t_vals.max()) <= 40.0 + 1e-3
        torch.testing.assert_close(t_dists, t_vals[:, 1:] - t_vals[:, :-1], rtol=0, atol=0)
        for i in (0, 1, 2, 3, 4):
            assert torch.equal(full[lvl][i], again[lvl][i]), 'run-to-run determinism, output %d' % i
            assert torch.equal(full[lvl][i], torch.cat([lo[lvl][i], hi[lvl][i]])), 'chunk invariance, output %d' % i


def test_train_step_full_size_properties(cuda):
    config, b, db, model, variables = _setup(cuda, 1, True)
    g = torch.Generator().manual_seed(8)
    noise = dict(t_rand=torch.rand(B, N + 1, generator=g).to(cuda), u_rand=torch.rand(B, N + 1, generator=g).to(cuda))
    prev = db['init'][0:1]
    flat0 = variables.flat.clone()
    grad, raw, _ = train_boxpose.loss_and_grad(model, config, 0, variables, db, 3.0, 10.0, prev, noise=noise)
    grad2, _, _ = train_boxpose.loss_and_grad(model, config, 0, variables, db, 3.0, 10.0, prev, noise=noise)
    assert torch.equal(grad, grad2), 'gradients are deterministic (fixed-order split-K sums, no atomics)'
    assert torch.isfinite(grad).all() and float(grad.norm()) > 0
    state = train_boxpose.create_train_state(variables)
    state, stats, _, _ = train_boxpose.train_step(model, config, 0, state, db, 5e-4, 3.0, 10.0, prev, noise=noise)
    # reported rgb losses == mean squared error of the rendered colours (lossmult == 1), train_boxpose.py:123-131
    ret = raw['ret']
    for lvl in range(2):
        mse = ((ret[lvl][0] - db["pixels"]) ** 2).sum() / B      # mask.sum() = B rays, not 3B elements (:124-127)
        torch.testing.assert_close(stats.losses[lvl], mse, rtol=1e-4, atol=1e-7)
    torch.testing.assert_close(stats.psnr, -10.0 / torch.log(torch.tensor(10.0)) * torch.log(stats.losses[-1].cpu()).to(cuda),
                               rtol=1e-5, atol=1e-5)
    # first Adam step: every touched weight moves by ~lr, none by more (train_boxpose.py:288, bias-corrected Adam)
    step = (state.variables.flat - flat0).abs()
    assert float(step.max()) <= 5e-4 * 1.001 and float(step.max()) > 4e-4


def test_weight_gradient_checksum_full_size(cuda):
    """db of the rgb head is the column sum of the bf16-rounded output gradient: a checksum of the whole
    dz_out -> k_dw_all -> k_dw_finalize path at 524 288 samples x 2 levels."""
    rows, W, IN = B * N, 256, 60
    torch.manual_seed(0)
    flat = (torch.rand(ops.mlp_param_count(W, IN), device=cuda) - 0.5) * 0.2
    wf, wb = ops.pack_weights(W, IN, flat, want_bwd=True)
    enc = (torch.randn(rows * 64, device=cuda) * 0.5).to(torch.bfloat16)
    view = (torch.randn(B * 32, device=cuda) * 0.5).to(torch.bfloat16)
    stash = torch.empty(ops.mlp_stash_bytes(W, rows), dtype=torch.uint8, device=cuda)
    mask = torch.empty(ops.mlp_mask_bytes(rows), dtype=torch.uint8, device=cuda)
    ops.mlp_fwd(W, rows, N, enc, view, wf, stash=stash, relu_mask=mask)
    draws = [torch.randn(rows, 4, device=cuda) * 1e-2 for _ in range(2)]
    dzs = [ops.mlp_bwd(W, rows, N, d, wb, mask) for d in draws]
    view_tile = ops.expand_view(rows, N, view)
    part, bpart = ops.dw_buffers(W, cuda)
    ops.mlp_dw(W, rows, N, [enc] * 2, [view_tile] * 2, [stash] * 2, [d[0] for d in dzs], [d[1] for d in dzs], part, bpart)
    grad = torch.zeros_like(flat)
    ops.mlp_dw_finalize(W, IN, rows, N, 2, part, bpart, grad, flat)
    off_b11 = ops.mlp_layer_offset(W, IN, 11, True)
    off_b8 = ops.mlp_layer_offset(W, IN, 8, True)
    want = sum(d.to(torch.bfloat16).double().sum(0) for d in draws)
    torch.testing.assert_close(grad[off_b11:off_b11 + 3].double(), want[:3], rtol=1e-4, atol=1e-4)     # rgb head bias
    torch.testing.assert_close(grad[off_b8:off_b8 + 1].double(), want[3:4], rtol=1e-4, atol=1e-4)       # density head bias


LAYERS = [(60, 256), (256, 256), (256, 256), (256, 256), (256, 256), (316, 256), (256, 256), (256, 256), (256, 1), (256, 256),
          (283, 128), (128, 3)]                       # flax Dense_l (fan_in, fan_out) of the 8x256 MLP (obbpose_model.py:305-354)


@pytest.mark.parametrize('rays,plan', [(4096, 'DW256_512WG'), (512, 'DW256_256WG')])
def test_weight_gradients_of_both_split_plans_against_untiled_matmuls(cuda, rays, plan):
    """Every Dense kernel / bias gradient of the background MLP from k_dw_all + k_dw_finalize + k_bottleneck_grads against
    float64 X^T dZ products of the UNTILED operands the launch read (train_boxpose.py:251-252: jax.grad of the Dense
    layers), under BOTH split plans of the weight-gradient launch: two rounds of 256 workgroups at the metric's 4096 rays x 128
    samples x 2 levels (what bench.py times) and one round below 3072 x 256 rows.  The operands are the kernels' own stash /
    dz buffers, so the comparison isolates the split-K GEMMs: 1e-5 for the direct products (fp32 partial sums; measured
    3e-7..1.3e-6), 5e-3 where the linear bottleneck's gradients are derived through its weights (measured 1.8e-3).  A
    transposed or shifted split offset is an O(1) error in the layers it touches."""
    rows, W, IN, KW = rays * N, 256, 60, 16
    torch.manual_seed(0)
    flat = (torch.rand(ops.mlp_param_count(W, IN), device=cuda) - 0.5) * 0.2
    wf, wb = ops.pack_weights(W, IN, flat, want_bwd=True)
    enc = (torch.randn(rows * 64, device=cuda) * 0.5).to(torch.bfloat16)
    view = (torch.randn(rays * 32, device=cuda) * 0.5).to(torch.bfloat16)
    stash = torch.empty(ops.mlp_stash_bytes(W, rows), dtype=torch.uint8, device=cuda)
    mask = torch.empty(ops.mlp_mask_bytes(rows), dtype=torch.uint8, device=cuda)
    ops.mlp_fwd(W, rows, N, enc, view, wf, stash=stash, relu_mask=mask)
    draws = [torch.randn(rows, 4, device=cuda) * 1e-2 for _ in range(2)]
    dzs = [ops.mlp_bwd(W, rows, N, d, wb, mask) for d in draws]
    view_tile = ops.expand_view(rows, N, view)
    part, bpart = ops.dw_buffers(W, cuda)
    ops.dispatch_reset()
    ops.mlp_dw(W, rows, N, [enc] * 2, [view_tile] * 2, [stash] * 2, [d[0] for d in dzs], [d[1] for d in dzs], part, bpart)
    assert plan in ops.dispatch_seen(), ops.dispatch_seen()
    grad = torch.zeros_like(flat)
    ops.mlp_dw_finalize(W, IN, rows, N, 2, part, bpart, grad, flat)

    def untile(t, nks, off_ks, perm):        # region at k-step offset off_ks of a [regions][rows / 32][nks][2][32][8] bf16 buffer
        nt = rows // 32
        v = t.view(torch.bfloat16).reshape(-1)[off_ks * nt * 512:(off_ks + nks) * nt * 512].reshape(nt, nks, 2, 32, 8)
        x = v.permute(0, 3, 1, 2, 4).reshape(rows, nks * 16).double()
        return x[:, H.cperm_cols(nks).to(x.device)] if perm else x

    def par(layer):
        fi, fo = LAYERS[layer]
        o, ob = ops.mlp_layer_offset(W, IN, layer, False), ops.mlp_layer_offset(W, IN, layer, True)
        return o, ob, fi, fo
    enc60, view27 = untile(enc, 4, 0, False)[:, :60], untile(view_tile, 2, 0, False)[:, :27]
    h = [untile(stash, KW, j * KW, True) for j in range(8)]
    hv = untile(stash, 8, 9 * KW, True)                                   # the view layer's output (region 9; 8 = the bottleneck, not stashed)
    o9, ob9, _, _ = par(9)
    K9, b9 = flat[o9:o9 + 256 * 256].reshape(256, 256).double(), flat[ob9:ob9 + 256].double()
    K10 = flat[par(10)[0]:par(10)[0] + 283 * 128].reshape(283, 128).double()
    bneck = h[7] @ K9 + b9
    X = {0: enc60, 5: torch.cat([h[4], enc60], 1), 8: h[7], 9: h[7], 10: torch.cat([bneck, view27], 1), 11: hv}
    for layer in (1, 2, 3, 4, 6, 7):
        X[layer] = h[layer - 1]
    want = {layer: [0.0, 0.0] for layer in range(12)}
    for dz, dzo in dzs:
        dZ = {j: untile(dz, KW, j * KW, True) for j in range(8)}
        dZ[10] = untile(dz, 8, 9 * KW, True)
        head = untile(dzo, 1, 0, False)
        dZ[8], dZ[11] = head[:, 3:4], head[:, :3]
        dZ[9] = dZ[10] @ K10[:256].T                                      # through the view layer's bottleneck rows
        for layer in range(12):
            want[layer][0] = want[layer][0] + X[layer].T @ dZ[layer]
            want[layer][1] = want[layer][1] + dZ[layer].sum(0)
    rel = lambda a, b: float((a - b).norm() / b.norm())
    for layer in range(12):
        o, ob, fi, fo = par(layer)
        gk, gb = grad[o:o + fi * fo].reshape(fi, fo).double(), grad[ob:ob + fo].double()
        tol = 5e-3 if layer in (9, 10) else 1e-5
        assert rel(gk, want[layer][0]) < tol, 'dK Dense_%d: rel %.3g' % (layer, rel(gk, want[layer][0]))
        assert rel(gb, want[layer][1]) < (5e-3 if layer == 9 else 1e-5), 'db Dense_%d: rel %.3g' % (layer, rel(gb, want[layer][1]))
    assert rel(grad[par(10)[0]:par(10)[0] + 283 * 128].reshape(283, 128)[256:].double(), want[10][0][256:]) < 1e-5   # its view rows: direct


@pytest.mark.parametrize('Bs,K', [(1, 1), (33, 2), (1000, 16)])
def test_odd_batch_sizes_and_max_objects(cuda, Bs, K):
    """Edge shapes: a single ray, a batch that fills neither a 256-sample block nor a compaction round, and the
    maximum object count (DURF_MAX_OBJ = 16): a full training step runs, stays finite and matches the oracle's loss."""
    from oracle import durf_ref as R
    Ns = 32
    utils.clear_gin()
    utils.parse_gin('MipNerfModel.num_samples = %d\nMipNerfModel.density_noise = 0.0\n'
                    'MipNerfModel.no_pose_opt = True\nMipNerfModel.no_yaw_opt = True\n'
                    'Config.randomized = False\nConfig.rand_bkgd = False\nConfig.grad_max_norm = 1.0\n'
                    'Config.grad_max_val = 0.1\nConfig.tv_loss_mult = 0.0\n' % Ns)
    config = utils.configured(utils.Config)
    b = synthetic.make_batch(Bs, K, seed=5 + K, far=40.0)
    ob, db = H.oracle_batch(b), H.device_batch(b, cuda)
    model, variables = obbpose_model.construct_mipnerf(2, db, device=cuda)
    params = H.oracle_params_from_variables(variables)
    state = train_boxpose.create_train_state(variables)
    state, stats, _, _ = train_boxpose.train_step(model, config, 0, state, db, 5e-4, 3.0, 10.0, db['init'][0:1])
    torch.cuda.synchronize()
    assert torch.isfinite(state.variables.flat).all() and torch.isfinite(stats.loss)
    ocfg = dict(R.CONFIG_DEFAULTS, randomized=False, tv_loss_mult=0.0)
    _, _, ostats, _ = R.train_step(params, R.new_opt_state(params), ob, ocfg, dict(num_samples=Ns), 5e-4, 3.0, 10.0,
                                   ob['init'][0:1], mlp_hook=R.mlp_apply_bf16)
    torch.testing.assert_close(stats.loss.cpu(), ostats['loss'], rtol=3e-3, atol=1e-6)


def _setup_cfg(cuda, K, Bs, pose_opt, precision, noise_boxes=0.0):
    utils.clear_gin()
    utils.parse_gin('MipNerfModel.num_samples = %d\nMipNerfModel.density_noise = 0.0\n'
                    'MipNerfModel.no_pose_opt = %s\nMipNerfModel.no_yaw_opt = %s\nMipNerfModel.mlp_precision = %r\n'
                    'Config.randomized = True\nConfig.rand_bkgd = False\nConfig.grad_max_norm = 1.0\n'
                    'Config.grad_max_val = 0.1\nConfig.tv_loss_mult = 0.0\n' % (N, not pose_opt, not pose_opt, precision))
    config = utils.configured(utils.Config)
    b = synthetic.make_batch(Bs, K, seed=90 + K, far=40.0, noise_boxes=noise_boxes, redraw_noisy_multi_hit=True)
    db = H.device_batch(b, cuda)
    model, variables = obbpose_model.construct_mipnerf(3, db, device=cuda)
    # bf16-representable MLP weights, so both precisions evaluate the SAME function and what is compared is the
    # arithmetic (activation / gradient rounding), not the effect of rounding the weights (a different network, whose
    # pose gradient -- a sum over rays with heavy cancellation at initialisation -- differs by tens of per cent)
    lay = variables.layout
    w = variables.flat[lay.box[1]:]
    w.copy_(w.to(torch.bfloat16).float())
    return config, b, db, model, variables


def _rel(a, b):
    return float((a - b).norm() / (b.norm() + 1e-30))


@pytest.mark.parametrize('K,pose_opt,alpha', [(8, False, 10.0), (3, True, 3.3)])
def test_per_rank_shapes_of_cfg5_and_cfg4_at_128_samples(cuda, K, pose_opt, alpha):
    """cfg5 (K = 8) and cfg4 (BARF pose optimisation, alpha ramp, box noise 0.5) at their per-rank shape
    (1024 rays x 128 samples x 2 levels): the bf16 production step against the exact-fp32 instrument on the same
    batch, parameters and sampling noise.  The instrument itself is pinned against the oracle at sizes the oracle
    can run (tests/test_gpu_f32_exact.py), so this carries oracle parity to the full sample count: rendered colours
    2e-2 (SURVEY.md 8c BF16 mode), loss terms 2e-3 rel, MLP gradients 5e-2 norm-wise, pose gradients 5e-2 norm-wise
    (see below), plus determinism of the whole gradient."""
    Bs = 1024
    g = torch.Generator().manual_seed(12)
    noise = dict(t_rand=torch.rand(Bs, N + 1, generator=g).to(cuda), u_rand=torch.rand(Bs, N + 1, generator=g).to(cuda))
    out = {}
    for prec in ('bf16', 'f32'):
        config, b, db, model, variables = _setup_cfg(cuda, K, Bs, pose_opt, prec, noise_boxes=0.5 if pose_opt else 0.0)
        prev = db['init'][0:1]
        grad, raw, _ = train_boxpose.loss_and_grad(model, config, 0, variables, db, 3.0, alpha, prev, noise=noise)
        stats = train_boxpose._assemble_stats(config, db, raw, prev, ops.STATS_ASSEMBLE | ops.STATS_PSNR)
        out[prec] = dict(grad=grad.clone(), rgb=[r[0].clone() for r in raw['ret']], stats=stats.clone(),
                         lay=variables.layout, ts=b['ts'])
        if prec == 'bf16':
            grad2, _, _ = train_boxpose.loss_and_grad(model, config, 0, variables, db, 3.0, alpha, prev, noise=noise)
            # (no float atomic is left anywhere in csrc/: the pose sums are fixed-order block reductions too)
            assert torch.equal(grad, grad2), 'deterministic gradients, with and without box-pose optimisation'
    a, f = out['bf16'], out['f32']
    assert torch.isfinite(a['grad']).all() and torch.isfinite(f['grad']).all()
    for lvl in range(2):
        assert float((a['rgb'][lvl] - f['rgb'][lvl]).abs().max()) < 2e-2
    L = 2
    st_a, st_f = ops.stats_views(a['stats'], L), ops.stats_views(f['stats'], L)
    for k in ('losses', 'd_losses', 'n_losses', 'e_losses', 's_losses', 'distr_losses'):
        torch.testing.assert_close(st_a[k], st_f[k], rtol=2e-3, atol=1e-6, msg=lambda m: k + ': ' + m)
    lay = a['lay']
    for name in lay.mlp_names():
        w, _ = lay.mlp_dims(name)
        sl = slice(lay.mlp_off[name], lay.mlp_off[name] + lay.mlp_size[w])
        if float(f['grad'][sl].norm()) > 0:
            r = _rel(a['grad'][sl], f['grad'][sl])
            assert r < 5e-2, '%s: bf16 vs exact-fp32 gradient rel err %g' % (name, r)
    # per piece, bf16 against the exact-fp32 instrument (no oracle here, so no structural zeros: exact zeros of the
    # instrument have to be exact zeros of the production path all the same).  MLP_0 at the bf16-vs-fp32 gates (measured
    # 6.9e-2 / 7.1e-2).  The object MLPs of cfg5 (K = 8 on 1,024 rays, measured 0.26 on BoxMLP_1's Dense_0 bias, 0.24 Dense_1,
    # 0.20-0.22 kernels, falling with depth to < 1e-2 at the head) sit above that ceiling, and that is bf16 rounding itself:
    # on this batch (make_batch(1024, 8, seed=98, far=40), N = 128, bf16-representable glorot weights, this test's sampling
    # noise) the CPU oracle with bf16-rounded GEMM operands (R.mlp_apply_bf16) is as far from the plain fp32 oracle --
    # BoxMLP_1 Dense_0 bias 0.263, Dense_1 bias 0.248, Dense_0 / Dense_1 kernels 0.219 / 0.201, MLP_0 at most 0.069 (~70 s on
    # the CPU, too slow for the suite).  Held at 0.75: a zeroed (1.0) or sign-flipped (2.0) piece still fails.
    gates = dict(LG.GATES['bf16_vs_f32'], **({} if pose_opt else {'BoxMLP.kernel': 0.75, 'BoxMLP.bias': 0.75}))
    pcs = LG.pieces_for(lay, a['ts'])
    print(LG.compare(a['grad'], f['grad'], pcs, gates, title='per-rank shape K=%d pose_opt=%s' % (K, pose_opt)))
    if pose_opt:
        # The pose gradient is a sum over ~100 hit rays x 128 samples that cancels to ~1 % of its summed magnitudes, so
        # bf16 rounding anywhere on the hit rays used to leave 3-38 % on it (round 2; tools/pose_grad_ablate.py shows the
        # object MLPs and the background MLP's evaluation of the hit rays each carry about half).  With pose optimisation
        # on the production path now evaluates the box-hit rays in fp32 (MipNerfModel.object_precision), and its pose
        # gradient must agree with the exact-fp32 instrument's NORM-WISE (measured: ~1e-6; the gate is the 5e-2 the MLP
        # gradients are held to).
        ga = a['grad'][lay.box[0]:lay.box[1]].view(lay.T, K, 6)[a['ts']]
        gf = f['grad'][lay.box[0]:lay.box[1]].view(lay.T, K, 6)[a['ts']]
        assert float(gf.abs().max()) > 0
        for sl, nm in ((slice(0, 3), 'position'), (slice(3, 6), 'rotation')):
            x, y = ga[:, sl].reshape(-1), gf[:, sl].reshape(-1)
            assert _rel(x, y) < 5e-2, 'pose gradient (%s), production precision vs exact fp32: rel err %g' % (nm, _rel(x, y))


def test_loss_terms_at_the_metric_shape_against_the_oracle(cuda):
    """The benchmarked shape itself -- 4096 rays x 128 samples x 2 levels, K = 3, Waymo loss terms -- straight against the
    oracle (plain fp32 restatement on the CPU, ~1 minute), not by induction from the small cases: every logged loss term of
    one training step.  The bf16 MLPs against fp32: 5e-3 relative (measured 1e-4 .. 1e-3); the fp32 stages around them would
    hold 2e-5 on their own.  (Gradients at this size stay with the property tests above: the autograd graph of 1 M samples
    does not fit a test.)"""
    from oracle import durf_ref as R
    B, K, N = 4096, 3, 128
    utils.clear_gin()
    utils.parse_gin('MipNerfModel.num_samples = %d\nMipNerfModel.density_noise = 0.0\nMipNerfModel.no_pose_opt = True\n'
                    'MipNerfModel.no_yaw_opt = True\nConfig.randomized = False\nConfig.rand_bkgd = False\nConfig.grad_max_norm = 1.0\n'
                    'Config.grad_max_val = 0.1\nConfig.tv_loss_mult = 0.0\n' % N)
    config = utils.configured(utils.Config)
    b = synthetic.make_batch(B, K, seed=77)
    ob, db = H.oracle_batch(b), H.device_batch(b, cuda)
    model, variables = obbpose_model.construct_mipnerf(1, db, device=cuda)
    params = H.oracle_params_from_variables(variables)
    state = train_boxpose.create_train_state(variables)
    _, stats, _, _ = train_boxpose.train_step(model, config, 0, state, db, 5e-4, 3.0, 10.0, db['init'][0:1])
    torch.cuda.synchronize()
    ocfg = dict(R.CONFIG_DEFAULTS, randomized=False, tv_loss_mult=0.0)
    with torch.no_grad():
        loss, S, ret = R.loss_fn(params, ob, ocfg, dict(num_samples=N), 3.0, 10.0, ob['init'][0:1])
    assert torch.isfinite(loss), 'the synthetic batch has a multi-hit ray: pick another seed'
    torch.testing.assert_close(stats.loss.cpu(), loss, rtol=5e-3, atol=0)
    for k in ('losses', 'd_losses', 'n_losses', 'e_losses', 's_losses', 'distr_losses'):
        torch.testing.assert_close(getattr(stats, k).cpu(), S[k], rtol=5e-3, atol=1e-7, msg=lambda m: k + ': ' + m)
    assert int((ret[0][8] > 0).sum()) > 100, 'box-hit rays take part'


@pytest.mark.parametrize('B,K,pose_opt,alpha', [(512, 3, False, 10.0), (512, 3, True, 3.3), (128, 8, False, 10.0)])
def test_gradients_at_the_reference_batch_and_128_samples_against_the_oracle(cuda, B, K, pose_opt, alpha):
    """The reference's own batch (configs/waymo.gin:17: 512 rays) at the metric's 128 samples per ray x 2 levels, K = 3, Waymo
    loss terms, stratified sampling: the HIP training step's GRADIENT straight against the autograd of the plain fp32
    restatement on the CPU (no bf16 emulation on the oracle's side, ~30 s), in both precisions of the product: the exact-fp32
    kernels 2e-3 norm-wise per MLP, the bf16 production path 5e-2; with box-pose optimisation on (cfg4: alpha 3.3, box noise
    0.5, TV prior) the pose gradient per object, position and rotation, 5e-2 in both (the box-hit rays run in fp32).  The MLP
    weights are bf16-representable, so both precisions and the oracle evaluate the same network (as in the test above).  This
    is the largest shape the oracle's autograd graph fits in a test; the 1024- and 4096-ray shapes are tied to it through the
    exact-fp32 instrument (test_per_rank_shapes_of_cfg5_and_cfg4) and the loss terms
    (test_loss_terms_at_the_metric_shape_against_the_oracle).  The third case is cfg5's object count at 128 samples: K = 8 on
    128 rays, half of them box-hit rays so that most object MLPs see samples (K = 8 met the oracle at N = 32 only)."""
    from oracle import durf_ref as R
    tv = 1e-2 if pose_opt else 0.0
    b = synthetic.make_batch(B, K, seed=205, far=40.0, noise_boxes=0.5 if pose_opt else 0.0, redraw_noisy_multi_hit=True,
                             **(dict(hit_range=(0.4, 0.6)) if K == 8 else {}))
    ob, db = H.oracle_batch(b), H.device_batch(b, cuda)
    g = torch.Generator().manual_seed(21)
    noise_c = dict(t_rand=torch.rand(B, N + 1, generator=g), u_rand=torch.rand(B, N + 1, generator=g))
    noise_d = {k: v.to(cuda) for k, v in noise_c.items()}
    prev_c, prev_d = ob['init'][0:1] + 0.01, db['init'][0:1] + 0.01
    flat0, grads = None, {}
    for prec in ('f32', 'bf16'):
        utils.clear_gin()
        utils.parse_gin('MipNerfModel.num_samples = %d\nMipNerfModel.density_noise = 0.0\nMipNerfModel.no_pose_opt = %s\n'
                        'MipNerfModel.no_yaw_opt = %s\nMipNerfModel.mlp_precision = %r\nConfig.randomized = True\n'
                        'Config.rand_bkgd = False\nConfig.grad_max_norm = 1.0\nConfig.grad_max_val = 0.1\n'
                        'Config.tv_loss_mult = %g\n' % (N, not pose_opt, not pose_opt, prec, tv))
        config = utils.configured(utils.Config)
        model, variables = obbpose_model.construct_mipnerf(9, db, device=cuda)
        lay = variables.layout
        if flat0 is None:
            for name in lay.mlp_names():
                for i in range(12):
                    bias = variables['params'][name]['Dense_%d' % i]['bias']
                    bias.copy_(((torch.rand(bias.shape, generator=g) - 0.5) * 0.1).to(cuda))
            w = variables.flat[lay.box[1]:]
            w.copy_(w.to(torch.bfloat16).float())
            flat0 = variables.flat.clone()
            params = H.oracle_params_from_variables(variables)
        else:
            variables.flat.copy_(flat0)
        grad, raw, _ = train_boxpose.loss_and_grad(model, config, 0, variables, db, 3.0, alpha, prev_d, noise=noise_d)
        torch.cuda.synchronize()
        grads[prec] = grad.cpu()
    ocfg = dict(R.CONFIG_DEFAULTS, randomized=True, tv_loss_mult=tv)
    mcfg = dict(num_samples=N, density_noise=0.0, no_pose_opt=not pose_opt, no_yaw_opt=not pose_opt)
    leaves = [z.detach().clone().requires_grad_(True) for z in R.params_leaves(params)]
    loss, S, _ = R.loss_fn(R.set_leaves(params, leaves), ob, ocfg, mcfg, 3.0, alpha, prev_c, noise=noise_c)
    assert torch.isfinite(loss), 'the batch must not contain rays that hit two boxes'
    og = torch.autograd.grad(loss, leaves, allow_unused=True)
    og = torch.cat([(torch.zeros_like(z) if gr is None else gr).reshape(-1) for gr, z in zip(og, leaves)])
    ts = b['ts']
    want = og[lay.box[0]:lay.box[1]].view(lay.T, K, 6)
    for prec, tol in (('f32', 2e-3), ('bf16', 5e-2)):
        grad, report = grads[prec], []
        assert og.numel() == grad.numel()
        for name in lay.mlp_names():
            w, _ = lay.mlp_dims(name)
            sl = slice(lay.mlp_off[name], lay.mlp_off[name] + lay.mlp_size[w])
            if float(og[sl].norm()) > 0:
                r = _rel(grad[sl], og[sl])
                report.append('%s %.2e' % (name, r))
                assert r < tol, '%s (%s): gradient rel err %g' % (name, prec, r)
        # per piece: the exact-fp32 kernels at the 'f32' gates, the bf16 path at the bf16-vs-fp32 ones -- its object MLPs at
        # the 'f32' gates under pose optimisation, where the box-hit rays run in fp32 (the box-pose rows are held above)
        pcs = LG.pieces_for(lay, ts)
        gates = LG.GATES['f32'] if prec == 'f32' else LG.mixed_gates('bf16_vs_f32', 'f32' if pose_opt else 'bf16_vs_f32')
        print(LG.compare(grad, og, pcs, gates,
                         LG.structural_zeros(pcs, frozen_pose=not pose_opt, unhit=LG.unhit_objects(ob, ts)),
                         title='reference batch B=%d K=%d pose_opt=%s %s' % (B, K, pose_opt, prec)))
        got = grad[lay.box[0]:lay.box[1]].view(lay.T, K, 6)
        if pose_opt:
            assert float(want[ts].abs().max()) > 0
            for k in range(K):
                if float(want[ts, k].abs().max()) == 0.0:
                    continue
                rp, rr = _rel(got[ts, k, :3], want[ts, k, :3]), _rel(got[ts, k, 3:], want[ts, k, 3:])
                report.append('pose %d %.2e / %.2e' % (k, rp, rr))
                assert rp < 5e-2 and rr < 5e-2, 'object %d (%s): position rel err %g, rotation rel err %g' % (k, prec, rp, rr)
        else:
            assert float(got.abs().max()) == 0.0 and float(want.abs().max()) == 0.0
        assert len(report) >= 1 + K // 2, 'most object MLPs take part (the synthetic boxes are not all in view): %s' % report
        print('%d rays x 128 samples x 2 levels, K=%d, pose_opt=%s, %s: gradient rel err vs the fp32 oracle: %s'
              % (B, K, pose_opt, prec, ', '.join(report)))
