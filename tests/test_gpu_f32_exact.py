"""Exact-fp32 MLP mode (csrc/mlp_f32.hip, MipNerfModel(mlp_precision='f32')) -- the parity instrument.

The reference computes in fp32 throughout (obbpose_model.py:326-327 Dense dtype, internal/math.py:22-24 HIGHEST
precision).  With the Dense layers on v_mfma_f32_32x32x2_f32 and fp32 encodings, the HIP path must match the fp32
oracle at SURVEY.md 8c's tight tolerances: rgb <= 1e-5 abs, weights <= 1e-5, depth <= 1e-4 * far, loss 1e-5 rel,
gradients <= 1e-3 norm-wise -- an order of magnitude or more below what the bf16 production path is held to, so a
logic error that hides under bf16 noise shows here."""
import pytest
import torch

from durf_amd import obbpose_model, ops, synthetic, train_boxpose, utils
from oracle import durf_ref as R
from tests import helpers as H
from tests import layer_grads as LG

pytestmark = pytest.mark.gpu


def _rel(a, b):
    return float((a - b).norm() / (b.norm() + 1e-30))


def _params(width, in_dim, seed, requires_grad=False):
    g = torch.Generator().manual_seed(seed)
    cfg = R.MLP_BKGD if width == 256 else R.MLP_BOX
    params, flat = [], []
    for fi, fo in R.mlp_layer_shapes(in_dim, 27, cfg):
        lim = (6.0 / (fi + fo)) ** 0.5
        k = ((torch.rand(fi, fo, generator=g) * 2 - 1) * lim).requires_grad_(requires_grad)
        bb = ((torch.rand(fo, generator=g) - 0.5) * 0.2).requires_grad_(requires_grad)
        params.append([k, bb])
        flat += [k.detach().reshape(-1), bb.detach()]
    return cfg, params, torch.cat(flat), g


@pytest.mark.parametrize('width,in_dim', [(256, 60), (128, 63)])
def test_mlp_f32_forward_backward(cuda, width, in_dim):
    """fwd / bwd / dW kernels against fp64 autograd of the oracle MLP: outputs 2e-6 rel, gradients 1e-5 norm-wise
    (fp32 round-off only); the object calling convention (ray_idx, count) with a count below the capacity.  N = 32, so every
    row count here is a whole number of 32-row tiles (19 valid of 21): the partial tiles are tests/test_gpu_f32_edges.py's."""
    N, Bn = 32, 21
    rows = N * Bn
    cfg, params, flat, g = _params(width, in_dim, 5, requires_grad=True)
    x = torch.randn(Bn, N, in_dim, generator=g)
    cond_all = torch.randn(50, 27, generator=g)
    ridx = torch.randperm(50, generator=g)[:Bn]
    cond = cond_all[ridx]
    draw_full = torch.randn(50 * N, 4, generator=g) * 0.1          # [B*N,4] buffer the object rows are gathered from
    cnt = 19                                                        # rays actually valid
    valid = cnt * N
    p64 = [[k.detach().double().requires_grad_(True), bb.detach().double().requires_grad_(True)] for k, bb in params]
    rgb, dens = R.mlp_apply(p64, x.double(), cond.double(), cfg)
    out = torch.cat([rgb.reshape(rows, 3), dens.reshape(rows, 1)], -1)
    draw_rows = draw_full.reshape(50, N, 4)[ridx].reshape(rows, 4)
    x64 = x.double().requires_grad_(True)
    rgb2, dens2 = R.mlp_apply(p64, x64, cond.double(), cfg)
    out2 = torch.cat([rgb2.reshape(rows, 3), dens2.reshape(rows, 1)], -1)
    (out2[:valid] * draw_rows[:valid].double()).sum().backward()
    d = lambda t: t.to(cuda).contiguous()
    count = torch.tensor([cnt], dtype=torch.int32, device=cuda)
    raw, act = ops.mlp_fwd_f32(width, in_dim, rows, N, d(x.reshape(rows, in_dim)), d(cond_all), d(flat),
                               ray_idx=d(ridx.int()), count=count, want_act=True)
    assert (raw[valid:] == 0).all(), 'rows beyond count are not written'
    torch.testing.assert_close(raw[:valid].cpu().double(), out[:valid].detach(), rtol=2e-6, atol=2e-6)
    dz, d_enc = ops.mlp_bwd_f32(width, in_dim, rows, N, d(draw_full), d(flat), act, ray_idx=d(ridx.int()), count=count,
                                want_d_enc=True)
    assert _rel(d_enc[:valid, :in_dim].cpu().double(), x64.grad.reshape(rows, in_dim)[:valid]) < 1e-5
    assert (d_enc[:, in_dim:] == 0).all()
    grad = torch.zeros_like(flat, device=cuda)
    ops.mlp_dw_f32(width, in_dim, rows, N, act, dz, grad, count=count, nsplit=7)
    grad = grad.cpu().double()
    off = 0
    for li, (k, bb) in enumerate(p64):
        gk = grad[off:off + k.numel()].reshape(k.shape); off += k.numel()
        gb = grad[off:off + bb.numel()]; off += bb.numel()
        assert _rel(gk, k.grad) < 1e-5, 'dW Dense_%d rel err %g' % (li, _rel(gk, k.grad))
        assert _rel(gb, bb.grad) < 1e-5, 'db Dense_%d rel err %g' % (li, _rel(gb, bb.grad))
    # deterministic: a second evaluation with another split count agrees to fp32 round-off, the same split bitwise
    g2, g3 = torch.zeros_like(flat, device=cuda), torch.zeros_like(flat, device=cuda)
    ops.mlp_dw_f32(width, in_dim, rows, N, act, dz, g2, count=count, nsplit=7)
    ops.mlp_dw_f32(width, in_dim, rows, N, act, dz, g3, count=count, nsplit=3)
    assert torch.equal(g2.cpu().double(), grad) and _rel(g3.cpu().double(), grad) < 1e-6


def _gin(N, pose_opt=False):
    utils.clear_gin()
    utils.parse_gin('MipNerfModel.num_samples = %d\nMipNerfModel.density_noise = 0.0\n'
                    'MipNerfModel.no_pose_opt = %s\nMipNerfModel.no_yaw_opt = %s\nMipNerfModel.mlp_precision = \'f32\'\n'
                    'Config.randomized = True\nConfig.rand_bkgd = False\nConfig.grad_max_norm = 1.0\n'
                    'Config.grad_max_val = 0.1\nConfig.tv_loss_mult = 0.0\n' % (N, not pose_opt, not pose_opt))
    return utils.configured(utils.Config)


def _setup(cuda, B, K, N, seed, pose_opt=False, noise_boxes=0.0):
    config = _gin(N, pose_opt)
    b = synthetic.make_batch(B, K, seed=seed, noise_boxes=noise_boxes)
    ob, db = H.oracle_batch(b), H.device_batch(b, cuda)
    model, variables = obbpose_model.construct_mipnerf(seed, db, device=cuda)
    assert model.mlp_precision == 'f32'
    g = torch.Generator().manual_seed(seed)
    for name in variables.layout.mlp_names():
        for i in range(12):
            bias = variables['params'][name]['Dense_%d' % i]['bias']
            bias.copy_(((torch.rand(bias.shape, generator=g) - 0.5) * 0.1).to(cuda))
    noise_c = dict(t_rand=torch.rand(B, N + 1, generator=g), u_rand=torch.rand(B, N + 1, generator=g))
    noise_d = {k: v.to(cuda) for k, v in noise_c.items()}
    return config, b, ob, db, model, variables, noise_c, noise_d


@pytest.mark.parametrize('K,N', [(0, 64), (1, 32), (3, 32)])
def test_forward_fp32_exact(cuda, K, N):
    """rendered outputs vs the fp32 oracle at SURVEY.md 8c's F32_EXACT tolerances"""
    far = 40.0
    B = 192
    config, b, ob, db, model, variables, noise_c, noise_d = _setup(cuda, B, K, N, 51 + K)
    ret = model.apply(variables, 0, db['rays'], db['init'], db['ext'], b['ts'], randomized=True, rand_bkgd=False,
                      white_bkgd=False, alpha=10.0, noise=noise_d)
    params = H.oracle_params_from_variables(variables)
    with torch.no_grad():
        ref = R.model_apply(params, ob['rays'], b['ts'], ob['ext'], True, False, False, 10.0, noise=noise_c,
                            cfg=dict(num_samples=N))
    for lvl in range(2):
        got, want = ret[lvl], ref[lvl]
        torch.testing.assert_close(got[0].cpu(), want[0], rtol=0, atol=1e-5, msg=lambda m: 'rgb L%d: %s' % (lvl, m))
        torch.testing.assert_close(got[2].cpu(), want[2], rtol=0, atol=1e-5, msg=lambda m: 'acc L%d: %s' % (lvl, m))
        torch.testing.assert_close(got[3].cpu(), want[3], rtol=0, atol=1e-5, msg=lambda m: 'weights L%d: %s' % (lvl, m))
        torch.testing.assert_close(got[1].cpu(), want[1], rtol=0, atol=1e-4 * far, msg=lambda m: 'depth L%d: %s' % (lvl, m))
        torch.testing.assert_close(got[4].cpu(), want[4], rtol=0, atol=1e-4 * far, msg=lambda m: 't_vals L%d: %s' % (lvl, m))


@pytest.mark.parametrize('K,N,B', [(1, 32, 160), (3, 32, 192)])
def test_train_step_fp32_exact(cuda, K, N, B):
    """loss terms 1e-5 rel, parameter gradients 1e-3 norm-wise (measured ~1e-5), Adam step 1e-3 vs the fp32 oracle"""
    config, b, ob, db, model, variables, noise_c, noise_d = _setup(cuda, B, K, N, 61 + K)
    params = H.oracle_params_from_variables(variables)
    flat0 = variables.flat.clone()
    lr, eps, alpha = 5e-4, 3.0, 10.0
    prev_c, prev_d = ob['init'][0:1], db['init'][0:1]
    grad, raw, pose = train_boxpose.loss_and_grad(model, config, 0, variables, db, eps, alpha, prev_d, noise=noise_d)
    state = train_boxpose.create_train_state(variables)
    new_state, stats, _, _ = train_boxpose.train_step(model, config, 0, state, db, lr, eps, alpha, prev_d, noise=noise_d)
    torch.cuda.synchronize()
    ocfg = dict(R.CONFIG_DEFAULTS, randomized=True, tv_loss_mult=0.0)
    p2, st2, ostats, ograds = R.train_step(params, R.new_opt_state(params), ob, ocfg, dict(num_samples=N), lr, eps, alpha,
                                           prev_c, noise=noise_c)
    assert not (ostats['losses'] != ostats['losses']).any()
    for k in ('losses', 'd_losses', 'n_losses', 'e_losses', 's_losses', 'distr_losses'):
        torch.testing.assert_close(getattr(stats, k).cpu(), ostats[k], rtol=2e-5, atol=1e-7, msg=lambda m: k + ': ' + m)
    torch.testing.assert_close(stats.loss.cpu(), ostats['loss'], rtol=1e-5, atol=1e-7)
    og = torch.cat([x.reshape(-1) for x in ograds])
    lay = variables.layout
    for name in lay.mlp_names():
        w, _ = lay.mlp_dims(name)
        sl = slice(lay.mlp_off[name], lay.mlp_off[name] + lay.mlp_size[w])
        if float(og[sl].norm()) > 0:
            r = _rel(grad.cpu()[sl], og[sl])
            assert r < 1e-3, '%s grad rel err %g' % (name, r)
    pcs = LG.pieces_for(lay, b['ts'])
    print(LG.compare(grad, og, pcs, LG.GATES['f32'], LG.structural_zeros(pcs, unhit=LG.unhit_objects(ob, b['ts'])),
                     title='fp32 exact K=%d N=%d B=%d' % (K, N, B)))
    torch.testing.assert_close(stats.grad_norm.cpu(), ostats['grad_norm'], rtol=1e-3, atol=0)
    # post-Adam parameters: the first step moves every weight by lr * sign(g) (bias-corrected Adam), so the update
    # only differs where a gradient is so close to zero that fp32 summation order decides its sign: <= 5e-2 here
    # (the bf16 path, whose gradients carry 1e-2 noise, is held to 0.15 in tests/test_gpu_train.py)
    newflat = torch.cat([x.reshape(-1) for x in R.params_leaves(p2)])
    step_ref = newflat - flat0.cpu()
    step_got = new_state.variables.flat.cpu() - flat0.cpu()
    assert _rel(step_got, step_ref) < 5e-2, _rel(step_got, step_ref)


def test_box_pose_gradients_fp32_exact(cuda):
    """Box-pose gradients with an fp32 d(loss)/d(encoding): what the bf16 production path's 12-20 % rotation error is
    made of.  In exact-fp32 mode position AND rotation gradients match the fp64 oracle to 2e-3 -- so that error is
    bf16 rounding of d(enc) through cancelling sums, not a logic error in the pose chain."""
    K, N, B, alpha = 2, 32, 256, 4.5
    config, b, ob, db, model, variables, noise_c, noise_d = _setup(cuda, B, K, N, 71, pose_opt=True, noise_boxes=0.3)
    grad, raw, pose = train_boxpose.loss_and_grad(model, config, 0, variables, db, 3.0, alpha, db['init'][0:1], noise=noise_d)
    params64 = H.oracle_params_from_variables(variables, torch.float64)
    ob64 = H.oracle_batch(b, torch.float64)
    ocfg = dict(R.CONFIG_DEFAULTS, randomized=True, tv_loss_mult=0.0)
    n64 = {k: v.double() for k, v in noise_c.items()}
    _, _, ostats, ograds = R.train_step(params64, R.new_opt_state(params64), ob64, ocfg,
                                        dict(num_samples=N, no_pose_opt=False, no_yaw_opt=False), 5e-4, 3.0, alpha,
                                        ob64['init'][0:1], noise=n64)
    lay = variables.layout
    gb = grad[lay.box[0]:lay.box[1]].view(lay.T, K, 6)[b['ts']].cpu().double()
    ob_ = ograds[0][b['ts']]
    assert float(ob_[:, :3].norm()) > 0 and float(ob_[:, 3:].norm()) > 0
    assert _rel(gb[:, :3], ob_[:, :3]) < 2e-3, 'position grad rel err %g' % _rel(gb[:, :3], ob_[:, :3])
    assert _rel(gb[:, 3:], ob_[:, 3:]) < 2e-3, 'rotation grad rel err %g' % _rel(gb[:, 3:], ob_[:, 3:])


def test_object_batch_calls_match_the_single_mlp_calls(cuda):
    """durf_encode_obj_f32_batch / durf_objf32_{fwd,bwd,dw}_batch (all K objects per launch: the production object
    branch when the pose is optimised) are the single-MLP fp32 entry points with the object index in the grid: raw,
    d(enc) and weight gradients BIT-identical per object, ragged hit counts, an object without hits included."""
    K, B, N, alpha = 4, 96, 32, 4.5
    g = torch.Generator().manual_seed(3)
    b = synthetic.make_batch(B, K, seed=17)
    db = H.device_batch(b, cuda)
    rays = db['rays']
    pose = db['init'][b['ts']].contiguous()
    radii = rays.radii.reshape(-1).contiguous()
    o_s, d_s, hit, zo = ops.ray_setup(rays.origins, rays.directions, pose, db['ext'].reshape(-1, 3).contiguous())
    hit[:, 3] = 0                                                      # object 3: no hit ray at all
    idx, count, slot = ops.compact_hits(hit)
    assert int(count.max()) > 0 and int(count[3]) == 0
    t_vals = ops.sample_t(rays.near.reshape(-1).contiguous(), rays.far.reshape(-1).contiguous(), N)
    view27 = ops.view_enc(rays.viewdirs, want_f32=True)[1]
    sz = ops.mlp_param_count(128, 63)
    flat = ((torch.rand(K * sz, generator=g) - 0.5) * 0.2).to(cuda)
    ws = ops.mlp_f32_pack(128, 63, flat, K=K, param_stride=sz)
    draw = (torch.randn(B * N, 4, generator=g) * 0.1).to(cuda)
    slabs = ops.ObjSlabsF32(K, B, N, cuda, True)
    ops.objf32_fwd_batch(slabs, idx, count, t_vals, o_s, d_s, radii, alpha, view27, flat, sz, ws, fused_encode=False)
    # the production call encodes inside the forward (one launch less per level): same raw, same records, bit for bit
    fused = ops.ObjSlabsF32(K, B, N, cuda, True)
    ops.objf32_fwd_batch(fused, idx, count, t_vals, o_s, d_s, radii, alpha, view27, flat, sz, ws)
    for k in range(K):
        c = int(count[k]) * N
        assert torch.equal(fused.raw[k, :c], slabs.raw[k, :c]), 'object %d: fused encode' % k
    astride = fused.act.numel() // K
    for k in range(K):
        nt = (int(count[k]) * N + 31) // 32
        rec = ops._lib.lib().durf_mlp_f32_act_floats(128, 63) * 32
        assert torch.equal(fused.act[k * astride:k * astride + nt * rec], slabs.act[k * astride:k * astride + nt * rec])
    ops.objf32_bwd_batch(slabs, idx, count, draw, flat, sz, ws, want_d_enc=True)
    grad = torch.zeros(K * sz, device=cuda)
    ops.objf32_dw_batch([slabs], count, grad, sz, nsplit=3)
    for k in range(K):
        c = int(count[k]) * N
        ck = count[k:k + 1]
        _, enc_k = ops.encode_obj(B, idx[k], ck, t_vals, o_s, d_s, radii, alpha, tile=False, f32=True)
        assert torch.equal(slabs.enc[k, :c], enc_k[:c])
        pk = flat[k * sz:(k + 1) * sz]
        wsz = ws.numel() // K
        raw_k, act_k = ops.mlp_fwd_f32(128, 63, B * N, N, enc_k, view27, pk, ray_idx=idx[k], count=ck, want_act=True,
                                       wstream=ws[k * wsz:(k + 1) * wsz])
        assert torch.equal(slabs.raw[k, :c], raw_k[:c])
        dz_k, denc_k = ops.mlp_bwd_f32(128, 63, B * N, N, draw, pk, act_k, ray_idx=idx[k], count=ck, want_d_enc=True,
                                       wstream=ws[k * wsz:(k + 1) * wsz])
        assert torch.equal(slabs.d_enc[k, :c], denc_k[:c])
        gk = torch.zeros(sz, device=cuda)
        ops.mlp_dw_f32(128, 63, B * N, N, act_k, dz_k, gk, count=ck, nsplit=3)
        assert torch.equal(grad[k * sz:(k + 1) * sz], gk), 'object %d' % k
    assert float(grad[3 * sz:].abs().max()) == 0.0


def test_constant_encoding_rows(cuda):
    """durf_mlp_fwd_f32 with enc = NULL (the background MLP's one evaluation of a box-hit ray: the encoding of a
    zero-masked Gaussian, [0 x 30, 1 x 30], obbpose_model.py:205-210) == the same call on that encoding spelled out,
    and == the fp64 oracle MLP on it"""
    B, cnt = 77, 41
    cfg, params, flat, g = _params(256, 60, 9)
    view_all = torch.randn(B, 27, generator=g)
    ridx = torch.randperm(B, generator=g)[:B].int()
    count = torch.tensor([cnt], dtype=torch.int32, device=cuda)
    const = torch.cat([torch.zeros(B, 30), torch.ones(B, 30)], 1)
    d = lambda t: t.to(cuda).contiguous()
    a = ops.mlp_fwd_f32(256, 60, B, 1, None, d(view_all), d(flat), ray_idx=d(ridx), count=count)
    bb = ops.mlp_fwd_f32(256, 60, B, 1, d(const), d(view_all), d(flat), ray_idx=d(ridx), count=count)
    assert torch.equal(a, bb) and (a[cnt:] == 0).all()
    p64 = [[k.double(), b_.double()] for k, b_ in params]
    rgb, dens = R.mlp_apply(p64, const[:cnt, None, :].double(), view_all[ridx[:cnt].long()].double(), cfg)
    want = torch.cat([rgb.reshape(cnt, 3), dens.reshape(cnt, 1)], -1)
    torch.testing.assert_close(a[:cnt].cpu().double(), want, rtol=2e-6, atol=2e-6)


def test_background_mlp_on_the_box_hit_rays(cuda):
    """durf_bkgd_hit_rays_f32 (trunk once + view layer per ray) == durf_mlp_fwd_f32(enc = NULL) to fp32 round-off (the
    two sum in different orders) and == the fp64 oracle MLP; rows past count untouched."""
    B, cnt = 203, 57
    cfg, params, flat, g = _params(256, 60, 11)
    view_all = torch.randn(B, 27, generator=g)
    ridx = torch.randperm(B, generator=g).int()
    count = torch.tensor([cnt], dtype=torch.int32, device=cuda)
    d = lambda t: t.to(cuda).contiguous()
    a = ops.mlp_fwd_f32(256, 60, B, 1, None, d(view_all), d(flat), ray_idx=d(ridx), count=count)
    tail = torch.full((B, 4), -1, dtype=torch.int32, device=cuda).view(torch.float32)          # 0xFF bytes: NaN
    got = ops.bkgd_hit_rays_f32(B, d(view_all), d(flat), d(ridx), count, raw_tail=tail)
    assert got.data_ptr() == tail.data_ptr() and bool((got[cnt:].view(torch.int32) == -1).all()), 'rows past count untouched'
    torch.testing.assert_close(got[:cnt], a[:cnt], rtol=2e-6, atol=2e-6)
    const = torch.cat([torch.zeros(cnt, 30), torch.ones(cnt, 30)], 1)
    p64 = [[k.double(), b_.double()] for k, b_ in params]
    rgb, dens = R.mlp_apply(p64, const[:, None, :].double(), view_all[ridx[:cnt].long()].double(), cfg)
    want = torch.cat([rgb.reshape(cnt, 3), dens.reshape(cnt, 1)], -1)
    torch.testing.assert_close(got[:cnt].cpu().double(), want, rtol=2e-6, atol=2e-6)
