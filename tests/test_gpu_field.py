"""The field at world points on the device (include/durf_field.h, csrc/field.hip, durf_amd/field.py) against tests/field_ref.py:
classification, lists, encoding rows, the MLPs and activations with the merge rule, the renderer's own samples, the one-call
walk against the staged calls, grids and columns, scene edits.  Shapes are the smallest that can go wrong: n = 1, 63, 64, 65
(one wave and its edges) and 257 (two workgroups), chunks that split a list between calls, an 8 x 8 x 33 grid.

Bounds come from the reference side: the float32 twin's distances (field_ref.YARDSTICK) times four plus four ulp, the MLP at
the gate tests/test_gpu_f32_edges.py holds durf_mlp_fwd_f32 to (rtol = atol = 2e-6; the forward leaves no row out: the
delicate-row rule of tests/mlp_rows_ref.py is the backward's), the renderer at tests/test_gpu_f32_exact.py's 1e-5."""
import numpy as np
import pytest
import torch

from durf_amd import field, obbpose_model, ops, synthetic, utils
from oracle import durf_ref as R
from tests import field_ref as F
from tests import helpers as H
from tests import lattice_ref

pytestmark = pytest.mark.gpu
I32 = torch.int32
MLP_TOL = 2e-6             # tests/test_gpu_f32_edges.py: raw rtol = atol = 2e-6
RENDER_TOL = 1e-5          # tests/test_gpu_f32_exact.py: rgb and acc of the fp32 model against the oracle
SENTINEL = -7
_S = {}


def _gin(extra=''):
    utils.clear_gin()
    utils.parse_gin('MipNerfModel.num_samples = 32\nMipNerfModel.density_noise = 0.0\nMipNerfModel.no_pose_opt = True\n'
                    'MipNerfModel.no_yaw_opt = True\nMipNerfModel.mlp_precision = \'f32\'\n' + extra)


def _biases(variables, seed, dev):
    g = torch.Generator().manual_seed(seed)
    for name in variables.layout.mlp_names():
        for i in range(12):
            bias = variables['params'][name]['Dense_%d' % i]['bias']
            bias.copy_(((torch.rand(bias.shape, generator=g) - 0.5) * 0.1).to(dev))


def _scene(cuda):
    """the planted K = 3 scene as a model on the device, its float64 parameters, the planted points and one query of them"""
    if 'scene' not in _S:
        _gin()
        pose, ext, en = F.scene()
        model, variables = obbpose_model.construct_mipnerf(7, dict(init=np.tile(pose[None], (2, 1, 1))), device=cuda)
        _biases(variables, 8, cuda)
        pts, tags = F.planted_points()
        g = np.random.default_rng(3)
        vd = g.normal(size=(pts.shape[0], 3))
        vd = (vd / np.linalg.norm(vd, axis=1, keepdims=True)).astype(np.float32)
        _S['scene'] = dict(model=model, variables=variables, params=H.oracle_params_from_variables(variables, torch.float64),
                           pose=pose, ext=ext, en=en, pts=pts, tags=tags, vd=vd, ref=F.classify(pts, pose, ext, en))
    return _S['scene']


def _d(a, cuda, dtype=torch.float32):
    return torch.as_tensor(np.asarray(a)).to(device=cuda, dtype=dtype).contiguous()


def _query(s, cuda, n=None, **kw):
    n = s['pts'].shape[0] if n is None else n
    kw.setdefault('box_enable', s['en'])
    return field.query(s['model'], s['variables'], _d(s['pts'][:n], cuda), _d(s['vd'][:n], cuda), ext=s['ext'], **kw)


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def _same(a, b, keys=('density', 'rgb', 'raw', 'owner', 'valid')):
    for k in keys:
        assert torch.equal(_bits(a[k]), _bits(b[k])), k


# ---- 1. classification --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', F.SIZES)
def test_classification(cuda, n):
    s = _scene(cuda)
    ref = s['ref']
    assert float(ref['margin'][:n].min()) >= F.MARGIN - 1e-6
    owner, local = ops.field_classify(_d(s['pts'][:n], cuda), _d(s['pose'], cuda), _d(s['ext'], cuda), _d(s['en'], cuda, I32), 0.0)
    assert (owner.cpu().numpy() == ref['owner'][:n]).all(), 'owner is exact on every planted point'
    want = ref['local'][:n]
    own = ref['owner'][:n]
    unit = F.ulp32(np.where(own >= 0, ref['dscale'][np.arange(n), np.maximum(own, 0)][:n], 0.0))[:, None]
    bound = np.where((own >= 0)[:, None], 4 * F.YARDSTICK['local'] * unit + 4 * F.ulp32(want), 0.0)
    err = np.abs(local.cpu().numpy().astype(np.float64) - want)
    print('local: worst err / bound %.3f' % float((err / np.maximum(bound, 1e-300))[own >= 0].max() if (own >= 0).any() else 0))
    assert (err <= bound).all()
    # K = 0: every owner is -1 and local is the point
    o0, l0 = ops.field_classify(_d(s['pts'][:n], cuda), None, None)
    assert (o0 == -1).all() and torch.equal(l0.cpu(), torch.tensor(s['pts'][:n]))


# ---- 2. lists -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', F.SIZES + (1025,))
def test_lists_are_a_stable_partition(cuda, n):
    g = np.random.default_rng(n)
    owner = g.integers(-2, 3, n).astype(np.int32)                 # K = 3: owners -2 .. 2
    K = 3
    idx = torch.full((K + 1, n), SENTINEL, dtype=I32, device=cuda)
    count = torch.full((K + 1,), SENTINEL, dtype=I32, device=cuda)
    ops.field_lists(_d(owner, cuda, I32), K, idx, count)
    want = F.lists(owner, K)
    idx, count = idx.cpu().numpy(), count.cpu().numpy()
    for c in range(K + 1):
        assert count[c] == want[c].size
        assert (idx[c, :count[c]] == want[c]).all() and (idx[c, count[c]:] == SENTINEL).all(), c
    owned, oc = ops.field_owned(_d(idx, cuda, I32), _d(count, cuda, I32), K)
    cat = np.concatenate(want[:K])
    assert int(oc) == cat.size and (owned.cpu().numpy()[:cat.size] == cat).all()


# ---- 3. encoding rows ---------------------------------------------------------------------------------------------------------
def _enc_rows(cuda, pts, sigma, contraction, alpha):
    """every point in the background list AND in box 0's list -> (enc_bkgd [m,60], enc_obj [m,63]) beyond a sentinel fill"""
    m = pts.shape[0]
    idx = torch.arange(m, dtype=I32, device=cuda).repeat(2, 1).contiguous()
    count = torch.tensor([m - 1, m], dtype=I32, device=cuda)       # box 0's list one short: its last row keeps the fill
    eb = torch.full((m, 60), float(SENTINEL), device=cuda)
    eo = torch.full((1, m, 63), float(SENTINEL), device=cuda)
    ops.field_encode(_d(pts, cuda), idx, count, 1, sigma, contraction, alpha, eb, eo)
    assert (eo[0, m - 1] == SENTINEL).all(), 'rows at or past count are not written'
    return eb.cpu().double(), eo[0].cpu().double()


@pytest.mark.parametrize('sigma', F.SIGMAS)
def test_encoding_rows(cuda, sigma):
    from tests import enc_rows_ref as E
    pts, labels = F.enc_points()
    m = len(labels)
    worst = {}
    for con in (False, True):
        t = F.encode_bkgd(pts, sigma, con)
        eb, _ = _enc_rows(cuda, pts, sigma, con, 10.0)
        b = F.enc_bound(t, *F.enc_yardstick(labels, con))
        r = ((eb - t['enc']).abs() / b)
        worst['bkgd con=%d' % con] = float(r.max())
        assert bool((r <= 1).all()), ('bkgd', con, [labels[i] for i in torch.nonzero((r > 1).any(1)).reshape(-1).tolist()], float(r.max()))
    for alpha in E.ALPHAS:
        t = F.encode_obj(pts, sigma, alpha)
        _, eo = _enc_rows(cuda, pts, sigma, True, alpha)
        w = R.barf_weights(alpha, 10, torch.float64)[:, None].expand(10, 6).reshape(60)
        b = F.enc_bound(t, *F.enc_yardstick(labels, False), weights=w)
        assert torch.equal(eo[:m - 1, :3], torch.tensor(pts[:m - 1]).double()), 'the coordinates lead the object row'
        r = ((eo[:m - 1, 3:] - t['enc'][:m - 1, 3:]).abs() / b[:m - 1])
        worst['obj alpha=%g' % alpha] = float(r.max())
        assert bool((r <= 1).all()), ('obj', alpha, [labels[i] for i in torch.nonzero((r > 1).any(1)).reshape(-1).tolist()], float(r.max()))
    print('sigma %g: worst err / bound %s' % (sigma, {k: round(v, 3) for k, v in worst.items()}))


# ---- 4. MLP and activations ---------------------------------------------------------------------------------------------------
def _staged(s, cuda, n):
    """the staged calls on the first n planted points -> everything they produce"""
    v = s['variables']
    lay = v.layout
    K = 3
    pts, vd = _d(s['pts'][:n], cuda), _d(s['vd'][:n], cuda)
    owner, local = ops.field_classify(pts, _d(s['pose'], cuda), _d(s['ext'], cuda), _d(s['en'], cuda, I32), 0.0)
    idx, count = ops.field_lists(owner, K)
    owned, ocount = ops.field_owned(idx, count, K)
    eb, eo = ops.field_encode(local, idx, count, K, 0.0, True, 10.0)
    v27 = ops.view_enc(vd, want_f32=True)
    v27 = v27[1] if isinstance(v27, tuple) else v27
    bk = v.mlp_flat('MLP_0')
    raw_b = ops.mlp_fwd_f32(256, 60, n, 1, eb, v27, bk, ray_idx=idx[K].contiguous(), count=count[K:K + 1])
    stride = lay.mlp_size[128]
    o0 = lay.mlp_off['BoxMLP_0']
    raw_o = torch.zeros(K, n, 4, device=cuda)
    for k in range(K):
        ops.mlp_fwd_f32(128, 63, n, 1, eo[k], v27, v.flat[o0 + k * stride:o0 + (k + 1) * stride], ray_idx=idx[k].contiguous(),
                        count=count[k:k + 1], raw=raw_o[k])
    raw_c = ops.bkgd_hit_rays_f32(n, v27, bk, owned, ocount, raw_tail=torch.zeros(n, 4, device=cuda))
    dens, rgb, raw, valid = ops.field_activate(idx, count, raw_b, raw_o, raw_c, owner, s['model'].density_bias)
    return dict(owner=owner, local=local, idx=idx, count=count, owned=owned, ocount=ocount, eb=eb, eo=eo, v27=v27, raw_b=raw_b,
                raw_o=raw_o, raw_c=raw_c, density=dens, rgb=rgb, raw=raw, valid=valid)


def test_mlp_and_activations_with_the_constant_term(cuda):
    s = _scene(cuda)
    n = 257
    st = _staged(s, cuda, n)
    P = s['params']
    own = s['ref']['owner'][:n]
    assert (st['owner'].cpu().numpy() == own).all()
    v27 = F.view_enc(s['vd'][:n])
    lists = F.lists(own, 3)
    want = torch.full((n, 4), float('nan'), dtype=torch.float64)
    nocst = want.clone()
    with torch.no_grad():
        b = lists[3]
        want[b] = F.mlp(P, 'MLP_0', st['eb'][:b.size].cpu().double(), v27[b])
        nocst[b] = want[b]
        zero = F.encode_bkgd(np.zeros((1, 3), np.float32), 0.0, True)['enc']
        for k in range(2):
            o = lists[k]
            assert o.size >= 4
            r = F.mlp(P, 'BoxMLP_%d' % k, st['eo'][k, :o.size].cpu().double(), v27[o])
            nocst[o] = r
            want[o] = r + F.mlp(P, 'MLP_0', zero.expand(o.size, 60), v27[o])
    ok = own != -2
    got = st['raw'].cpu().double()
    gate = lambda ref: ((got[ok] - ref[ok]).abs() <= MLP_TOL + MLP_TOL * ref[ok].abs())
    print('raw: worst |err| / gate %.3f' % float(((got[ok] - want[ok]).abs() / (MLP_TOL + MLP_TOL * want[ok].abs())).max()))
    assert bool(gate(want).all())
    owned = torch.tensor(own >= 0)[ok]
    assert not bool(gate(nocst)[owned].all(1).any()), 'control: without the constant background term no object-owned row passes'
    # activations of the device's own raw: four twin errors plus four ulp
    d64, c64 = F.activations(st['raw'].cpu().numpy()[ok], s['model'].density_bias)
    dr, ca = F.YARDSTICK['act']
    dens, rgb = st['density'].cpu().numpy().astype(np.float64)[ok], st['rgb'].cpu().numpy().astype(np.float64)[ok]
    assert (np.abs(dens - d64) <= 4 * dr * d64 + 4 * F.ulp32(d64)).all()
    assert (np.abs(rgb - c64) <= 4 * ca + 4 * F.ulp32(c64)).all()
    assert (st['valid'].cpu().numpy() == ok).all()
    multi = ~ok
    assert multi.any() and np.isnan(st['density'].cpu().numpy()[multi]).all() and np.isnan(st['raw'].cpu().numpy()[multi]).all()


# ---- 5. against the renderer --------------------------------------------------------------------------------------------------
def test_query_of_the_renderers_samples_composites_to_its_picture(cuda):
    B, K, N = 64, 2, 32
    _gin('MipNerfModel.disable_integration = True\nMipNerfModel.ray_shape = \'cylinder\'\n')
    b = synthetic.make_batch(B, K, seed=21)
    db = H.device_batch(b, cuda)
    model, variables = obbpose_model.construct_mipnerf(22, db, device=cuda)
    assert model.mlp_precision == 'f32' and model.disable_integration
    _biases(variables, 23, cuda)
    ret = model.apply(variables, 0, db['rays'], db['init'], db['ext'], b['ts'], randomized=False, rand_bkgd=False, white_bkgd=False,
                      alpha=10.0)
    rgb_r, _, acc_r, _, t_vals, t_mids = (ret[-1][i] for i in range(6))
    masks = ret[-1][8].reshape(-1).cpu().numpy()
    free = np.nonzero(masks == 0)[0]
    assert free.size >= 16
    o, d = db['rays'].origins[free].cpu(), db['rays'].directions[free].cpu()
    tm = t_mids[free].cpu()
    X = (d[:, None, :] * tm[:, :, None] + o[:, None, :]).reshape(-1, 3)            # the cylinder's mean: d t_mid + o, in fp32
    vd = db['rays'].viewdirs[free].cpu()[:, None, :].expand(-1, N, -1).reshape(-1, 3)
    q = field.query(model, variables, X.to(cuda), vd.contiguous().to(cuda), sigma=0.0, ts=b['ts'], ext=db['ext'])
    assert (q['owner'] == -1).all(), 'a sample of a ray that hits no box lies in no box'
    dens = q['density'].cpu().double().reshape(-1, N)
    col = q['rgb'].cpu().double().reshape(-1, N, 3)
    tv = t_vals[free].cpu().double()
    delta = (tv[:, 1:] - tv[:, :-1]) * d.double().norm(dim=-1, keepdim=True)
    a = dens * delta
    trans = torch.exp(-torch.cat([torch.zeros_like(a[:, :1]), torch.cumsum(a[:, :-1], -1)], -1))
    w = (1 - torch.exp(-a)) * trans
    acc = w.sum(-1)
    rgb = (w[..., None] * col).sum(1) + 0.5 * (1 - acc)[:, None]
    print('renderer: rgb %.2e acc %.2e' % (float((rgb - rgb_r[free].cpu().double()).abs().max()),
                                           float((acc - acc_r[free].cpu().double()).abs().max())))
    torch.testing.assert_close(rgb, rgb_r[free].cpu().double(), rtol=0, atol=RENDER_TOL)
    torch.testing.assert_close(acc, acc_r[free].cpu().double(), rtol=0, atol=RENDER_TOL)


# ---- 6. one call --------------------------------------------------------------------------------------------------------------
def test_one_call_is_the_staged_calls_for_every_chunk(cuda):
    s = _scene(cuda)
    n = 257
    st = _staged(s, cuda, n)
    base = _query(s, cuda, n, chunk=n)
    _same(base, st)
    for chunk in (64, 96, n - 1, n + 1):
        _same(_query(s, cuda, n, chunk=chunk), base)
    _same(_query(s, cuda, n, chunk=n), base)                       # two runs, the same bits
    own = base['owner'].cpu().numpy()
    multi = np.nonzero(own == -2)[0]
    assert multi.size and (base['valid'].cpu().numpy()[multi] == 0).all() and torch.isnan(base['rgb'][multi]).all()
    # a multi-owner point's neighbours in its wave are what they are without it: move it out of both boxes and compare the rest
    pts = s['pts'][:n].copy()
    pts[multi] = (5.0, 5.0, 5.0)
    moved = field.query(s['model'], s['variables'], _d(pts, cuda), _d(s['vd'][:n], cuda), ext=s['ext'], box_enable=s['en'], chunk=n)
    rest = torch.tensor(own != -2, device=cuda)
    _same({k: v[rest] for k, v in moved.items()}, {k: v[rest] for k, v in base.items()})
    assert (moved['valid'] == 1).all()
    # density only: no view direction, the same density bits
    dq = field.query(s['model'], s['variables'], _d(s['pts'][:n], cuda), None, ext=s['ext'], box_enable=s['en'], chunk=96)
    assert dq['rgb'] is None
    _same(dq, base, keys=('density', 'owner', 'valid'))
    assert torch.equal(_bits(dq['raw'][:, 3]), _bits(base['raw'][:, 3]))
    assert field.query(s['model'], s['variables'], torch.zeros(0, 3, device=cuda), None, ext=s['ext'])['density'].numel() == 0


# ---- 7. grid and columns ------------------------------------------------------------------------------------------------------
def test_grid_is_the_query_of_its_points(cuda):
    s = _scene(cuda)
    origin, shape = (0.05, -0.55, -0.45), (5, 7, 9)
    axes = ((0.11, 0.01, 0.0), (-0.01, 0.09, 0.02), (0.0, -0.015, 0.1))
    view = (0.6, -0.64, 0.48)
    g = field.grid(s['model'], s['variables'], origin, shape, axes=axes, view=view, ext=s['ext'], box_enable=s['en'], chunk=100,
                   want_points=True)
    pts = g['points'].reshape(-1, 3)
    want = lattice_ref.points(dict(origin=origin, du=axes[0], dv=axes[1], dw=axes[2]), shape, np.float64)
    err = np.abs(pts.cpu().numpy().astype(np.float64) - want)
    assert (err <= 2 * F.ulp32(np.maximum(np.abs(want), np.abs(np.asarray(origin))[None]))).all()
    n = pts.shape[0]
    vd = torch.tensor(view).to(cuda).expand(n, 3).contiguous()
    q = field.query(s['model'], s['variables'], pts.contiguous(), vd, ext=s['ext'], box_enable=s['en'], chunk=64)
    _same({k: g[k].reshape((n,) + tuple(g[k].shape[3:])) for k in ('density', 'rgb', 'raw', 'owner', 'valid')}, q)
    assert set(np.unique(q['owner'].cpu().numpy())) >= {-2, -1, 0}, 'the grid crosses the boxes and their overlap'
    g2 = field.grid(s['model'], s['variables'], origin, shape, axes=axes, view=None, ext=s['ext'], box_enable=s['en'], chunk=n + 5)
    assert g2['rgb'] is None and torch.equal(_bits(g2['density']), _bits(g['density']))


def test_columns_are_bit_reproducible(cuda):
    shape = (8, 8, 33)
    g = np.random.default_rng(11)
    d = (g.gamma(0.5, 4.0, shape)).astype(np.float32)
    v = np.ones(shape, np.uint8)
    d[1, 2, :] = np.nan; v[1, 2, :] = 0                            # a column with nothing in it
    d[3, 3, 5] = np.nan                                            # a NaN the valid plane does not flag
    v[4, 4, ::2] = 0
    d[5, 5, :] = 0.0
    d[6, 6, 32] = 1e6
    step, thr = 0.125, 6.0
    cm, co, cf = ops.field_columns(_d(d.reshape(-1), cuda), _d(v.reshape(-1), cuda, torch.uint8), shape, step, thr)
    wmax, wsum, wop, wfirst = F.columns(d, v, shape, step, thr)
    got = cm.cpu().numpy()
    assert (np.isnan(got) == np.isnan(wmax)).all() and (got[~np.isnan(wmax)] == wmax[~np.isnan(wmax)]).all()
    assert (cf.cpu().numpy() == wfirst).all() and (wfirst == -1).any() and (wfirst > 0).any()
    nw = shape[2]
    x = step * wsum
    bound = (nw + 4) * 2.0 ** -24 * x * np.exp(-x) + 4 * 2.0 ** -24
    assert (np.abs(co.cpu().numpy().astype(np.float64) - wop) <= bound).all()
    cm2, co2, cf2 = ops.field_columns(_d(d.reshape(-1), cuda), _d(v.reshape(-1), cuda, torch.uint8), shape, step, thr)
    assert torch.equal(_bits(co), _bits(co2)) and torch.equal(cf, cf2)
    m = field.columns(dict(density=_d(d, cuda), valid=_d(v, cuda, torch.uint8)), step=step, threshold=thr)
    assert torch.equal(_bits(m['opacity']), _bits(co)) and tuple(m['first'].shape) == (8, 8)


# ---- 8. scene edits -----------------------------------------------------------------------------------------------------------
def test_scene_edits(cuda):
    s = _scene(cuda)
    n = 257
    # box 1 off == the tree without box 1 (boxes 0 and 2; 2 stays off)
    off = _query(s, cuda, n, box_enable=[1, 0, 0])
    lay = s['variables'].layout
    keep = [0, 2]
    lay2 = obbpose_model.ParamLayout(lay.T, 2)
    flat2 = torch.zeros(lay2.total, device=cuda)
    v2 = obbpose_model.Variables(flat2, lay2)
    v2['params']['box_centers'].copy_(s['variables']['params']['box_centers'][:, keep])
    v2.mlp_flat('MLP_0').copy_(s['variables'].mlp_flat('MLP_0'))
    for j, k in enumerate(keep):
        v2.mlp_flat('BoxMLP_%d' % j).copy_(s['variables'].mlp_flat('BoxMLP_%d' % k))
    two = field.query(s['model'], v2, _d(s['pts'][:n], cuda), _d(s['vd'][:n], cuda), ext=s['ext'][keep], box_enable=[1, 0])
    _same(off, two, keys=('density', 'rgb', 'raw', 'valid'))
    assert torch.equal(off['owner'], two['owner']) and (off['owner'] <= 0).all() and (off['owner'] == 0).any()
    assert (off['valid'] == 1).all(), 'with box 1 off nothing is owned twice'
    # pose= == the query with box_centers overwritten
    pose = s['pose'].copy()
    pose[0, :3] += (0.05, -0.02, 0.03)
    pose[1, 3:] += (0.1, 0.0, -0.1)
    a = _query(s, cuda, n, pose=pose)
    keepc = s['variables']['params']['box_centers'].clone()
    try:
        s['variables']['params']['box_centers'][0].copy_(_d(pose, cuda))
        b = _query(s, cuda, n, ts=0)
    finally:
        s['variables']['params']['box_centers'].copy_(keepc)
    _same(a, b)
    assert not torch.equal(a['owner'], _query(s, cuda, n)['owner'])
