"""Scene layers on the GPU: boxes switched off on the device (box_enable), edited poses (pose=) and durf_render_layers --
the composite, the image without the boxes, the objects on their own and the per-pixel instance map in one call.

Every expected value is "the model on a particular parameter tree": a masked render is held, bit for bit, to the render of
the tree with the disabled boxes' rows cut out (tests/test_layers_host.py checks that construction on the oracle), and both
to the oracle on that tree at the bf16 forward tolerances of tests/test_golden_ref_model.py.

One deliberate difference from the reduced tree: entry 7 of the 10-tuple ([box_pose, box_rot0]) keeps all K rows under a
mask -- it reports the poses rendered with, and compacting it would need the mask on the host -- so its ENABLED rows are
compared with the reduced tree's.

Rays that hit several boxes: the reference sums their object-frame origins (obbpose_model.py:120-122) and what it renders
for them is garbage -- NaN at the last level, arbitrary finite values before (durf_amd/synthetic.py make_batch) -- so no
tolerance against the oracle means anything on them.  Bit-identity, the instance map and the background layer are checked
on scenes WITH such rays; the comparisons of rendered values against the oracle run on the same shapes drawn without them,
and on the scenes with them under every mask that leaves no ray hitting several ENABLED boxes (decided from the oracle's
intersection).  Wherever values are compared, every ray is: nothing is skipped."""
import numpy as np
import pytest
import torch

from durf_amd import obbpose_model, ops, synthetic, train_boxpose, utils
from oracle import durf_ref as R
from tests import helpers as H
from tests import test_layers_host as LH

pytestmark = pytest.mark.gpu

# (K, num_samples, image, chunk, rays that hit several boxes allowed): 37*53 and 40*50 are not multiples of their chunk.
# Seed 40: checked on the CPU to meet the conditions _scene asserts.
SCENES = [(1, 32, (37, 53), 512, False), (3, 128, (48, 64), 1024, True), (8, 32, (40, 50), 768, True)]
SEED = 40
BF16_TOL = dict(rgb=2e-2, acc=2e-2, weights=2e-2, distance=0.1, t_vals=0.05)      # tests/test_golden_ref_model.py (bf16)
NAMES = ('rgb', 'distance', 'acc', 'weights', 't_vals')


def _scene(cuda, K, N, hw, multi):
    utils.clear_gin()
    utils.parse_gin('MipNerfModel.num_samples = %d\nMipNerfModel.density_noise = 0.0\nMipNerfModel.no_pose_opt = True\n'
                    'MipNerfModel.no_yaw_opt = True\n' % N)
    b = synthetic.make_batch(hw[0] * hw[1], K, seed=SEED, allow_multi_hit=multi)
    ob, db = H.oracle_batch(b), H.device_batch(b, cuda)
    model, variables = obbpose_model.construct_mipnerf(1, db, device=cuda)
    inter = LH.oracle_intersection(ob['init'][b['ts']], ob['ext'], ob['rays'])
    # what keeps the tests below from passing vacuously
    assert float((inter.sum(-1) > 0).float().mean()) >= 0.05, 'at least 5 % box-hit rays'
    assert (inter.sum(0) > 0).all(), 'every box is hit by a ray'
    if multi:
        assert (inter.sum(-1) > 1).any(), 'a ray that hits several boxes'
    return b, ob, db, model, variables, inter


def _image(db, hw):
    return utils.namedtuple_map(lambda r: r.reshape(hw[0], hw[1], -1), db['rays'])


def _bits(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype, what
    assert torch.allclose(a, b, rtol=0, atol=0, equal_nan=True), what       # (multi-hit rays render NaN on every path)


def _same_tuples(got, want, keep, full_pose, what):
    assert len(got) == len(want)
    for lvl, (x, y) in enumerate(zip(got, want)):
        for i in range(7):
            _bits(x[i], y[i], '%s: level %d output %d' % (what, lvl, i))
        if keep is None:
            assert torch.equal(x[7][0], y[7][0]) and torch.equal(x[7][1], y[7][1]), what
        else:
            assert torch.equal(x[7][0][keep], y[7][0]), what + ': box_pose of the enabled boxes'
            assert torch.equal(x[7][0], full_pose[:, :3]) and torch.equal(x[7][1], full_pose[0, 3:]), what
        assert torch.equal(x[8].reshape(-1).int(), y[8].reshape(-1).int()), what + ': dyn_mask'
        _bits(x[9], y[9], what + ': zo')


def _oracle_check(ret, oracle, what):
    for lvl in range(len(oracle)):
        for i, nm in enumerate(NAMES):
            got, want = ret[lvl][i].double().cpu().numpy(), oracle[lvl][i].double().numpy()
            assert np.array_equal(np.isnan(got), np.isnan(want)), '%s level %d %s: NaN pattern' % (what, lvl, nm)
            err = float(np.nanmax(np.abs(got - want)))
            print('%s level %d %s: max abs error %.3e (tolerance %.1e)' % (what, lvl, nm, err, BF16_TOL[nm]))
            np.testing.assert_allclose(got, want, rtol=0, atol=BF16_TOL[nm], err_msg='%s level %d %s' % (what, lvl, nm))
    assert torch.equal(ret[0][8].reshape(-1).cpu().long(), oracle[0][8].reshape(-1))


@pytest.mark.parametrize('K,N,hw,chunk,multi', SCENES)
def test_masked_box_test_matches_the_oracle_intersection(cuda, K, N, hw, chunk, multi):
    """stage level (durf_ray_setup_masked): hit == the oracle's intersection with the disabled columns zeroed, bit-exact; the
    selected origins / directions / zo follow the enabled boxes only"""
    b, ob, db, model, variables, inter = _scene(cuda, K, N, hw, multi)
    pose = db['init'][b['ts']].contiguous()
    rays = db['rays']
    plain = ops.ray_setup(rays.origins, rays.directions, pose, db['ext'])
    for mask in LH.masks_for(K):
        keep = LH.keep_of(mask)
        got = ops.ray_setup(rays.origins, rays.directions, pose, db['ext'], box_enable=torch.tensor(mask, device=cuda))
        want_hit = inter * torch.tensor(mask)[None, :]
        assert torch.equal(got[2].cpu().long(), want_hit), 'hit masks must be bit-exact (mask %s)' % mask
        sub = ops.ray_setup(rays.origins, rays.directions, pose[keep].contiguous(), db['ext'][keep].contiguous()) if keep else None
        if sub is None:
            _bits(got[0], rays.origins, 'no box: the world-frame origins')
            _bits(got[1], rays.directions, 'no box: the world-frame directions')
            assert not got[3].any()
        else:
            for i in (0, 1, 3):
                _bits(got[i], sub[i], 'mask %s output %d against the reduced box list' % (mask, i))
            assert torch.equal(got[2][:, keep], sub[2])
        if all(mask):
            for g, p in zip(got, plain):
                _bits(g.float(), p.float(), 'all ones is durf_ray_setup')


@pytest.mark.parametrize('K,N,hw,chunk,multi', SCENES)
def test_nothing_changes_when_the_knobs_are_unused(cuda, K, N, hw, chunk, multi):
    b, ob, db, model, variables, inter = _scene(cuda, K, N, hw, multi)
    args = (variables, 0, db['rays'], db['init'], db['ext'], b['ts'])
    kw = dict(randomized=False, rand_bkgd=False, white_bkgd=False, alpha=6.5)
    base = model.apply_one_call(*args, **kw)
    ones = torch.ones(K, dtype=torch.int32, device=cuda)
    _same_tuples(model.apply_one_call(*args, box_enable=None, pose=None, **kw), base, None, None, 'apply_one_call, None')
    _same_tuples(model.apply_one_call(*args, box_enable=ones, **kw), base, None, None, 'apply_one_call, all ones')
    _same_tuples(model.apply(*args, box_enable=ones, **kw), model.apply(*args, **kw), None, None, 'apply, all ones')
    _same_tuples(model.apply(*args, box_enable=ones, **kw), base, None, None, 'apply against apply_one_call')
    img = _image(db, hw)
    want = model.render_image_one_call(variables, img, db['init'], db['ext'], b['ts'], False, 6.5, chunk=chunk)
    for be in (None, ones):
        got = model.render_layers(variables, img, db['init'], db['ext'], b['ts'], False, 6.5, chunk=chunk, box_enable=be, layers=())
        assert sorted(got) == ['acc', 'distance', 'rgb']
        for name, w in zip(('rgb', 'distance', 'acc'), want):
            _bits(got[name], w, 'render_layers %s with nothing asked for' % name)
    # ... and against the C entry point itself
    flat = utils.namedtuple_map(lambda r: r.reshape(hw[0] * hw[1], -1), img)
    lay = variables.layout
    o0 = lay.mlp_off['BoxMLP_0']
    direct = ops.render_image_call(flat, db['init'][b['ts']].contiguous(), db['ext'].reshape(-1, 3).contiguous(), variables.mlp_flat('MLP_0'),
                                   variables.flat[o0:o0 + K * lay.mlp_size[128]], lay.mlp_size[128], N, 2, 6.5, ops.ENC_CONTRACT, chunk)
    for g, w in zip(direct, want):
        _bits(g.reshape(w.shape), w, 'durf_render_image')


def _with_and_without_multi_hit(scenes):
    """every scene, and for those with multi-hit rays the same shape drawn without them (oracle=True: values are held to the oracle)"""
    out = []
    for K, N, hw, chunk, multi in scenes:
        if multi:
            out.append((K, N, hw, chunk, True, False))
        out.append((K, N, hw, chunk, False, True))
    return out


@pytest.mark.parametrize('K,N,hw,chunk,multi,oracle_values', _with_and_without_multi_hit(SCENES))
def test_a_masked_render_is_the_render_of_the_tree_without_those_boxes(cuda, K, N, hw, chunk, multi, oracle_values):
    b, ob, db, model, variables, inter = _scene(cuda, K, N, hw, multi)
    params = H.oracle_params_from_variables(variables)
    full_pose = variables['params']['box_centers'][b['ts']]
    kw = dict(randomized=False, rand_bkgd=False, white_bkgd=True, alpha=6.5)
    for mask in LH.masks_for(K):
        keep = LH.keep_of(mask)
        en = torch.tensor(mask, dtype=torch.int32, device=cuda)
        sub = LH.reduce_variables(variables, keep)
        got = model.apply_one_call(variables, 0, db['rays'], db['init'], db['ext'], b['ts'], box_enable=en, **kw)
        want = model.apply_one_call(sub, 0, db['rays'], db['init'][:, keep], db['ext'][keep], b['ts'], **kw)
        _same_tuples(got, want, keep, full_pose, 'K=%d mask %s' % (K, mask))
        # the Python-issued path takes the same switch
        _same_tuples(model.apply(variables, 0, db['rays'], db['init'], db['ext'], b['ts'], box_enable=en, **kw), want, keep, full_pose,
                     'apply, K=%d mask %s' % (K, mask))
        if oracle_values or not ((inter * torch.tensor(mask)[None, :]).sum(-1) > 1).any():
            with torch.no_grad():
                oracle = R.model_apply(LH.reduce_oracle_params(params, keep), ob['rays'], b['ts'], ob['ext'][keep], False, False, True,
                                       6.5, cfg=dict(num_samples=N))
            _oracle_check(got, oracle, 'masked K=%d %s' % (K, mask))
            _oracle_check(want, oracle, 'reduced K=%d %s' % (K, mask))
        assert int(got[0][8].sum()) == int((inter * torch.tensor(mask)[None, :]).sum())


def test_the_fp32_model_takes_the_switch_too(cuda):
    """mlp_precision='f32': apply() issues the masked prologue with no weight streams to pack; same contract, bit for bit"""
    K, N, hw = 3, 32, (30, 40)
    b, ob, db, model, variables, inter = _scene(cuda, K, N, hw, False)
    model.mlp_precision = 'f32'
    full_pose = variables['params']['box_centers'][b['ts']]
    kw = dict(randomized=False, rand_bkgd=False, white_bkgd=False, alpha=6.5)
    for mask in LH.masks_for(K):
        keep = LH.keep_of(mask)
        en = torch.tensor(mask, dtype=torch.int32, device=cuda)
        ops.dispatch_reset()
        got = model.apply(variables, 0, db['rays'], db['init'], db['ext'], b['ts'], box_enable=en, **kw)
        assert 'BOX_MASK' in ops.layer_log_seen()
        want = model.apply(LH.reduce_variables(variables, keep), 0, db['rays'], db['init'][:, keep], db['ext'][keep], b['ts'], **kw)
        _same_tuples(got, want, keep, full_pose, 'f32, mask %s' % mask)
    ops.dispatch_reset()


@pytest.mark.parametrize('K,N,hw,chunk,multi', SCENES)
def test_pose_argument_equals_writing_the_poses_into_the_tree(cuda, K, N, hw, chunk, multi):
    b, ob, db, model, variables, inter = _scene(cuda, K, N, hw, multi)
    ts = b['ts']
    g = torch.Generator().manual_seed(3)
    new = variables['params']['box_centers'][ts].clone()
    new[:, :3] += (torch.rand(K, 3, generator=g) * 0.1 - 0.05).to(cuda)
    new[:, 4] += (torch.rand(K, generator=g) * 0.4 - 0.2).to(cuda)
    moved = variables.like(variables.flat.clone())
    moved['params']['box_centers'][ts] = new
    kw = dict(randomized=False, rand_bkgd=False, white_bkgd=False, alpha=6.5)
    args = (0, db['rays'], db['init'], db['ext'], ts)
    want = model.apply_one_call(moved, *args, **kw)
    assert not torch.equal(want[0][8], model.apply_one_call(variables, *args, **kw)[0][8]), 'the edit must move a box across a ray'
    _same_tuples(model.apply_one_call(variables, *args, pose=new, **kw), want, None, None, 'apply_one_call(pose=)')
    _same_tuples(model.apply(variables, *args, pose=new, **kw), want, None, None, 'apply(pose=)')
    img = _image(db, hw)
    w_img = model.render_image_one_call(moved, img, db['init'], db['ext'], ts, False, 6.5, chunk=chunk)
    got = model.render_layers(variables, img, db['init'], db['ext'], ts, False, 6.5, chunk=chunk, pose=new, layers=())
    for name, w in zip(('rgb', 'distance', 'acc'), w_img):
        _bits(got[name], w, 'render_layers(pose=) ' + name)


@pytest.mark.parametrize('white', [False, True])
@pytest.mark.parametrize('K,N,hw,chunk,multi,oracle_values', _with_and_without_multi_hit(SCENES))
def test_layers(cuda, K, N, hw, chunk, multi, white, oracle_values):
    b, ob, db, model, variables, inter = _scene(cuda, K, N, hw, multi)
    params = H.oracle_params_from_variables(variables)
    img = _image(db, hw)
    n = hw[0] * hw[1]
    nothing = LH.reduce_variables(variables, [])
    bg_want = model.render_image_one_call(nothing, img, db['init'][:, []], db['ext'][[]], b['ts'], white, 6.5, chunk=chunk)
    for mask in LH.masks_for(K):
        keep = LH.keep_of(mask)
        what = 'K=%d mask %s' % (K, mask)
        en = torch.tensor(mask, dtype=torch.int32, device=cuda)
        out = model.render_layers(variables, img, db['init'], db['ext'], b['ts'], white, 6.5, chunk=chunk, box_enable=en)
        torch.cuda.synchronize()
        assert sorted(out) == ['acc', 'bg_acc', 'bg_distance', 'bg_rgb', 'distance', 'instance', 'obj_rgba', 'rgb']
        # the composite: render_image_one_call of the tree without the disabled boxes
        sub = LH.reduce_variables(variables, keep)
        comp = model.render_image_one_call(sub, img, db['init'][:, keep], db['ext'][keep], b['ts'], white, 6.5, chunk=chunk)
        for name, w in zip(('rgb', 'distance', 'acc'), comp):
            _bits(out[name], w, what + ' composite ' + name)
        # the background: every box disabled
        for name, w in zip(('bg_rgb', 'bg_distance', 'bg_acc'), bg_want):
            _bits(out[name], w, what + ' ' + name)
            assert not torch.isnan(out[name]).any()
        # the instance map: exact, from the oracle's intersection
        inst = LH.instance_from(inter, mask)
        assert out['instance'].dtype == torch.int32 and out['instance'].shape == hw
        assert torch.equal(out['instance'].reshape(-1).cpu().long(), inst), what + ' instance'
        hit_rays = inst != -1
        if keep:
            assert hit_rays.any()
            if white or not multi:       # (where the composite differs from the background at all: a visible box)
                assert not torch.equal(out['bg_rgb'], out['rgb'])
        # the objects: exactly zero off the boxes; on them the oracle's composite with no background colour, and its acc
        rgba = out['obj_rgba'].reshape(n, 4).cpu()
        assert rgba[~hit_rays].eq(0).all(), what + ': obj_rgba is exactly zero off the boxes'
        _bits(out['obj_rgba'][..., 3][out['instance'] != -1], out['acc'][out['instance'] != -1], what + ': alpha is acc')
        if not oracle_values and (inst == -2).any():
            continue
        with torch.no_grad():
            oracle = R.model_apply(LH.reduce_oracle_params(params, keep), ob['rays'], b['ts'], ob['ext'][keep], False, True, False, 6.5,
                                   cfg=dict(num_samples=N))[-1]
        want = torch.cat([oracle[0], oracle[2].reshape(-1, 1)], -1)
        got_h, want_h = rgba[hit_rays].double().numpy(), want[hit_rays].double().numpy()
        assert not np.isnan(got_h).any() and not np.isnan(want_h).any()
        if got_h.size:
            print('%s white=%s obj_rgba: max abs error %.3e over %d rays' % (what, white, float(np.abs(got_h - want_h).max()), got_h.shape[0]))
        np.testing.assert_allclose(got_h, want_h, rtol=0, atol=2e-2, err_msg=what + ' obj_rgba')


def test_layers_not_asked_for_cost_no_launch(cuda):
    K, N, hw, chunk, multi = SCENES[1]
    b, ob, db, model, variables, inter = _scene(cuda, K, N, hw, multi)
    img = _image(db, hw)
    args = (variables, img, db['init'], db['ext'], b['ts'], False, 6.5)
    ops.dispatch_reset()
    model.render_image_one_call(*args, chunk=chunk)
    plain = ops.dispatch_seen()
    assert plain and ops.layer_log_seen() == set()
    ops.dispatch_reset()
    model.render_layers(*args, chunk=chunk, layers=())
    assert ops.dispatch_seen() == plain and ops.layer_log_seen() == set(), 'the composite alone is durf_render_image\'s launch sequence'
    ops.dispatch_reset()
    model.render_layers(*args, chunk=chunk, layers=('instance', 'objects'))
    assert ops.dispatch_seen() == plain and ops.layer_log_seen() == {'SELECT'}, 'no second pass unless the background is asked for'
    ops.dispatch_reset()
    model.render_layers(*args, chunk=chunk, box_enable=torch.ones(K, dtype=torch.int32, device=cuda))
    assert ops.dispatch_seen() >= plain and ops.layer_log_seen() == {'SELECT', 'PASS2', 'BOX_MASK'}
    ops.dispatch_reset()


def test_an_undersized_layer_workspace_is_refused(cuda, monkeypatch):
    K, N, hw, chunk, multi = SCENES[0]
    b, ob, db, model, variables, inter = _scene(cuda, K, N, hw, multi)
    img = _image(db, hw)
    args = (variables, img, db['init'], db['ext'], b['ts'], False, 6.5)
    good = model.render_layers(*args, chunk=chunk)
    need = int(ops._lib.lib().durf_render_layers_workspace_bytes(hw[0] * hw[1], chunk, N, K, 2))
    real = ops._workspace
    monkeypatch.setattr(ops, '_workspace', lambda dev, nb: real(dev, nb)[:nb - 256])
    with pytest.raises(ops._lib.DurfError, match=r'durf_render_layers: workspace of %d bytes.* = %d' % (need - 256, need)):
        model.render_layers(*args, chunk=chunk)
    monkeypatch.setattr(ops, '_workspace', real)
    again = model.render_layers(*args, chunk=chunk)
    for k in good:
        _bits(again[k].float(), good[k].float(), k)


def test_evaluate_carries_the_layers_on_request(cuda):
    K, N, hw, chunk, multi = SCENES[0]
    b, ob, db, model, variables, inter = _scene(cuda, K, N, hw, multi)
    config = utils.configured(utils.Config)
    case = dict(rays=_image(db, hw), pixels=db['pixels'].reshape(hw[0], hw[1], -1), init=db['init'], ext=db['ext'], ts=b['ts'])
    plain = train_boxpose.evaluate(model, config, variables, case, 10.0, chunk=chunk)
    assert 'instance' not in plain and 'bg_rgb' not in plain
    ev = train_boxpose.evaluate(model, config, variables, case, 10.0, chunk=chunk, layers=True)
    _bits(ev['rgb'], plain['rgb'], 'rgb')
    assert float(ev['psnr']) == float(plain['psnr'])
    assert {'instance', 'bg_rgb', 'bg_distance', 'bg_acc', 'obj_rgba'} <= set(ev)
    assert torch.equal(ev['instance'].reshape(-1).cpu().long(), LH.instance_from(inter, [1] * K))
