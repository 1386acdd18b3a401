"""Scene layers, the part that needs no GPU: the new entry points are declared, bound and exported; the construction the GPU
tests use for "the model without the disabled boxes" (cut their rows out of the tree) is itself checked on the oracle
against the other way of saying it (shrink a box to a point so that every ray misses it); argument validation of
MipNerfModel.render_layers.  The helpers at the top are shared with tests/test_gpu_layers.py."""
import os

import numpy as np
import pytest
import torch

from durf_amd import _lib, _sigs, obbpose_model, ops, synthetic, utils
from oracle import durf_ref as R
from tests import helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ('durf_ray_setup_masked', 'durf_ray_prologue_pack_masked', 'durf_forward_masked',
                'durf_render_layers_workspace_bytes', 'durf_render_layers')


# ---- shared helpers ---------------------------------------------------------------------------------------------------
def masks_for(K):
    """{all on, all off, one off, only one on} for K boxes (K = 1: the last two coincide with the first two)"""
    on, off = [1] * K, [0] * K
    one_off, one_on = list(on), list(off)
    one_off[K // 2] = 0
    one_on[K - 1] = 1
    out = []
    for m in (on, off, one_off, one_on):
        if m not in out:
            out.append(m)
    return out


def reduce_oracle_params(params, keep):
    """the oracle's parameter tree without the boxes not in `keep`: their box_centers columns and BoxMLP_k deleted"""
    out = {'box_centers': params['box_centers'][:, keep].clone(), 'MLP_0': params['MLP_0']}
    for j, k in enumerate(keep):
        out['BoxMLP_%d' % j] = params['BoxMLP_%d' % k]
    return out


def reduce_variables(variables, keep):
    """the same cut on the product's flat parameter buffer -> Variables with K' = len(keep) boxes"""
    lay = variables.layout
    new = obbpose_model.ParamLayout(lay.T, len(keep), lay.use_viewdirs)
    out = obbpose_model.Variables(torch.zeros(new.total, dtype=torch.float32, device=variables.flat.device), new)
    if keep:
        out['params']['box_centers'].copy_(variables['params']['box_centers'][:, keep])
    out.mlp_flat('MLP_0').copy_(variables.mlp_flat('MLP_0'))
    for j, k in enumerate(keep):
        out.mlp_flat('BoxMLP_%d' % j).copy_(variables.mlp_flat('BoxMLP_%d' % k))
    return out


def oracle_intersection(pose, ext, rays):
    """the oracle's `intersection` [B,K] (obbpose_model.py:99-115 as oracle/durf_ref.py:522-535 restates it)"""
    Bn, K = rays.origins.shape[0], pose.shape[0]
    if K == 0:
        return torch.zeros(Bn, 0, dtype=torch.int64)
    box_pose = pose[:, :3].expand(Bn, K, 3)
    box_mat = R.aa2matrix(pose[:, 3:]).expand(Bn, K, 3, 3)
    oo, do = R.world2object_rpy(rays.origins, rays.directions, box_pose, box_mat)
    dims = ext.expand(Bn, K, 3)
    return R.ray_box_intersection(oo, do, -dims, dims)[2]


def instance_from(inter, mask):
    """instance [B] from the oracle's intersection and the mask: k if exactly the enabled box k is hit, -1 none, -2 several"""
    inter = inter * torch.as_tensor(mask, dtype=inter.dtype)[None, :] if inter.shape[1] else inter
    n = inter.sum(-1)
    which = (inter * torch.arange(inter.shape[1])[None, :]).sum(-1)
    return torch.where(n == 0, torch.full_like(n, -1), torch.where(n == 1, which, torch.full_like(n, -2)))


def keep_of(mask):
    return [k for k, m in enumerate(mask) if m]


# ---- tests ------------------------------------------------------------------------------------------------------------
def test_the_layer_entry_points_are_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, 'include', 'durf_hip.h')).read()
    stub = open(os.path.join(ROOT, 'include', 'durf_ctypes_stub.py')).read()
    doc = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    for name in ENTRY_POINTS:
        assert name + '(' in hdr, name
        assert 'L.%s.argtypes' % name in stub, name
        assert name in doc, name
        assert name in _sigs.SIGS and name in _lib.symbols(), name
        assert hasattr(_lib.lib(), name), name
    assert _lib.lib().durf_version() == 41
    # the workspace of the layered call holds the image call's and the per-image buffers on top
    L = _lib.lib()
    assert L.durf_render_layers_workspace_bytes(4000, 512, 32, 3, 2) > L.durf_render_image_workspace_bytes(512, 32, 3, 2)


@pytest.mark.parametrize('K,seed,multi', [(1, 11, False), (3, 12, True), (4, 13, False)])
def test_cutting_a_box_out_of_the_tree_is_the_oracle_with_that_box_missed(K, seed, multi):
    """float64 oracle: a box whose half extents are 0 is missed by every ray (t_far > t_near fails), so it contributes
    mask * (...) = 0 to every sum -- the outputs must equal those of the tree with the box's rows cut out, which is what
    reduce_oracle_params / reduce_variables build; all boxes off equals the K = 0 oracle."""
    b = synthetic.make_batch(192, K, seed=seed, allow_multi_hit=multi)
    ob = R.batch_from_numpy(b, torch.float64)
    params = R.init_params(5, ob['init'], K, dtype=torch.float64)
    cfg = dict(num_samples=8)
    inter = oracle_intersection(params['box_centers'][b['ts']], ob['ext'], ob['rays'])
    assert (inter.sum(0) > 0).all(), 'every box is hit'
    for mask in masks_for(K):
        keep = keep_of(mask)
        ext0 = ob['ext'] * torch.tensor(mask, dtype=torch.float64)[:, None]
        with torch.no_grad():
            a = R.model_apply(params, ob['rays'], b['ts'], ext0, False, False, False, 6.5, cfg=cfg)
            r = R.model_apply(reduce_oracle_params(params, keep), ob['rays'], b['ts'], ob['ext'][keep], False, False, False, 6.5,
                              cfg=cfg)
        for lvl in range(2):
            for i in (0, 1, 2, 3, 4, 5, 6, 9):
                np.testing.assert_allclose(a[lvl][i].numpy(), r[lvl][i].numpy(), rtol=0, atol=0, err_msg='mask %s output %d' % (mask, i))
            assert torch.equal(a[lvl][8], r[lvl][8])
        assert torch.equal(a[0][8].reshape(-1), (inter * torch.tensor(mask)[None, :]).sum(-1))
        assert torch.equal(instance_from(inter, mask) >= 0, a[0][8].reshape(-1) == 1)
    if multi:
        assert (instance_from(inter, [1] * K) == -2).any(), 'the scene has a ray that hits several boxes'


def test_reduce_variables_mirrors_the_oracle_cut():
    b = synthetic.make_batch(64, 3, seed=2)
    utils.clear_gin()
    model, variables = obbpose_model.construct_mipnerf(0, {'init': torch.tensor(b['init'])}, device='cpu')
    keep = [0, 2]
    got = H.oracle_params_from_variables(reduce_variables(variables, keep))
    want = reduce_oracle_params(H.oracle_params_from_variables(variables), keep)
    assert sorted(got) == sorted(want) == ['BoxMLP_0', 'BoxMLP_1', 'MLP_0', 'box_centers']
    assert torch.equal(got['box_centers'], want['box_centers'])
    for name in ('MLP_0', 'BoxMLP_0', 'BoxMLP_1'):
        for (gk, gb), (wk, wb) in zip(got[name], want[name]):
            assert torch.equal(gk, wk) and torch.equal(gb, wb)
    assert reduce_variables(variables, []).layout.K == 0


def test_render_layers_validates_its_arguments():
    b = synthetic.make_batch(6 * 8, 3, seed=2)
    utils.clear_gin()
    model, variables = obbpose_model.construct_mipnerf(0, {'init': torch.tensor(b['init'])}, device='cpu')
    rays = utils.BoxRays(**{k: torch.tensor(v).reshape(6, 8, -1) for k, v in b['rays'].items()})
    args = (variables, rays, torch.tensor(b['init']), torch.tensor(b['ext']), b['ts'], False, 10.0)
    with pytest.raises(ValueError, match='unknown layers'):
        model.render_layers(*args, layers=('instance', 'shadows'))
    with pytest.raises(ValueError, match='box_enable: 2 values for K = 3'):
        model.render_layers(*args, box_enable=[1, 0])
    with pytest.raises(ValueError, match=r'pose: shape \(3, 3\), expected \(3, 6\)'):
        model.render_layers(*args, pose=torch.zeros(3, 3))
    with pytest.raises(NotImplementedError, match='durf_render_layers covers'):       # (CPU tensors: outside supports_one_call)
        model.render_layers(*args)
