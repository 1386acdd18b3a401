"""The float64 row oracle of tests/test_gpu_mlp_edges.py, checked on the CPU alone: its forward is
oracle.durf_ref.mlp_apply_bf16, its backward without roundings is the exact reverse mode of oracle.durf_ref.mlp_apply, and
the chosen seeds give base rows on which a swapped ray, row, view direction or region cannot pass."""
import pytest
import torch

from oracle import durf_ref as R
from tests import mlp_rows_ref as MR


@pytest.mark.parametrize('width', [256, 128])
def test_forward_restatement_is_the_projects_bf16_oracle(width):
    o = MR.oracle(width)
    assert torch.equal(o['fwd']['raw'], o['fwd']['raw_ref'])
    assert o['fwd']['raw'].dtype == torch.float64
    for a in o['fwd']['h'] + [o['fwd']['hc']]:
        assert torch.equal(a, MR.bf(a)), 'stashed activations are bf16 values'


@pytest.mark.parametrize('width', [256, 128])
def test_backward_restatement_without_roundings_is_autograd_of_the_plain_mlp(width):
    b = MR.make_base(width)
    params = [[k.double().requires_grad_(True), bb.double().requires_grad_(True)] for k, bb in b['params']]
    x = b['x'].double().requires_grad_(True)
    rgb, dens = R.mlp_apply(params, x, b['cond'].double(), MR.cfg_of(width))
    raw = torch.cat([rgb.reshape(MR.ROWS, 3), dens.reshape(MR.ROWS, 1)], -1)
    (raw * b['draw'].double()).sum().backward()
    cond_rows = b['cond'][:, None, :].expand(MR.RAYS, MR.N, 27).reshape(MR.ROWS, 27)
    fwd = MR.forward64(b['params'], b['x'].reshape(MR.ROWS, -1), cond_rows, rnd=MR.ident)
    torch.testing.assert_close(fwd['raw'], raw.detach(), rtol=1e-12, atol=1e-12)
    bwd = MR.backward64(b['params'], fwd, b['draw'], rnd=MR.ident)
    torch.testing.assert_close(bwd['d_enc'][:, :b['in_dim']], x.grad.reshape(MR.ROWS, -1), rtol=1e-10, atol=1e-13)
    assert (bwd['d_enc'][:, b['in_dim']:] == 0).all()
    # a Dense layer's bias gradient is the column sum of its pre-activation gradient: region j <-> Dense_j, 9 <-> Dense_10
    for j in MR.STASHED:
        layer = 10 if j == 9 else j
        torch.testing.assert_close(bwd['dz'][j].sum(0), params[layer][1].grad, rtol=1e-10, atol=1e-13)
        if j in (1, 2, 3, 4, 6, 7):                # ... and its kernel gradient the product with the layer's input
            torch.testing.assert_close(fwd['h'][j - 1].T @ bwd['dz'][j], params[layer][0].grad, rtol=1e-10, atol=1e-13)


@pytest.mark.parametrize('width', [256, 128])
def test_chosen_seeds_satisfy_the_conditions(width):
    vals, bad = MR.conditions(width)
    print(width, MR.SEEDS[width], vals)
    assert not bad, bad


def test_roundings_change_the_backward_by_bf16_noise_only():
    """the rounded oracle stays within bf16 noise of the exact reverse mode: the roundings are where they belong, not more"""
    o = MR.oracle(256)
    b = o['base']
    exact = MR.backward64(b['params'], o['fwd'], b['draw'], rnd=MR.ident)
    rel = lambda a, c: float((a - c).norm() / c.norm())
    for j in MR.STASHED:
        assert 0 < rel(o['bwd']['dz'][j], exact['dz'][j]) < 2e-2
    assert 0 < rel(o['bwd']['d_enc'], exact['d_enc']) < 2e-2
