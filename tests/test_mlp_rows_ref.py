"""The float64 row oracle of tests/test_gpu_mlp_edges.py, checked on the CPU alone: its forward is
oracle.durf_ref.mlp_apply_bf16, its backward without roundings is the exact reverse mode of oracle.durf_ref.mlp_apply, and
the chosen seeds give base rows on which a swapped ray, row, view direction or region cannot pass.

The exact-fp32 side (tests/test_gpu_f32_edges.py): records64 is that same forward / reverse mode with every Dense's input,
pre-activation and pre-activation gradient exposed, and the "delicate" rows -- a ReLU pre-activation within 2e-6 of zero, where
the fp32 kernel's own mask may legitimately differ from float64's -- stay under 2 % of every base (asserted below).  For the
committed seeds (W = 256: 11, W = 128: 12; the N = 24 base draws from seed + 1000):
  W = 256: N = 32 base: 4 delicate rows of 512, smallest |z| 1.2e-7, 2 units below 1e-6 and 24 below 1e-5 of 1 114 112;
           N = 24 base: 5 of 504, 7.8e-7, 2 and 27 of 1 096 704; the 16 tail rows: none, 2.2e-6.
  W = 128: N = 32 base: 5 of 512, 1.6e-7, 1 and 11 of 589 824; N = 24 base: 3 of 504, 1.1e-7, 1 and 14 of 580 608; tail: none,
           3.2e-4.
  N = 24 base, ReLUs active per layer 0-7, 10: W = 256 0.501 0.493 0.505 0.502 0.502 0.503 0.529 0.540 0.460, smallest
           max-abs distance between two raw rows 2.2e-2; W = 128 0.503 0.501 0.475 0.539 0.478 0.494 0.499 0.481 0.494, 2.1e-2."""
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


# ---------------------------------------------------------------------------------------------------------------------
# the exact-fp32 record oracle
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('width', [256, 128])
def test_record_oracle_is_the_unrounded_restatement_and_autograd_of_every_dense(width):
    o = MR.oracle_f32(width)
    b, rec = o['base'], o['main']
    cond_rows = b['cond'][:, None, :].expand(MR.RAYS, MR.N, 27).reshape(MR.ROWS, 27)
    fwd = MR.forward64(b['params'], b['x'].reshape(MR.ROWS, -1), cond_rows, rnd=MR.ident)
    bwd = MR.backward64(b['params'], fwd, b['draw'], rnd=MR.ident)
    assert torch.equal(rec['raw'], fwd['raw']) and torch.equal(rec['d_enc'], bwd['d_enc'])
    for j in range(8):
        assert torch.equal(rec['X'][8 if j == 7 else j + 1][:, :width], fwd['h'][j])
    assert torch.equal(rec['X'][11], fwd['hc'])
    for j in MR.STASHED:
        assert torch.equal(rec['dz'][10 if j == 9 else j], bwd['dz'][j])
    # the concatenations, as the header of csrc/mlp_f32.hip lists them
    x = b['x'].reshape(MR.ROWS, -1).double()
    assert torch.equal(rec['X'][0], x) and torch.equal(rec['X'][5][:, width:], x)
    assert torch.equal(rec['X'][10][:, width:], cond_rows.double()) and torch.equal(rec['X'][10][:, :width], rec['Z'][9])
    assert rec['X'][9] is rec['X'][8]
    # every Dense of the autograd graph: db = column sums of dz, dK = X^T dz -- the heads and the linear bottleneck included
    params = [[k.double().requires_grad_(True), bb.double().requires_grad_(True)] for k, bb in b['params']]
    rgb, dens = R.mlp_apply(params, b['x'].double(), b['cond'].double(), MR.cfg_of(width))
    raw = torch.cat([rgb.reshape(MR.ROWS, 3), dens.reshape(MR.ROWS, 1)], -1)
    (raw * b['draw'].double()).sum().backward()
    for l in range(12):
        assert rec['X'][l].shape[1] == params[l][0].shape[0] and rec['dz'][l].shape[1] == params[l][0].shape[1]
        torch.testing.assert_close(rec['dz'][l].sum(0), params[l][1].grad, rtol=1e-10, atol=1e-13)
        torch.testing.assert_close(rec['X'][l].T @ rec['dz'][l], params[l][0].grad, rtol=1e-10, atol=1e-13)


@pytest.mark.parametrize('width', [256, 128])
def test_f32_spec_restatement(width):
    in_dim = MR.IN_DIM[width]
    S = MR.f32_spec(width, in_dim)
    rec = MR.oracle_f32(width)['main']
    for l, Ly in enumerate(S['L']):
        assert (Ly['fi'], Ly['fo']) == (rec['X'][l].shape[1], rec['dz'][l].shape[1])
    assert [Ly['fi'] * Ly['fo'] + Ly['fo'] for Ly in S['L']] == [k.numel() + bb.numel() for k, bb in MR.make_base(width)['params']]
    # act: every Dense's input once, Dense_9 sharing Dense_8's; dz: every Dense's output, in Dense order, back to back
    assert S['act'] == sum(Ly['fi'] for l, Ly in enumerate(S['L']) if l != 9) == {256: 2579, 128: 1433}[width]
    assert S['dz'] == sum(Ly['fo'] for Ly in S['L']) == {256: 2436, 128: 1284}[width]
    assert S['L'][9]['x_off'] == S['L'][8]['x_off']
    spans = sorted((Ly['x_off'], Ly['x_off'] + Ly['fi']) for l, Ly in enumerate(S['L']) if l != 9)
    assert spans[0][0] == 0 and all(a[1] == c[0] for a, c in zip(spans, spans[1:])) and spans[-1][1] == S['act']
    assert all(S['L'][l]['dz_off'] + S['L'][l]['fo'] == S['L'][l + 1]['dz_off'] for l in range(11))


@pytest.mark.parametrize('width', [256, 128])
def test_delicate_rows_and_the_n24_base_satisfy_the_conditions(width):
    vals, bad = MR.conditions_f32(width)
    print(width, MR.SEEDS[width], vals)
    assert not bad, bad
    for name in ('main', 'n24'):
        assert vals[name]['delicate_rows'] <= 10 and vals[name]['min_abs_z'] < MR.DELICATE
    assert vals['tail']['delicate_rows'] == 0
    assert MR.ROWS24 == 504 and MR.ROWS24 % 32 == 24, 'a partial last tile; tiles that straddle rays'
    # the committed make_base draws are what tests/test_gpu_mlp_edges.py was measured on: the second base must not move them
    assert MR.make_base24(width)['x'].shape == (MR.RAYS24, MR.N24, MR.IN_DIM[width])
