"""The per-ray float64 oracle of tests/test_gpu_pose_edges.py (tests/pose_rows_ref.py), pinned on the CPU alone: its rows,
summed over rays and pushed through pose_finish_ref, are the float64 autograd of the whole chain aa2matrix -> world2object_rpy
-> cast_rays -> encoding . d_enc with respect to the pose; that autograd agrees with central differences; the scale's terms
add up to the rows; the committed seed gives base rays that reach the branches the GPU test is about; and the recorded
float32 floors are what the twin gives."""
import math

import pytest
import torch

from oracle import durf_ref as R
from tests import pose_rows_ref as PR

C, NI, CY = PR.C, PR.NI, PR.CY
N = 24


def _rel(a, b):
    return float((a - b).norm() / b.norm())


def _chain_loss(kind, b, pose, hit, t, de, flags, alpha, raw, draw):
    o_s, d_s = PR.object_frame(b['o_w'].double(), b['d_w'].double(), pose, hit)
    radii = b['radii'].double()
    if kind == 'obj':
        enc, nf = PR.enc_obj(o_s, d_s, radii, t.double(), alpha, flags), 63
    else:
        enc, nf = PR.enc_bkgd(o_s, d_s, radii, t.double(), flags), 60
    L = (enc * de.double().reshape(enc.shape[0], enc.shape[1], 64)[..., :nf]).sum()
    if raw is not None:
        gn, _ = PR.norm_term(raw, draw, o_s.shape[0], torch.float64)
        L = L + (gn * torch.log(torch.sqrt((d_s * d_s).sum(-1)))).sum()         # d/dd = gn d / |d|^2
    return L, o_s, d_s


def _case(kind, variant, zero_rot):
    b = PR.make_base(zero_rot=zero_rot)
    if variant == 'two':
        b = PR.variant_base('two')
    hit = PR.base_hits(b)
    n = b['o_w'].shape[0]
    raw, draw = PR.make_raw_draw(n, N) if variant in ('raw', 'two') else (None, None)
    return b, hit, PR.make_t_vals(b, N), PR.make_d_enc(n, N), raw, draw


def _oracle_grad(kind, b, hit, t, de, flags, alpha, raw, draw):
    pose = b['pose'].double().requires_grad_(True)
    L, o_s, d_s = _chain_loss(kind, b, pose, hit, t, de, flags, alpha, raw, draw)
    L.backward()
    pr = b['pose'].double()[b['obj']]
    if kind == 'obj':
        rows, _ = PR.rows_obj(o_s.detach(), d_s.detach(), b['radii'], t, de, alpha, flags, b['o_w'], b['d_w'], pr, want_scale=False)
    else:
        rows, _ = PR.rows_bkgd(o_s.detach(), d_s.detach(), b['radii'], t, de, flags, b['o_w'], b['d_w'], pr, raw, draw,
                               want_scale=False)
    sums = torch.stack([(rows * hit[:, k:k + 1].double()).sum(0) for k in range(b['pose'].shape[0])])
    return PR.pose_finish_ref(b['pose'].double(), sums), pose.grad


@pytest.mark.parametrize('zero_rot', [False, True])
@pytest.mark.parametrize('alpha', [0.0, 3.3, 10.0])
@pytest.mark.parametrize('flags', [0, CY, NI, CY | NI])
def test_object_rows_sum_to_the_autograd_of_the_whole_chain(flags, alpha, zero_rot):
    b, hit, t, de, _, _ = _case('obj', 'plain', zero_rot)
    assert int(hit.sum()) == PR.K * PR.RAYS
    got, want = _oracle_grad('obj', b, hit, t, de, flags, alpha, None, None)
    for k in range(PR.K):
        assert _rel(got[k], want[k]) < 1e-9, (k, got[k], want[k])


# ('two' doubles box 0, whose rotation is not the zeroed one: no such case)
@pytest.mark.parametrize('variant,zero_rot', [('plain', False), ('plain', True), ('raw', False), ('raw', True), ('two', False)])
@pytest.mark.parametrize('flags', [0, C, NI, CY, C | NI, C | CY, NI | CY, C | NI | CY])
def test_background_rows_sum_to_the_autograd_of_the_whole_chain(flags, variant, zero_rot):
    b, hit, t, de, raw, draw = _case('bkgd', variant, zero_rot)
    assert int(hit.sum()) == hit.numel() if variant == 'two' else int(hit.sum()) == PR.K * PR.RAYS
    got, want = _oracle_grad('bkgd', b, hit, t, de, flags, 0.0, raw, draw)
    for k in range(PR.K):
        assert _rel(got[k], want[k]) < 1e-9, (k, got[k], want[k])


@pytest.mark.parametrize('kind,flags,variant', [('obj', 0, 'plain'), ('bkgd', C, 'raw'), ('bkgd', C, 'two')])
def test_autograd_agrees_with_central_differences(kind, flags, variant):
    b, hit, t, de, raw, draw = _case(kind, variant, False)
    pose = b['pose'].double().requires_grad_(True)
    _chain_loss(kind, b, pose, hit, t, de, flags, PR.ALPHA, raw, draw)[0].backward()
    g = torch.Generator().manual_seed(3)
    h = 1e-6
    for _ in range(3):
        v = torch.randn(pose.shape, generator=g, dtype=torch.float64)
        with torch.no_grad():
            lp = _chain_loss(kind, b, pose + h * v, hit, t, de, flags, PR.ALPHA, raw, draw)[0]
            lm = _chain_loss(kind, b, pose - h * v, hit, t, de, flags, PR.ALPHA, raw, draw)[0]
        fd, an = float(lp - lm) / (2 * h), float((pose.grad * v).sum())
        assert abs(fd - an) < 1e-6 * abs(an), (fd, an)


@pytest.mark.parametrize('kind,case', [('obj', (65, 0, PR.ALPHA)), ('obj', (65, NI | CY, PR.ALPHA)), ('bkgd', (65, C, 'raw')),
                                       ('bkgd', (65, C, 'two')), ('bkgd', (65, C | NI, 'plain'))])
def test_the_scales_terms_add_up_to_the_rows(kind, case):
    """the forward-mode terms whose absolute values make the scale sum to the backward's g_o, g_d; the scale bounds the rows"""
    b = PR.variant_base(case[2] if kind == 'bkgd' else 'plain')
    o_s, d_s = PR.cpu_object_frame(b)
    n, nf = b['o_w'].shape[0], 63 if kind == 'obj' else 60
    t, de = PR.make_t_vals(b, case[0]), PR.make_d_enc(n, case[0])

    def fn(o, d):
        if kind == 'obj':
            return PR.enc_obj(o, d, b['radii'].double(), t.double(), case[2], case[1])
        return PR.enc_bkgd(o, d, b['radii'].double(), t.double(), case[1])
    g_o, g_d = PR._ray_grads(fn, o_s, d_s, de, nf, torch.float64)
    a_o, a_d, s_o, s_d = PR._abs_sums(fn, o_s, d_s, de, nf)
    assert float((s_o - g_o).abs().max() / a_o.max()) < 1e-12 and float((s_d - g_d).abs().max() / a_d.max()) < 1e-12
    rows, scale = PR.case_rows(kind, case, b, o_s, d_s)
    assert bool((scale > 0).all()) and bool((rows.abs() <= scale * (1 + 1e-9)).all())


def test_pose_finish_ref_is_the_autograd_of_the_rotation():
    for Kf, first in PR.FINISH_CASES:
        pose, sums, _, names = PR.make_finish_case(Kf, Kf * 10 + first, first)
        got, want = PR.pose_finish_ref(pose.double(), sums.double()), PR.pose_finish_autograd(pose, sums)
        for k in range(Kf):
            assert _rel(got[k], want[k]) < 1e-9, (names[k], got[k], want[k])
        only_rot = PR.pose_finish_ref(pose.double(), sums.double(), False, True)
        assert torch.equal(only_rot[:, 3:], got[:, 3:]) and float(only_rot[:, :3].abs().max()) == 0.0
    assert {n for n, _ in PR.ROTATIONS} == {'zero', 'below', 'above', 'one', 'near_pi'}
    pose = PR.make_finish_case(5, 0, 0)[0].double()
    s0 = (pose[:, 3:] ** 2).sum(-1)
    assert [bool(x) for x in s0.float() < 1e-12] == [True, True, False, False, False]       # either side of k_pose_finish's `tiny`


# ---------------------------------------------------------------------------
# the seed conditions the GPU test relies on
# ---------------------------------------------------------------------------
def test_every_base_ray_hits_its_own_box_only():
    b = PR.make_base()
    hit = PR.base_hits(b)
    want = torch.zeros(PR.K * PR.RAYS, PR.K, dtype=hit.dtype)
    want[torch.arange(PR.K * PR.RAYS), b['obj']] = 1
    assert torch.equal(hit, want)
    assert bool((PR.base_hits(PR.variant_base('two')) == 1).all())
    assert float(b['ext'].min()) >= 2.0 and float(b['o_w'].abs().min()) > 1e-3 and float(b['d_w'].abs().min()) > 1e-3
    o_s, _ = PR.cpu_object_frame(b)
    assert bool((o_s.abs() > b['ext'][b['obj']]).any(-1).all()), 'origins lie outside the boxes'


@pytest.mark.parametrize('n', (8,) + PR.N_LIST)
def test_base_samples_reach_the_wrap_and_the_contraction_threshold(n):
    b = PR.make_base()
    o_s, d_s = PR.cpu_object_frame(b)
    t = PR.make_t_vals(b, n)
    assert bool((t[:, 1:] > t[:, :-1]).all())
    x = PR._samples(o_s.double(), d_s.double(), b['radii'].double(), t.double(), 0)[0]          # [rays, n, 3]
    # the safe_sin wrap: |x_i| 2^9 >= 314.16, on both signs
    pos = int((x.max(-1).values.max(-1).values * 512 >= 314.16).sum())
    neg = int((x.min(-1).values.min(-1).values * 512 <= -314.16).sum())
    assert pos >= 2 and neg >= 2, (pos, neg)
    if n >= 64:
        nx = x.norm(dim=-1)
        small, large = int((nx <= 0.1).any(-1).sum()), int((nx > 0.1).any(-1).sum())
        assert small >= 2 and large >= 2, (small, large)
        near = (nx <= 0.1).any(-1).nonzero().flatten().tolist()
        assert set(near) == {k * PR.RAYS + r for k in range(PR.K) for r in PR.NEAR_ORIGIN}
        # 'two' doubles the summed origin and direction: its near-origin rays still have samples on both sides
        b2 = PR.variant_base('two')
        o2, d2 = PR.cpu_object_frame(b2)
        n2 = PR._samples(o2.double(), d2.double(), b2['radii'].double(), PR.make_t_vals(b2, n).double(), 0)[0].norm(dim=-1)
        assert int((n2 <= 0.1).any(-1).sum()) >= 2


@pytest.mark.parametrize('n', [8, 65])
def test_raw_covers_the_three_softplus_branches(n):
    raw, _ = PR.make_raw_draw(PR.K * PR.RAYS, n)
    x = (raw[:, 3] + PR.DENSITY_BIAS).reshape(PR.K * PR.RAYS, n)
    assert bool((x < -15).any(-1).all()) and bool((x > 20).any(-1).all()) and bool(((x >= -15) & (x <= 20)).any(-1).all())


def test_case_lists_cover_the_dispatch():
    assert PR.N_LIST == (1, 64, 65, 128, 129, 256)
    assert {c[0] for c in PR.OBJ_CASES} >= set(PR.N_LIST) and {c[0] for c in PR.BKGD_CASES if c[1] == C} >= set(PR.N_LIST)
    assert {c[1] for c in PR.OBJ_CASES if c[0] == 65} == {0, CY, NI, CY | NI}
    assert {c[2] for c in PR.OBJ_CASES if c[0] == 64} == {0.0, PR.ALPHA, 10.0}
    assert {c[1] for c in PR.BKGD_CASES if c[0] == 65} == {C, 0, C | NI, C | CY}
    # the BARF window edges: alpha = 0 leaves only the identity features, alpha >= 10 sets every weight to 1
    assert float(R.barf_weights(0.0, 10, torch.float64).abs().max()) == 0.0
    assert float((R.barf_weights(10.0, 10, torch.float64) - 1).abs().max()) < 1e-15
    w = R.barf_weights(PR.ALPHA, 10, torch.float64)
    assert 0 < float(w[3]) < 1 and float(w[2]) == 1.0 and float(w[4]) == 0.0
    assert math.isclose(PR.WRAP, 100 * math.pi / 512, rel_tol=1e-7)


def test_recorded_floors_are_the_float32_twins():
    """FLOOR / FINISH_FLOOR of tests/test_gpu_pose_edges.py, from which its gates are made, against a fresh run of the twin
    (within a factor of 1.5 either way: the figure moves with the host's libm)"""
    from tests import test_gpu_pose_edges as T
    keys = [('obj',) + c for c in PR.OBJ_CASES] + [('bkgd',) + c for c in PR.BKGD_CASES]
    assert set(T.FLOOR) == set(keys)
    # a case without a recorded device figure is an error in the test file
    assert set(T.MEASURED) == {k + (p,) for k in keys if k[0] == 'obj' for p in (0, 1)} | {k for k in keys if k[0] == 'bkgd'}
    assert set(T.FINISH_MEASURED) == set(T.FINISH_FLOOR)
    for key, m in T.MEASURED.items():
        assert all(x <= g for x, g in zip(m, T._gates(key[0], key[1:4], key[4] if key[0] == 'obj' else 1))), key
    for key in keys:
        now = PR.twin_floor(key[0], key[1:])
        for a, r in zip(now, T.FLOOR[key]):
            assert r / 1.5 <= a <= r * 1.5, (key, now, T.FLOOR[key])
    now = PR.finish_floors()
    assert set(T.FINISH_FLOOR) == set(now)
    for key, a in now.items():
        assert T.FINISH_FLOOR[key] / 1.5 <= a <= T.FINISH_FLOOR[key] * 1.5, (key, a, T.FINISH_FLOOR[key])
