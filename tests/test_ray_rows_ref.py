"""tests/ray_rows_ref.py (the float64 oracle of tests/test_gpu_ray_edges.py, its float32 twin and its inputs) pinned on the CPU
alone: the oracle against oracle/durf_ref.py's restatement of the reference, the literal expectations of the hand-aimed table,
the exactness that makes that table decided, TAU against a fresh measurement, the <= 1 % undecided budget, the balance of
hits and misses, the twin against the oracle on every decided pair, and the recorded floors against a fresh run of the twin."""
import numpy as np
import pytest
import torch

from oracle import durf_ref as R
from tests import ray_rows_ref as RR

F32, F64 = np.float32, np.float64


def _durf_ref_setup(o, d, pose, ext):
    """obbpose_model.py:99-131 through oracle/durf_ref.py in float64"""
    o, d, pose, ext = (torch.from_numpy(np.asarray(x, F32)).double() for x in (o, d, pose, ext))
    B, K = o.shape[0], pose.shape[0]
    mat = R.aa2matrix(pose[:, 3:]).expand(B, K, 3, 3)
    oo, do = R.world2object_rpy(o, d, pose[:, :3].expand(B, K, 3), mat)
    dims = ext.expand(B, K, 3)
    _, zo, inter = R.ray_box_intersection(oo, do, -dims, dims)
    f = inter.double()
    bk = (inter.sum(-1) == 0).double()
    return ((oo * f[..., None]).sum(-2) + bk[:, None] * o, (do * f[..., None]).sum(-2) + bk[:, None] * d, inter, (f * zo).sum(-1))


@pytest.mark.parametrize('name', list(RR.GENERIC_CASES))
def test_oracle_is_the_reference_restated(name):
    c = RR.generic(name)
    ref = RR.ray_setup(c['o'], c['d'], c['pose'], c['ext'])
    o_s, d_s, inter, zo = _durf_ref_setup(c['o'], c['d'], c['pose'], c['ext'])
    pairs, rays = RR.decided(ref)
    assert np.array_equal(inter.numpy()[pairs], ref['hit'][pairs])
    for got, want, scale in ((o_s, 'o_s', 's_o'), (d_s, 'd_s', 's_d'), (zo, 'zo', 's_z')):
        err = np.abs(got.numpy() - ref[want]).reshape(RR.RAYS, -1).max(1) / ref[scale].reshape(RR.RAYS, -1).max(1)
        assert float(err[rays].max()) < 1e-13, (want, float(err[rays].max()))
    Rm = RR.aa2matrix(c['pose'][:, 3:])
    assert float(np.abs(Rm - R.aa2matrix(torch.from_numpy(c['pose'][:, 3:]).double()).numpy()).max()) < 1e-15
    assert float(np.abs(Rm @ Rm.transpose(0, 2, 1) - np.eye(3)).max()) < 1e-9       # a rotation, in every class


def test_oracle_of_the_other_stages_is_the_reference_restated():
    for N in (1, 2, 31):
        for lindisp in (False, True):
            near, far = np.full(3, 0.05, F32), np.full(3, 1e4, F32)
            tr = RR.t_rand_of('random', 3, N)
            for t_rand in (None, tr):
                want, _ = R.sample_along_rays(None if t_rand is None else torch.from_numpy(t_rand), torch.zeros(3, 3, dtype=torch.float64),
                                              torch.ones(3, 3, dtype=torch.float64), torch.ones(3, 1, dtype=torch.float64), N,
                                              torch.from_numpy(near).double()[:, None], torch.from_numpy(far).double()[:, None],
                                              t_rand is not None, lindisp)
                got = RR.sample_t(near, far, N, t_rand, lindisp)
                # (durf_ref's grid is torch.linspace's, i * (1 / N): an ulp from the kernel's i / N unless N is a power of two)
                assert float(np.abs(got / want.numpy() - 1).max()) < (1e-14 if N < 3 else 3e-7)
    v = RR.view_inputs(40)
    assert float(np.abs(RR.pos_enc(v) - R.pos_enc(torch.from_numpy(v).double(), 0, 4).numpy()).max()) < 1e-15
    assert RR.pos_enc(v).shape == (40, 27)
    assert float(RR.HALF_PI_F32) == float(F32(0.5 * np.pi)) and abs(float(RR.HALF_PI_F32) - 0.5 * np.pi) < 2.0 ** -24
    x = np.array([1.0, 1.00390625, 1.01171875, -1.00390625, 3.0e-39], F32)      # exact, tie to even (down, up), negative tie
    assert RR.bf16_rne(x).tolist()[:4] == [0x3F80, 0x3F80, 0x3F82, 0x3F80 - 0x8000]
    assert np.array_equal(RR.bf16_rne(x), torch.from_numpy(x).bfloat16().view(torch.int16).numpy())


# ---------------------------------------------------------------------------
# the hand-aimed table
# ---------------------------------------------------------------------------
def test_zero_rotation_is_exactly_the_identity():
    pose, _, _ = RR.table_scene()
    assert not pose[:, 3:].any()
    for dt in (F32, F64):
        Rm = RR.aa2matrix(pose[:, 3:], dt)
        assert np.array_equal(Rm, np.broadcast_to(np.eye(3, dtype=dt), Rm.shape)) and not np.signbit(Rm).any()


def _dyadic(x):
    return bool(np.array_equal(np.asarray(x, F64) * 1024, np.round(np.asarray(x, F64) * 1024)))


@pytest.mark.parametrize('K', RR.TABLE_KS)
@pytest.mark.parametrize('masked', [True, False])
def test_table_literals_are_the_oracles_and_the_twin_is_exact(K, masked):
    pose, ext, enable = RR.table_scene()
    T = RR.table()
    assert _dyadic(pose) and _dyadic(ext) and _dyadic(T['o']) and _dyadic(T['d'])
    axis = (T['d'] != 0).sum(1) == 1
    assert int(axis.sum()) == len(T['names']) - 2 and int(np.signbit(T['d'][axis]).sum(1).max()) == 3
    en = enable[:K] if masked else None
    ref, twin = (RR.ray_setup(T['o'], T['d'], pose[:K], ext[:K], en, dt) for dt in (F64, F32))
    want = (T['want'] if masked else T['want_all'])[:, :K]
    for i, name in enumerate(T['names']):
        assert ref['hit'][i].tolist() == want[i].tolist(), name
        assert twin['hit'][i].tolist() == want[i].tolist(), name
        for key in ('o_s', 'd_s', 'zo') + (('tn', 'tf') if axis[i] else ()):
            assert RR.same_bits(twin[key][i], ref[key][i]), (name, key)
        if not axis[i]:                      # the grazing diagonals: tf == tn against box 0 in either precision
            assert ref['tf'][i, 0] == ref['tn'][i, 0] and twin['tf'][i, 0] == twin['tn'][i, 0], name
        zo = RR.TABLE_ZO.get(name.replace(' (-0.0)', ''))
        if zo is not None and zo[0] == K:
            assert RR.same_bits(F32(zo[1]), ref['zo'][i]), (name, ref['zo'][i])
    if K == 16:
        assert enable[5] == 0 and T['want'][:, 5].sum() == 0 and T['want_all'][:, 5].sum() == 2      # the switched-off box
        # the cases the table is for
        assert (want.sum(1) == 2).any() and (want.sum(1) == 3).any() and (want[:, [0, 15]].sum(1) == 2).any()
        assert np.isnan(ref['tf'][:, 0]).sum() == 4 and (ref['tf'][:, 0] == 0).sum() == 2      # the NaN path; tf == 0
        assert np.isinf(ref['tf'][:, 0]).sum() == 2


# ---------------------------------------------------------------------------
# the generic cases
# ---------------------------------------------------------------------------
def test_tau_is_four_times_the_measured_distance():
    tau = RR.measure_tau()
    assert 4 * tau <= RR.TAU <= 6 * tau, (tau, RR.TAU)


def test_generic_cases_cover_the_classes_and_sizes():
    assert {len(c) for c in RR.GENERIC_CASES.values()} == {1, 3, 16}
    assert {cl for c in RR.GENERIC_CASES.values() for cl in c} == set(RR.ROTATIONS)
    for name, classes in RR.GENERIC_CASES.items():
        rot = RR.generic(name)['pose'][:, 3:].astype(F64)
        for k, cl in enumerate(classes):
            n2 = float((rot[k] ** 2).sum())
            assert {'zero': n2 == 0, 'below': 0 < n2 < 1e-12, 'one': abs(n2 - 1) < 1e-6, 'near_pi': 0 < np.pi - n2 ** 0.5 < 2e-3,
                    'above_pi': abs(n2 - 16) < 1e-5}[cl], (name, k, cl, n2)


@pytest.mark.parametrize('masked', [False, True])
@pytest.mark.parametrize('name', list(RR.GENERIC_CASES))
def test_generic_case_conditions(name, masked):
    c = RR.generic(name)
    en = c['enable'] if masked else None
    on = np.ones(len(c['enable']), bool) if en is None else c['enable'] != 0
    ref, twin = (RR.ray_setup(c['o'], c['d'], c['pose'], c['ext'], en, dt) for dt in (F64, F32))
    pairs, rays = RR.decided(ref)
    assert float(1 - pairs[:, on].mean()) <= 0.01
    assert np.array_equal(twin['hit'][pairs], ref['hit'][pairs]), 'the twin agrees with the oracle on every decided pair'
    frac = float(ref['hit'][:, on].mean())
    assert 0.2 <= frac <= 0.8, frac
    if len(on) > 1:
        assert int((ref['dyn'] >= 2).sum()) >= 1 and not ref['hit'][:, ~on].any()
    inside = (np.abs(ref['tn'][:RR.INSIDE]) > 0) & (ref['tn'][:RR.INSIDE] < 0) & (ref['hit'][:RR.INSIDE] == 1)
    assert masked or inside.any(1).all(), 'the first rays start inside a box'
    assert np.isfinite(ref['zo']).all() and np.isfinite(twin['zo']).all()


def test_recorded_floors_are_the_float32_twins():
    """FLOOR / T_FLOOR / VIEW_FLOOR of tests/test_gpu_ray_edges.py against a fresh run of the twin (within a factor of 1.5 either way:
    the figure moves with the host's libm), and a device figure recorded for every case"""
    from tests import test_gpu_ray_edges as T
    keys = {(n, m) for n in RR.GENERIC_CASES for m in (0, 1)}
    assert set(T.FLOOR) == keys and set(T.MEASURED) == keys
    for key in keys:
        now = RR.setup_floor(*key)
        for a, r, m in zip(now, T.FLOOR[key], T.MEASURED[key]):
            assert r / 1.5 <= a <= r * 1.5, (key, now, T.FLOOR[key])
            assert m <= 4 * r, (key, m, r)
    tkeys = {(i, l, k) for i in list(range(len(RR.NEAR_FAR))) + ['inf'] for l in (0, 1) for k in RR.T_RANDS if i != 'inf' or l}
    assert set(T.T_FLOOR) == tkeys and set(T.T_MEASURED) == tkeys
    for key in tkeys:
        now = RR.t_floor(RR.NEAR_FAR_INF if key[0] == 'inf' else RR.NEAR_FAR[key[0]], key[1], key[2])
        assert abs(now - T.T_FLOOR[key]) <= 0.01 + 0.02 * now, (key, now, T.T_FLOOR[key])      # (no libm in this one)
        assert T.T_MEASURED[key] <= 4 * T.T_FLOOR[key], key
    assert T.VIEW_FLOOR / 1.5 <= RR.view_floor() <= T.VIEW_FLOOR * 1.5 and T.VIEW_MEASURED <= 4 * T.VIEW_FLOOR + RR.VIEW_SHIFT


# ---------------------------------------------------------------------------
# the integer oracle and the patterns
# ---------------------------------------------------------------------------
def test_compaction_oracle_on_a_case_done_by_hand():
    hit = np.array([[1, 0, 0], [0, 0, 0], [7, -1, 0], [0, 0, 1], [1, 1, 1]], np.int32)
    r = RR.compact_ref(hit, 4)
    assert r['count'].tolist() == [3, 2, 2] and [i.tolist() for i in r['idx']] == [[0, 2, 4], [2, 4], [3, 4]]
    assert r['slot'].tolist() == [[0, -1, -1], [-1, -1, -1], [1, 0, -1], [-1, -1, 0], [2, 1, 1]]
    assert r['dyn'].tolist() == [1, 0, 2, 1, 3]
    assert r['ccount'].tolist() == [3, 2, 3 * 4 + 2, 2, 0b111] and [i.tolist() for i in r['cidx']] == [[1, 2, 4], [0, 3]]
    assert r['cslot'].tolist() == [[-1, 0], [0, -1], [1, -1], [-1, 1], [2, -1]]
    for p in RR.PATTERNS:
        for B in (1, 1025):
            h = RR.hit_pattern(p, B, 16, value=-1)
            assert set(np.unique(h)) <= {0, -1}
            assert {'zeros': not h.any(), 'ones': h.all(), 'first': h[0].all() and h.sum() == -16,
                    'last': h[B - 1].all() and h.sum() == -16, 'round_edge': h.sum() == (-32 if B > 1024 else 0)}.get(p, True), p
    assert RR.compact_ref(RR.hit_pattern('ones', 3, 16), 1)['ccount'].tolist() == [3, 0, 3, 3, 0xFFFF]
    src = RR.shuffled_copies(3000, 256, 1)
    assert len(src) == 3000 and set(src) == set(range(256)) and len(RR.shuffled_copies(63, 256, 1)) == 63
