"""The conditions tests/test_gpu_enc_edges.py relies on, held on the CPU: the engineered rays of tests/enc_rows_ref.py land
in their classes, nothing in-domain is excluded, the float64 truth wraps as the reference does, and the float32 twin's
yardstick written into that module is what a fresh run gives."""
import math

import numpy as np
import torch

from oracle import durf_ref as R
from tests import enc_rows_ref as E


def test_every_class_is_populated_and_nothing_in_domain_is_excluded():
    pop, share = E.classify()
    print('samples per class:', pop)
    assert set(pop) == set(E.CLASSES) and all(n > 0 for n in pop.values()), pop
    assert share == 0.0
    # the declared out-of-domain rows: the two-hit ray, only where hit columns exist, between in-domain neighbours
    for g in E.GROUPS:
        dom = E.in_domain(g)
        bad = [i for i in range(E.B) if not dom[i]]
        assert bad == (E.rays_of('hit2') if g[0] == 'bkgd' and g[2] else []), g
    i = E.rays_of('hit2')[0]
    assert E.LABELS[i - 1] == 'plain' and E.LABELS[i + 1] == 'plain'
    assert E.B * E.N % 32 == 0


def test_the_branch_switch_rays_share_waves():
    lo, hi = E.rays_of('switch_lo'), E.rays_of('switch_hi')
    assert [h - l for l, h in zip(lo, hi)] == [1] * 4 and all(l % 2 == 0 for l in lo)      # N = 32: rays 2i, 2i + 1 = one wave
    t = E.encode(('bkgd', 0, 0, None))
    for rows, sign in ((lo, -1), (hi, 1)):
        a = t['x'][rows].abs().amax(-1)
        assert bool(((a - E.SWITCH) * sign > 2e-5).all())
    x = t['x'][lo + hi]
    assert bool((x.amin(-1) < -3.99).any()) and bool((x.amax(-1) > 3.99).any()), 'both signs'


def test_the_truth_wraps_by_the_float32_period():
    # the oracle in float32 IS the reference's wrap: the remainder by the float32-rounded 100 pi
    y = torch.tensor([400.0, -400.0, 1e5, -1e5, 314.16, -314.16, 314.159], dtype=torch.float32)
    want = torch.sin(torch.tensor(np.where(np.abs(y.numpy()) < np.float32(E.T32), y.numpy(),
                                           np.remainder(y.numpy(), np.float32(E.T32)))))
    assert torch.equal(R.safe_sin(y), want)
    # in float64 the oracle's own period is the double 100 pi: 5.9e-6 rad per wrap away from the reference's
    assert abs((E.T32 - 100 * math.pi) - 5.9e-6) < 1e-7
    y64 = y.double()
    with E._reference_wrap():
        got = R.safe_sin(torch.cat([y64, y64]))[:7]
    assert float((got - want.double()).abs().max()) < 1e-6               # float32 sine of an exactly wrapped argument
    q = torch.floor(y64[2] / E.T32)
    assert abs(float(R.safe_sin(y64)[2] - got[2])) > 0.9 * 5.9e-6 * float(q) * abs(math.cos(float(y64[2]) - float(q) * E.T32))
    assert R.safe_sin is not None and R.safe_sin(y64).dtype == torch.float64       # (the swap is undone)
    # the wrap classes: arguments on both sides of +-T32, sine and cosine, for several degrees
    t = E.encode(('bkgd', 0, 0, None))
    rows = E.rays_of('wrap')
    _, _, _, yy = E.conditioning(t['x'][rows], t['var'][rows])
    for deg in (0, 4, 9):
        for arg in (yy, yy + E.HALF_PI32):
            a = arg[..., deg * 3 + deg % 3]
            for sign in (1, -1):
                r = sign * a / E.T32
                assert bool(((r > 0.996) & (r < 1)).any()) and bool(((r > 1) & (r < 1.004)).any()), (deg, sign)


def test_the_yardstick_is_the_float32_twins_distance():
    fresh = E.twin_distance()
    assert set(fresh) == set(E.YARDSTICK)
    for k, (dx, dv) in fresh.items():
        print('%-22s dx %.2f ulp  dvar %.1e' % (k, dx, dv))
        wx, wv = E.YARDSTICK[k]
        assert dx <= wx + 1e-9 and dx >= wx - 0.011, (k, dx, wx)          # written rounded up to 0.01 ulp
        assert dv <= wv and dv >= 0.9 * wv - 1e-12, (k, dv, wv)           # written 5 % up, two digits
    assert max(v[0] for v in E.YARDSTICK.values()) < 6, 'no label is ill-conditioned enough to make its gate vacuous'


def test_the_budgets_are_finite_and_the_controls_are_visible():
    for g in (('bkgd', 0, 0, None), ('bkgd', 1, 3, None), ('obj', 2, 0, 4.5)):
        t = E.encode(g)
        b = E.bounds(g, t)
        dom = E.in_domain(g)
        for k in ('cond', 'small', 'big'):
            assert bool(torch.isfinite(b[k][dom]).all()) and bool((b[k][dom] >= 0).all()), (g, k)
        assert bool(torch.isfinite(t['enc'][dom]).all())
    # exact BARF patterns: alpha 4.5 -> weights 1 1 1 1 .5 0 ..., alpha 0 -> all 0, alpha 10 -> all 1
    w = lambda a: R.barf_weights(a, 10, torch.float64)
    assert torch.allclose(w(4.5), torch.tensor([1, 1, 1, 1, .5, 0, 0, 0, 0, 0], dtype=torch.float64), atol=1e-15)
    assert bool((w(0.0) == 0).all()) and bool((w(10.0) == 1).all())
