"""Prints what tests/test_gpu_ray_edges.py and tests/ray_rows_ref.py record from the CPU: TAU's measurement, the float32 twin's
floors of the ray setup, the sample positions and the view encoding, and the balance of every generic case.
Run from the repository root: python tests/scripts/ray_rows_floors.py"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from tests import ray_rows_ref as RR  # noqa: E402

if __name__ == '__main__':
    tau = RR.measure_tau()
    print('measure_tau() = %.2e -> TAU >= %.2e (recorded %.2e)' % (tau, 4 * tau, RR.TAU))
    for name in RR.GENERIC_CASES:
        c = RR.generic(name)
        for masked in (False, True):
            ref = RR.ray_setup(c['o'], c['d'], c['pose'], c['ext'], c['enable'] if masked else None)
            pairs, rays = RR.decided(ref)
            on = np.ones(len(c['enable']), bool) if not masked else c['enable'] != 0
            print("    ('%s', %d): (%s),   # hits %.2f undecided %.4f multi-hit rays %d" % (
                name, masked, ', '.join('%.1e' % f for f in RR.setup_floor(name, masked)), ref['hit'][:, on].mean(),
                1 - pairs.mean(), int((ref['dyn'] >= 2).sum())))
    for i, pair in enumerate(RR.NEAR_FAR):
        for lindisp in (0, 1):
            for kind in RR.T_RANDS:
                print("    (%d, %d, '%s'): %.2f," % (i, lindisp, kind, RR.t_floor(pair, lindisp, kind)))
    for kind in RR.T_RANDS:
        print("    ('inf', 1, '%s'): %.2f," % (kind, RR.t_floor(RR.NEAR_FAR_INF, 1, kind)))
    print('VIEW_FLOOR = %.1e' % RR.view_floor())
