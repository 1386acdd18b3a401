"""include/durf_shade.h on the host: the oracle against itself -- the any-hit walk of the implicit tree equals the definition by
brute force in every integer, whatever the order of the build; float32 against the float64 twin under a written-down margin;
the properties a shaded picture rests on; the 8-bit rule; and durf_amd/shade.py's checks, none of which needs a device."""
import os
import re

import numpy as np
import pytest
import torch

from durf_amd import _lib, shade
from tests import cast_ref as R, shade_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


@pytest.mark.parametrize('name', ['ground_n257', 'ground_S65', 'ground_contact', 'ground_inf', 'ground_bias0', 'ground_cull1', 'soup_T1025',
                                  'duplicates_300', 'sheets_one_ulp_bias0', 'dirty', 'odd_directions', 'reach_below_t', 'reach_at_t', 'reach_above_t'])
def test_the_walk_equals_brute_force_whatever_the_order(name):
    c, (used, blocked) = S.cases()[name], S.expected(name)
    T = c['t'].shape[0]
    orders = dict(morton=R.morton_order(c['v'], c['t']), random=np.random.default_rng(7).permutation(T).astype(np.int32), identity=np.arange(T, dtype=np.int32))
    for which, order in orders.items():
        u, b = S.occlusion32(c['v'], c['t'], c['points'], c['normals'], c['dirs'], c['bias'], c['reach'], c['cull'], order=order)
        assert np.array_equal(u, used) and np.array_equal(b, blocked), (name, which, np.argwhere(b != blocked)[:5])


def test_the_big_case_by_the_walk_equals_brute_force_on_its_first_samples():
    c, (used, blocked) = S.big_case()
    u, b = S.occlusion32(c['v'], c['t'], c['points'][:48], c['normals'][:48], c['dirs'], c['bias'], c['reach'])
    assert np.array_equal(u, used[:48]) and np.array_equal(b, blocked[:48]) and int(blocked.sum()) > 1000


# float32 against float64: the icosphere resting on the ground, 2000 samples on each of three seeds, 64 directions.  A pair whose
# margin (occlusion64) is at most 1e-4 is excused; section 14's cap of 0.5 % bounds the share of excused pairs.  Uniform samples
# stay under the cap on this scene (the shares are in the docstring below), so the samples are uniform over the faces, not
# pulled away from the edges.
MARGIN, CAP = 1e-4, 0.005


@pytest.mark.parametrize('seed', [0, 1, 2])
def test_float32_agrees_with_float64_beyond_the_margin(seed):
    """Measured here on the CPU, excused share of the 128 000 pairs per seed: see the printed line (DESIGN.md 17 records them)."""
    v, t = S.sphere_on_ground()
    dirs, reach = S.fibonacci(64), 0.5
    tri, bary = S.face_samples(v, t, 2000, 100 + seed)
    p, nr = S.surface32(v, t, tri, bary)
    _, o, used32 = S._pairs32(p, nr, dirs, reach / 1024.0)
    i, s = np.nonzero(used32)
    hit = R.cast32(v, t, o[i], dirs[s], 0.0, reach)[0] >= 0
    blocked32 = np.zeros(used32.shape, bool)
    blocked32[i, s] = hit
    twin = S.occlusion64(v, t, p, nr, dirs, reach / 1024.0, reach)
    judged = twin['margin'] > MARGIN
    share = 1.0 - judged.mean()
    print('seed %d: %d of %d pairs excused (%.4f %%), %d used, %d blocked' % (seed, int((~judged).sum()), judged.size, 100 * share, int(used32.sum()), int(blocked32.sum())))
    assert share <= CAP, share
    assert np.array_equal(used32[judged], twin['used'][judged])
    assert np.array_equal(blocked32[judged], twin['blocked'][judged]), np.argwhere((blocked32 != twin['blocked']) & judged)[:5]
    assert int(blocked32.sum()) > 2000                                        # the contact shadow is there


def test_a_closed_surface_from_outside_and_from_inside():
    v, t = R.icosphere(2)
    dirs = S.fibonacci(64)
    tri, bary = S.face_samples(v, t, 400, 5)
    p, nr = S.surface32(v, t, tri, bary)
    reach = 0.5
    # outside, the sphere alone: nothing blocks a direction that leaves a convex surface
    used, blocked = S.occlusion32(v, t, p, nr, dirs, reach / 1024.0, reach)
    twin = S.occlusion64(v, t, p, nr, dirs, reach / 1024.0, reach)
    sure = (twin['margin'] > MARGIN).all(1)
    assert sure.sum() > 300 and (blocked[sure] == 0).all() and (used[sure] > 16).all()
    # inside with no limit: every used direction meets the surface
    used, blocked = S.occlusion32(v, t, p, -nr, dirs, 1.0 / 1024.0, np.inf)
    twin = S.occlusion64(v, t, p, -nr, dirs, 1.0 / 1024.0, np.inf)
    sure = (twin['margin'] > MARGIN).all(1)
    assert sure.sum() > 300 and np.array_equal(blocked[sure], used[sure]) and (used[sure] > 16).all()


def test_samples_that_are_no_surface_give_nothing():
    v, t = S.flat_and_sliver()
    tri = np.asarray([0, 1, 2, 3, 4, 5, 6, -1, -2, 7, 2 ** 31 - 1], np.int32)
    bary = np.tile(np.asarray([[0.5, 0.25, 0.25]], F32), (len(tri), 1))
    bary[8] = np.nan                                                         # what a cast writes beside tri = -2
    p, nr = S.surface32(v, t, tri, bary, toward=np.tile(np.asarray([[0.0, 0.0, 1.0]], F32), (len(tri), 1)))
    assert np.array_equal(nr[0], [0, 0, -1]) and np.array_equal(p[0], [0.25, 0.25, 0])      # faces the viewer
    dead = [1, 2, 4, 5, 7, 8, 9, 10]                                         # flat, repeated vertex, NaN vertex, bad index, -1, -2, t >= T
    assert not nr[dead].any() and not p[[4, 5, 7, 8, 9, 10]].any() and np.isfinite(p).all()
    assert np.abs(np.linalg.norm(nr[[3, 6]].astype(np.float64), axis=1) - 1).max() < 2e-7     # slivers still have a normal
    used, blocked = S.occlusion32(v, t, p, nr, S.fibonacci(32), 0.01, np.inf)
    assert not used[dead].any() and not blocked[dead].any() and used[0] > 0
    bad = p.copy()
    bad[0, 1] = np.inf                                                       # a point that is not finite is not live either
    assert S.occlusion32(v, t, bad, nr, S.fibonacci(32), 0.01, np.inf)[0][0] == 0
    out, out8 = S.compose32(tri, nr, used, blocked, (0, 0, -1), 0.25, (0.5, 1.0, 0.0))
    assert np.array_equal(out[[7, 8]], np.tile(np.asarray([[0.5, 1.0, 0.0]], F32), (2, 1))) and np.array_equal(out8[7], [128, 255, 0])
    # a sample on a triangle without area is no background: it has no normal, so it gets the ambient term alone
    assert np.array_equal(out[[1, 4]], np.full((2, 3), 0.25, F32))


def test_compose_8_bit_is_torch_round_of_the_clamped_float():
    rng = np.random.default_rng(3)
    n = 4096
    nr = S.random_samples(n, 4)[1]
    used = rng.integers(0, 65, n)
    blocked = (used * rng.random(n)).astype(np.int64)
    tri = rng.integers(-2, 50, n)
    albedo = rng.uniform(-0.2, 1.4, (n, 3)).astype(F32)
    albedo[::97, 1] = np.nan
    albedo[5::101] = np.asarray([0.5 / 255.0 * 1.0, 1.5 / 255.0, 2.5 / 255.0], F32)      # ties of the rounding where shade is 1
    for ambient, sun in ((0.0, None), (1.0, None), (0.4, rng.integers(0, 2, n))):
        out, out8 = S.compose32(tri, nr, used, blocked, (0.0, 0.6, 0.8), ambient, (1.0, 0.5, 0.0), sun_blocked=sun, albedo=albedo)
        x = torch.from_numpy(out)
        want = torch.round(torch.nan_to_num(x, nan=0.0).clamp(0, 1) * 255).to(torch.uint8).numpy()
        assert np.array_equal(out8, want)
        assert np.array_equal(out8, shade.to_u8(x).numpy())
    assert np.array_equal(S.u8([0.5 / 255, 1.5 / 255, 2.5 / 255, np.nan, -1, 2]), [0, 2, 2, 0, 0, 255])


def test_the_generated_table_names_the_headers_entry_points():
    hdr = open(os.path.join(ROOT, 'include', 'durf_shade.h')).read()
    body = re.sub(r'/\*.*?\*/', ' ', hdr, flags=re.S)
    declared = set(re.findall(r'\b(durf_[a-z0-9_]+)\s*\(', body))
    from durf_amd import _shade_sigs
    assert declared == set(_shade_sigs.SIGS) == {'durf_shade_surface', 'durf_shade_occlusion', 'durf_shade_compose', 'durf_shade_workspace_bytes',
                                                 'durf_shade_cameras'}
    assert _shade_sigs.DURF_SHADE_MAX_DIRS == shade.MAX_DIRS == 256 and 'shade' in _lib.SATELLITES
    assert len(_lib.symbols()) == 118                                        # libdurf_hip.so keeps its entry points


def test_directions_are_unit_and_reproducible():
    for n in (1, 2, 3, 64, 256):
        d = shade.directions(n)
        assert d.dtype == np.float32 and d.shape == (n, 3) and np.array_equal(d, shade.directions(n)) and np.array_equal(d, S.fibonacci(n))
        assert np.abs(np.linalg.norm(d.astype(np.float64), axis=1) - 1.0).max() <= 2.0 ** -23
    d = shade.directions(64)
    assert np.abs(d.astype(np.float64).mean(0)).max() < 1.0 / 64             # evenly spread: the mean of a spiral of S points is O(1 / S)
    assert not np.array_equal(shade.directions(64, seed=1), d)
    assert len({tuple(x) for x in d.tolist()}) == 64


def test_every_argument_error_is_a_valueerror_with_no_device():
    b = dict(ws=0, T=1, V=3, vertices=0, triangles=0)
    z, z3 = np.zeros(4, np.float32), np.zeros((4, 3), np.float32)
    zi = np.zeros(4, np.int32)
    cam = np.zeros((1, 17), np.float32)
    bad = [
        (lambda: shade.directions(0), 'shade.directions'), (lambda: shade.directions(257), 'shade.directions'), (lambda: shade.directions(2.5), 'shade.directions'),
        (lambda: shade.directions(4, seed=0.5), 'shade.directions'),
        (lambda: shade.surface({}, zi, z3), 'shade.surface'), (lambda: shade.surface(b, zi, z), 'shade.surface'),
        (lambda: shade.surface(b, zi, z3, toward=z), 'shade.surface'),
        (lambda: shade.occlusion({}, z3, z3, 4, 1.0), 'shade.occlusion'), (lambda: shade.occlusion(b, z3, z3, 4, 0.0), 'shade.occlusion'),
        (lambda: shade.occlusion(b, z3, z3, 4, float('nan')), 'shade.occlusion'), (lambda: shade.occlusion(b, z3, z3, 4, float('inf')), 'shade.occlusion'),
        (lambda: shade.occlusion(b, z3, z3, 4, 1.0, bias=-1.0), 'shade.occlusion'), (lambda: shade.occlusion(b, z3, z3, 4, 1.0, bias=float('nan')), 'shade.occlusion'),
        (lambda: shade.occlusion(b, z3, z3, 4, 1.0, cull=3), 'shade.occlusion'), (lambda: shade.occlusion(b, z3, z3, 0, 1.0), 'shade.occlusion'),
        (lambda: shade.occlusion(b, z3, z3, 257, 1.0), 'shade.occlusion'), (lambda: shade.occlusion(b, z3, z3, np.zeros((4, 2)), 1.0), 'shade.occlusion'),
        (lambda: shade.occlusion(b, z3, z3, np.zeros((300, 3)), 1.0), 'shade.occlusion'), (lambda: shade.occlusion(b, z3, z, 4, 1.0), 'shade.occlusion'),
        (lambda: shade.compose(zi, z3, zi, zi, ambient=1.5), 'shade.compose'), (lambda: shade.compose(zi, z3, zi, zi, ambient=float('nan')), 'shade.compose'),
        (lambda: shade.compose(zi, z3, zi, zi, light=(0, 1)), 'shade.compose'), (lambda: shade.compose(zi, z3, zi, zi, light=(0, float('inf'), 0)), 'shade.compose'),
        (lambda: shade.compose(zi, z3, zi, zi, background=(0, float('nan'), 0)), 'shade.compose'), (lambda: shade.compose(zi, z, zi, zi), 'shade.compose'),
        (lambda: shade.compose(zi, z3, zi, zi[:2]), 'shade.compose'), (lambda: shade.compose(zi, z3, zi, zi, albedo=z), 'shade.compose'),
        (lambda: shade.compose(zi, z3, zi, zi, sun_blocked=z3), 'shade.compose'),
        (lambda: shade.cameras({}, cam), 'shade.cameras'), (lambda: shade.cameras(b, np.zeros((1, 5))), 'shade.cameras'),
    ]
    from durf_amd import camera
    from tests import camera_ref
    rows = camera.rows([camera_ref.look_at((0.0, 0.0, 3.0), (0.0, 0.0, 0.0))], 20.0, (4.0, 3.0), 6, 8)
    nan_row = rows.copy()
    nan_row[0, 3] = np.nan
    bad += [
        (lambda: shade.cameras(b, nan_row), 'shade.cameras'), (lambda: shade.cameras(b, rows, dirs=0, reach=1.0), 'shade.cameras'),
        (lambda: shade.cameras(b, rows, reach=-1.0), 'shade.cameras'), (lambda: shade.cameras(b, rows, reach=float('inf')), 'shade.cameras'),
        (lambda: shade.cameras(b, rows, reach=1.0, ambient=2.0), 'shade.cameras'), (lambda: shade.cameras(b, rows, reach=1.0, light=(0, 0, 0)), 'shade.cameras'),
        (lambda: shade.cameras(b, rows, reach=1.0, albedo=3), 'shade.cameras'), (lambda: shade.cameras(b, rows, reach=1.0, cull=5), 'shade.cameras'),
        (lambda: shade.cameras(b, rows, reach=1.0, tmin=-1.0), 'shade.cameras'), (lambda: shade.cameras(b, rows, reach=1.0, background=(1, 1)), 'shade.cameras'),
    ]
    for call, entry in bad:
        with pytest.raises(ValueError, match='^' + re.escape(entry) + ':'):
            call()
