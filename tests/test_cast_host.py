"""include/durf_cast.h on the host: the proof exercised (the numpy walk of the implicit tree equals brute force in every bit),
the box rule's monotonicity, the float32 definition against its float64 twin, watertightness measured, the key rule, and the
library's refusals (every argument is checked before anything is launched, so they need no device)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from durf_amd import _lib
from durf_amd import _cast_sigs as S
from tests import cast_ref as R, mesh_ref

U = 2.0 ** -24
F32 = np.float32


@pytest.mark.parametrize('name', sorted(R.scenes()))
def test_the_walk_of_any_tree_equals_brute_force_in_every_bit(name):
    s, want = R.scenes()[name], R.expected(name)
    T = s['t'].shape[0]
    orders = (('morton', R.morton_order(s['v'], s['t'])), ('random', np.random.default_rng(3).permutation(T)), ('identity', np.arange(T)))
    for what, order in orders[:1 if s['o'].shape[0] > 1000 else 3]:      # (the largest scene: the walk it is timed with)
        got = R.bvh32(s['v'], s['t'], order, s['o'], s['d'], s['tmin'], s['tmax'], s['cull'])
        for k, a, b in zip(('tri', 't', 'bary'), got, want):
            assert np.array_equal(R.bits(a), R.bits(b)), (name, what, k)
    hit = R.bvh32(s['v'], s['t'], R.morton_order(s['v'], s['t']), s['o'], s['d'], s['tmin'], s['tmax'], s['cull'], any_hit=True)
    assert np.array_equal(hit, np.where(want[0] >= 0, 1, np.where(want[0] == -2, -2, 0)))


def walk_counts():
    """per scene and query, over the Morton order: [node boxes tested, leaves entered] summed over the scene's rays"""
    out = {'nearest': {}, 'any': {}}
    for name, s in sorted(R.scenes().items()):
        order = R.morton_order(s['v'], s['t'])
        for what in out:
            stats = {}
            R.bvh32(s['v'], s['t'], order, s['o'], s['d'], s['tmin'], s['tmax'], s['cull'], any_hit=what == 'any', stats=stats)
            out[what][name] = [int(stats['nodes'].sum()), int(stats['leaves'].sum())]
    return out


def test_the_walk_visits_what_it_visited_before_the_walks_were_merged():
    """the outputs cannot show a changed traversal (the header proves them independent of it); the counts can.
    tests/golden/tree_walk_stats.json holds walk_counts() of this file and of tests/test_closest_host.py as the two separate
    walks gave them, before cast_ref.tree_walk32 replaced both loops"""
    assert walk_counts() == json.load(open(os.path.join(os.path.dirname(__file__), 'golden', 'tree_walk_stats.json')))['cast']


def test_the_scenes_reach_what_they_are_for():
    e = R.expected
    for T in R.TRIANGLE_COUNTS + R.BUILD_EDGES:                              # every build is cast at with rays that hit it
        tri = e('soup_T%d' % T)[0]
        assert len(tri) >= 5 and not (tri == -2).any()
        if T == 0:
            assert (tri == -1).all()
        else:
            assert (tri >= 0).sum() >= len(tri) // 2 and (tri == -1).any() and len(set(tri[tri >= 0].tolist())) >= min(T, 3) - 1, T
    for n in R.RAY_COUNTS:
        tri = e('soup_T300_n%d' % n)[0]
        assert len(tri) == n and (n == 0 or (tri >= 0).sum() >= (n + 1) // 2), n
    assert set(e('duplicates_300')[0].tolist()) == {-1, 0} and (e('duplicates_300')[0] == 0).sum() > 10      # the tie goes to the lowest id
    sheets = e('sheets_one_ulp')[0]
    # from above the upper sheet (id 0) is nearer or ties; from below the lower (id 1) wins unless the two t round to one value
    assert (sheets[:40] == 0).all() and set(sheets[40:].tolist()) == {0, 1}
    bad = e('bad_rays')
    assert bad[0].tolist() == [-2] * 7 + [0] and np.isnan(bad[1][:7]).all() and np.isnan(bad[2][:7]).all()
    tri = e('bounds_at_t')[0].reshape(6, -1)
    hit = R.cast32(*[R.scenes()['bounds_at_t'][k] for k in ('v', 't')], R.scenes()['bounds_at_t']['o'][:48], R.scenes()['bounds_at_t']['d'][:48])[0] >= 0
    assert hit.sum() > 10
    assert (tri[0][hit] >= 0).all() and (tri[1][hit] >= 0).all() and (tri[4][hit] >= 0).all() and (tri[5][hit] >= 0).all()   # a bound at t counts
    assert not np.array_equal(tri[2][hit], tri[1][hit]) and not np.array_equal(tri[3][hit], tri[4][hit])     # one ulp inside t: another answer
    dirty = e('dirty')[0]
    assert not set(dirty.tolist()) & {3, 7, 11, 12, 13, 20, 21, 22}          # degenerate and invalid triangles never win
    grid = {c: e('grid_cull%d' % c)[0] for c in (0, 1, 2)}
    assert ((grid[1] >= 0) | (grid[2] >= 0)).sum() == (grid[0] >= 0).sum() and not ((grid[1] >= 0) & (grid[2] >= 0)).any()
    assert (e('random_T5000_n3000')[0] >= 0).sum() > 2000


def test_the_box_rule_is_monotone_under_enlarging_the_box():
    rng = np.random.default_rng(17)
    n = 100000
    lo = rng.normal(size=(n, 3)).astype(F32)
    hi = (lo + np.abs(rng.normal(size=(n, 3))) * rng.choice([0.0, 1e-3, 1.0], (n, 3))).astype(F32)       # flat boxes on a third of the axes
    grow = lambda: (np.abs(rng.normal(size=(n, 3))) * rng.choice([0.0, 1e-6, 1.0], (n, 3))).astype(F32)
    lo2, hi2 = lo - grow(), hi + grow()
    lo2, hi2 = np.where(rng.random((n, 3)) < 0.2, np.nextafter(lo, -R.INF), lo2), np.where(rng.random((n, 3)) < 0.2, np.nextafter(hi, R.INF), hi2)
    assert (lo2 <= lo).all() and (hi <= hi2).all()
    o = (rng.normal(size=(n, 3)) * 2).astype(F32)
    face = rng.random((n, 3))
    o = np.where(face < 0.15, lo, np.where(face < 0.3, hi, np.where(face < 0.4, lo2, o))).astype(F32)       # origins on faces
    d = rng.normal(size=(n, 3)).astype(F32)
    kind = rng.random((n, 3))
    d = np.where(kind < 0.2, F32(0), np.where(kind < 0.3, F32(1e-42) * np.sign(d), np.where(kind < 0.35, F32(3e-39) * np.sign(d), d))).astype(F32)
    tmin = np.where(rng.random(n) < 0.5, 0, np.abs(rng.normal(size=n))).astype(F32)
    tmax = np.where(rng.random(n) < 0.5, np.inf, tmin + np.abs(rng.normal(size=n)) * 3).astype(F32)
    r = R.ray_setup(o, d, tmin, tmax)
    us = r['usable']
    assert us.sum() > 0.9 * n and (r['zero'].sum(0) > 0.2 * n).all()
    small, bn, bf = R.box_rule(lo, hi, r['o'], r['inv'], r['zero'], r['tmin'], r['tmax'])
    large, bn2, bf2 = R.box_rule(lo2, hi2, r['o'], r['inv'], r['zero'], r['tmin'], r['tmax'])
    assert 0.02 * n < (small & us).sum() < 0.98 * n
    assert not (small & ~large & us).any()                                   # no triple passes the small box and fails the large one
    assert (bn2[us] <= bn[us]).all() and (bf2[us] >= bf[us]).all() and not np.isnan(bn[us]).any() and not np.isnan(bf[us]).any()


EXCUSED_CAP = 0.005       # the share of rays float64 cannot call: measured 0, 0.001 and 0 on the three seeds below


@pytest.mark.parametrize('seed', [21, 22, 23])
def test_float32_against_its_float64_twin_on_the_sphere(seed):
    v, t = R.icosphere(2)
    rng = np.random.default_rng(seed)
    o = (3 * rng.normal(size=(4000, 3))).astype(F32)
    o[:1000] *= F32(0.1)                                                    # a quarter of the origins inside the sphere
    d = (rng.normal(size=(4000, 3)) * 0.7 - o).astype(F32)
    tri, t32, _ = R.cast32(v, t, o, d)
    c = R.cast64(v, t, o, d)
    hit = c['tri'] >= 0
    # float64 separates the two nearest candidates by 1e-4 t, the hit lies 1e-4 inside the winner's edges, and the winner's det
    # keeps a thousandth of its terms' magnitude; a ray float64 sees miss every triangle must miss in float32 by the same margin
    rel_gap = np.where(np.isfinite(c['gap']), c['gap'] / np.maximum(np.abs(c['t']), 1e-30), np.inf)
    clear = (rel_gap > 1e-4) & (c['edge'] > 1e-4) & (c['cancel'] > 1e-3)
    excused = hit & ~clear
    assert excused.mean() <= EXCUSED_CAP, excused.mean()
    judged = hit & clear
    assert judged.sum() > 2500 and np.array_equal(tri[judged], c['tri'][judged])
    # t within four times the float32 formula's own first-order error (cast64's err32); measured: 0.27 of it at most
    factor = np.abs(t32[judged].astype(np.float64) - c['t'][judged]) / c['err32'][judged]
    print('seed %d: excused %d of %d, factor %.3f' % (seed, excused.sum(), hit.sum(), factor.max()))
    assert factor.max() <= 4.0
    near_miss = R.cast64(v * F32(1 + 1e-4), t, o, d)['tri'] >= 0               # a slightly larger sphere: misses it too
    assert (tri[~hit & ~near_miss] == -1).all()


def _inside_rays(n, seed, centre, spread):
    rng = np.random.default_rng(seed)
    return (np.asarray(centre) + spread * (rng.random((n, 3)) - 0.5)).astype(F32), rng.normal(size=(n, 3)).astype(F32)


def test_watertightness_is_measured_not_promised():
    """the rays of a fixed seeded set, cast from inside a closed surface, that the definition says hit nothing: pinned as the
    oracle gives them (DESIGN section 14 records them)"""
    v, t = R.icosphere(3)
    assert mesh_ref.is_closed(t)
    tri = R.cast32(v, t, *_inside_rays(4000, 11, (0, 0, 0), 0.6))[0]
    assert int((tri == -1).sum()) == 0 and not (tri == -2).any()
    frame = mesh_ref.unit_frame(0.25, (-2.0, -2.0, -2.0))
    s = mesh_ref.surface(mesh_ref.sphere_field(frame, (17, 17, 17), (0.03, 0.01, -0.02), 1.4), None, 0.0, frame, dt=np.float32, normals=False)
    assert mesh_ref.is_closed(s['triangles']) and s['triangles'].shape[0] == 3492
    tri = R.cast32(s['vertices'], s['triangles'], *_inside_rays(4000, 12, (0.03, 0.01, -0.02), 0.8))[0]
    assert int((tri == -1).sum()) == 0 and not (tri == -2).any()


def test_keys_follow_the_headers_rule():
    v = np.asarray([(0, 0, 0), (0, 0, 0), (0, 0, 0), (1, 2, 4), (1, 2, 4), (1, 2, 4), (1, 0, 0), (1, 0, 0), (1, 0, 0), (0, 2, 0), (0, 0, 4),
                    (0.5, 1, 2), (np.nan, 0, 0)], F32)
    t = np.asarray([(0, 1, 2), (3, 4, 5), (6, 7, 8), (9, 9, 9), (10, 10, 10), (11, 11, 11), (0, 1, 12), (0, 1, 13), (3, 3, 3)], np.int32)
    k = R.keys(v, t, [0, 0, 0, 1, 2, 4])
    ones = lambda axis: sum(1 << (3 * b + (2 - axis)) for b in range(21))
    assert k[0] == 0 and k[1] == 2 ** 63 - 1 and k[2] == ones(0) and k[3] == ones(1) and k[4] == ones(2)
    assert k[5] == (1 << 62) | (1 << 61) | (1 << 60)                        # the middle: 2^20 on each axis
    assert k[6] == k[7] == np.iinfo(np.int64).max and k[8] == k[1]          # invalid: a NaN vertex, an index out of range
    assert (R.keys(v, t, [0, 0, 0, 1, 0, 4])[:6] & ones(1) == 0).all()      # a zero-extent axis gives 0
    assert (R.keys(v, t, [2, 3, 5, 1, 2, 4])[:6] == 0).all()                # a negative extent too
    assert S.DURF_CAST_KEY_BITS == R.KEY_BITS and S.DURF_CAST_LEAF == R.LEAF and S.DURF_CAST_STACK == R.STACK
    o = R.morton_order(*R.dirty_mesh())
    assert sorted(o.tolist()) == list(range(200)) and set(o[-6:].tolist()) == {11, 12, 13, 20, 21, 22}       # the invalid sort last


def test_the_workspace_is_what_the_header_lays_out():
    L = _lib.cast_lib()
    up = lambda x: (x + 255) // 256 * 256
    for T in (1, 4, 5, 1023, 1024, 1025, 4097, 10 ** 7):
        n, nodes = (T + 3) // 4, 0
        n0 = n
        while True:
            nodes += n
            if n == 1:
                break
            n = (n + 1) // 2
        assert L.durf_cast_workspace_bytes(T) == up(n0 * 4 * 4 * S.DURF_CAST_RECORD_FLOATS) + up(nodes * 4 * S.DURF_CAST_NODE_FLOATS), T
    assert L.durf_cast_workspace_bytes(0) == 256
    assert L.durf_cast_workspace_bytes(-1) == 0 and L.durf_cast_workspace_bytes(S.DURF_CAST_MAX_TRIANGLES) == 0
    assert L.durf_cast_workspace_bytes(S.DURF_CAST_MAX_TRIANGLES - 1) > 40 * (S.DURF_CAST_MAX_TRIANGLES - 1)


def test_every_refusal_by_its_message():
    """none of these launches anything: the pointers are never followed"""
    L = _lib.cast_lib()
    P, ws = 0x10000, 0x20000                                                 # a pointer that is not NULL; one aligned to 256 bytes
    need = L.durf_cast_workspace_bytes(8)
    inf = float('inf')

    def refused(rc, text):
        assert rc != 0
        msg = _lib.lib().durf_last_error().decode()
        assert text in msg, (text, msg)
    refused(L.durf_cast_keys(None, -1, 8, P, P, P, P), 'V >= 0, V = -1')
    refused(L.durf_cast_keys(None, 3, -1, P, P, P, P), 'T = -1')
    refused(L.durf_cast_keys(None, 3, S.DURF_CAST_MAX_TRIANGLES, P, P, P, P), 'T = %d' % S.DURF_CAST_MAX_TRIANGLES)
    refused(L.durf_cast_keys(None, 3, 8, None, P, P, P), 'vertices for V = 3')
    refused(L.durf_cast_keys(None, 3, 8, P, None, P, P), 'triangles for T = 8')
    refused(L.durf_cast_keys(None, 3, 8, P, P, None, P), 'bounds and keys')
    refused(L.durf_cast_keys(None, 3, 8, P, P, P, None), 'bounds and keys')
    refused(L.durf_cast_build(None, 3, 8, P, P, None, ws, need), 'order for T = 8')
    refused(L.durf_cast_build(None, 3, 8, P, P, P, None, need), 'workspace aligned to 256 bytes')
    refused(L.durf_cast_build(None, 3, 8, P, P, P, ws + 4, need), 'workspace aligned to 256 bytes')
    refused(L.durf_cast_build(None, 3, 8, P, P, P, ws, need - 1), 'workspace of %d bytes, durf_cast_workspace_bytes(8) = %d' % (need - 1, need))
    rays = lambda **kw: L.durf_cast_rays(None, kw.get('n', 4), kw.get('o', P), kw.get('d', P), kw.get('tmin_rays'), kw.get('tmax_rays'),
                                         kw.get('tmin', 0.0), kw.get('tmax', inf), kw.get('cull', 0), kw.get('T', 8), kw.get('ws', ws),
                                         kw.get('bytes', need), kw.get('tri', P), kw.get('t', P), kw.get('bary'))
    refused(rays(n=-1), 'n >= 0, n = -1')
    refused(rays(T=-2), 'T = -2')
    refused(rays(cull=3), 'cull in 0 .. 2, cull = 3')
    refused(rays(tmin=-1.0), 'tmin >= 0, tmin = -1')
    refused(rays(tmin=float('nan')), 'tmin >= 0')
    refused(rays(tmax=float('nan')), 'tmax is a number')
    refused(rays(o=None), 'origins and directions')
    refused(rays(d=None), 'origins and directions')
    refused(rays(tri=None), 'outputs for n = 4')
    refused(rays(t=None), 'outputs for n = 4')
    refused(rays(ws=None), 'workspace aligned')
    refused(rays(bytes=need - 256), 'durf_cast_workspace_bytes(8)')
    refused(rays(T=100), 'durf_cast_workspace_bytes(100)')                      # a workspace sized for another tree
    assert rays(n=0, o=None, d=None, tri=None, t=None) == 0                 # no rays: success, no launch
    assert rays(n=0, tmin=-1.0, tmin_rays=P, o=None, d=None, tri=None, t=None) == 0       # a scalar bound that is not in use is not read
    any_ = lambda **kw: L.durf_cast_any(None, kw.get('n', 4), P, P, None, None, kw.get('tmin', 0.0), 1.0, kw.get('cull', 0), 8, ws, need, kw.get('hit', P))
    refused(any_(hit=None), 'outputs for n = 4')
    refused(any_(cull=-1), 'cull = -1')
    refused(any_(tmin=-0.5), 'tmin = -0.5')
    cams = lambda **kw: L.durf_cast_cameras(None, kw.get('F', 2), kw.get('h', 4), kw.get('w', 4), kw.get('cams', P), kw.get('tmin', 0.0), inf,
                                            kw.get('cull', 0), 8, ws, kw.get('bytes', need), kw.get('tri', P), kw.get('depth', P), None)
    refused(cams(F=-1), 'F = -1')
    refused(cams(h=0), 'h = 0')
    refused(cams(w=0), 'w = 0')
    refused(cams(F=40000, h=300, w=300), 'F h w < 2^31')
    refused(cams(cams=None), 'cams_dev, tri and depth')
    refused(cams(depth=None), 'cams_dev, tri and depth')
    refused(cams(tmin=-1.0), 'tmin = -1')
    refused(cams(bytes=0), 'durf_cast_workspace_bytes(8)')
    assert cams(F=0, cams=None, tri=None, depth=None) == 0
    assert L.durf_cast_build(None, 0, 0, None, None, None, ws, 256) == 0     # T = 0 is legal: no launch
    assert L.durf_cast_keys(None, 0, 0, None, None, None, None) == 0


def test_the_host_module_refuses_before_it_touches_the_device():
    from durf_amd import cast
    v, t = R.quad_grid(2)
    for m, text in ((None, 'm is a dict'), (dict(vertices=v), 'm is a dict'), (dict(vertices=v.reshape(-1), triangles=t), 'expected [V,3] and [T,3]'),
                    (dict(vertices=v, triangles=t[:, :2]), 'expected [V,3] and [T,3]')):
        with pytest.raises(ValueError, match='cast.build') as e:
            cast.build(m)
        assert text in str(e.value)
    for kw, text in ((dict(tmin=-1.0), 'tmin = -1.0'), (dict(tmax=float('nan')), 'tmax = nan'), (dict(cull=3), 'cull = 3')):
        with pytest.raises(ValueError, match='cast.rays') as e:
            cast.rays({}, v, v, **kw)
        assert text in str(e.value)
    with pytest.raises(ValueError, match='cast.cameras'):
        cast.cameras({}, np.zeros((2, 5), F32))


def test_the_command_line_refuses_before_anything_is_read():
    from durf_amd import cast_mesh
    check = lambda *argv: cast_mesh.check_args(cast_mesh.build_parser().parse_args(list(argv) + ['--eval_dir', 'x']))
    assert check('--synthetic') is None
    assert check('--ply', 'a.ply', '--traj', 't.npz', '--focal', '50', '--size', '4', '6') is None
    assert check('--ply', 'a.ply', '--sweeps', 's.npy') is None
    assert check('--synthetic', '--frames', '0') == '--frames 0'
    assert '--ply is required' in check('--traj', 't.npz')
    assert 'one of --traj' in check('--ply', 'a.ply') and 'one of --traj' in check('--ply', 'a.ply', '--traj', 't', '--sweeps', 's')
    assert '--focal and --size' in check('--ply', 'a.ply', '--traj', 't.npz')
    assert check('--ply', 'a.ply', '--traj', 't.npz', '--focal', '0', '--size', '4', '6').startswith('--focal 0')
    assert check('--ply', 'a.ply', '--sweeps', 's.npy', '--ts', '2') == '--ts needs --poses'
    assert check('--synthetic', '--near', '2', '--far', '1').startswith('--near 2')
    assert check('--synthetic', '--beams', '0').startswith('--beams 0')
    with pytest.raises(SystemExit, match='cast_mesh: --ply is required'):
        cast_mesh.main(['--eval_dir', 'x'])
