"""The rasteriser's definition on the host (include/durf_raster.h through tests/raster_ref.py; no GPU): the float32 oracle the
library is held to bit for bit is itself held to float64, the tie rule is shown to partition, and the host side of
durf_amd.raster and the command line are exercised as far as they go without a device."""
import numpy as np
import pytest

from durf_amd import mesh, ops, raster, render_mesh
from tests import raster_ref as R

U = 2.0 ** -24                      # the unit roundoff of float32
SEED = 0                            # of R.random_scene: the gap rule leaves out at most 2 % of the covered pixels (asserted)


@pytest.fixture(scope='module')
def scene():
    cams, v, t = R.random_scene(SEED)
    return cams, v, t, R.draw32(cams, 48, 64, v, t, 0.5), R.draw64(cams, 48, 64, v, t, 0.5)


def test_draw32_against_draw64_on_the_random_scene(scene):
    """Both oracles share the snapped coordinates, so the coverage, the tallies and the candidates of every pixel are the
    same; they differ by float32 roundings alone, counted here to first order in u = 2^-24 (relative, on the depth).
      z of a vertex: each d_j = P_j - o_j one rounding, each product one, the two additions one each: every term of
        z = -sum_j R[j][2] d_j carries at most 4 u of itself, so |dz| <= 4 u sum_j |R[j][2] d_j| = 4 u gamma z, with gamma the
        cancellation factor of the scene, computed from the inputs in float64 (R.gamma).
      iz = 1 / z: 1.  w_i = (float) E_i / (float) |A2|: two conversions and a division, 3.  w_i iz_i: 1.  The two additions
        of positive terms: 2.  depth = 1 / s: 1.
    Total (4 gamma + 8) u; one more u covers the second-order terms: BOUND = (4 gamma + 9) u.
    Owner: with |d32 - d64| <= BOUND d64 for both candidates, the float32 order of the nearest two is the float64 order
    whenever d2 / d1 > (1 + BOUND) / (1 - BOUND), which (d2 - d1) / d1 > 3 BOUND guarantees for BOUND < 1/3: GAP = 3 BOUND."""
    cams, v, t, a, b = scene
    g = R.gamma(cams, v, t)
    bound = (4.0 * g + 9.0) * U
    gap = 3.0 * bound
    assert g < 64.0 and bound < 1e-4, (g, bound)
    assert np.array_equal(a['counts'], b['counts']) and np.array_equal(a['cover'], b['cover'])
    covered = b['tri'] >= 0
    assert np.array_equal(covered, a['tri'] >= 0) and covered.sum() > 3000
    sure = covered & (b['gap'] > gap)
    left_out = int(covered.sum() - sure.sum())
    print('gamma %.3f, bound %.3e, gap %.3e, covered %d, left out %d' % (g, bound, gap, covered.sum(), left_out))
    assert left_out <= 0.02 * covered.sum()
    assert np.array_equal(a['tri'][sure], b['tri'][sure])
    rel = np.abs(a['depth'][sure].astype(np.float64) - b['depth'][sure]) / b['depth'][sure]
    print('depth: max relative error %.3e' % rel.max())
    assert rel.max() <= bound
    # the weights: q_i = fl(wz_i depth), depth = fl(1 / s), s = fl(fl(wz_0 + wz_1) + wz_2): the exact sum of the q_i is 1 to within
    # one rounding of each q_i, the two of s and the one of depth, 4 u to first order
    q = a['bary'][covered].astype(np.float64)
    assert (q >= 0).all() and np.abs(q.sum(1) - 1.0).max() <= 4 * U * 1.001
    assert (a['depth'][~covered] == 0).all() and (a['bary'][~covered] == 0).all() and (a['tri'][~covered] == -1).all()
    # a list longer than one LDS batch: the scene stacks more than 600 triangles on one tile of the first camera
    assert a['counts'][0] > 0 and a['cover'][0, 16:32, 16:32].max() > 3
    assert a['counts'][1:].sum() == 3 * t.shape[0]


def _tiling_cover(pts, tris, h, w, focal=64.0, z=4.0):
    cam = R.camera(h, w, focal, pp=(0.0, 0.0))
    out = R.draw32(cam[None], h, w, R.to_world(cam, pts, z), tris, 0.5)
    assert out['counts'][1] == len(tris), out['counts']
    return out['cover'][0]


@pytest.mark.parametrize('rect', [(2.0, 3.0, 20.0, 17.0), (2.5, 3.5, 20.5, 16.5), (0.0, 0.0, 16.0, 16.0), (1.25, 2.0, 18.0, 19.75)])
def test_a_fan_and_a_grid_partition_their_rectangle(rect):
    """Triangles that tile a rectangle, with vertices on pixel centres, on half pixels and on quarter pixels, shared edges
    through pixel centres: every pixel of the rectangle is covered exactly once -- a count, not a minimum.  The rectangle
    itself owns the pixel centres with x0 < px <= x1 and y0 < py <= y1: of its four sides the rule admits the two with
    dY > 0, or dY == 0 and dX < 0, once it is oriented with A2 > 0 (the right and the bottom side)."""
    x0, y0, x1, y1 = rect
    h, w = 24, 26
    py, px = np.mgrid[0:h, 0:w]
    want = ((px > x0) & (px <= x1) & (py > y0) & (py <= y1)).astype(np.int64)
    assert want.sum() > 100
    cx, cy = np.floor((x0 + x1) / 2), np.floor((y0 + y1) / 2)                # a pixel centre: every spoke passes through some
    for name, (pts, tris) in (('fan', R.fan(x0, y0, x1, y1, cx, cy, 6)), ('fan, reversed', R.fan(x0, y0, x1, y1, cx, cy, 6)),
                              ('grid', R.grid(x0, y0, x1, y1, 6, 4)), ('grid, mixed windings', R.grid(x0, y0, x1, y1, 3, 7))):
        if 'reversed' in name:
            tris = tris[:, ::-1].copy()
        if 'mixed' in name:
            tris[::3] = tris[::3, ::-1]
        pts = np.round(pts * 256.0) / 256.0                                   # exactly representable: the snap moves nothing
        got = _tiling_cover(pts, tris, h, w)
        assert np.array_equal(got, want), (name, np.argwhere(got != want)[:5])


def test_merge_offsets_ids_and_places_objects():
    rng = np.random.default_rng(1)
    bg = dict(vertices=rng.normal(size=(5, 3)).astype(np.float32), triangles=np.array([[0, 1, 2], [2, 3, 4]], np.int32),
              normals=rng.normal(size=(5, 3)).astype(np.float32), rgb=np.full((5, 3), 255, np.uint8), owner=np.full(5, -1, np.int32))
    ob = dict(vertices=rng.normal(size=(4, 3)).astype(np.float32), triangles=np.array([[0, 1, 3]], np.int32),
              normals=rng.normal(size=(4, 3)).astype(np.float32), rgb=rng.random((4, 3)).astype(np.float32), owner=np.zeros(4, np.int32),
              component=np.zeros(4, np.int32))
    pose = np.array([1.0, -2.0, 0.5, 0.1, 0.7, -0.3])
    m = raster.merge([bg, ob], [None, pose])
    assert m['vertices'].dtype == np.float32 and m['triangles'].dtype == np.int32
    assert m['triangles'].tolist() == [[0, 1, 2], [2, 3, 4], [5, 6, 8]] and m['part'].tolist() == [0] * 5 + [1] * 4
    Rm = mesh.aa2matrix(pose[3:])
    assert np.allclose(m['vertices'][5:], pose[:3] + ob['vertices'].astype(np.float64) @ Rm, atol=1e-6)
    assert np.array_equal(m['vertices'][:5], bg['vertices'])
    # world -> object of the placed vertices gives the object's own coordinates back: P = R (X - c)
    assert np.allclose((m['vertices'][5:].astype(np.float64) - pose[:3]) @ Rm.T, ob['vertices'], atol=1e-5)
    assert np.allclose(m['normals'][5:], ob['normals'].astype(np.float64) @ Rm, atol=1e-6)
    assert np.allclose(m['rgb'][:5], 1.0) and m['owner'].tolist() == [-1] * 5 + [0] * 4 and 'component' not in m
    # the same through extract_scene's dict, and through (c, R)
    s = raster.merge(dict(background=bg, objects=[ob], poses=np.stack([np.zeros((1, 6)), pose[None]])), ts=1)
    assert np.array_equal(s['vertices'], m['vertices']) and np.array_equal(s['triangles'], m['triangles'])
    assert np.array_equal(raster.merge([bg, ob], [None, (pose[:3], Rm)])['vertices'], m['vertices'])
    with pytest.raises(ValueError, match='ts = 2 of 2'):
        raster.merge(dict(background=bg, objects=[ob], poses=np.zeros((2, 1, 6))), ts=2)
    with pytest.raises(ValueError, match='2 meshes and 1 poses'):
        raster.merge([bg, ob], [None])


def test_render_mesh_refuses_on_the_host_before_any_device_work():
    m = dict(vertices=np.zeros((3, 3), np.float32), triangles=np.array([[0, 1, 2]], np.int32), owner=np.zeros(3, np.int32))
    cam = R.camera(8, 8, 8.0)
    bad = [(dict(m={}), 'dict with vertices'),
           (dict(m=dict(m, vertices=np.zeros((3, 2), np.float32))), r'shape \(3, 2\)'),
           (dict(cams=np.zeros((2, 16), np.float32)), r'cams of shape \(2, 16\)'),
           (dict(cams=np.stack([cam, R.camera(8, 9, 8.0)])), 'share one frame size'),
           (dict(cams=R.camera(8, 5000, 8.0)), '8 x 5000'),
           (dict(cams=np.where(np.arange(17) == 3, np.nan, cam).astype(np.float32)), 'not finite'),
           (dict(znear=0.0), 'znear = 0.0'), (dict(znear=float('nan')), 'znear = nan'), (dict(znear=-1.0), 'znear = -1.0'),
           (dict(cull=3), 'cull = 3'), (dict(attrs='rgb'), "attrs = 'rgb'"),
           (dict(m=dict(m, owner=np.zeros(2, np.int32))), r"m\['owner'\] has 2 rows for 3 vertices"),
           (dict(frames_per_call=0), 'frames_per_call = 0')]
    for kw, msg in bad:
        args = dict(dict(m=m, cams=cam), **kw)
        with pytest.raises(ValueError, match=msg):
            raster.render_mesh(args.pop('m'), args.pop('cams'), **args)
    assert raster.default_frames_per_call(20, 3_000_000, 320, 480) == 5            # 40 bytes x 5 x 3e6 = 600 MB <= 1 GiB < 10 frames'
    assert raster.default_frames_per_call(20, 1000, 320, 480) == 20 and raster.default_frames_per_call(1, 10 ** 9, 8, 8) == 1
    assert raster.COUNT_FIELDS == ops.RASTER_COUNT_FIELDS == R.COUNT_FIELDS
    assert (ops.RASTER_SUBPIXEL, ops.RASTER_MAX_COORD, ops.RASTER_TILE, ops.RASTER_COUNTS) == (R.SUB, R.MAX_COORD, R.TILE, 8)


def test_depth_error_counts_and_measures():
    d = np.array([[0.0, 2.0, 4.0], [1.0, 0.0, 3.0]], np.float32)
    r = np.array([[5.0, 2.5, 4.0], [1.0, 2.0, np.nan]], np.float32)
    a = np.array([[1.0, 1.0, 0.9], [0.2, 1.0, 1.0]], np.float32)
    e = raster.depth_error(d, r, a)
    assert (e['pixels'], e['both'], e['mesh_only'], e['render_only']) == (6, 2, 2, 2)
    assert e['abs_mean'] == pytest.approx(0.25) and e['abs_max'] == pytest.approx(0.5) and e['rel_mean'] == pytest.approx(0.1)
    assert raster.depth_error(np.zeros((2, 2)), np.ones((2, 2)), np.ones((2, 2)))['abs_mean'] is None


def test_the_command_line():
    p = render_mesh.build_parser()
    a = p.parse_args(['--ply', 'a.ply', '--ply', 'b.ply', '--traj', 't.npz', '--focal', '100', '--size', '48', '64', '--eval_dir', 'out'])
    assert a.ply == ['a.ply', 'b.ply'] and a.size == [48, 64] and a.cull == 'none' and a.znear == 1e-2 and render_mesh.check_args(a) is None
    assert render_mesh.check_args(p.parse_args(['--synthetic', '--eval_dir', 'out'])) is None
    for argv, msg in ((['--eval_dir', 'o'], '--ply is required'), (['--ply', 'a.ply', '--eval_dir', 'o'], '--traj, --focal and --size'),
                      (['--ply', 'a.ply', '--traj', 't', '--focal', '0', '--size', '4', '4', '--eval_dir', 'o'], '--focal 0'),
                      (['--ply', 'a.ply', '--traj', 't', '--focal', '9', '--size', '4', '4', '--znear', '0', '--eval_dir', 'o'], '--znear 0'),
                      (['--ply', 'a.ply', '--traj', 't', '--focal', '9', '--size', '4', '4', '--ts', '2', '--eval_dir', 'o'], '--ts needs --poses'),
                      (['--synthetic', '--frames', '0', '--eval_dir', 'o'], '--frames 0')):
        with pytest.raises(SystemExit, match=msg):
            render_mesh.main(argv)
    with pytest.raises(SystemExit):
        p.parse_args(['--ply', 'a.ply'])                           # --eval_dir is required
