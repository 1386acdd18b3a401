"""The box overlay without a device: tests/overlay_ref.py -- the float64 restatement the GPU tests hold csrc/overlay.hip to --
against the ray generator and the oracle's box test (so that it is the conventions that are checked, not a second copy of
the same formulas), its edge numbering, culling, cutting and rectangle on hand-made boxes, the cap on undecided pixels for
every GPU case, and the argument handling of durf_amd/overlay.py."""
import numpy as np
import pytest
import torch

from oracle import durf_ref as R
from tests import overlay_ref as O

F64 = np.float64


def test_corners_satisfy_the_oracles_box_test():
    rng = np.random.default_rng(1)
    K = 5
    poses = np.concatenate([rng.uniform(-3, 3, (1, K, 3)), rng.normal(size=(1, K, 3))], -1)
    poses[0, 0, 3:] = 0.0
    ext = rng.uniform(0.2, 1.0, (K, 3))
    P = O.world_corners(poses, ext, F64)[0]                              # [K,8,3]
    rot = R.aa2matrix(torch.tensor(poses[0, :, 3:]))
    np.testing.assert_allclose(O.aa2matrix(poses[0, :, 3:], F64), rot.numpy(), atol=1e-14)
    for k in range(K):
        for _ in range(20):
            wts = rng.dirichlet(np.ones(8)) * 0.98 + 0.02 / 8            # strictly inside the hull of the eight corners
            target = wts @ P[k]
            o = target + rng.normal(size=3) * 4.0
            while np.all(np.abs(rot[k].numpy() @ (o - poses[0, k, :3])) <= ext[k]):    # an origin outside the box
                o = target + rng.normal(size=3) * 4.0
            d = (target - o) * rng.uniform(0.2, 3.0)
            B = 1
            oo, do = R.world2object_rpy(torch.tensor(o[None]), torch.tensor(d[None]), torch.tensor(poses[0, :, :3]).expand(B, K, 3),
                                        rot.expand(B, K, 3, 3))
            dims = torch.tensor(ext).expand(B, K, 3)
            _, _, hit = R.ray_box_intersection(oo, do, -dims, dims)
            assert int(hit[0, k]) == 1, (k, hit)
    # and a corner pushed outward is outside: a ray through it along the box's own axis misses
    k = 1
    out = poses[0, k, :3] + 1.05 * (P[k, 7] - poses[0, k, :3])
    axis_w = rot[k].numpy().T @ np.array([0.0, 0.0, 1.0])
    oo, do = R.world2object_rpy(torch.tensor((out - 5 * axis_w)[None]), torch.tensor(axis_w[None]),
                                torch.tensor(poses[0, :, :3]).expand(1, K, 3), rot.expand(1, K, 3, 3))
    assert int(R.ray_box_intersection(oo, do, -torch.tensor(ext).expand(1, K, 3), torch.tensor(ext).expand(1, K, 3))[2][0, k]) == 0


def test_edge_numbering():
    ec = O.edge_corners()
    assert ec.tolist() == [[0, 1], [2, 3], [4, 5], [6, 7], [0, 2], [1, 3], [4, 6], [5, 7], [0, 4], [1, 5], [2, 6], [3, 7]]
    for e, (a, b) in enumerate(ec):
        assert (a ^ b) == 1 << (e // 4) and a < b


# a camera at the origin looking along the world's -z, x to the right, y up: picture x = ppx + f X / (-Z), y = ppy - f Y / (-Z)
CAM = O.camera_row(np.concatenate([np.eye(3), np.zeros((3, 1))], 1), 40.0, 26.0, 18.0, 37, 53).astype(F64)[None]


def hand_box(centre, ext=(1.0, 0.5, 0.25), znear=0.5, enable=None):
    poses = np.zeros((1, 1, 6))
    poses[0, 0, :3] = centre
    return O.project_boxes(CAM, poses, np.array([ext]), enable, znear, F64)


def test_box_in_front():
    seg, rect = hand_box((0.0, 0.0, -8.0))
    assert np.isfinite(seg).all()
    # edge 0 joins corner 0 (-,-,-) to corner 1 (+,-,-): Z = -8.25, the far face
    np.testing.assert_allclose(seg[0, 0, 0], [26 - 40 / 8.25, 18 + 20 / 8.25, 26 + 40 / 8.25, 18 + 20 / 8.25], atol=1e-12)
    # edge 11 joins corner 3 (+,+,-) to corner 7 (+,+,+): from the far face to the near one
    np.testing.assert_allclose(seg[0, 0, 11], [26 + 40 / 8.25, 18 - 20 / 8.25, 26 + 40 / 7.75, 18 - 20 / 7.75], atol=1e-12)
    np.testing.assert_allclose(rect[0, 0], [26 - 40 / 7.75, 18 - 20 / 7.75, 26 + 40 / 7.75, 18 + 20 / 7.75, 8.0, 1.0], atol=1e-12)


def test_box_straddling_znear():
    seg, rect = hand_box((0.0, 0.0, -0.6), ext=(1.0, 0.5, 0.25))        # depths 0.35 .. 0.85 around znear = 0.5
    culled = np.isnan(seg[0, 0]).all(1)
    assert np.isnan(seg[0, 0]).any(1).tolist() == culled.tolist()        # a segment is NaN whole or not at all
    # corners with bit 2 set have Z = -0.35 (nearer than znear): the four edges among them (axis 0 and 1, j = 2, 3) are culled
    assert culled.tolist() == [False, False, True, True, False, False, True, True, False, False, False, False]
    # the four z-edges run from depth 0.85 (kept) to 0.35: cut at 0.5, x and y are constant along them
    for j, (sx, sy) in enumerate(((-1, -1), (1, -1), (-1, 1), (1, 1))):
        np.testing.assert_allclose(seg[0, 0, 8 + j], [26 + 40 * sx / 0.85, 18 - 20 * sy / 0.85, 26 + 40 * sx / 0.5, 18 - 20 * sy / 0.5], atol=1e-12)
    # the rectangle: the cut ends reach 26 +- 80 and 18 +- 40, outside the 37 x 53 picture on every side
    np.testing.assert_allclose(rect[0, 0], [0.0, 0.0, 52.0, 36.0, 0.6, 1.0], atol=1e-12)


def test_box_behind_and_disabled():
    seg, rect = hand_box((0.0, 0.0, 5.0))
    assert np.isnan(seg).all() and np.isnan(rect[0, 0, :4]).all() and rect[0, 0, 5] == 0.0 and rect[0, 0, 4] == -5.0
    seg, rect = hand_box((0.0, 0.0, -8.0), enable=[0])
    assert np.isnan(seg).all() and np.isnan(rect[0, 0, :4]).all() and rect[0, 0, 5] == 0.0 and rect[0, 0, 4] == 8.0


def test_box_off_screen():
    seg, rect = hand_box((30.0, 0.0, -8.0))
    assert np.isfinite(seg).all() and seg[0, 0, :, 0].min() > 52.0        # every edge is kept, right of the picture
    assert np.isnan(rect[0, 0, :4]).all() and rect[0, 0, 5] == 0.0 and rect[0, 0, 4] == 8.0


def test_box_around_the_camera():
    seg, rect = hand_box((0.0, 0.0, 0.0), ext=(1.0, 1.0, 2.0))
    culled = np.isnan(seg[0, 0]).all(1)
    # only the face Z = -2 is in front: its four edges whole, the z-edges cut, the face Z = +2 culled
    assert culled.tolist() == [False, False, True, True, False, False, True, True, False, False, False, False]
    np.testing.assert_allclose(seg[0, 0, 8], [26 - 20, 18 + 20, 26 - 80, 18 + 80], atol=1e-12)
    np.testing.assert_allclose(rect[0, 0], [0.0, 0.0, 52.0, 36.0, 0.0, 1.0], atol=1e-12)


def test_zero_length_segment_and_owner_rule():
    seg = np.full((1, 2, 12, 4), np.nan, np.float32)
    seg[0, 1, 0] = (3.0, 2.0, 3.0, 2.0)                                   # a point, box 1
    seg[0, 0, 5] = (0.0, 2.0, 6.0, 2.0)                                   # a horizontal line through it, box 0
    d = O.box_distances(seg, 5, 7, F64)
    assert d[0, 1, 2, 3] == 0.0 and d[0, 1, 2, 4] == 1.0 and abs(d[0, 1, 1, 2] - np.sqrt(2.0)) < 1e-15
    lab = O.owners(d, 0.75)
    assert (lab[0, 2] == 0).all() and (lab[0, [0, 1, 3, 4]] == -1).all()   # the lowest box wins where both are within reach
    assert O.owners(d[:, 1:], 0.75)[0].tolist()[2] == [-1, -1, -1, 0, -1, -1, -1]


@pytest.mark.parametrize('name', [c[0] for c in O.GPU_CASES])
def test_gpu_cases_hold_the_cap_on_undecided_pixels(name):
    """The condition the rasteriser tests rest on, on float64 alone: pixels where some box's distance lies within EDGE (4 x the
    fp32 twin's largest distance error, at least 1e-4 px) of the half width are at most 5 % of the drawn pixels, for every case
    and width tests/test_gpu_overlay.py runs -- here on the float64 projection's segments rounded to fp32."""
    c = O.gpu_case(name)
    seg, rect = O.project_boxes(c['cams'], c['poses'], c['ext'], c['enable'], c['znear'], F64)
    finite = seg[np.isfinite(seg)]
    assert finite.size and np.abs(finite).max() < 1e4
    for width in c['widths']:
        ref = O.raster_reference(seg.astype(np.float32), c['h'], c['w'], width / 2.0)
        print('%s width %.1f: drawn %d, undecided %d (%.2f %%), EDGE %.2e' % (name, width, ref['drawn'].sum(), ref['undecided'].sum(),
                                                                            100 * ref['share'], ref['edge']))
        assert ref['drawn'].sum() > 0
        assert ref['share'] <= 0.05, (name, width, ref['share'])


def test_gpu_cases_contain_the_special_poses():
    c = O.gpu_case('k8')
    seg, rect = O.project_boxes(c['cams'], c['poses'], c['ext'], c['enable'], c['znear'], F64)
    kinds = {n: k for k, n in enumerate(O.SPECIAL)}
    assert (c['poses'][:, kinds['zero_rot'], 3:] == 0).all()
    assert abs(np.linalg.norm(c['poses'][0, kinds['near_pi'], 3:]) - np.pi) < 2e-3
    s = seg[0, kinds['straddle']]
    assert np.isnan(s).all(1).any() and np.isfinite(s).all(1).any() and rect[0, kinds['straddle'], 5] == 1.0
    assert np.isnan(seg[:, kinds['behind']]).all() and (rect[:, kinds['behind'], 5] == 0).all()
    assert np.isfinite(seg[:, kinds['offscreen']]).all() and (rect[:, kinds['offscreen'], 5] == 0).all()
    e = seg[0, kinds['edge_on']]
    assert ((e[:, 0] == e[:, 2]) & (e[:, 1] == e[:, 3])).any()             # an edge seen end-on: a segment of length zero
    assert np.isnan(seg[:, kinds['disabled']]).all() and (rect[:, kinds['disabled'], 5] == 0).all()
    assert (rect[:, [kinds['zero_rot'], kinds['near_pi']], 5] == 1).all()


def test_overlay_arguments():
    from durf_amd import overlay
    assert overlay.PALETTE.shape == (16, 3) and overlay.PALETTE.dtype == np.uint8
    assert len({tuple(c) for c in overlay.PALETTE.tolist()}) == 16
    cams = np.zeros((2, 17), np.float32)
    with pytest.raises(ValueError, match='poses'):
        overlay.project_boxes(cams, torch.zeros(2, 3, 5), torch.zeros(3, 3))
    with pytest.raises(ValueError, match='at most 16'):
        overlay.project_boxes(cams, torch.zeros(2, 17, 6), torch.zeros(17, 3))
    with pytest.raises(ValueError, match='cams'):
        overlay.project_boxes(cams[:1], torch.zeros(2, 3, 6), torch.zeros(3, 3))
    with pytest.raises(ValueError, match='ext'):
        overlay.project_boxes(cams, torch.zeros(2, 3, 6), torch.zeros(4, 3))
    with pytest.raises(ValueError, match='znear'):
        overlay.project_boxes(cams, torch.zeros(2, 3, 6), torch.zeros(3, 3), znear=0.0)
    seg = torch.zeros(2, 3, 12, 4)
    with pytest.raises(ValueError, match='frames'):
        overlay.draw_boxes(torch.zeros(2, 5, 7, dtype=torch.uint8), seg)
    with pytest.raises(ValueError, match='uint8 or float32'):
        overlay.draw_boxes(torch.zeros(2, 5, 7, 3, dtype=torch.float64), seg)
    with pytest.raises(ValueError, match='segments'):
        overlay.draw_boxes(torch.zeros(3, 5, 7, 3, dtype=torch.uint8), seg)
    with pytest.raises(ValueError, match='segments'):
        overlay.draw_boxes(torch.zeros(2, 5, 7, 3, dtype=torch.uint8), torch.zeros(2, 3, 12, 2))
    with pytest.raises(ValueError, match='at most 16'):
        overlay.draw_boxes(torch.zeros(2, 5, 7, 3, dtype=torch.uint8), torch.zeros(2, 17, 12, 4))
    with pytest.raises(ValueError, match='colors'):
        overlay.draw_boxes(torch.zeros(2, 5, 7, 3, dtype=torch.uint8), seg, colors=np.zeros((2, 3), np.uint8))
    with pytest.raises(ValueError, match='opacity'):
        overlay.draw_boxes(torch.zeros(2, 5, 7, 3, dtype=torch.uint8), seg, opacity=1.5)
    with pytest.raises(ValueError, match='poses'):
        overlay.overlay_trajectory(dict(rgb8=torch.zeros(2, 35, 3, dtype=torch.uint8)), cams, torch.zeros(3, 3))


def test_symbols_are_declared_bound_and_exported_by_a_library_of_their_own():
    """libdurf_overlay.so has the two entry points (that its header, its table and its symbol table name the same ones, and no
    other library does: tests/test_satellites_host.py); refusals need no device and are read from libdurf_hip.so's
    durf_last_error."""
    from durf_amd import _lib, ops
    assert {'durf_project_boxes', 'durf_draw_boxes'} == set(_lib.overlay_symbols())
    L = _lib.overlay_lib()
    assert ops.BOX_EDGES == O.EDGES                    # (the constants against the header: tests/test_headers_host.py)
    assert ops.BOX_RECT_FLOATS == len(ops.BOX_RECT_FIELDS)
    assert L.durf_project_boxes(None, 1, 17, None, None, None, None, 0.5, None, None) != 0
    assert b'durf_project_boxes' in _lib.lib().durf_last_error() and b'DURF_MAX_OBJ' in _lib.lib().durf_last_error()
    assert L.durf_project_boxes(None, 0, 3, None, None, None, None, 0.5, None, None) == 0          # F * K == 0: nothing to do
    assert L.durf_draw_boxes(None, 0, 4, 4, 3, None, None, 0.75, 1.0, None, None, None) == 0
    assert L.durf_draw_boxes(None, 1, 4, 4, 3, None, None, 0.75, 1.0, None, None, None) != 0
    assert b'at least one' in _lib.lib().durf_last_error()
