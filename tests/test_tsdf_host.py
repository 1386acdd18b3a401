"""The TSDF fusion's definition on the host (include/durf_tsdf.h through tests/tsdf_ref.py; no GPU): the float32 oracle the
library is held to bit for bit is itself held to float64, the fused sphere is where the sphere is, the properties the header
promises (split invariance, the weight clamp, rintf's ties) hold for the oracle, and the host side of durf_amd.tsdf and the
command line are exercised as far as they go without a device."""
import numpy as np
import pytest

from durf_amd import fuse_tsdf, mesh, tsdf
from tests import tsdf_ref as R

U = 2.0 ** -24                      # the unit roundoff of float32
SEED = 0                            # of R.random_scene: the margin rule leaves out at most 2 % of the updating pairs (asserted)
SPHERE_FRACTION = 0.3157            # measured below with integrate64: the worst zero crossing, in voxel steps
F32 = np.float32


def _all_inputs(s):
    return dict(acc=s['acc'], min_acc=0.1, rgb=s['rgb'], label=s['label'], select=1, other_mode=1, xform=s['xform'], frame_weight=s['frame_weight'])


def test_integrate32_against_integrate64_on_the_random_scene():
    """Both oracles read the same float32 inputs and differ by float32 roundings alone, counted to first order in u = 2^-24.
      P_j: three products and three additions, every term carries at most 4 u: |dP_j| <= 4 u mag(P_j), mag(P_j) = |origin_j| + i
        |du_j| + j |dv_j| + k |dw_j|.  X_c through the xform: three products, three additions on top: |dX_c| <= 9 u mag(X_c),
        mag(X_c) = sum_j |M[c][j]| mag(P_j) + |M[c][3]|.
      z = -sum_c R[c][2] (X_c - o_c): the subtraction, the product and the two additions, 4 u on every term, plus dX:
        |dz| <= 13 u G, G = sum_c |R[c][2]| (mag(X_c) + |o_c|), the cancellation factor, computed from the inputs below as its
        maximum over all frames and voxels.
      dn = min(sdf / trunc, 1), sdf = dep - z: where dn < 1, |sdf| <= trunc, so the subtraction and the division cost 2 u and
        |d dn| <= 13 u G / trunc + 2 u; min is 1-Lipschitz.
      D = (W D + wf dn) / Wn is a convex combination: it keeps the largest error of its terms and adds its own roundings (two
        products, the sum, the division, Wn: 4 u on values within [-1, 1]) and what the weights' own error does: W differs by at
        most f u relatively after f frames, which moves the combination by at most 2 f u.  Over F frames: (4 F + F (F + 1)) u.
      BOUND = (13 G / trunc + 2 + 4 F + F (F + 1)) u; the colour has the same recurrence on exact inputs: (4 F + F (F + 1)) u.
    Decisions: z and sdf are off by at most 13 u G + u (dep + z) =: EZ scene units; x = ppx + focal pc_0 / z by at most
    focal (13 u G (1 + T) / z) + 4 u (|x| + |ppx|) pixels with T = |pc_0| / z <= (max(h, w) + 1 + |pp|) / focal where it matters
    (near the frame) =: EX.  A pair is SURE when every margin integrate64 reports exceeds twice these."""
    s = R.random_scene(SEED)
    st = R.new_state(s['shape'])
    kw = _all_inputs(s)
    a = R.integrate32(st, s['frame'], s['shape'], s['cams'], s['depth'], s['trunc'], **kw)
    b = R.integrate64(st, s['frame'], s['shape'], s['cams'], s['depth'], s['trunc'], **kw)
    F, h, w = s['depth'].shape
    fr = {k: np.abs(np.asarray(s['frame'][k], np.float64)) for k in ('origin', 'du', 'dv', 'dw')}
    nu, nv, nw = s['shape']
    magP = fr['origin'] + (nu - 1) * fr['du'] + (nv - 1) * fr['dv'] + (nw - 1) * fr['dw']
    G = 0.0
    for f in range(F):
        M, c = np.abs(s['xform'][f].astype(np.float64)), s['cams'][f].astype(np.float64)
        magX = M[:, :3] @ magP + M[:, 3]
        G = max(G, float(np.abs(c[[2, 6, 10]]) @ (magX + np.abs(c[[3, 7, 11]]))))
    bound = (13.0 * G / s['trunc'] + 2.0 + 4.0 * F + F * (F + 1.0)) * U
    finite = np.isfinite(s['depth'])
    zmax = 2.0 * float(np.abs(s['cams'][:, [3, 7, 11]]).max() + magP.max())
    ez = (13.0 * G + float(s['depth'][finite].max()) + zmax) * U
    corners = R.voxels(s['frame'], s['shape'], np.float64).reshape(s['shape'] + (3,))[::nu - 1, ::nv - 1, ::nw - 1].reshape(8, 3)
    zmin = np.inf                                                            # z is linear in P: its least value is at a corner
    for f in range(F):
        M, c = s['xform'][f].astype(np.float64), s['cams'][f].astype(np.float64)
        zmin = min(zmin, float((-((corners @ M[:, :3].T + M[:, 3]) - c[[3, 7, 11]]) @ c[[2, 6, 10]]).min()))
    focal, pp = float(s['cams'][0, 12]), float(np.abs(s['cams'][:, 13:15]).max())
    ex = (focal * 13.0 * G * (1.0 + (max(h, w) + 1.0 + pp) / focal) / zmin + 4.0 * (max(h, w) + 1.0 + pp)) * U
    assert G < 32.0 and zmin > 1.0 and bound < 1e-4 and ex < 1e-3 and ez < 1e-4, (G, zmin, bound, ex, ez)
    m = b['margin']
    sure = (m[..., :2] > 2.0 * ex).all(-1) & (m[..., 2:] > 2.0 * ez).all(-1)
    updating = b['why'] == 0
    left_out = int((~sure).sum())
    print('G %.3f, bound %.3e, ex %.3e px, ez %.3e, pairs %d, updating %d, left out %d' % (G, bound, ex, ez, sure.size, updating.sum(), left_out))
    print('tallies', dict(zip(R.RULES, b['tally'].tolist())))
    assert updating.sum() > 5000 and left_out <= 0.02 * updating.sum()
    assert all(b['tally'][R.RULES.index(k)] > 100 for k in ('outside', 'hole', 'faint', 'occluded', 'other'))
    # the updated set and every skip tally agree on the sure pairs
    assert np.array_equal(a['why'][sure], b['why'][sure])
    for rule in range(len(R.RULES)):
        assert ((a['why'] == rule) & sure).sum() == ((b['why'] == rule) & sure).sum()
    vox = sure.all(0) & updating.any(0)                                      # a voxel with an unsure pair may have taken another path
    assert vox.sum() > 1500
    err = np.abs(a['tsdf'][vox].astype(np.float64) - b['tsdf'][vox]).max()
    cerr = np.abs(a['colour'][vox, :3].astype(np.float64) - b['colour'][vox, :3]).max()
    print('D: max error %.3e (%.1f u), colour %.3e (%.1f u)' % (err, err / U, cerr, cerr / U))
    assert err <= bound and cerr <= (4.0 * F + F * (F + 1.0)) * U
    assert np.abs(a['weight'][vox] - b['weight'][vox]).max() <= F * U * b['weight'][vox].max()
    assert a['tsdf'].dtype == F32 and a['colour'].dtype == F32 and np.abs(a['tsdf']).max() <= 1.0


def test_the_fused_sphere_is_where_the_sphere_is():
    """(The cameras are not a ring: a ring never looks at the poles, and the device test that carries this figure on draws its
    sphere from six cameras; so the sphere stands alone here, without its plane, seen from the six half axes, and the recorded
    0.3157 is this arrangement's alone.  The ring, the plane and the holes are the random scene's above.)
    A unit sphere seen by one camera on each half axis at distance 4 (64 x 64, focal 60, analytic depth), fused into 24^3
    voxels of step 3 / 23 with a band of two steps: the zero crossings on the seven edges mesh.surface puts vertices on lie
    within SPHERE_FRACTION = 0.3157 of a voxel step of the sphere -- the value measured here with integrate64 (mean 0.068, 99th
    percentile 0.27; the error is the projective distance's and the nearest pixel's, not the arithmetic's).  Asserted: twice
    that, which covers nearest-pixel depth from other cameras and meshes; tests/test_gpu_tsdf.py holds the device to the same."""
    N = 24
    step, shape = 3.0 / (N - 1), (N, N, N)
    frame = R.frame_of([-1.5] * 3, step)
    cams = R.six_cameras(64, 64, 60.0, 4.0)
    depth = R.sphere_depth(cams, 64, 64, plane=False)
    b = R.integrate64(R.new_state(shape, False), frame, shape, cams, depth, 2.0 * step)
    pts = R.crossings(b['tsdf'], b['weight'], R.voxels(frame, shape, np.float64), shape)
    err = np.abs(np.linalg.norm(pts, axis=1) - 1.0) / step
    print('crossings %d, max %.4f, mean %.4f, p99 %.4f of a step' % (len(pts), err.max(), err.mean(), np.percentile(err, 99)))
    assert len(pts) > 3000
    assert abs(err.max() - SPHERE_FRACTION) < 5e-4, 'the recorded measurement'
    assert err.max() <= 2.0 * SPHERE_FRACTION
    # every direction is covered: the crossings surround the centre
    assert (pts.min(0) < -0.9).all() and (pts.max(0) > 0.9).all()


def test_split_invariance_and_the_weight_clamp():
    s = R.random_scene(SEED + 1)
    kw = _all_inputs(s)
    kw.update(max_weight=2.0)
    args = (s['frame'], s['shape'])
    F = s['depth'].shape[0]

    def run(cuts):
        st = R.new_state(s['shape'])
        for f0, f1 in zip(cuts[:-1], cuts[1:]):
            per = {k: (v[f0:f1] if isinstance(v, np.ndarray) else v) for k, v in kw.items()}
            o = R.integrate32(st, *args, s['cams'][f0:f1], s['depth'][f0:f1], s['trunc'], **per)
            st = dict(tsdf=o['tsdf'], weight=o['weight'], colour=o['colour'])
        return st
    one = run([0, F])
    for cuts in ([0, 2, F], list(range(F + 1))):
        other = run(cuts)
        for k in ('tsdf', 'weight', 'colour'):
            assert np.array_equal(one[k].view(np.int32), other[k].view(np.int32)), (cuts, k)
    assert one['weight'].max() == 2.0 and (one['weight'] == 2.0).sum() > 100 and one['colour'][:, 3].max() == 2.0
    unclamped = R.integrate32(R.new_state(s['shape']), *args, s['cams'], s['depth'], s['trunc'], **dict(kw, max_weight=64.0))
    assert unclamped['weight'].max() > 2.0 and not np.array_equal(unclamped['tsdf'], one['tsdf'])


def tie_scene(w=8, h=6):
    """an identity camera with focal 1 and principal point (0, 0), and voxels at z = -1 whose x IS the pixel coordinate: the lattice
    has nu = 2 rows of nw points along x at -0.5, 0.5, 1.5 and w - 0.5, ... (step 1 from -0.5) -> frame, shape, cams, depth"""
    cams = R.camera(h, w, 1.0, pp=(0.0, 0.0))[None]
    frame = R.frame_of([0.0, 0.0, -1.0], axes=((0.0, 0.0, -1.0), (0.0, -1.0, 0.0), (1.0, 0.0, 0.0)))
    frame['origin'] = [-0.5, 0.0, -1.0]
    depth = (2.0 + np.arange(w, dtype=F32))[None, None, :].repeat(h, 1)      # depth says which pixel was read
    return frame, (2, 2, w + 2), cams, depth


def test_rintf_ties_go_to_even():
    """x = -0.5 reads pixel 0 (rintf(-0.5) = -0), 0.5 pixel 0, 1.5 pixel 2, w - 0.5 = 7.5 pixel 8: outside for w = 8"""
    w = 8
    frame, shape, cams, depth = tie_scene(w)
    o = R.integrate32(R.new_state(shape, False), frame, shape, cams, depth, 100.0)
    D, why = o['tsdf'].reshape(shape)[0, 0], o['why'][0].reshape(shape)[0, 0]
    read = D * F32(100.0) + F32(1.0) - F32(2.0)                              # sdf = dep - 1, dep = 2 + px
    assert np.allclose(read[:w], [0, 0, 2, 2, 4, 4, 6, 6], atol=1e-4), read
    assert why[:w].tolist() == [0] * w and why[w] == R.RULES.index('outside') and why[w + 1] == R.RULES.index('outside')


def test_box_xforms_against_aa2matrix():
    rng = np.random.default_rng(3)
    poses = rng.normal(size=(5, 3, 6))
    poses[2, 1, 3:] = 0.0                                                    # no rotation: the identity
    M = tsdf.box_xforms(poses, 1)
    assert M.shape == (5, 3, 4) and M.dtype == np.float32
    for f in range(5):
        Rm = mesh.aa2matrix(poses[f, 1, 3:])
        assert np.array_equal(M[f, :, :3], Rm.T.astype(np.float32)) and np.array_equal(M[f, :, 3], poses[f, 1, :3].astype(np.float32))
        P = rng.normal(size=3)                                               # X = c + R^T P, and R X' = P for X' = X - c
        assert np.allclose(Rm @ (M[f, :, :3].astype(np.float64) @ P), P, atol=1e-6)
    assert np.array_equal(M[2, :, :3], np.eye(3, dtype=np.float32))
    for bad in (dict(poses_fk6=poses, k=3), dict(poses_fk6=poses, k=-1), dict(poses_fk6=poses[0], k=0), dict(poses_fk6=poses[..., :5], k=0)):
        with pytest.raises(ValueError, match='tsdf.box_xforms'):
            tsdf.box_xforms(**bad)


def test_host_argument_checks():
    F, h, w = 2, 4, 5
    cams, depth = np.zeros((F, 17), np.float32), np.ones((F, h, w), np.float32)
    assert tsdf.check_frames(cams, depth) == (F, h, w)
    assert tsdf.check_frames(cams, depth, label=np.zeros((F, h, w), np.int32), select=1, carve=True) == (F, h, w)
    for kw, text in ((dict(cams=cams[:, :16]), r'cams of shape \(2, 16\)'), (dict(depth=depth[0]), 'depth of shape'),
                     (dict(depth=depth[:1]), 'for 2 cameras'), (dict(acc=depth[:, :3]), 'acc of shape'),
                     (dict(rgb=depth), 'rgb of shape'), (dict(label=depth[..., 0], select=0), 'label of shape'),
                     (dict(xform=np.zeros((F, 4, 4))), 'xform of shape'), (dict(frame_weight=np.ones(3)), 'frame_weight of shape'),
                     (dict(select=1), 'without label'), (dict(carve=True), 'without label'),
                     (dict(label=np.zeros((F, h, w), np.int32)), 'select = None'),
                     (dict(label=np.zeros((F, h, w), np.int32), select=0.5), 'select = 0.5'), (dict(max_weight=0.0), 'max_weight'),
                     (dict(znear=0.0), 'znear'), (dict(acc=depth, min_acc=float('nan')), 'min_acc'),
                     (dict(depth=np.ones((F, 4097, 1), np.float32)), '4097 x 1')):
        with pytest.raises(ValueError, match=text):
            tsdf.check_frames(**dict(dict(cams=cams, depth=depth), **kw))
    for kw, text in ((dict(step=None), 'give step or axes'), (dict(step=0.1, axes=((1, 0, 0), (0, 1, 0), (0, 0, 1))), 'give step or axes'),
                     (dict(shape=(1, 4, 4)), 'a lattice of 1 x 4 x 4'), (dict(shape=(512, 512, 512)), 'fewer than 2\\^27'),
                     (dict(trunc=None), 'trunc = None'), (dict(trunc=0.0), 'trunc = 0.0'), (dict(trunc=float('inf')), 'trunc = inf'),
                     (dict(origin=(0, 0)), 'three components'),
                     (dict(step=None, axes=((1, 0, 0), (2, 0, 0), (0, 0, 1))), 'a singular frame')):
        with pytest.raises(ValueError, match=text):
            tsdf.volume(**dict(dict(origin=(0, 0, 0), shape=(4, 4, 4), step=0.1, trunc=0.3, device='cpu'), **kw))
    for fn in (tsdf.lattice, tsdf.surface, lambda v: tsdf.sample(v, np.zeros((1, 3))), lambda v: tsdf.integrate(v, cams, depth)):
        with pytest.raises(ValueError, match='vol is tsdf.volume\'s dict'):
            fn(dict(tsdf=None))


def test_the_commands_argument_parsing():
    ap = fuse_tsdf.build_parser()
    a = ap.parse_args(['--synthetic', '--objects', '--eval_dir', 'out'])
    assert a.synthetic and a.write_objects is True and a.synthetic_boxes == 3 and a.trunc is None and a.min_weight == 1.0
    origin, shape, step = fuse_tsdf.check_args(a)
    assert shape == (24, 24, 12) and step == 0.17 and list(origin) == [-2.0, -2.0, -1.0]
    a = ap.parse_args(['--eval_dir', 'out', '--grid', '0,0,0;8,9,10;0.5', '--trunc', '1.5', '--obj_step', '0.1', '--min_weight', '2',
                       '--min_component', '7', '--largest', '2', '--traj', 't.npz', '--data_dir', 'd', '--train_dir', 'c', '--carve'])
    assert fuse_tsdf.check_args(a) == ((0.0, 0.0, 0.0), (8, 9, 10), 0.5) or list(fuse_tsdf.check_args(a)[1]) == [8, 9, 10]
    assert (a.trunc, a.obj_step, a.min_weight, a.min_component, a.largest, a.carve, a.write_objects) == (1.5, 0.1, 2.0, 7, 2, True, False)
    for argv, text in ((['--eval_dir', 'o'], 'are required'), (['--eval_dir', 'o', '--synthetic', '--grid', '0,0,0;1,4,4;0.5'], 'at least two points'),
                       (['--eval_dir', 'o', '--synthetic', '--grid', 'nonsense'], 'fuse_tsdf: '), (['--eval_dir', 'o', '--synthetic', '--trunc', '0'], '--trunc'),
                       (['--eval_dir', 'o', '--synthetic', '--obj_step', '-1'], '--obj_step'), (['--eval_dir', 'o', '--synthetic', '--batch', '0'], '--batch'),
                       (['--eval_dir', 'o', '--synthetic', '--min_weight', 'nan'], '--min_weight')):
        with pytest.raises(SystemExit, match=text):
            fuse_tsdf.check_args(ap.parse_args(argv))
