"""Depth visualisations on the GPU (csrc/vis.hip through durf_amd/vis.py and ops.vis_*), held to the float64 restatement of
the reference's internal/vis.py (tests/vis_ref.py; pinned to the reference by tests/test_vis_host.py).  Inputs: the small
planes committed in tests/golden/ref_vis_cases.npz, and two seeded ones (three frames of 37 x 53; 320 x 480, which takes more
than one reduction workgroup) drawn by vis_ref.case -- expected values are always computed from the very arrays the
kernels get.  Neither the reference nor matplotlib is read here.

Tolerances (absolute):
  colour-map pictures   1e-5 against the table row the float64 value picks.  The map is a step function, so a pixel whose
                        float64 value * 256 lies within 1e-2 of an integer may take either neighbouring row (the float32
                        twin moves value * 256 by <= 8e-5 on these inputs, <= 5e-4 under the modulus).  Such pixels are
                        first shown to be <= 5 % of every case on the float64 restatement alone (measured: none on the
                        planes of <= 30 pixels, 1.2 .. 2.6 % on the others).  A value the clip set to 0 or 1 is not such
                        a pixel: it has no second row to fall into.
  sinebow pictures      1e-4 (slope <= pi, value error ~5e-6).
  statistics            1e-6 relative where finite; NaN and inf in the same places.
  normals               4 x |float32 twin of the restatement - float64| on the same inputs, at least 1e-6, computed per
                        frame when the test runs.  Measured twin errors (max over the picture): p1x1 0 (white), p1x7 7.9e-8,
                        p7x1 4.4e-8, p3x3 6.6e-8, p37x53 6.8e-7, nan_acc0 0 (acc = 0: white), nan_noacc 9.5e-7 / 1.4e-6,
                        const 0 (white), f3_37x53 1.2e-6 / 1.1e-6 / 5.7e-7, big 1.4e-5 (the twin's normal scale is an fp32
                        variance of 153600 values); scaling = 2 without acc: p3x3 3.9e-8, p37x53 1.2e-6, nan_noacc 1.1e-6 /
                        1.3e-6; raw normals: p3x3 6.5e-8, p37x53 1.5e-6, nan_noacc 1.3e-6 / 1.4e-6.
  8-bit pictures        equal rint(clamp(float picture, 0, 1) * 255), the product in fp32 as the kernel forms it, of the same
                        call exactly (NaN -> 0)."""
import os

import numpy as np
import pytest
import torch

from durf_amd import ops, vis
from tests import vis_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, 'tests', 'golden', 'ref_vis_cases.npz')
SMALL = ('p1x1', 'p1x7', 'p7x1', 'p3x3', 'p37x53', 'nan_acc0', 'nan_noacc', 'const')
ALL = SMALL + ('f3_37x53', 'big')
TINY = ('p1x1', 'p1x7', 'p7x1', 'p3x3', 'const')          # automatic planes are (near) degenerate there: far - near ~ 2 eps
LUT_TOL, BOW_TOL, EDGE, EDGE_FRACTION = 1e-5, 1e-4, 1e-2, 0.05


class _Cases:
    """inputs (numpy float32 [F,H,W]) of every case, their device copies, and float64 results computed once and shared"""

    def __init__(self, dev):
        self.dev = dev
        with np.load(FIXTURE) as z:
            self.turbo = z['turbo']
            self.sinebow = (z['sinebow_h'], z['sinebow'])
            self.np = {n: (z[n + '/depth'], z[n + '/acc'] if n + '/acc' in z.files else None) for n in SMALL}
        for n in ALL:
            if n not in self.np:
                self.np[n] = R.case(n)
        self.t = {n: tuple(None if x is None else torch.tensor(x, device=dev) for x in da) for n, da in self.np.items()}
        self.memo = {}

    def ref(self, key, fn):
        if key not in self.memo:
            self.memo[key] = fn()
        return self.memo[key]

    def frames(self, name):
        d, a = self.np[name]
        return [(d[f], None if a is None else a[f]) for f in range(d.shape[0])]


@pytest.fixture(scope='module')
def cs(cuda):
    return _Cases(cuda)


def _np(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _same(a, b):
    """the same values, a NaN (a NaN depth under a modulus) equal to a NaN"""
    return a.shape == b.shape and a.dtype == b.dtype and torch.allclose(a, b, rtol=0, atol=0, equal_nan=True)


def _check_lut(got, value, a, lut, what, cyclic=False):
    """got [H,W,3] against the row of `lut` that the float64 `value` picks, blended with a; near a step either row passes"""
    lut = np.asarray(lut, np.float64)
    k = np.nan_to_num(value * 256.0)
    r = np.rint(k)
    # (a value the clip set to 0 or 1, or a NaN one, has no second row to fall into: rows -1 and 256 do not exist --
    # under a modulus they do, the map is cyclic there)
    edge = (np.abs(k - r) < EDGE) & ~np.isnan(value) & (cyclic | ((r > 0) & (r < 256)))
    assert edge.mean() <= EDGE_FRACTION, '%s: %.1f %% of the pixels sit on a step of the map' % (what, 100 * edge.mean())

    def colour(row):
        c = np.where(np.isnan(value)[..., None], 0.0, lut[row])
        return c * a[..., None] + (1.0 - a)[..., None]

    def close(row):
        return np.abs(got - colour(row)).max(-1) <= LUT_TOL
    rows = (lambda x: np.mod(x, 256)) if cyclic else (lambda x: np.clip(x, 0, 255))
    ok = close(np.minimum(np.floor(k).astype(np.int64), 255))
    ok |= edge & (close(rows(r - 1).astype(np.int64)) | close(rows(r).astype(np.int64)))
    assert ok.all(), '%s: %d pixels off their table row, worst %.3e' % (
        what, (~ok).sum(), np.abs(got - colour(np.minimum(np.floor(k).astype(np.int64), 255)))[~ok].max())
    return edge.mean()


def _check_u8(rgb, rgb8, what):
    # k_frame_pack's rule, in its arithmetic: one fp32 multiply, then round-half-even
    x = np.clip(np.nan_to_num(rgb.cpu().numpy(), nan=0.0), np.float32(0), np.float32(1))
    want = np.rint(x * np.float32(255)).astype(np.uint8)
    assert x.dtype == np.float32 and rgb8.dtype == torch.uint8 and np.array_equal(rgb8.cpu().numpy(), want), what + ': 8-bit picture'


# ---- statistics -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ALL)
def test_stats_record(cs, name):
    got = ops.vis_stats(cs.t[name][0]).cpu().numpy().astype(np.float64)
    assert got.shape == (cs.np[name][0].shape[0], ops.VIS_STATS_FLOATS)
    for f, (d, _) in enumerate(cs.frames(name)):
        want = R.stats(d)
        print(name, f, 'got', got[f], 'want', want)
        assert np.array_equal(np.isnan(got[f]), np.isnan(want)) and np.array_equal(np.isinf(got[f]), np.isinf(want)), (got[f], want)
        fin = np.isfinite(want)
        assert (np.abs(got[f][fin] - want[fin]) <= 1e-6 * np.abs(want[fin])).all(), (got[f], want)
    if name == 'const':
        assert got[0, 6] == 0.0 and np.isinf(got[0, 2]), 'a constant plane: var depth is exactly 0'
    if name == 'nan_noacc':
        assert np.isnan(got[:, 1]).all() and np.isfinite(got[:, 0]).all(), 'far is NaN as soon as one depth is, near is not'


# ---- visualize_depth through a colour map ---------------------------------------------------------------------------------
def _step_lut():
    rs = np.random.default_rng(5)
    return rs.uniform(0.0, 1.0, (256, 3)).astype(np.float32)


#            variant: (kwargs of vis.visualize_depth / vis_ref.visualize_depth, cases)
DEPTH_VARIANTS = {
    'auto': (dict(), tuple(n for n in ALL if n not in TINY)),
    'given': (dict(near=0.5, far=45.0), ALL),
    'far_only': (dict(near=0, far=45.0), ('p37x53',)),
    'flipped_identity': (dict(near=30.0, far=5.0, curve_fn='identity'), ('p37x53', 'f3_37x53')),
    'inverse': (dict(curve_fn='inverse'), ('p37x53', 'big')),
    'identity': (dict(curve_fn='identity'), ('p37x53',)),
    'ignore_frac': (dict(ignore_frac=0.05), ('p37x53', 'f3_37x53', 'nan_noacc')),
    'custom_lut': (dict(colormap=True), ('p37x53', 'nan_acc0')),
    'custom_lut_mod': (dict(colormap=True, modulus=0.1), ('p37x53', 'nan_noacc')),
}


@pytest.mark.parametrize('variant,name', [(v, n) for v, (_, names) in DEPTH_VARIANTS.items() for n in names])
def test_depth_colour_map(cs, variant, name):
    kw = dict(DEPTH_VARIANTS[variant][0])
    lut, dev_kw = cs.turbo, {}
    if kw.pop('colormap', False):
        lut = _step_lut()
        dev_kw = dict(colormap=torch.tensor(lut, device=cs.dev))
    d, a = cs.t[name]
    got = vis.visualize_depth(d, a, **kw, **dev_kw)
    assert got.shape == d.shape + (3,) and got.dtype == torch.float32
    for f, (df, af) in enumerate(cs.frames(name)):
        _, value, w = R.visualize_depth(df, af, lut=lut, parts=True, **kw)
        frac = _check_lut(_np(got[f]), value, w, lut, '%s %s frame %d' % (variant, name, f), cyclic=bool(kw.get('modulus')))
        print(variant, name, f, 'pixels on a step: %.2f %%' % (100 * frac))
    _check_u8(got, vis.visualize_depth(d, a, out8=True, **kw, **dev_kw), variant + ' ' + name)


def test_three_frames_three_ranges(cs):
    """the frame axis: near / far as one value per frame, near > far in the middle one"""
    d, a = cs.t['f3_37x53']
    near, far = [2.0, 35.0, 0.5], [38.0, 4.0, 45.0]
    got = vis.visualize_depth(d, a, near=torch.tensor(near), far=torch.tensor(far, device=cs.dev))
    for f, (df, af) in enumerate(cs.frames('f3_37x53')):
        _, value, w = R.visualize_depth(df, af, near=near[f], far=far[f], lut=cs.turbo, parts=True)
        _check_lut(_np(got[f]), value, w, cs.turbo, 'frame %d' % f)
        one = vis.visualize_depth(d[f], a[f], near=near[f], far=far[f])
        assert torch.equal(one, got[f]), 'a frame of a batch is that frame alone, bit for bit'


# ---- visualize_depth with a modulus: the sinebow ---------------------------------------------------------------------------
@pytest.mark.parametrize('name', ALL)
def test_depth_mod_sinebow(cs, name):
    d, a = cs.t[name]
    rgb, rgb8 = ops.vis_depth(d, a, None, modulus=0.1, want_u8=True)
    assert _same(rgb, vis.visualize_depth(d, a, modulus=0.1))
    for f, (df, af) in enumerate(cs.frames(name)):
        want = R.visualize_depth(df, af, modulus=0.1)
        g = _np(rgb[f])
        assert np.array_equal(np.isnan(g), np.isnan(want)), 'a NaN depth stays NaN under a modulus, as in the reference'
        err = np.nanmax(np.abs(g - want), initial=0.0)
        print(name, f, 'sinebow err %.3e' % err)
        assert err <= BOW_TOL
    _check_u8(rgb, rgb8, name)


def test_sinebow(cs):
    h, want = cs.sinebow
    got = vis.sinebow(torch.tensor(h, dtype=torch.float32, device=cs.dev))
    assert got.shape == (41, 3) and np.abs(_np(got) - want).max() <= BOW_TOL


# ---- normals --------------------------------------------------------------------------------------------------------------
def _normals_tol(fn64, fn32):
    twin = np.abs(fn32().astype(np.float64) - fn64())
    twin = np.nanmax(twin, initial=0.0)
    return twin, max(4.0 * twin, 1e-6)


@pytest.mark.parametrize('name', ALL)
def test_normals(cs, name):
    d, a = cs.t[name]
    rgb, rgb8 = ops.vis_normals(d, a, ops.vis_stats(d)[:, 2], want_u8=True)
    assert _same(rgb, vis.visualize_normals(d, a))
    for f, (df, af) in enumerate(cs.frames(name)):
        want = R.visualize_normals(df, af)
        twin, tol = _normals_tol(lambda: want, lambda: R.visualize_normals(df, af, dt=np.float32))
        g = _np(rgb[f])
        assert np.array_equal(np.isnan(g), np.isnan(want))
        err = np.nanmax(np.abs(g - want), initial=0.0)
        print(name, f, 'normals err %.3e twin %.3e tol %.3e' % (err, twin, tol))
        assert err <= tol
    _check_u8(rgb, rgb8, name)


@pytest.mark.parametrize('name', ('p3x3', 'p37x53', 'nan_noacc'))
def test_normals_given_scale_no_acc_and_raw(cs, name):
    d, _ = cs.t[name]
    got = vis.visualize_normals(d, None, scaling=2.0)
    raw = vis.depth_to_normals(d)
    for f, (df, _) in enumerate(cs.frames(name)):
        want = R.visualize_normals(df, None, scaling=2.0)
        _, tol = _normals_tol(lambda: want, lambda: R.visualize_normals(df, None, scaling=2.0, dt=np.float32))
        assert np.abs(_np(got[f]) - want).max() <= tol
        want = R.depth_to_normals(df)
        twin, tol = _normals_tol(lambda: want, lambda: R.depth_to_normals(df, dt=np.float32))
        g = _np(raw[f])
        assert np.array_equal(np.isnan(g), np.isnan(want))
        print(name, f, 'raw normals err %.3e twin %.3e' % (np.nanmax(np.abs(g - want), initial=0.0), twin))
        assert np.nanmax(np.abs(g - want), initial=0.0) <= tol


# ---- outputs: guards, alignment, repeatability -----------------------------------------------------------------------------
def _guarded(n, dtype, dev, lead):
    """n elements with `lead` + 64 guard elements in front and 64 behind, all poisoned"""
    buf = torch.full((lead + 64 + n + 64,), 0xA5 if dtype == torch.uint8 else -777.0, dtype=dtype, device=dev)
    return buf, buf[lead + 64:lead + 64 + n]


@pytest.mark.parametrize('lead', (0, 1))            # 1: neither output is 16- / 4-byte aligned -- the element-wise stores
@pytest.mark.parametrize('op', ('depth', 'depth_mod', 'normals'))
def test_only_the_requested_outputs_are_written(cs, op, lead):
    d, a = cs.t['f3_37x53']                          # 3 * 37 * 53 pixels: not a multiple of four, the last lane takes three
    F, H, W = d.shape
    n = F * H * W * 3
    stats = ops.vis_stats(d)

    def call(**kw):
        if op == 'normals':
            return ops.vis_normals(d, a, stats[:, 2], **kw)
        return ops.vis_depth(d, a, stats, modulus=0.1 if op == 'depth_mod' else 0.0, **kw)
    ref, ref8 = call(want_u8=True)
    fbuf, fview = _guarded(n, torch.float32, cs.dev, lead)
    bbuf, bview = _guarded(n, torch.uint8, cs.dev, lead)
    poison_f, poison_b = fbuf.clone(), bbuf.clone()
    # 8-bit only: the float buffer keeps its poison, every byte outside the picture keeps its guard
    r, r8 = call(want_float=False, want_u8=True, rgb=fview.view(F, H, W, 3), rgb8=bview.view(F, H, W, 3))
    assert r is None and torch.equal(fbuf, poison_f), 'an 8-bit-only call writes no float'
    assert torch.equal(bview.view(F, H, W, 3), ref8)
    assert torch.equal(bbuf[:lead + 64], poison_b[:lead + 64]) and torch.equal(bbuf[-64:], poison_b[-64:])
    # float only
    bbuf.copy_(poison_b)
    r, r8 = call(want_float=True, want_u8=False, rgb=fview.view(F, H, W, 3), rgb8=bview.view(F, H, W, 3))
    assert r8 is None and torch.equal(bbuf, poison_b)
    assert np.array_equal(fview.cpu().numpy().view(np.uint32), ref.reshape(-1).cpu().numpy().view(np.uint32)), 'same bits at any alignment'
    assert torch.equal(fbuf[:lead + 64], poison_f[:lead + 64]) and torch.equal(fbuf[-64:], poison_f[-64:])


def test_misaligned_inputs_take_the_same_values(cs):
    d, a = cs.t['p37x53']
    want = vis.visualize_suite(d, a)
    dd = torch.empty(d.numel() + 1, device=cs.dev)[1:].view(d.shape).copy_(d)
    aa = torch.empty(a.numel() + 1, device=cs.dev)[1:].view(a.shape).copy_(a)
    assert dd.data_ptr() % 16 != 0 and dd.is_contiguous()
    got = vis.visualize_suite(dd, aa)
    for k in want:
        assert torch.equal(got[k], want[k]), k


def test_two_identical_calls_are_bit_identical(cs):
    d, a = cs.t['big']
    one, two = vis.visualize_suite(d, a), vis.visualize_suite(d, a)
    s1, s2 = ops.vis_stats(d), ops.vis_stats(d)
    assert np.array_equal(s1.cpu().numpy().view(np.uint32), s2.cpu().numpy().view(np.uint32))
    for k in ('depth', 'depth_mod', 'depth_normals'):
        assert np.array_equal(one[k].cpu().numpy().view(np.uint32), two[k].cpu().numpy().view(np.uint32)), k


def test_suite_batches_frames_and_leading_dimensions(cs):
    d, a = cs.t['f3_37x53']
    whole = vis.visualize_suite(d, a)
    whole8 = vis.visualize_suite(d, a, out8=True)
    assert set(whole) == {'depth', 'depth_mod', 'depth_normals'}
    for k in whole:
        assert whole[k].shape == (3, 37, 53, 3)
        _check_u8(whole[k], whole8[k], k)
        for f in range(3):
            assert torch.equal(vis.visualize_suite(d[f], a[f])[k], whole[k][f]), '%s frame %d' % (k, f)
    lead = vis.visualize_suite(d[:2].reshape(2, 1, 37, 53), a[:2].reshape(2, 1, 37, 53))
    assert lead['depth'].shape == (2, 1, 37, 53, 3) and torch.equal(lead['depth'].reshape(2, 37, 53, 3), whole['depth'][:2])
    # the suite against the restatement, frame 0
    df, af = cs.frames('f3_37x53')[0]
    want = R.visualize_suite(df, af, cs.turbo)
    assert np.abs(_np(whole['depth_mod'][0]) - want['depth_mod']).max() <= BOW_TOL
    _, value, w = R.visualize_depth(df, af, lut=cs.turbo, parts=True)
    _check_lut(_np(whole['depth'][0]), value, w, cs.turbo, 'suite depth')


# ---- where users meet it ---------------------------------------------------------------------------------------------------
def test_evaluate_carries_the_pictures_on_request(cuda):
    from durf_amd import obbpose_model, synthetic, train_boxpose, utils
    from tests import helpers as H
    hw, N, K = (37, 53), 32, 1
    utils.clear_gin()
    utils.parse_gin('MipNerfModel.num_samples = %d\nMipNerfModel.density_noise = 0.0\nMipNerfModel.no_pose_opt = True\n'
                    'MipNerfModel.no_yaw_opt = True\n' % N)
    b = synthetic.make_batch(hw[0] * hw[1], K, seed=40)
    db = H.device_batch(b, cuda)
    model, variables = obbpose_model.construct_mipnerf(1, db, device=cuda)
    config = utils.configured(utils.Config)
    rays = utils.namedtuple_map(lambda r: r.reshape(hw[0], hw[1], -1), db['rays'])
    case = dict(rays=rays, pixels=db['pixels'].reshape(hw[0], hw[1], -1), init=db['init'], ext=db['ext'], ts=b['ts'])
    plain = train_boxpose.evaluate(model, config, variables, case, 10.0, chunk=512)
    assert set(plain) == {'psnr', 'ssim', 'rgb', 'distance', 'acc', 'rays'}
    ev = train_boxpose.evaluate(model, config, variables, case, 10.0, chunk=512, vis=True)
    assert set(ev) == set(plain) | {'vis'} and set(ev['vis']) == {'depth', 'depth_mod', 'depth_normals'}
    assert torch.equal(ev['rgb'], plain['rgb']) and float(ev['psnr']) == float(plain['psnr'])
    want = vis.visualize_suite(ev['distance'], ev['acc'])
    for k in want:
        assert ev['vis'][k].shape == (hw[0], hw[1], 3)
        assert np.array_equal(ev['vis'][k].cpu().numpy().view(np.uint32), want[k].cpu().numpy().view(np.uint32)), k
    utils.clear_gin()


def test_render_traj_command_writes_the_pictures(cuda, tmp_path):
    import subprocess
    import sys
    out = str(tmp_path / 'frames')
    cmd = [sys.executable, '-m', 'durf_amd.render_traj', '--synthetic', '--vis', '--eval_dir', out, '--frames', '3',
           '--gin_param', 'MipNerfModel.num_samples = 32', '--gin_param', 'MipNerfModel.no_pose_opt = True',
           '--gin_param', 'MipNerfModel.no_yaw_opt = True']
    p = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)      # a fresh child process
    assert p.returncode == 0, p.stdout.decode()
    h, w = 64, 96                                                        # SyntheticTimestepDataset's image
    names = ['%s%04d.ppm' % (pre, f) for pre in ('', 'depth_', 'depth_mod_', 'normals_') for f in range(3)]
    assert sorted(os.listdir(out)) == sorted(names + ['distance.npy'])
    header = b'P6\n%d %d\n255\n' % (w, h)
    dist = torch.tensor(np.load(os.path.join(out, 'distance.npy')), device=cuda)
    assert dist.shape == (3, h, w)
    for name in names:
        blob = open(os.path.join(out, name), 'rb').read()
        assert blob[:len(header)] == header and len(blob) == len(header) + h * w * 3, name
    # the normals need no acc where it is 1; the file is what the library draws from the saved distance wherever acc == 1
    # (acc itself is not saved), so only check that the pictures are pictures and differ between frames
    for pre in ('depth_', 'depth_mod_', 'normals_'):
        a, b = [np.frombuffer(open(os.path.join(out, '%s%04d.ppm' % (pre, f)), 'rb').read()[len(header):], np.uint8) for f in (0, 2)]
        assert len(np.unique(a)) > 16 and not np.array_equal(a, b), pre
