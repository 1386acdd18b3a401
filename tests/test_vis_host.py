"""Depth visualisations, the part that needs no GPU: the float64 restatement (tests/vis_ref.py) against what the reference's
own internal/vis.py returned (tests/golden/ref_vis_cases.npz, tests/golden/make_vis_fixture.py), the built-in turbo table
against matplotlib and against the fixture's copy, the surface of the new entry points, and evaluate()'s default result."""
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from durf_amd import _lib, ops, train_boxpose
from tests import vis_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, 'tests', 'golden', 'ref_vis_cases.npz')
NEW_SYMBOLS = ('durf_vis_scratch_bytes', 'durf_vis_stats', 'durf_vis_depth', 'durf_vis_normals', 'durf_vis_sinebow',
               'durf_vis_turbo_lut')
# float64 against float64: the restatement performs the reference's operations (a reordered sum would show ~1e-16)
TOL = 1e-12


@pytest.fixture(scope='module')
def fx():
    with np.load(FIXTURE) as z:
        return {k: z[k] for k in z.files}


def _restate(fx, name, what):
    d = fx[name + '/depth'][0]
    a = fx[name + '/acc'][0] if name + '/acc' in fx else None
    lut = fx['turbo']
    if what == 'normals_raw':
        return R.depth_to_normals(d)
    if what == 'normals':
        return R.visualize_normals(d, a)
    if what == 'normals_s2':
        return R.visualize_normals(d, a, scaling=2.0)
    if what == 'depth_mod':
        return R.visualize_depth(d, a, modulus=0.1)
    if what == 'depth_given':
        return R.visualize_depth(d, a, near=0.5, far=45.0, lut=lut)
    if what == 'depth_auto':
        return R.visualize_depth(d, a, lut=lut)
    if what.startswith('suite_'):
        return R.visualize_suite(d, a, lut)[what[len('suite_'):]]
    if what == 'depth_flipped_identity':
        return R.visualize_depth(d, a, near=30.0, far=5.0, curve_fn='identity', lut=lut)
    if what == 'depth_inverse':
        return R.visualize_depth(d, a, curve_fn='inverse', lut=lut)
    if what == 'depth_ignore':
        return R.visualize_depth(d, a, ignore_frac=0.05, lut=lut)
    if what == 'depth_far_only':
        return R.visualize_depth(d, a, near=0, far=45.0, lut=lut)
    raise KeyError(what)


def test_restatement_matches_the_reference(fx):
    assert np.abs(R.sinebow(fx['sinebow_h']) - fx['sinebow']).max() <= TOL
    keys = [k for k in fx if '/' in k and k.split('/')[1] not in ('depth', 'acc')]
    assert len(keys) >= 45
    seen = set()
    for k in keys:
        name, what = k.split('/')
        got, want = _restate(fx, name, what), fx[k]
        assert got.shape == want.shape and got.dtype == np.float64, k
        assert np.array_equal(np.isnan(got), np.isnan(want)), k + ': NaN pattern'
        ok = ~np.isnan(want)
        assert np.abs(got[ok] - want[ok]).max(initial=0.0) <= TOL, k
        seen.add(what)
    assert {'depth_auto', 'depth_mod', 'normals', 'depth_ignore', 'depth_flipped_identity', 'depth_inverse', 'suite_depth'} <= seen
    # the fixture exercises what it is there for: NaN pictures, white pixels, a far plane lost to a NaN
    assert np.isnan(fx['nan_noacc/depth_mod']).any() and (fx['nan_acc0/depth_auto'] == 1.0).all()
    gone = np.isnan(fx['nan_noacc/depth'][0])
    assert gone.any() and (fx['nan_noacc/depth_auto'][~gone] == fx['turbo'][0]).all(), 'far = NaN: every depth takes the first colour'
    assert (fx['nan_noacc/depth_auto'][gone] == 1.0).all(), 'and a NaN depth is white'
    assert (fx['const/normals'][..., :] == 1.0).all(), 'a constant plane: scale = inf, every normal NaN, every pixel white'


def test_fixture_inputs_are_the_seeded_cases(fx):
    for name in ('p1x1', 'p1x7', 'p7x1', 'p3x3', 'p37x53', 'nan_acc0', 'nan_noacc', 'const'):
        depth, acc = R.case(name)
        np.testing.assert_allclose(depth, fx[name + '/depth'], rtol=0, atol=1e-5, equal_nan=True)
        assert (acc is None) == (name + '/acc' not in fx)
        assert depth.dtype == np.float32 and np.nanmin(depth) >= 1.0 and np.nanmax(depth) <= 40.0


def test_float32_twin_is_close_and_is_float32(fx):
    d, a = fx['p37x53/depth'][0], fx['p37x53/acc'][0]
    twin = R.visualize_normals(d, a, dt=np.float32)
    assert twin.dtype == np.float32
    err = np.abs(twin.astype(np.float64) - R.visualize_normals(d, a)).max()
    assert 0 < err < 1e-4, err
    assert R.visualize_depth(d, a, modulus=0.1, dt=np.float32).dtype == np.float32


def test_stats_restatement():
    d = np.array([[1.0, 2.0, np.nan], [4.0, 5.0, 6.0]], np.float32)
    s = R.stats(d)
    eps = float(np.finfo(np.float32).eps)
    assert s[0] == 1.0 - eps and np.isnan(s[1]) and s[3] == 5
    np.testing.assert_allclose(s[4:8], [np.var([0, 1, 0, 1, 2]), np.var([0, 0, 1, 1, 1]), np.var([1, 2, 4, 5, 6]), 3.6], rtol=1e-15)
    np.testing.assert_allclose(s[2], np.sqrt((s[4] + s[5]) / 2 / s[6]), rtol=1e-15)
    c = R.stats(np.full((3, 4), 7.25, np.float32))
    assert c[6] == 0.0 and np.isinf(c[2]) and c[1] == 7.25 + eps
    assert np.isnan(R.stats(np.full((1, 1), 3.0, np.float32))[2]), '0 / 0'
    assert np.isnan(R.stats(np.full((2, 2), np.nan, np.float32))[[0, 1, 2]]).all()


# ---- the turbo table ------------------------------------------------------------------------------------------------------
def _header_table():
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    try:
        import gen_turbo_lut
    finally:
        sys.path.pop(0)
    return gen_turbo_lut, gen_turbo_lut.parse(open(gen_turbo_lut.HDR).read())


def test_turbo_header_is_the_fixtures_copy_and_the_library_exports_it(fx):
    _, tab = _header_table()
    assert tab.shape == (256, 3) and tab.dtype == np.float32
    assert np.array_equal(tab, fx['turbo'].astype(np.float32))
    assert np.array_equal(ops.vis_turbo_lut(), tab)


def test_turbo_header_is_matplotlibs():
    matplotlib = pytest.importorskip('matplotlib')
    gen, tab = _header_table()
    assert np.array_equal(tab, np.asarray(matplotlib.colormaps['turbo'](np.arange(256))[:, :3], np.float32))
    assert open(gen.HDR).read() == gen.render(gen.table()), 'stale: run python tools/gen_turbo_lut.py'


# ---- the surface ----------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, 'include', 'durf_hip.h')).read()
    L = _lib.lib()
    for name in NEW_SYMBOLS:
        assert re.search(r'\b%s\s*\(' % name, hdr), name + ' is not in include/durf_hip.h'
        assert name in _lib._SIGS, name + ' is not in durf_amd/_sigs.py'
        assert hasattr(L, name)
    assert L.durf_version() == 41
    assert set(ops.VIS_CURVES) == {'neglog', 'identity', 'inverse'}       # (DURF_VIS_* against the header: tests/test_headers_host.py)
    assert len(ops.VIS_STATS_FIELDS) == ops.VIS_STATS_FLOATS
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'gen_integration_stub.py'), '--check'], cwd=ROOT)
    assert p.returncode == 0, 'the header, durf_amd/_sigs.py, the stub and INTEGRATION.md have drifted apart'
    # the scratch grows with the frames and, past one workgroup's pixels, with the plane -- up to a cap
    sb = L.durf_vis_scratch_bytes
    assert sb(0, 4, 4) == 0 and sb(1, 1, 1) > 0 and sb(3, 37, 53) == 3 * sb(1, 37, 53)
    assert sb(1, 320, 480) > sb(1, 37, 53), 'more than one reduction workgroup at 320 x 480'
    assert sb(1, 4000, 4000) == sb(1, 8000, 8000) <= 64 * 12 * 8


def test_refusals_need_no_device():
    import ctypes as C
    L = _lib.lib()
    fake = C.c_void_p(256)                                  # never dereferenced: every call below is refused first
    assert L.durf_vis_depth(None, 1, 4, 4, fake, None, fake, 2, 0, 0.0, None, None, None) == -1
    assert 'at least one output' in L.durf_last_error().decode()
    assert L.durf_vis_depth(None, 1, 4, 4, fake, None, fake, 2, 7, 0.0, None, fake, None) == -1
    assert 'DURF_VIS_CURVE' in L.durf_last_error().decode()
    assert L.durf_vis_depth(None, 1, 4, 4, fake, None, None, 0, 0, 0.0, None, fake, None) == -1
    assert 'range' in L.durf_last_error().decode()
    assert L.durf_vis_depth(None, 1, 0, 4, fake, None, fake, 2, 0, 0.0, None, fake, None) == -1
    assert L.durf_vis_normals(None, 1, 4, 4, fake, None, None, 1, 2, fake, None) == -1
    assert L.durf_vis_stats(None, 2, 37, 53, fake, fake, fake, int(L.durf_vis_scratch_bytes(2, 37, 53)) - 8) == -1
    assert re.search(r'durf_vis_stats: scratch of \d+ bytes, durf_vis_scratch_bytes\(2, 37, 53\)', L.durf_last_error().decode())
    assert L.durf_vis_turbo_lut(None) == -1
    # F == 0 is nothing to do
    assert L.durf_vis_depth(None, 0, 4, 4, fake, None, fake, 2, 0, 0.0, None, fake, None) == 0
    from durf_amd import vis
    with pytest.raises(ValueError, match='curve_fn'):
        ops.vis_depth(torch.zeros(1, 2, 2), None, torch.zeros(1, 2), curve='log')
    assert [p for p in inspect.signature(vis.visualize_depth).parameters][:8] == [
        'depth', 'acc', 'near', 'far', 'ignore_frac', 'curve_fn', 'modulus', 'colormap']
    assert [p for p in inspect.signature(vis.visualize_normals).parameters][:3] == ['depth', 'acc', 'scaling']
    assert [p for p in inspect.signature(vis.visualize_suite).parameters][:2] == ['depth', 'acc']


# ---- evaluate -------------------------------------------------------------------------------------------------------------
class _FakeModel:
    def supports_one_call(self, variables):
        return True

    def render_image_one_call(self, variables, rays, init, ext, ts, white_bkgd, alpha, chunk=8192):
        g = torch.Generator().manual_seed(0)
        return torch.rand(6, 5, 3, generator=g), torch.rand(6, 5, generator=g), torch.rand(6, 5, generator=g)


def test_evaluate_default_result_is_unchanged():
    assert inspect.signature(train_boxpose.evaluate).parameters['vis'].default is False
    case = dict(rays=None, init=None, ext=None, ts=0, pixels=torch.zeros(6, 5, 3))
    config = type('C', (), dict(white_bkgd=False))()
    ev = train_boxpose.evaluate(_FakeModel(), config, None, case, 10.0)
    assert set(ev) == {'psnr', 'ssim', 'rgb', 'distance', 'acc', 'rays'}


def test_command_offers_the_vis_flags():
    p = subprocess.run([sys.executable, '-m', 'durf_amd.render_traj', '--help'], cwd=ROOT, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=120)
    assert p.returncode == 0, p.stdout.decode()
    for flag in ('--vis', '--vis_near', '--vis_far'):
        assert flag in p.stdout.decode()
