"""Whole-set evaluation, the part that needs no GPU: the float64 restatement of the per-frame record (tests/eval_ref.py) on
cases worked by hand, the surface of durf_eval_frames, its refusals, eval_set() of both loaders and the command's flags."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from durf_amd import _lib, datasets, ops, raygen, train_boxpose, utils
from tests import eval_ref as R
from tests.test_datasets import N_CAM, N_OBJ, N_TS, _config, _write_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ('durf_eval_scratch_bytes', 'durf_eval_frames')


# ---- the restatement ------------------------------------------------------------------------------------------------------
def test_identical_images():
    rgb = R.make_case(1, 13, 17, seed=1)[0][0]
    m = R.frame_metrics(rgb, rgb)
    assert m['mse'] == 0.0 and m['psnr'] == np.inf and abs(m['ssim'] - 1.0) <= 1e-12
    assert m['nonfinite'] == 0 and m['obj_count'] == 0 and m['depth_count'] == 0
    assert np.isnan(m['obj_mse']) and np.isnan(m['depth_abs']), 'no mask, no depth plane: NaN'


def test_hand_computed_11x11():
    """two constant images p and q: every window mean is p (q), every variance 0, so the one SSIM output is
    (2 p q + c1) / (p^2 + q^2 + c1); mse = (p - q)^2; the object MSE sums the three channels over the mask: 3 (p - q)^2;
    two LIDAR returns with errors 1 and -3: abs 2, rmse sqrt(5)"""
    p, q = 0.25, 0.75
    rgb, gt = np.full((11, 11, 3), p, np.float32), np.full((11, 11, 3), q, np.float32)
    mask = np.zeros((11, 11), np.float32)
    mask[2:4, 3:7] = 1.0
    gd = np.zeros((11, 11), np.float32)
    dist = np.full((11, 11), 9.0, np.float32)
    gd[0, 0], gd[10, 10] = 8.0, 12.0
    m = R.frame_metrics(rgb, gt, dist, gd, mask)
    c1 = 0.01 ** 2
    np.testing.assert_allclose(m['ssim'], (2 * p * q + c1) / (p * p + q * q + c1), rtol=1e-12)
    np.testing.assert_allclose(m['mse'], 0.25, rtol=1e-15)
    np.testing.assert_allclose(m['psnr'], -10 * np.log10(0.25), rtol=1e-15)
    assert m['obj_count'] == 8 and m['depth_count'] == 2
    np.testing.assert_allclose([m['obj_mse'], m['obj_psnr']], [0.75, -10 * np.log10(0.75)], rtol=1e-15)
    np.testing.assert_allclose([m['depth_abs'], m['depth_rmse']], [2.0, np.sqrt(5.0)], rtol=1e-15)
    # the deliberately wrong variants of the negative controls are wrong
    assert R.frame_metrics(rgb, gt, dist, gd, mask, obj_div3=True)['obj_mse'] == pytest.approx(0.25)
    assert R.frame_metrics(rgb, gt, dist, gd, mask, depth_all=True)['depth_count'] == 121


def test_empty_mask_no_lidar_and_a_nan():
    rgb, gt, dist, gd, mask = [t[0] for t in R.make_case(1, 12, 15, seed=2)]
    m = R.frame_metrics(rgb, gt, dist, np.zeros_like(gd), np.zeros_like(mask))
    assert m['obj_count'] == 0 and np.isnan(m['obj_mse']) and np.isnan(m['obj_psnr']), '0 / 0'
    assert m['depth_count'] == 0 and m['depth_abs'] == 0 and m['depth_rmse'] == 0
    bad = rgb.copy()
    bad[5, 6, 1] = np.nan
    m = R.frame_metrics(bad, gt, dist, gd, mask)
    assert m['nonfinite'] == 1 and np.isnan(m['mse']) and np.isnan(m['psnr']) and np.isnan(m['ssim'])
    bad[0, 0, :] = np.inf
    assert R.frame_metrics(bad, gt)['nonfinite'] == 4
    assert R.frames_metrics(*R.make_case(2, 11, 12)).shape == (2, 10)


# ---- the surface ----------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, 'include', 'durf_hip.h')).read()
    L = _lib.lib()
    for name in NEW_SYMBOLS:
        assert re.search(r'\b%s\s*\(' % name, hdr), name + ' is not in include/durf_hip.h'
        assert name in _lib._SIGS, name + ' is not in durf_amd/_sigs.py'
        assert hasattr(L, name)
    assert len(_lib._SIGS) == 118
    assert L.durf_version() == 41
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'gen_integration_stub.py'), '--check'], cwd=ROOT)
    assert p.returncode == 0, 'the header, durf_amd/_sigs.py, the stub and INTEGRATION.md have drifted apart'
    assert ops.EVAL_FLOATS == len(ops.EVAL_FIELDS) == 10          # (DURF_EVAL_* against the header: tests/test_headers_host.py)
    for i, name in enumerate(ops.EVAL_FIELDS):
        assert i == ops.EVAL_INDEX[name]
    assert ops.EVAL_FIELDS == R.FIELDS
    sb = L.durf_eval_scratch_bytes
    assert sb(0, 37, 53) == 0 and sb(1, 37, 53) > 0
    assert sb(3, 37, 53) == 3 * sb(1, 37, 53) and sb(7, 320, 480) == 7 * sb(1, 320, 480), 'linear in F'
    assert sb(1, 320, 480) > sb(1, 37, 53)


def test_refusals_need_no_device():
    L = _lib.lib()
    fake = C.c_void_p(256)                                  # never dereferenced: every call below is refused first
    big = 1 << 30
    assert L.durf_eval_frames(None, 1, 10, 40, fake, fake, None, None, None, fake, fake, big) == -1
    assert 'image smaller than the window' in L.durf_last_error().decode()
    assert L.durf_eval_frames(None, 1, 40, 10, fake, fake, None, None, None, fake, fake, big) == -1
    assert L.durf_eval_frames(None, 1, 37, 53, fake, fake, fake, None, None, fake, fake, big) == -1
    assert 'distance and gt_depth' in L.durf_last_error().decode()
    assert L.durf_eval_frames(None, 1, 37, 53, fake, fake, None, fake, None, fake, fake, big) == -1
    need = int(L.durf_eval_scratch_bytes(2, 37, 53))
    assert L.durf_eval_frames(None, 2, 37, 53, fake, fake, fake, fake, fake, fake, fake, need - 8) == -1
    assert re.search(r'durf_eval_frames: scratch of %d bytes, durf_eval_scratch_bytes\(2, 37, 53\) = %d' % (need - 8, need),
                     L.durf_last_error().decode())
    assert L.durf_eval_frames(None, 0, 37, 53, fake, fake, fake, fake, fake, fake, fake, 0) == 0, 'F == 0 is nothing to do'
    with pytest.raises(ValueError, match='together'):
        ops.eval_frames(torch.zeros(1, 11, 11, 3), torch.zeros(1, 11, 11, 3), distance=torch.zeros(1, 11, 11))
    with pytest.raises(ValueError, match=r'\[F,H,W,3\]'):
        ops.eval_frames(torch.zeros(11, 11, 3), torch.zeros(11, 11, 3))


# ---- eval_set() -----------------------------------------------------------------------------------------------------------
def _host_generate_batch(td, ray_indices, near, far):
    """raygen.generate_batch without the device: the full images of the timestep in order, rays of zeros"""
    assert ray_indices is None
    z = lambda c: torch.zeros(td.n_rays, c)
    return utils.BoxRays(z(3), z(3), z(3), z(1), z(1), z(1), z(1)), td.images, td.depth.reshape(-1, 1), td.sky.reshape(-1, 1)


def _check_against_iteration(es, cases, cams_of):
    F = len(cases)
    assert es['cams'].shape == (F, 17) and es['cams'].dtype == np.float32
    assert np.issubdtype(np.asarray(es['ts']).dtype, np.integer) and len(es['ts']) == F
    assert all(len(es[k]) == F for k in ('pixels', 'depth', 'sky', 'ext'))
    for f, case in enumerate(cases):
        h, w = case['pixels'].shape[:2]
        assert np.array_equal(es['cams'][f], cams_of(f)) and (es['cams'][f, 15], es['cams'][f, 16]) == (h, w)
        assert int(es['ts'][f]) == case['ts']
        assert torch.equal(es['ext'][f], case['ext']) and torch.equal(es['init'], case['init'])
        assert es['pixels'][f].shape == (h, w, 3) and es['depth'][f].shape == (h, w, 1) and es['sky'][f].shape == (h, w, 1)
        for k in ('pixels', 'depth', 'sky'):
            assert torch.equal(es[k][f], case[k]), k


@pytest.mark.parametrize('split', ['test', 'render'])
def test_waymo_eval_set_is_the_split_in_iteration_order(tmp_path, monkeypatch, split):
    _write_scene(str(tmp_path))
    ds = datasets.Waymo(split, str(tmp_path), _config(), device='cpu', seed=5)
    es = ds.eval_set()
    assert ds.it == 0 and ds._peek is None, 'the iterator is not advanced'
    F = ds.n_examples
    assert F == (len(datasets.TEST_IMAGES) if split == 'test' else N_TS * N_CAM) and es['init'].shape == (N_TS, N_OBJ, 6)
    monkeypatch.setattr(raygen, 'generate_batch', _host_generate_batch)
    cases = [next(ds) for _ in range(F)]
    _check_against_iteration(es, cases, lambda f: raygen.camera_row(ds.camtoworlds[f], ds.focal[f], ds.principal_point[f],
                                                                    ds.h[f], ds.w[f]))
    # views of the resident data: no copy was made
    td = ds.ts_data[0]
    assert es['pixels'][0].data_ptr() == td.images.data_ptr()
    if split == 'render':
        assert sorted({int(t) for t in es['ts']}) == list(range(N_TS)), 'every timestep: more than one group'


def test_synthetic_eval_set(monkeypatch):
    utils.clear_gin()
    ds = train_boxpose.SyntheticTimestepDataset(utils.Config(), K=3, T=3, hw=(12, 16), n_cams=2, device='cpu', split='test')
    es = ds.eval_set()
    assert len(es['ts']) == 6 and list(es['ts']) == [0, 0, 1, 1, 2, 2] and es['cams'].shape == (6, 17)
    for f in range(6):
        row = ds.ts_data[f // 2].cams[f % 2]
        assert np.array_equal(es['cams'][f], raygen.camera_row(row[:12].reshape(3, 4), row[12], row[13:15], row[15], row[16]))
        assert np.array_equal(es['cams'][f], row)
        assert es['pixels'][f].shape == (12, 16, 3) and es['depth'][f].shape == (12, 16, 1) and es['sky'][f].shape == (12, 16, 1)
        assert es['pixels'][f].data_ptr() == ds.ts_data[f // 2].images[(f % 2) * 192:].data_ptr()
    # next() yields the first camera of a random timestep: frame ts * n_cams of the set
    monkeypatch.setattr(raygen, 'generate_batch', _host_generate_batch)
    for _ in range(4):
        case = next(ds)
        f = case['ts'] * 2
        assert int(es['ts'][f]) == case['ts'] and es['ext'][f] is case['ext'] and es['init'] is case['init']
        for k in ('pixels', 'depth', 'sky'):
            assert torch.equal(es[k][f], case[k]), k


def test_evaluate_set_refuses_what_one_call_does_not_cover():
    class Model:
        def supports_one_call(self, variables):
            return False
    with pytest.raises(NotImplementedError, match='supports_one_call'):
        train_boxpose.evaluate_set(Model(), None, None, None, 10.0)


def test_command_lists_its_flags():
    p = subprocess.run([sys.executable, '-m', 'durf_amd.eval_set', '--help'], cwd=ROOT, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=120)
    assert p.returncode == 0, p.stdout.decode()
    for flag in ('--gin_file', '--data_dir', '--train_dir', '--split', '--eval_dir', '--synthetic', '--obj_mask', '--vis',
                 '--frames', '--chunk'):
        assert flag in p.stdout.decode(), flag
