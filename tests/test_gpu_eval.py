"""Whole-set evaluation on the GPU: durf_eval_frames (csrc/metrics.hip) against the float64 restatement tests/eval_ref.py,
and train_boxpose.evaluate_set / python -m durf_amd.eval_set on the synthetic scene.

Tolerances.  ssim: 2e-5 absolute, the project's gate for durf_ssim against the same oracle (fp32 blur against float64).  The
fields the kernel sums in fp64 (mse, obj_mse, depth_abs, depth_rmse and the two PSNRs): rtol 2.4e-7 = two fp32 ulp -- at most
3e4 non-negative fp64 terms per frame lose under 1e-11 relative, the one rounding to float loses 6e-8.  The three counts are
exact.  Inputs are seeded, in [0, 1], gt = clip(rgb + N(0, 0.1)), F = 3 frames of different content so that a frame-stride
error shows.  Shapes: (11, 11) has one SSIM output, (11, 40) and (40, 11) one degenerate axis, (37, 53) two tiles along each
axis, (75, 140) 3 x 5 tiles of 32 x 32 with a remainder along both axes."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from durf_amd import metrics, obbpose_model, ops, raygen, train_boxpose, utils
from tests import eval_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(11, 11), (11, 40), (40, 11), (37, 53), (75, 140)]
SSIM_ATOL, SUM_RTOL = 2e-5, 2.4e-7
IDX = {k: i for i, k in enumerate(R.FIELDS)}
_CASES = {}


def _case(cuda, hw):
    """(host arrays, device tensors, the device record, the float64 reference) of one shape, made once"""
    if hw not in _CASES:
        host = R.make_case(3, hw[0], hw[1], seed=hw[0] * 1000 + hw[1])
        dev = [torch.tensor(t, device=cuda) for t in host]
        got, fields = ops.eval_frames(*dev)
        assert fields == R.FIELDS and got.shape == (3, 10) and got.dtype == torch.float32
        _CASES[hw] = (host, dev, got, R.frames_metrics(*host))
    return _CASES[hw]


def _gate(got, want, what=''):
    """None if the [F,10] record `got` is inside the tolerances of the float64 `want`, otherwise what is not"""
    got = np.asarray(got, np.float64)
    for k in R.FIELDS:
        g, w = got[:, IDX[k]], want[:, IDX[k]]
        print('%s %-11s got %s want %s' % (what, k, g, w))
        if not np.array_equal(np.isnan(g), np.isnan(w)):
            return k + ': NaN pattern'
        ok = ~np.isnan(w)
        if k in R.COUNTS:
            if not np.array_equal(g[ok], w[ok]):
                return k + ': count'
        elif k == 'ssim':
            if np.abs(g[ok] - w[ok]).max(initial=0.0) > SSIM_ATOL:
                return 'ssim: %g' % np.abs(g[ok] - w[ok]).max()
        elif not np.allclose(g[ok], w[ok], rtol=SUM_RTOL, atol=0.0):
            return '%s: %g relative' % (k, np.abs(g[ok] / w[ok] - 1).max())
    return None


@pytest.mark.parametrize('hw', SHAPES)
def test_kernel_against_the_restatement(cuda, hw):
    host, dev, got, want = _case(cuda, hw)
    assert _gate(got.cpu().numpy(), want, str(hw)) is None
    assert (want[:, IDX['depth_count']] > 0).all() and (want[:, IDX['obj_count']] > 0).all(), 'the case exercises every field'
    assert len(np.unique(want[:, IDX['mse']])) == 3, 'frames of different content'
    # the dict form: any dtype and layout, a single frame
    d = metrics.evaluate_frames(dev[0][1].double().permute(2, 0, 1).contiguous().permute(1, 2, 0), dev[1][1], dev[2][1].half().float(),
                                dev[3][1], dev[4][1].to(torch.bfloat16))
    assert sorted(d) == sorted(R.FIELDS) and all(v.shape == (1,) and v.is_cuda for v in d.values())
    assert torch.equal(d['mse'], got[1:2, IDX['mse']]) and torch.equal(d['ssim'], got[1:2, IDX['ssim']])
    assert torch.equal(d['obj_count'], got[1:2, IDX['obj_count']])


@pytest.mark.parametrize('hw', [(37, 53), (75, 140)])
def test_record_is_reproducible_and_independent_of_the_neighbours(cuda, hw):
    host, dev, got, _ = _case(cuda, hw)
    again = ops.eval_frames(*dev)[0]
    assert got.cpu().numpy().tobytes() == again.cpu().numpy().tobytes()
    one = ops.eval_frames(*[t[1:2].contiguous() for t in dev])[0]
    assert one.cpu().numpy().tobytes() == got[1:2].cpu().numpy().tobytes(), 'frame 1 of F = 3 is the F = 1 call on it'


def test_nullable_inputs(cuda):
    host, dev, got, _ = _case(cuda, (37, 53))
    bare = ops.eval_frames(dev[0], dev[1])[0].cpu().numpy()
    full = got.cpu().numpy()
    for k in ('obj_mse', 'obj_psnr', 'depth_abs', 'depth_rmse'):
        assert np.isnan(bare[:, IDX[k]]).all(), k
    assert (bare[:, IDX['obj_count']] == 0).all() and (bare[:, IDX['depth_count']] == 0).all()
    same = [IDX[k] for k in ('mse', 'psnr', 'ssim', 'nonfinite')]
    assert bare[:, same].tobytes() == full[:, same].tobytes()
    # one of the two alone
    depth_only = ops.eval_frames(dev[0], dev[1], dev[2], dev[3])[0].cpu().numpy()
    keep = [IDX[k] for k in ('mse', 'psnr', 'ssim', 'depth_count', 'depth_abs', 'depth_rmse', 'nonfinite')]
    assert depth_only[:, keep].tobytes() == full[:, keep].tobytes() and np.isnan(depth_only[:, IDX['obj_mse']]).all()


def test_a_nan_stays_in_its_frame(cuda):
    host, dev, got, _ = _case(cuda, (75, 140))
    rgb = dev[0].clone()
    rgb[1, 40, 70, 2] = float('nan')
    bad = ops.eval_frames(rgb, *dev[1:])[0].cpu().numpy()
    clean = got.cpu().numpy()
    assert bad[1, IDX['nonfinite']] == 1
    assert np.isnan(bad[1, [IDX['mse'], IDX['psnr'], IDX['ssim']]]).all()
    assert bad[[0, 2]].tobytes() == clean[[0, 2]].tobytes()
    keep = [IDX[k] for k in ('depth_count', 'depth_abs', 'depth_rmse', 'obj_count')]
    assert bad[1, keep].tobytes() == clean[1, keep].tobytes()
    want = R.frames_metrics(rgb.cpu().numpy(), *host[1:])
    assert _gate(bad, want, 'nan') is None, 'and the restatement agrees, NaN pattern included'


def test_negative_controls(cuda):
    """the gate rejects a record that is wrong in the ways it is there to catch"""
    host, dev, got, want = _case(cuda, (37, 53))
    got = got.cpu().numpy()
    assert _gate(got, want) is None
    assert _gate(got, R.frames_metrics(*host, obj_div3=True), 'obj / 3') is not None
    assert _gate(got, R.frames_metrics(*host, depth_all=True), 'depth H*W') is not None


def test_negative_control_blur_order(cuda):
    """the restatement with the blur along H first, on a non-square anisotropic image: the gate must fail -- unless the
    swapped order lands inside 2e-5, and then this control cannot tell the orders apart and is skipped.  It does land inside:
    the two Gaussian passes commute in exact arithmetic and the 'valid' region is the same either way, so the float64 SSIM
    moves by rounding only."""
    host, dev, got, want = _case(cuda, (37, 53))
    swapped = R.frames_metrics(*host, swap_blur=True)
    gap = np.abs(swapped[:, IDX['ssim']] - want[:, IDX['ssim']]).max()
    if _gate(got.cpu().numpy(), swapped, 'swapped') is None:
        pytest.skip('the blur order swapped moves the float64 SSIM by %g, inside the gate of %g: no control' % (gap, SSIM_ATOL))


# ---- evaluate_set ---------------------------------------------------------------------------------------------------------
HW, K, T, N, CHUNK, N_CAMS, ALPHA = (24, 32), 3, 3, 32, 200, 2, 6.5


@pytest.fixture(scope='module')
def scene(cuda):
    utils.clear_gin()
    utils.parse_gin('MipNerfModel.num_samples = %d\nMipNerfModel.density_noise = 0.0\nMipNerfModel.no_pose_opt = True\n'
                    'MipNerfModel.no_yaw_opt = True\n' % N)
    config = utils.configured(utils.Config)
    ds = train_boxpose.SyntheticTimestepDataset(config, K=K, T=T, hw=HW, n_cams=N_CAMS, device=cuda, split='test')
    model, variables = obbpose_model.construct_mipnerf(3, ds.peek(), device=cuda)
    # evaluate_set's own float frames: what its render_trajectory calls returned, kept as they pass by
    calls, render = [], model.render_trajectory

    def recording(variables, cams, times, ext, *a, **kw):
        out = render(variables, cams, times, ext, *a, **kw)
        calls.append(dict(times=list(times), ext=ext, outputs=kw['outputs'], out=out))
        return out
    model.render_trajectory = recording
    try:
        res = train_boxpose.evaluate_set(model, config, variables, ds, ALPHA, chunk=CHUNK, obj_mask='boxes', vis=True, frames=True)
    finally:
        del model.render_trajectory
    return config, ds, model, variables, res, calls


def _test_case(ds, config, t, c):
    """the test case SyntheticTimestepDataset._test_case builds, for camera c of timestep t"""
    td = ds.ts_data[t]
    rays, px, dp, sk = raygen.generate_batch(td, None, config.near, config.far)
    n = HW[0] * HW[1]
    img = lambda x: x[c * n:(c + 1) * n].reshape(HW[0], HW[1], -1)
    return dict(rays=utils.namedtuple_map(img, rays), pixels=img(px), depth=img(dp), sky=img(sk), init=ds.init, ext=ds.ext, ts=t)


def test_evaluate_set_is_the_loop_it_replaces(cuda, scene):
    config, ds, model, variables, res, calls = scene
    F = T * N_CAMS
    assert res['frames'] == F >= 2 and res['rays'] == F * HW[0] * HW[1] and res['fields'] == ops.EVAL_FIELDS
    assert res['per_frame'].shape == (F, 10) and res['per_frame'].is_cuda
    assert all(v.is_cuda and v.dim() == 0 for v in res['mean'].values())
    assert sorted(res['mean']) == ['depth_abs', 'depth_rmse', 'obj_psnr', 'psnr', 'ssim']
    # one render_trajectory call per (h, w, ts) group: here the N_CAMS cameras of each timestep, at that integer time
    assert [c['times'] for c in calls] == [[float(t)] * N_CAMS for t in range(T)]
    assert all(c['outputs'] == ('rgb', 'distance', 'acc', 'rgb8') and c['ext'] is ds.ext for c in calls)
    rgbs, dists, gts, gds, masks = [], [], [], [], []
    for f in range(F):
        t, c = f // N_CAMS, f % N_CAMS
        case = _test_case(ds, config, t, c)
        ev = train_boxpose.evaluate(model, config, variables, case, ALPHA, chunk=CHUNK)
        for k in ('rgb', 'distance', 'acc'):      # EVERY frame evaluate_set rendered is evaluate()'s, bit for bit
            assert torch.equal(calls[t]['out'][k][c], ev[k]) and not torch.isnan(ev[k]).any(), (f, k)
        assert torch.equal(res['rgb8'][f], calls[t]['out']['rgb8'][c]), f
        assert torch.equal(res['rgb8'][f], torch.round(ev['rgb'].clamp(0, 1) * 255).to(torch.uint8)), f
        lay = model.render_layers(variables, case['rays'], case['init'], case['ext'], t, config.white_bkgd, ALPHA, chunk=CHUNK,
                                  layers=('instance',))
        mask = (lay['instance'] != -1).to(torch.float32)
        rgbs.append(ev['rgb']); dists.append(ev['distance']); gts.append(case['pixels'][..., :3]); gds.append(case['depth'][..., 0])
        masks.append(mask)
        # the record against the metrics of the loop: PSNR of torch's fp32 mean (an fp32 sum of 2304 terms is off by at most
        # 2304 * 6e-8 = 1.4e-4 relative, i.e. 10 / ln 10 * 1.4e-4 = 6e-4 dB), SSIM of durf_ssim (both fp32 blurs: each within 2e-5
        # of the oracle)
        rec = res['per_frame'][f].cpu().numpy().astype(np.float64)
        assert abs(rec[IDX['psnr']] - float(ev['psnr'])) <= 1e-3 and abs(rec[IDX['ssim']] - float(ev['ssim'])) <= 2 * SSIM_ATOL
        assert rec[IDX['obj_count']] == float(mask.sum()), 'the boxes mask is render_layers\' instance != -1'
    stack = lambda ts: torch.stack(ts).contiguous()
    direct = ops.eval_frames(stack(rgbs), stack(gts), stack(dists), stack(gds), stack(masks))[0]
    assert direct.cpu().numpy().tobytes() == res['per_frame'].cpu().numpy().tobytes()
    host = [stack(ts).cpu().numpy() for ts in (rgbs, gts, dists, gds, masks)]
    assert _gate(res['per_frame'].cpu().numpy(), R.frames_metrics(*host), 'evaluate_set') is None
    per = res['per_frame']
    assert torch.equal(res['mean']['psnr'], per[:, IDX['psnr']].mean()) and torch.equal(res['mean']['ssim'], per[:, IDX['ssim']].mean())
    pf = per.cpu().numpy()
    assert (pf[:, IDX['depth_count']] > 0).all() and (pf[:, IDX['obj_count']] > 0).any()
    have = pf[:, IDX['obj_count']] > 0
    np.testing.assert_allclose(float(res['mean']['obj_psnr']), pf[have, IDX['obj_psnr']].astype(np.float64).mean(), rtol=1e-6)
    np.testing.assert_allclose(float(res['mean']['depth_rmse']), pf[:, IDX['depth_rmse']].astype(np.float64).mean(), rtol=1e-6)
    # the pictures are visualize_suite's
    assert len(res['vis']) == F and sorted(res['vis'][0]) == ['depth', 'depth_mod', 'depth_normals']
    assert res['vis'][1]['depth'].shape == HW + (3,) and res['vis'][1]['depth'].dtype == torch.uint8


def test_next_yields_a_frame_of_the_set(cuda, scene):
    config, ds, model, variables, res, _ = scene
    for _ in range(2):
        case = next(ds)
        ev = train_boxpose.evaluate(model, config, variables, case, ALPHA, chunk=CHUNK)
        f = case['ts'] * N_CAMS
        rec = ops.eval_frames(ev['rgb'][None], case['pixels'][None, ..., :3].contiguous(), ev['distance'][None],
                              case['depth'][None, ..., 0].contiguous())[0][0]
        keep = [IDX[k] for k in ('mse', 'psnr', 'ssim', 'depth_count', 'depth_abs', 'depth_rmse', 'nonfinite')]
        assert rec[keep].cpu().numpy().tobytes() == res['per_frame'][f, keep].cpu().numpy().tobytes()


def test_list_of_masks_and_no_mask(cuda, scene):
    config, ds, model, variables, res, _ = scene
    F = T * N_CAMS
    planes = [torch.zeros(HW) for _ in range(F)]
    planes[2][3:9, 4:20] = 1.0
    got = train_boxpose.evaluate_set(model, config, variables, ds, ALPHA, chunk=CHUNK, obj_mask=planes)
    pf = got['per_frame'].cpu().numpy()
    assert list(pf[:, IDX['obj_count']]) == [0, 0, 96, 0, 0, 0] and np.isnan(pf[[0, 1, 3, 4, 5], IDX['obj_psnr']]).all()
    assert float(got['mean']['obj_psnr']) == pf[2, IDX['obj_psnr']], 'the mean over the frames that have a count'
    assert 'rgb8' not in got and 'vis' not in got
    bare = train_boxpose.evaluate_set(model, config, variables, ds, ALPHA, chunk=CHUNK)
    assert torch.isnan(bare['mean']['obj_psnr']) and torch.equal(bare['per_frame'][:, :3], res['per_frame'][:, :3])


def test_command_writes_the_table_and_the_pictures(cuda, tmp_path):
    out = str(tmp_path / 'eval')
    cmd = [sys.executable, '-m', 'durf_amd.eval_set', '--synthetic', '--eval_dir', out, '--vis', '--frames', '--obj_mask', 'boxes',
           '--gin_param', 'MipNerfModel.num_samples = 32', '--gin_param', 'MipNerfModel.no_pose_opt = True',
           '--gin_param', 'MipNerfModel.no_yaw_opt = True']
    p = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)      # a fresh child process
    assert p.returncode == 0, p.stdout.decode()
    F, h, w = 10, 64, 96                                                 # SyntheticTimestepDataset: 5 timesteps of 2 cameras
    names = ['%s%04d.ppm' % (pre, f) for pre in ('', 'depth_', 'depth_mod_', 'normals_') for f in range(F)]
    assert sorted(os.listdir(out)) == sorted(names + ['metrics.json'])
    doc = json.load(open(os.path.join(out, 'metrics.json')))
    assert doc['fields'] == list(ops.EVAL_FIELDS) and doc['frames'] == F and doc['rays'] == F * h * w
    assert len(doc['per_frame']) == F and all(len(r) == 10 for r in doc['per_frame'])
    assert sorted(doc['mean']) == ['depth_abs', 'depth_rmse', 'obj_psnr', 'psnr', 'ssim']
    psnr = [r[IDX['psnr']] for r in doc['per_frame']]
    assert all(isinstance(v, float) for v in psnr) and abs(doc['mean']['psnr'] - np.mean(psnr)) <= 1e-4
    assert all(r[IDX['nonfinite']] == 0 for r in doc['per_frame'])
    header = b'P6\n%d %d\n255\n' % (w, h)
    for n in names:
        blob = open(os.path.join(out, n), 'rb').read()
        assert blob.startswith(header) and len(blob) == len(header) + h * w * 3, n
