"""The box overlay on the GPU (csrc/overlay.hip through durf_amd/overlay.py and ops.project_boxes / ops.draw_boxes), held to the
float64 restatement tests/overlay_ref.py (pinned to the ray generator and the oracle's box test by tests/test_overlay_host.py).
Inputs are seeded and built by overlay_ref.gpu_case: F = 3 frames of 37 x 53 with K = 1, 3, 8, 16, one frame of 5 x 7, F = 2 of
320 x 480 (many tiles, a frame stride), and K = 0 / F = 0; from K = 8 on the boxes include a rotation vector of exactly 0, one of
length pi - 1e-3, a box straddling znear, one behind the camera, one off-screen, one with an edge seen end-on (a segment of
length zero) and a disabled one.

Tolerances:
  segments, rect   per box, 4 x the largest |float32 twin - float64| over that box's segments and rectangle on the same inputs,
                   at least 1e-5 px, computed when the test runs; NaNs in the same places, `visible` exact.  Measured twin
                   errors (largest / median over the boxes of a case, px): k1 2.6e-6 / 2.0e-6, k3 1.2e-5 / 3.6e-6, k8 1.3e-3 /
                   2.6e-6 (the largest is the box cut at znear, coordinates up to 2460 px), k16 9.5e-5 / 2.0e-6, tiny 4.2e-7 /
                   4.1e-7, big 7.3e-5 / 2.2e-5.
  rasteriser       the float64 reference is fed the device's own fp32 segments.  `label` equals it except at undecided pixels:
                   some box's float64 distance within EDGE of the half width, EDGE = 4 x the twin's largest distance error on
                   the case, at least 1e-4 px (measured twin distance errors: k1 4.8e-6, k3 6.5e-6, k8 6.9e-5, k16 3.2e-5, tiny
                   3.8e-7, big 4.9e-5, so EDGE is 1e-4 on k1, k3, tiny; 2.8e-4 on k8, 1.3e-4 on k16, 2.0e-4 on big).
                   Undecided pixels are first shown to be <= 5 % of the reference's drawn pixels (measured: none on k1, k3, tiny
                   and k8 at width 1.0; 1.8 % on k8 at width 1.5, 0.5 % on k16, 0.02 % on big).
                   Measured device errors against float64, as a share of the tolerance: 0.07 (tiny) .. 0.55 (k16).
  colours          opacity 1: owned pixels are the palette's bytes / col / 255 as fp32 exactly; opacity 0.5: within one level of
                   the float64 blend; pixels no box owns are the input's bits."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from durf_amd import ops, overlay, raygen
from tests import overlay_ref as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = [c[0] for c in O.GPU_CASES]
_CACHE = {}


def case(name, dev):
    """the case's inputs, the float64 reference and its twin (computed once), and the device's table"""
    if name not in _CACHE:
        c = O.gpu_case(name)
        c['ref'] = O.project_boxes(c['cams'], c['poses'], c['ext'], c['enable'], c['znear'], np.float64)
        c['twin'] = O.project_boxes(c['cams'], c['poses'], c['ext'], c['enable'], c['znear'], np.float32)
        c['dev'] = overlay.project_boxes(c['cams'], torch.tensor(c['poses'], device=dev), torch.tensor(c['ext'], device=dev),
                                         box_enable=c['enable'], znear=c['znear'])
        c['raster'] = {}
        _CACHE[name] = c
    return _CACHE[name]


def raster(c, width):
    """the float64 rasteriser reference on the device's own segments (computed once per case and width)"""
    if width not in c['raster']:
        c['raster'][width] = O.raster_reference(c['dev']['segments'].cpu().numpy(), c['h'], c['w'], width / 2.0)
    return c['raster'][width]


def seeded_frames(c, dtype, dev, seed=7):
    rng = np.random.default_rng(seed)
    shape = (c['F'], c['h'], c['w'], 3)
    if dtype == torch.uint8:
        return torch.tensor(rng.integers(0, 256, shape, dtype=np.uint8), device=dev)
    return torch.tensor(rng.uniform(0.0, 1.0, shape).astype(np.float32), device=dev)


@pytest.mark.parametrize('name', NAMES)
def test_segments_and_rect(cuda, name):
    c = case(name, cuda)
    (s64, r64), (s32, r32) = c['ref'], c['twin']
    seg, rect = c['dev']['segments'].cpu().numpy(), c['dev']['rect'].cpu().numpy()
    F, K = c['F'], c['K']
    assert seg.shape == (F, K, 12, 4) and rect.shape == (F, K, 6) and seg.dtype == np.float32
    assert (np.isnan(s32) == np.isnan(s64)).all() and (np.isnan(r32) == np.isnan(r64)).all()
    assert (np.isnan(seg) == np.isnan(s64)).all(), 'culled segments'
    assert (np.isnan(rect) == np.isnan(r64)).all()
    assert (rect[..., 5] == r64[..., 5]).all(), 'visible'
    assert (c['dev']['visible'].cpu().numpy() == (r64[..., 5] == 1.0)).all()
    assert torch.equal(c['dev']['depth'], c['dev']['rect'][..., 4])
    both64 = np.concatenate([s64.reshape(F, K, -1), r64[..., :5]], -1)
    both32 = np.concatenate([s32.reshape(F, K, -1), r32[..., :5]], -1).astype(np.float64)
    got = np.concatenate([seg.reshape(F, K, -1), rect[..., :5]], -1).astype(np.float64)
    ok = ~np.isnan(both64)
    twin_err = np.where(ok, np.abs(both32 - both64), 0.0).max(-1)                     # [F,K]
    err = np.where(ok, np.abs(got - both64), 0.0).max(-1)
    tol = np.maximum(4.0 * twin_err, 1e-5)
    print('%s: twin error per box max %.2e median %.2e; device error max %.2e, worst error / tolerance %.2f'
          % (name, twin_err.max(), np.median(twin_err), err.max(), (err / tol).max()))
    assert (err <= tol).all(), (name, np.argwhere(err > tol).tolist(), err.max())


@pytest.mark.parametrize('name,width', [(c[0], wd) for c in O.GPU_CASES for wd in c[5]])
def test_rasteriser_and_colours(cuda, name, width):
    c = case(name, cuda)
    ref = raster(c, width)
    print('%s width %.1f: drawn %d, undecided %d (%.2f %%), EDGE %.2e, twin distance error %.2e'
          % (name, width, ref['drawn'].sum(), ref['undecided'].sum(), 100 * ref['share'], ref['edge'], ref['twin_err']))
    assert ref['drawn'].sum() > 0
    assert ref['share'] <= 0.05, 'undecided pixels are at most 5 % of the drawn ones'
    seg = c['dev']['segments']
    K = c['K']
    pal = overlay.PALETTE[:K]
    src8 = seeded_frames(c, torch.uint8, cuda)
    srcf = seeded_frames(c, torch.float32, cuda)
    out8, lab = overlay.draw_boxes(src8, seg, width=width, label=True)
    outf, labf = overlay.draw_boxes(srcf, seg, width=width, label=True)
    half8, labh = overlay.draw_boxes(src8, seg, width=width, opacity=0.5, label=True)
    assert out8.data_ptr() != src8.data_ptr() and lab.dtype == torch.int32
    assert torch.equal(lab, labf) and torch.equal(lab, labh)
    lab = lab.cpu().numpy()
    decided = ~ref['undecided']
    assert (lab[decided] == ref['label'][decided]).all(), np.argwhere(decided & (lab != ref['label']))[:5].tolist()
    assert ((lab >= -1) & (lab < K)).all()
    # every drawn reference pixel that is not undecided is drawn, every undrawn one is untouched
    a8, b8 = src8.cpu().numpy(), out8.cpu().numpy()
    af, bf = srcf.cpu().numpy(), outf.cpu().numpy()
    h8 = half8.cpu().numpy()
    owned = lab >= 0
    assert owned[decided & ref['drawn']].all() and not owned[decided & ~ref['drawn']].any()
    for a, b in ((a8, b8), (af, bf), (a8, h8)):
        assert (a[~owned].view(np.uint8) == b[~owned].view(np.uint8)).all(), 'pixels no box owns keep their bits'
    # opacity 1: the palette itself
    assert (b8[owned] == pal[lab[owned]]).all()
    assert (bf[owned] == (pal.astype(np.float32) / np.float32(255.0))[lab[owned]]).all()
    # opacity 0.5: within one level of the float64 blend
    want = a8[owned].astype(np.float64) + 0.5 * (pal[lab[owned]].astype(np.float64) - a8[owned].astype(np.float64))
    assert np.abs(h8[owned].astype(np.float64) - want).max() <= 1.0
    assert (h8[owned] != b8[owned]).any()


def test_float_blend(cuda):
    c = case('k3', cuda)
    srcf = seeded_frames(c, torch.float32, cuda)
    out, lab = overlay.draw_boxes(srcf, c['dev']['segments'], opacity=0.25, label=True)
    lab, a, b = lab.cpu().numpy(), srcf.cpu().numpy().astype(np.float64), out.cpu().numpy().astype(np.float64)
    owned = lab >= 0
    want = a[owned] + 0.25 * (overlay.PALETTE[lab[owned]].astype(np.float64) / 255.0 - a[owned])
    assert np.abs(b[owned] - want).max() <= 4 * 2.0 ** -24                # three fp32 roundings of values in [0, 1]
    assert (a[~owned] == b[~owned]).all()


def test_inplace_custom_colours_and_label_alone(cuda):
    c = case('k3', cuda)
    seg = c['dev']['segments']
    src8 = seeded_frames(c, torch.uint8, cuda)
    want, lab = overlay.draw_boxes(src8, seg, colors=[[1, 2, 3], [4, 5, 6], [7, 8, 9]], label=True)
    mine = src8.clone()
    assert overlay.draw_boxes(mine, seg, colors=torch.tensor([[1, 2, 3], [4, 5, 6], [7, 8, 9]]), inplace=True) is mine
    assert torch.equal(mine, want)
    owned = lab >= 0
    assert torch.equal(want[owned].to(torch.int32), (3 * lab[owned])[:, None] + torch.tensor([1, 2, 3], device=cuda, dtype=torch.int32))
    only = torch.full((c['F'], c['h'], c['w']), 99, dtype=torch.int32, device=cuda)
    ops.draw_boxes(seg, torch.tensor(overlay.PALETTE[:3], device=cuda), 0.75, label=only)
    assert torch.equal(only, lab)


@pytest.mark.parametrize('name', ['k3', 'tiny', 'big'])
def test_alignment(cuda, name):
    """frames that start 1 byte (uint8) / 4 bytes (float) into their allocation get the pixels the aligned ones get"""
    c = case(name, cuda)
    seg, col = c['dev']['segments'], torch.tensor(overlay.PALETTE[:c['K']], device=cuda)
    shape = (c['F'], c['h'], c['w'], 3)
    n = int(np.prod(shape))
    for dtype, key in ((torch.uint8, 'frames8'), (torch.float32, 'framesf')):
        src = seeded_frames(c, dtype, cuda)
        aligned = src.clone()
        buf = torch.zeros(n + 16, dtype=dtype, device=cuda)
        shifted = buf[1:1 + n].view(shape)
        shifted.copy_(src)
        assert aligned.data_ptr() % 16 == 0 and shifted.data_ptr() % 16 == (1 if dtype == torch.uint8 else 4)
        ops.draw_boxes(seg, col, 0.75, 0.5, **{key: aligned})
        ops.draw_boxes(seg, col, 0.75, 0.5, **{key: shifted})
        assert torch.equal(aligned, shifted) and not torch.equal(aligned, src)
        assert buf[0] == 0 and (buf[1 + n:] == 0).all(), 'nothing is written outside the frames'


def test_no_boxes_and_no_frames(cuda):
    cams = O.gpu_case('k1')['cams']
    ext0 = torch.zeros(0, 3, device=cuda)
    p = overlay.project_boxes(cams, torch.zeros(3, 0, 6, device=cuda), ext0)
    assert tuple(p['segments'].shape) == (3, 0, 12, 4) and tuple(p['rect'].shape) == (3, 0, 6) and tuple(p['visible'].shape) == (3, 0)
    src = torch.tensor(np.random.default_rng(0).integers(0, 256, (3, 37, 53, 3), dtype=np.uint8), device=cuda)
    out, lab = overlay.draw_boxes(src, p['segments'], label=True)
    assert torch.equal(out, src) and (lab == -1).all()
    assert torch.equal(overlay.draw_boxes(src, p['segments']), src)
    p = overlay.project_boxes(cams[:0], torch.zeros(0, 3, 6, device=cuda), torch.ones(3, 3, device=cuda))
    assert tuple(p['segments'].shape) == (0, 3, 12, 4)
    out, lab = overlay.draw_boxes(torch.zeros(0, 37, 53, 3, dtype=torch.uint8, device=cuda), p['segments'], label=True)
    assert tuple(out.shape) == (0, 37, 53, 3) and tuple(lab.shape) == (0, 37, 53)


def test_refusals(cuda):
    L, last = ops._lib.overlay_lib(), ops._lib.lib().durf_last_error       # (errors are reported through libdurf_hip.so)
    buf = torch.zeros(17 * 48 * 4, device=cuda)
    p = buf.data_ptr()
    assert L.durf_project_boxes(None, 1, 17, p, p, p, None, 0.5, p, p) != 0
    assert b'DURF_MAX_OBJ' in last()
    assert L.durf_project_boxes(None, 1, 1, p, p, p, None, 0.0, p, p) != 0
    assert b'znear' in last()
    assert L.durf_draw_boxes(None, 1, 4, 4, 17, p, p, 0.75, 1.0, p, None, None) != 0
    assert b'DURF_MAX_OBJ' in last()
    assert L.durf_draw_boxes(None, 1, 4, 4, 1, p, p, 0.75, 1.0, None, None, None) != 0
    assert b'at least one' in last()
    assert L.durf_draw_boxes(None, 1, 4, 4, 1, p, p, 0.75, 1.5, p, None, None) != 0
    assert b'opacity' in last()
    assert (buf == 0).all()


def test_agrees_with_the_renderers_box_test(cuda):
    """Guards the conventions: for a camera of raygen.camera_rays and three boxes wholly in view, the pixels whose rays
    ops.ray_setup says hit box k lie inside rect[k] (grown by 1 px), span it (within 1 px), and none lies farther than the
    half width outside the outline drawn for that box alone.  (How far the outermost pixel CENTRE inside a silhouette lies from
    the silhouette's outermost vertex depends on how sharp that vertex is: over eight seeds of this scene the float64 box test
    gave 0.4 .. 1.3 px.  The seed used here gives 0.53 / 0.42 / 0.93 px for the three boxes on float64 alone.)"""
    h, w, K = 48, 64, 3
    rng = np.random.default_rng(2)
    cam = O.camera_row(O.look_at((0.1, -0.2, 0.05), (6.0, 0.3, -0.1)), 0.9 * w, (w - 1) / 2.0 + 0.3, (h - 1) / 2.0 - 0.2, h, w)
    poses = np.zeros((1, K, 6), np.float32)
    poses[0, :, :3] = [[6.0, -1.3, 0.5], [7.5, 0.3, -0.8], [5.5, 1.3, 0.3]]
    poses[0, :, 3:] = rng.normal(size=(K, 3)) * 0.8
    ext = rng.uniform(0.45, 0.8, (K, 3)).astype(np.float32)
    pose_d, ext_d = torch.tensor(poses, device=cuda), torch.tensor(ext, device=cuda)
    rays = raygen.camera_rays(cam, 0.1, 30.0, device=cuda)
    hit = ops.ray_setup(rays.origins.reshape(-1, 3).contiguous(), rays.directions.reshape(-1, 3).contiguous(), pose_d[0], ext_d)[2]
    hit = hit.reshape(h, w, K).cpu().numpy() != 0
    p = overlay.project_boxes(cam[None], pose_d, ext_d)
    rect = p['rect'][0].cpu().numpy()
    for k in range(K):
        ys, xs = np.nonzero(hit[:, :, k])
        assert len(xs) > 20
        xmin, ymin, xmax, ymax = rect[k, :4]
        assert rect[k, 5] == 1.0 and xmin > 0 and ymin > 0 and xmax < w - 1 and ymax < h - 1, 'wholly in view'
        assert xs.min() >= xmin - 1 and xs.max() <= xmax + 1 and ys.min() >= ymin - 1 and ys.max() <= ymax + 1
        assert abs(xs.min() - xmin) <= 1 and abs(xs.max() - xmax) <= 1 and abs(ys.min() - ymin) <= 1 and abs(ys.max() - ymax) <= 1
        seg_k = torch.full_like(p['segments'], float('nan'))
        seg_k[:, k] = p['segments'][:, k]
        lab = overlay.draw_boxes(torch.zeros(1, h, w, 3, dtype=torch.uint8, device=cuda), seg_k, width=1.5, label=True)[1]
        drawn = lab[0].cpu().numpy() == k
        # the outline's hull, row by row: between the first and the last drawn pixel of the row
        for y in np.unique(ys):
            row = np.nonzero(drawn[y])[0]
            assert len(row), 'a row with hit pixels crosses the outline'
            x_hit = xs[ys == y]
            assert x_hit.min() >= row.min() - 0.75 and x_hit.max() <= row.max() + 0.75, (k, y)


def test_overlay_trajectory(cuda):
    c = case('k3', cuda)
    F, h, w, K = c['F'], c['h'], c['w'], c['K']
    src8 = seeded_frames(c, torch.uint8, cuda)
    srcf = seeded_frames(c, torch.float32, cuda)
    out = dict(rgb8=src8.reshape(F, h * w, 3), rgb=srcf.reshape(F, h * w, 3), poses=torch.tensor(c['poses'], device=cuda))
    keep8 = src8.clone()
    res = overlay.overlay_trajectory(out, c['cams'], c['ext'], box_enable=c['enable'], znear=c['znear'], label=True)
    assert torch.equal(src8, keep8), 'the rendered frames are left as they are'
    same = lambda a, b: torch.equal(a.view(torch.int32), b.view(torch.int32))        # bits: the NaNs of culled boxes too
    assert same(res['rect'], c['dev']['rect']) and same(res['segments'], c['dev']['segments'])
    assert tuple(res['rgb8'].shape) == (F, h * w, 3) and tuple(res['rgb'].shape) == (F, h * w, 3)
    want8, lab = overlay.draw_boxes(src8, c['dev']['segments'], label=True)
    assert torch.equal(res['rgb8'].reshape(F, h, w, 3), want8) and torch.equal(res['label'], lab)
    assert torch.equal(res['rgb'].reshape(F, h, w, 3), overlay.draw_boxes(srcf, c['dev']['segments']))


def test_render_traj_command_with_boxes(cuda, tmp_path):
    """--boxes adds boxes_%04d.ppm and boxes2d.npy; the frames themselves are what a run without it writes (one child process
    runs the command twice)"""
    plain, boxes = str(tmp_path / 'plain'), str(tmp_path / 'boxes')
    common = ['--synthetic', '--frames', '2', '--gin_param', 'MipNerfModel.num_samples = 32', '--gin_param',
              'MipNerfModel.no_pose_opt = True', '--gin_param', 'MipNerfModel.no_yaw_opt = True', '--disable_box', '1']
    code = ('import sys; from durf_amd import render_traj as r; a = %r; '
            'sys.exit(r.main(a + ["--eval_dir", %r]) or r.main(a + ["--eval_dir", %r, "--boxes", "--box_width", "2"]))'
            % (common, plain, boxes))
    p = subprocess.run([sys.executable, '-c', code], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert p.returncode == 0, p.stdout.decode()
    assert sorted(os.listdir(plain)) == ['0000.ppm', '0001.ppm', 'distance.npy']
    assert sorted(os.listdir(boxes)) == ['0000.ppm', '0001.ppm', 'boxes2d.npy', 'boxes_0000.ppm', 'boxes_0001.ppm', 'distance.npy']
    read = lambda d, n: open(os.path.join(d, n), 'rb').read()
    for n in ('0000.ppm', '0001.ppm', 'distance.npy'):
        assert read(plain, n) == read(boxes, n), n
    h, w = 64, 96                                                        # SyntheticTimestepDataset's image
    header = b'P6\n%d %d\n255\n' % (w, h)
    frame, drawn = read(boxes, '0000.ppm'), read(boxes, 'boxes_0000.ppm')
    assert drawn[:len(header)] == header and len(drawn) == len(frame)
    rect = np.load(os.path.join(boxes, 'boxes2d.npy'))
    assert rect.shape == (2, 3, 6) and rect.dtype == np.float32
    assert (rect[:, 1, 5] == 0).all() and np.isnan(rect[:, 1, :4]).all(), 'the box switched off is not drawn'
    a = np.frombuffer(frame, np.uint8, offset=len(header)).reshape(h, w, 3)
    b = np.frombuffer(drawn, np.uint8, offset=len(header)).reshape(h, w, 3)
    changed = (a != b).any(-1)
    assert rect[0, :, 5].sum() >= 1 and changed.any(), 'a visible box is drawn'
    ys, xs = np.nonzero(changed)
    vis = rect[0, rect[0, :, 5] == 1]
    assert xs.min() >= vis[:, 0].min() - 2 and xs.max() <= vis[:, 2].max() + 2 and ys.min() >= vis[:, 1].min() - 2 and ys.max() <= vis[:, 3].max() + 2
    colours = {tuple(px) for px in b[changed].tolist()}
    assert any(tuple(overlay.PALETTE[k].tolist()) in colours for k in np.nonzero(rect[0, :, 5] == 1)[0])
