"""Host side of the trajectory render (no GPU): keyframe interpolation, trajectory files, PPM frames, the float64
restatement of the box-pose interpolation rule that tests/test_gpu_trajectory.py holds k_pose_interp to, and the
surface of the new entry points."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from durf_amd import _lib, obbpose_model, synthetic, trajectory, utils
from tests import helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ('durf_render_trajectory', 'durf_render_trajectory_workspace_bytes', 'durf_camera_rays')


# ---- the interpolation rule, restated in float64 (include/durf_hip.h durf_render_trajectory) ------------------------------
def wrap_pi(d):
    """d onto [-pi, pi)"""
    return (np.asarray(d, np.float64) + np.pi) % (2.0 * np.pi) - np.pi


def interp_pose_f64(box_centers, t):
    """box_centers [T,K,6] (any float dtype, taken as they are), t in [0, T - 1] -> [K,6] float64: position
    p_i + w (p_{i+1} - p_i), each angle a_i + w wrap(a_{i+1} - a_i), with i = floor(t), w = t - i; w == 0 is row i itself
    and touches no other row"""
    bc = np.asarray(box_centers, np.float64)
    t = float(t)
    i = int(np.floor(t))
    w = t - i
    assert 0 <= i <= bc.shape[0] - 1
    if w == 0.0:
        return bc[i].copy()
    a, b = bc[i], bc[i + 1]
    out = np.empty_like(a)
    out[:, :3] = a[:, :3] + w * (b[:, :3] - a[:, :3])
    out[:, 3:] = a[:, 3:] + w * wrap_pi(b[:, 3:] - a[:, 3:])
    return out


def test_restatement_takes_the_shorter_arc_and_copies_at_integer_times():
    bc = np.zeros((3, 1, 6))
    bc[0, 0] = [1.0, 2.0, 3.0, 0.1, 3.0, -0.2]
    bc[1, 0] = [2.0, 0.0, 3.5, 0.3, -3.0, -0.4]
    bc[2, 0] = np.nan                                 # w == 0 at t = 1 must not look at row 2
    mid = interp_pose_f64(bc, 0.5)
    assert abs(mid[0, 4]) > 3.0, 'yaw 3.0 -> -3.0 passes through pi, not through 0'
    np.testing.assert_allclose(abs(mid[0, 4]), np.pi, atol=1e-12)      # 3 + 0.5 * (2 pi - 6)
    np.testing.assert_allclose(mid[0, :4], [1.5, 1.0, 3.25, 0.2], atol=1e-15)
    np.testing.assert_allclose(mid[0, 5], -0.3, atol=1e-15)
    for t in (0, 1):
        assert np.array_equal(interp_pose_f64(bc, float(t)), bc[t])
    assert np.array_equal(interp_pose_f64(bc[:2], 1.0), bc[1]), 't = T - 1 is legal'
    np.testing.assert_allclose(wrap_pi([np.pi, -np.pi, 0.0, 2 * np.pi + 0.25]), [-np.pi, -np.pi, 0.0, 0.25], atol=1e-12)


# ---- make_trajectory ------------------------------------------------------------------------------------------------------
def _rz(deg):
    a = np.deg2rad(deg)
    return np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])


def _keys(seed=0, m=4):
    rs = np.random.default_rng(seed)
    keys = np.zeros((m, 3, 4))
    for i in range(m):
        q, _ = np.linalg.qr(rs.normal(size=(3, 3)))
        keys[i, :, :3] = q * np.sign(np.linalg.det(q))
        keys[i, :, 3] = rs.uniform(-2, 2, 3)
    return keys, np.linspace(0.0, 4.0, m)


def test_make_trajectory_endpoints_and_orthonormal_rotations():
    keys, t_keys = _keys()
    c2w, times = trajectory.make_trajectory(keys, t_keys, 31)
    assert c2w.shape == (31, 3, 4) and times.shape == (31,)
    np.testing.assert_allclose(c2w[0], keys[0], atol=1e-12)
    np.testing.assert_allclose(c2w[-1], keys[-1], atol=1e-12)
    assert times[0] == t_keys[0] and times[-1] == t_keys[-1]
    np.testing.assert_allclose(c2w[10], keys[1], atol=1e-12)          # 31 frames over 3 intervals: every 10th is a keyframe
    assert np.all(np.diff(times) > 0)
    for f in range(31):
        R = c2w[f, :, :3]
        np.testing.assert_allclose(R.T @ R, np.eye(3), atol=1e-12)
        assert np.linalg.det(R) > 0
    # positions and times are lerped
    np.testing.assert_allclose(c2w[5, :, 3], 0.5 * (keys[0, :, 3] + keys[1, :, 3]), atol=1e-12)
    np.testing.assert_allclose(times[5], 0.5 * (t_keys[0] + t_keys[1]), atol=1e-12)
    one, t1 = trajectory.make_trajectory(keys[:1], t_keys[:1], 3)
    assert np.array_equal(one, np.repeat(keys[:1], 3, 0)) and np.array_equal(t1, np.repeat(t_keys[:1], 3))
    with pytest.raises(ValueError):
        trajectory.make_trajectory(keys, t_keys[:2], 5)


def test_half_turn_about_z_passes_through_a_quarter_turn():
    keys = np.zeros((2, 3, 4))
    keys[0, :, :3], keys[1, :, :3] = _rz(0.0), _rz(180.0)
    c2w, _ = trajectory.make_trajectory(keys, [0.0, 1.0], 3)
    mid = c2w[1, :, :3]
    assert np.allclose(mid, _rz(90.0), atol=1e-12) or np.allclose(mid, _rz(-90.0), atol=1e-12), mid
    # (a plain lerp of the matrices would give the singular diag(0, 0, 1))
    np.testing.assert_allclose(mid.T @ mid, np.eye(3), atol=1e-12)


# ---- files ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('notebook_format', [False, True])
def test_trajectory_files_round_trip(tmp_path, notebook_format):
    keys, t_keys = _keys(3)
    c2w, times = trajectory.make_trajectory(keys, t_keys, 7)
    path = str(tmp_path / 'traj.npz')
    trajectory.save_trajectory(path, c2w, times, notebook_format=notebook_format)
    with np.load(path, allow_pickle=True) as z:
        assert z.files == (['arr_0'] if notebook_format else ['c2w', 'times'])
        if notebook_format:         # what the notebook's np.savez(path, traj) leaves: [F,2] objects, 4x4 matrices
            assert z['arr_0'].dtype == object and z['arr_0'].shape == (7, 2) and z['arr_0'][0, 0].shape == (4, 4)
    got_c2w, got_t = trajectory.load_trajectory(path)
    assert np.array_equal(got_c2w, c2w) and np.array_equal(got_t, times)
    # the notebook's own way of writing it: a list of [c2w, ts]
    if notebook_format:
        p2 = str(tmp_path / 'nb.npz')
        np.savez(p2, np.array([[np.vstack([c, [0, 0, 0, 1]]), t] for c, t in zip(c2w, times)], dtype=object))
        c3, t3 = trajectory.load_trajectory(p2)
        assert np.array_equal(c3, c2w) and np.array_equal(t3, times)


def test_load_trajectory_refuses_what_it_does_not_know(tmp_path):
    path = str(tmp_path / 'bad.npz')
    np.savez(path, a=np.zeros(3), b=np.zeros(3))
    with pytest.raises(ValueError, match='c2w and times'):
        trajectory.load_trajectory(path)


def test_write_ppm_bytes(tmp_path):
    img = np.arange(18, dtype=np.uint8).reshape(2, 3, 3) * 13        # 2 rows of 3 pixels
    path = str(tmp_path / 'f.ppm')
    trajectory.write_ppm(path, img)
    blob = open(path, 'rb').read()
    header = b'P6\n3 2\n255\n'                                       # width first
    assert blob[:len(header)] == header
    assert blob[len(header):] == img.tobytes() and len(blob) == len(header) + 18
    trajectory.write_ppm(path, torch.from_numpy(img))
    assert open(path, 'rb').read() == blob
    with pytest.raises(ValueError):
        trajectory.write_ppm(path, img.astype(np.float32))


# ---- the surface ----------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, 'include', 'durf_hip.h')).read()
    L = _lib.lib()
    for name in NEW_SYMBOLS:
        assert re.search(r'\b%s\s*\(' % name, hdr), name + ' is not in include/durf_hip.h'
        assert name in _lib._SIGS, name + ' is not in durf_amd/_sigs.py'
        assert hasattr(L, name)
    assert len(_lib._SIGS['durf_render_trajectory'][1]) == 18
    # the workspace does not grow with the image, and grows with the frames by the poses only
    ws = L.durf_render_trajectory_workspace_bytes
    K = 3
    assert ws(8, 8192, 128, K, 2) - ws(2, 8192, 128, K, 2) <= 6 * K * 24 + 256
    img = L.durf_render_image_workspace_bytes(8192, 128, K, 2)
    assert 0 < ws(2, 8192, 128, K, 2) - img <= 8192 * 12 * 4 + 7 * 256 + 2 * K * 24 + 256, 'one chunk of rays beside the image call\'s'
    from durf_amd import ops
    assert {'TRAJ_RAYS', 'TRAJ_POSE', 'TRAJ_PACK'} <= set(ops.LAYER_LOG)
    for m in re.finditer(r'#define DURF_LAYERLOG_(\w+) (0x[0-9a-fA-F]+)', hdr):
        assert ops.LAYER_LOG[m.group(1)] == int(m.group(2), 16)


def test_refusals_need_no_device():
    """the argument checks of durf_render_trajectory run before anything touches the GPU"""
    import ctypes as C
    from durf_amd import ops
    L = _lib.lib()
    a = ops.ForwardArgs()
    a.N, a.K, a.num_levels = 32, 0, 2
    cams = np.zeros((2, 17), np.float32)
    cams[:, 15:] = (24, 32)
    fake = C.c_void_p(256)                                            # never dereferenced: every call below is refused first

    def call(F, cams, times, T=5, rgb=fake, ws_bytes=1 << 40):
        arr = (C.c_float * cams.size)(*cams.reshape(-1).tolist())
        return L.durf_render_trajectory(None, C.byref(a), None, None, T, F, arr, (C.c_float * len(times))(*times), 0.0, 40.0, 200,
                                        None, rgb, None, None, None, fake, ws_bytes)
    assert call(2, cams, [0.0, 4.5]) == -1
    assert re.search(r'time 4\.5 of frame 1 is outside \[0, 4\]', L.durf_last_error().decode())
    assert call(2, cams, [-0.25, 1.0]) == -1 and 'frame 0' in L.durf_last_error().decode()
    mixed = cams.copy()
    mixed[1, 15] = 20
    assert call(2, mixed, [0.0, 1.0]) == -1
    assert re.search(r'frame 1 is 20 x 32, frame 0 is 24 x 32', L.durf_last_error().decode())
    assert call(0, cams, [0.0]) == -1 and 'F > 0' in L.durf_last_error().decode()
    assert call(2, cams, [0.0, 1.0], rgb=None) == -1 and 'at least one output' in L.durf_last_error().decode()
    need = int(L.durf_render_trajectory_workspace_bytes(2, 200, 32, 0, 2))
    assert call(2, cams, [0.0, 1.0], ws_bytes=need - 256) == -1
    assert re.search(r'durf_render_trajectory: workspace of %d bytes.* = %d' % (need - 256, need), L.durf_last_error().decode())


def test_cpu_tensors_are_refused_like_the_sibling_calls():
    utils.clear_gin()
    utils.parse_gin('MipNerfModel.num_samples = 32\nMipNerfModel.no_pose_opt = True\nMipNerfModel.no_yaw_opt = True\n')
    b = synthetic.make_batch(64, 2, seed=3)
    model, variables = obbpose_model.construct_mipnerf(0, H.oracle_batch(b), device='cpu')
    cams = trajectory.camera_rows(np.eye(4)[None, :3], 30.0, (16.0, 12.0), 24, 32)
    with pytest.raises(NotImplementedError, match=r'durf_render_trajectory covers the bf16 inference path'):
        model.render_trajectory(variables, cams, [0.0], torch.as_tensor(b['ext']), False, 6.5, near=0.0, far=40.0)
    with pytest.raises(NotImplementedError, match=r'durf_render_trajectory covers the bf16 inference path'):
        model.interpolate_pose(variables, 0.5)
    utils.clear_gin()


def test_command_help_exits_cleanly():
    p = subprocess.run([sys.executable, '-m', 'durf_amd.render_traj', '--help'], cwd=ROOT, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=120)
    assert p.returncode == 0, p.stdout.decode()
    out = p.stdout.decode()
    for flag in ('--eval_dir', '--traj', '--train_dir', '--cam', '--disable_box', '--synthetic'):
        assert flag in out
