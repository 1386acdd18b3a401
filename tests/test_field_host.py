"""The field at world points without a device: tests/field_ref.py pinned on closed forms and against the oracle's own model
(the semantics pin: what "the field at X" means, and the documented difference from a render), the three-way agreement of
include/durf_field.h, durf_amd/_field_sigs.py and libdurf_field.so's symbol table, every refusal of the entry points (they need
no device), the workspace sizer, and the refusals and writers of durf_amd/field.py."""
import ctypes as C
import json
import os
import re
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

from durf_amd import _lib, field, ops, synthetic
from oracle import durf_ref as R
from tests import enc_rows_ref as E
from tests import field_ref as F
from tests import lattice_ref
from tests import overlay_ref as OR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = {'durf_field_classify', 'durf_field_lists', 'durf_field_owned', 'durf_field_encode', 'durf_field_activate',
         'durf_field_workspace_bytes', 'durf_field_query', 'durf_field_grid', 'durf_field_columns'}
FAKE = 4096              # a non-null, 256-byte aligned address no refused call may touch


def _err():
    return _lib.lib().durf_last_error().decode()


# ---- the oracle ---------------------------------------------------------------------------------------------------------------
def test_sigma_zero_is_the_positional_encoding_of_the_contracted_point():
    pts, _ = F.enc_points()
    t = F.encode_bkgd(pts, 0.0, True)
    with E._reference_wrap():
        want = R.pos_enc(t['x'], 0, 10, False)
    # pos_enc takes a plain sine of y + pi/2 in float64; the reference's cosine half is at fl32(y + fl32(pi/2)) and wrapped
    sc = torch.tensor([2.0 ** g for g in range(10)], dtype=torch.float64)
    y = (t['x'][:, None, :] * sc[:, None]).reshape(-1, 30)
    ref = E._reference_sin(torch.cat([y, y + 0.5 * np.pi], -1))
    assert float((t['enc'] - ref).abs().max()) <= 1e-12
    small = (torch.cat([y, y], -1).abs() < 100).all(-1)             # where neither statement wraps nor rounds visibly
    assert bool(small.any())
    assert float((t['enc'] - want)[small].abs().max()) <= 1e-12 + float(np.float32(2.0 ** -17))
    o = F.encode_obj(pts, 0.0, 10.0)
    assert float((o['enc'][:, :3] - torch.tensor(pts).double()).abs().max()) == 0.0


def test_a_wide_gaussian_has_no_sine_features():
    pts, _ = F.enc_points()
    assert float(F.encode_bkgd(pts, 1e3, False)['enc'].abs().max()) == 0.0
    # (through the contraction only inside its inner ball: further out it shrinks the Gaussian with the point, by 1 / n^2)
    inner = (pts[:9] * np.float32(0.09)).astype(np.float32)
    assert float(F.encode_bkgd(inner, 1e3, True)['enc'].abs().max()) == 0.0
    o = F.encode_obj(pts[:9], 1e3, 10.0)['enc']
    assert float(o[:, 3:].abs().max()) == 0.0 and float(o[:, :3].abs().max()) > 0


def test_the_contraction_is_the_references_and_switches_at_a_tenth():
    """the reference contracts from norm 0.1 (internal/mip360.py:47-60), not from 1: below it a point is untouched, between
    0.1 and 1 it is NOT (2 - 1/n is negative up to 0.5)"""
    u = np.array([0.6, -0.64, 0.48])
    inner = np.stack([u * r for r in (0.0, 1e-3, 0.05, 0.0999)]).astype(np.float32)
    x, v = F.gaussian(inner, 0.1, True)
    assert float((x - torch.tensor(inner).double()).abs().max()) == 0.0
    assert float((v - float(np.float32(0.1)) ** 2).abs().max()) <= 1e-18
    mid = np.stack([u * r for r in (0.1001, 0.3, 0.9)]).astype(np.float32)
    x, _ = F.gaussian(mid, 0.0, True)
    n = np.linalg.norm(mid.astype(np.float64), axis=1)
    want = (2 - 1 / n)[:, None] * mid.astype(np.float64) / n[:, None]
    assert float((x.numpy() - want).__abs__().max()) <= 1e-12 and float(np.abs(want - mid).min(0).max()) > 1e-3


def test_corners_of_a_rotated_box_against_the_overlays():
    pose, ext, _ = F.scene()
    for s, inside in ((0.99, True), (1.02, False)):
        P = OR.world_corners(pose[None], ext * s, np.float64)[0]               # [K,8,3]
        for k in range(3):
            c = F.classify(P[k], pose[k:k + 1], ext[k:k + 1])
            assert bool((c['inside'][:, 0] == inside).all()), (s, k)
            assert bool((c['owner'] == (0 if inside else -1)).all())
            if inside:
                np.testing.assert_allclose(np.abs(c['local']), np.tile(ext[k] * s, (8, 1)), rtol=1e-6)


def test_the_planted_points_keep_their_margin_and_cover_every_owner():
    pose, ext, en = F.scene()
    pts, tags = F.planted_points()
    c = F.classify(pts, pose, ext, en)
    assert float(c['margin'].min()) >= F.MARGIN - 1e-6
    assert set(np.unique(c['owner'])) == {-2, -1, 0, 1} and 'disabled' in tags and 'overlap' in tags
    dis = [i for i, t in enumerate(tags) if t == 'disabled']
    assert (c['owner'][dis] == -1).all() and (F.classify(pts[dis], pose, ext)['owner'] == 2).all()
    assert (c['owner'][[i for i, t in enumerate(tags) if t == 'overlap']] == -2).all()
    for n in F.SIZES:
        p, _ = F.planted_points(n)
        assert p.shape == (n, 3) and (p == pts[:n]).all()
    ls = F.lists(c['owner'], 3)
    assert sum(l.size for l in ls) == int((c['owner'] != -2).sum()) and ls[2].size == 0
    assert all((np.diff(l) > 0).all() for l in ls if l.size > 1)


def test_the_yardstick_is_the_float32_twins_distance():
    fresh = F.twin_local()
    assert F.YARDSTICK['local'] - 0.011 <= fresh <= F.YARDSTICK['local'] + 1e-9, fresh
    for got, want in zip(F.twin_act(), F.YARDSTICK['act']):
        assert 0.9 * want - 1e-12 <= got <= want, (got, want)
    enc = F.twin_enc()
    assert set(enc) == set(F.YARDSTICK['enc']) == {(l, c) for l in F.ENC_LABELS for c in (False, True)}
    for k, (dx, dv) in enc.items():
        wx, wv = F.YARDSTICK['enc'][k]
        assert wx - 0.011 <= dx <= wx + 1e-9, (k, dx, wx)
        assert 0.9 * wv - 1e-12 <= dv <= wv, (k, dv, wv)
    assert max(v[0] for v in F.YARDSTICK['enc'].values()) < 6
    doc = F.__doc__
    for l in F.ENC_LABELS:
        a, b = F.YARDSTICK['enc'][(l, False)], F.YARDSTICK['enc'][(l, True)]
        assert '%-11s (%.2f, %.1e) | (%.2f, %.1e)' % (l, a[0], a[1], b[0], b[1]) in doc, l
    out = subprocess.run([sys.executable, '-m', 'tests.field_ref'], cwd=ROOT, check=True, capture_output=True, text=True).stdout
    assert "'local': %.2f," % F.YARDSTICK['local'] in out


def test_columns_and_grid_oracle():
    g = lattice_ref.points(dict(origin=(1, 2, 3), du=(0.5, 0, 0), dv=(0, 0.25, 0), dw=(0, 0, 2)), (2, 3, 4), np.float64)
    assert g.shape == (24, 3) and (g[1] == (1, 2, 5)).all() and (g[4] == (1, 2.25, 3)).all() and (g[12] == (1.5, 2, 3)).all()
    d = np.array([[[0.5, np.nan, 3.0, 2.0], [1.0, 1.0, 1.0, 1.0]]], np.float32)
    v = np.array([[[1, 1, 0, 1], [0, 0, 0, 0]]], np.uint8)
    cmax, s, op, first = F.columns(d, v, (1, 2, 4), 0.5, 1.5)
    assert cmax[0, 0] == 2.0 and np.isnan(cmax[0, 1]) and s[0, 0] == 2.5 and s[0, 1] == 0
    assert first[0, 0] == 3 and first[0, 1] == -1 and abs(op[0, 0] - (1 - np.exp(-1.25))) < 1e-15 and op[0, 1] == 0


# ---- the semantics pin --------------------------------------------------------------------------------------------------------
def _captured_model(params, ob, ts, N):
    """the oracle's model with disable_integration on cylinder rays (the sample mean is origins_s + t_mid dirs_s), its MLP
    calls recorded -> per level a dict raw [B,N,4] (the sum the reference forms), t_mids [B,N], hit [B,K]"""
    calls = []

    def hook(p, x, cond, cfg):
        out = R.mlp_apply(p, x, cond, cfg)
        calls.append((p, out))
        return out
    cfg = dict(num_samples=N, disable_integration=True, ray_shape='cylinder')
    with torch.no_grad(), E._reference_wrap():
        ret = R.model_apply(params, ob['rays'], ts, ob['ext'], False, False, False, 10.0, cfg=cfg, mlp_hook=hook)
    K = params['box_centers'].shape[1]
    hit = (ret[0][8].reshape(-1) > 0)
    levels = []
    for lvl in range(2):
        cs = calls[lvl * (K + 1):(lvl + 1) * (K + 1)]
        levels.append(dict(obj=[torch.cat(c[1], -1) for c in cs[:K]], bkgd=torch.cat(cs[K][1], -1), t_mids=ret[lvl][5]))
    return levels, ret


def test_the_field_at_a_sample_is_what_the_model_evaluates_there():
    """On rays that hit no box the oracle's per-sample raw is the query at origins + t_mid dirs; on a ray that hits one box
    it is the query at c + R^T (origins_s + t_mid dirs_s) on the samples inside the box -- and NOT on the samples outside it,
    which a render hands to the BoxMLP and the query to the background: the documented difference."""
    B, K, N, ts = 48, 2, 32, 1
    b = synthetic.make_batch(B, K, seed=9, hit_range=(0.3, 0.4))
    ob = R.batch_from_numpy(b, torch.float64)
    ob['init'] = ob['init'].float().double()                   # (pose and extents are fp32 values in the library's hands)
    ob['ext'] = ob['ext'].float().double()
    params = R.init_params(3, ob['init'], K, dtype=torch.float64)
    g = torch.Generator().manual_seed(1)
    for name in ('MLP_0', 'BoxMLP_0', 'BoxMLP_1'):
        for kb in params[name]:
            kb[1] += (torch.rand(kb[1].shape, generator=g, dtype=torch.float64) - 0.5) * 0.1
    levels, ret = _captured_model(params, ob, ts, N)
    rays = ob['rays']
    pose = params['box_centers'][ts].numpy()
    ext = ob['ext'].numpy().reshape(K, 3)
    e = ob['ext'].reshape(K, 3).expand(B, K, 3)
    o_o, d_o = R.world2object_rpy(rays.origins, rays.directions, params['box_centers'][ts, :, :3].expand(B, K, 3),
                                  R.aa2matrix(params['box_centers'][ts, :, 3:]).expand(B, K, 3, 3))
    _, _, inter = R.ray_box_intersection(o_o, d_o, -e, e)
    nh = inter.sum(-1)
    assert int((nh == 0).sum()) >= 8 and int((nh == 1).sum()) >= 8
    seen = dict(free=0, inside=0, outside=0)
    for lvl in range(2):
        lv = levels[lvl]
        tm = lv['t_mids']
        for r in range(B):
            vd = np.tile(rays.viewdirs[r].numpy(), (N, 1))
            if nh[r] == 0:
                X = (rays.origins[r] + tm[r][:, None] * rays.directions[r]).numpy()
                q = F.query(params, X, vd, pose, ext, exact=True)
                assert (q['owner'] == -1).all() or (F.classify(X, pose, ext, exact=True)['owner'] != -1).any()
                free = q['owner'] == -1
                assert np.abs(q['raw'][free] - lv['bkgd'][r].numpy()[free]).max() <= 1e-9, 'ray %d' % r
                seen['free'] += int(free.sum())
            elif nh[r] == 1:
                k = int(torch.argmax(inter[r]))
                P = (o_o[r, k] + tm[r][:, None] * d_o[r, k]).numpy()
                q = F.query(params, F._world(pose[k], P), vd, pose, ext, exact=True)
                want = (lv['bkgd'][r] + lv['obj'][k][r]).numpy()
                inside, outside = q['owner'] == k, q['owner'] == -1
                assert (inside == (np.abs(P) <= ext[k]).all(1)).all()
                if inside.any():
                    assert np.abs(q['raw'][inside] - want[inside]).max() <= 1e-9, 'ray %d' % r
                if outside.any():
                    assert np.abs(q['raw'][outside] - want[outside]).max(1).min() > 1e-6, 'ray %d: the render is the BoxMLP there' % r
                seen['inside'] += int(inside.sum())
                seen['outside'] += int(outside.sum())
    assert min(seen.values()) >= 8, seen


# ---- the library --------------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_bound_and_exported_by_a_library_of_their_own():
    # (header == table == symbol table: tests/test_satellites_host.py; the constants and durf_field_args, field for field,
    # against the header: tests/test_headers_host.py)
    assert ENTRY == set(_lib.field_symbols())
    assert len(_lib.symbols()) == 118
    assert ops.FIELD_ENC_BKGD == 60 and ops.FIELD_ENC_OBJ == 63


def test_staged_refusals_and_zero_work():
    L = _lib.field_lib()
    cls = lambda n=4, K=1, tol=0.0, pts=FAKE, pose=FAKE: L.durf_field_classify(None, n, pts, K, pose, FAKE, None, tol, FAKE, FAKE, FAKE)
    assert cls(n=0) == 0
    for kw, text in ((dict(n=-1), 'n = -1'), (dict(K=17), 'K = 17'), (dict(K=-1), 'K = -1'), (dict(tol=-0.5), 'inside_tol = -0.5'),
                     (dict(tol=float('nan')), 'inside_tol = nan'), (dict(pts=None), 'points, owner and local'),
                     (dict(pose=None), 'pose, ext and pose_scratch for K = 1')):
        assert cls(**kw) != 0 and text in _err() and 'durf_field_classify' in _err(), (kw, _err())
    assert L.durf_field_lists(None, 0, 2, FAKE, FAKE, FAKE) == 0
    assert L.durf_field_lists(None, 1 << 27, 2, FAKE, FAKE, FAKE) != 0 and 'n = %d' % (1 << 27) in _err()
    assert L.durf_field_lists(None, 4, 2, None, FAKE, FAKE) != 0 and 'owner, idx and count' in _err()
    assert L.durf_field_owned(None, 4, 0, None, None, None, None) == 0
    assert L.durf_field_owned(None, 4, 1, FAKE, FAKE, None, FAKE) != 0 and 'owned' in _err()
    w = (C.c_float * 10)(*([1.0] * 10))
    enc = lambda n=4, K=1, sigma=0.0, fl=1, outs=(FAKE, FAKE), bw=w: L.durf_field_encode(None, n, K, FAKE, FAKE, FAKE, sigma, fl, bw, *outs)
    assert enc(n=0) == 0
    for kw, text in ((dict(sigma=-1.0), 'sigma = -1'), (dict(sigma=float('nan')), 'sigma = nan'), (dict(fl=2), 'enc_flags = 2'),
                     (dict(outs=(None, None)), 'at least one output'), (dict(bw=None), 'barf_w'), (dict(K=99), 'K = 99')):
        assert enc(**kw) != 0 and text in _err(), (kw, _err())
    act = lambda n=4, K=1, ro=FAKE, dens=FAKE: L.durf_field_activate(None, n, K, FAKE, FAKE, FAKE, ro, FAKE, FAKE, -1.0, dens, None, None, FAKE)
    assert act(n=0) == 0
    assert act(ro=None) != 0 and 'raw_obj and raw_const for K = 1' in _err()
    assert act(dens=None) != 0 and 'density and valid' in _err()
    assert act(ro=FAKE + 4) != 0 and '16-byte aligned' in _err()
    col = lambda nu=2, nv=2, nw=3, step=0.5, outs=(FAKE, None, None), d=FAKE: L.durf_field_columns(None, nu, nv, nw, d, FAKE, step, 1.0, *outs)
    for kw, text in ((dict(nu=0), '0 x 2 x 3'), (dict(nu=65536, nv=65536), '65536 x 65536'), (dict(step=-1.0), 'step = -1'),
                     (dict(outs=(None, None, None)), 'at least one output'), (dict(d=None), 'density and valid')):
        assert col(**kw) != 0 and text in _err(), (kw, _err())


def _args(K=1, **kw):
    a = ops.FieldArgs()
    a.K, a.enc_flags, a.sigma, a.inside_tol, a.density_bias = K, 1, 0.0, 0.0, -1.0
    for n in ('bkgd_params', 'bkgd_wstream', 'obj_params', 'obj_wstream', 'const_trunk', 'pose', 'ext', 'points', 'density'):
        setattr(a, n, FAKE)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_query_and_grid_refusals_and_the_workspace_sizer():
    L = _lib.field_lib()
    q = lambda a, n=8, chunk=4, ws=FAKE, nbytes=1 << 40: L.durf_field_query(None, C.addressof(a), n, chunk, ws, nbytes)
    assert q(_args(), n=0) == 0 and q(_args(density=None, points=None), n=0) == 0          # n == 0: nothing to do
    assert L.durf_field_query(None, None, 8, 4, FAKE, 1 << 40) != 0 and 'arguments' in _err()
    for a, kw, text in ((_args(), dict(n=-2), 'n >= 0'), (_args(), dict(chunk=0), '0 < chunk'), (_args(K=17), {}, 'K = 17'),
                        (_args(sigma=-1.0), {}, 'sigma >= 0'), (_args(inside_tol=-1.0), {}, 'inside_tol >= 0'),
                        (_args(enc_flags=3), {}, 'enc_flags'), (_args(bkgd_wstream=None), {}, 'bkgd_params and bkgd_wstream'),
                        (_args(const_trunk=None), {}, 'const_trunk'), (_args(density=None), {}, 'density'),
                        (_args(points=None), {}, 'points'), (_args(rgb=FAKE), {}, 'rgb needs viewdirs'),
                        (_args(), dict(ws=None), 'workspace aligned'), (_args(), dict(ws=FAKE + 8), 'workspace aligned')):
        assert q(a, **kw) != 0 and text in _err() and 'durf_field_query' in _err(), (text, _err())
    need = L.durf_field_workspace_bytes(4, 1)
    assert q(_args(), nbytes=need - 1) != 0
    assert 'workspace of %d bytes' % (need - 1) in _err() and 'durf_field_workspace_bytes(4, 1) = %d' % need in _err()
    # monotone in chunk and in K, and independent of anything else
    sizes = [[L.durf_field_workspace_bytes(c, K) for c in (1, 64, 65, 4096, 65536)] for K in (0, 1, 2, 16)]
    for row in sizes:
        assert all(b > a for a, b in zip(row, row[1:])), row
    for lo, hi in zip(sizes, sizes[1:]):
        assert all(b > a for a, b in zip(lo, hi)), (lo, hi)
    assert sizes[3][4] < 65536 * (16 * (63 + 4 + 1) + 60 + 27 + 40) * 4 + (1 << 16)          # chunk (K (enc + raw + idx) + ...) floats
    f3 = (C.c_float * 3)(0.0, 0.0, 0.0)
    g = lambda a, shape=(2, 2, 2), hv=0, org=f3: L.durf_field_grid(None, C.addressof(a), org, f3, f3, f3, *shape, hv, 0.0, 0.0, 1.0, 4, FAKE,
                                                                 1 << 40, None)
    for a, kw, text in ((_args(), dict(shape=(0, 2, 2)), 'nu = 0'), (_args(), dict(shape=(2048, 2048, 2048)), 'nu nv nw < 2^31'),
                        (_args(), dict(org=None), 'origin, du, dv and dw'), (_args(rgb=FAKE), {}, 'rgb needs a view direction'),
                        (_args(sigma=-2.0), {}, 'sigma >= 0')):
        assert g(a, **kw) != 0 and text in _err() and 'durf_field_grid' in _err(), (text, _err())


# ---- durf_amd/field.py --------------------------------------------------------------------------------------------------------
def _fake(K=2, use_viewdirs=True, dynamics=True, device='cuda'):
    model = types.SimpleNamespace(use_viewdirs=use_viewdirs, dynamics=dynamics)
    variables = types.SimpleNamespace(layout=types.SimpleNamespace(K=K, use_viewdirs=use_viewdirs),
                                      flat=types.SimpleNamespace(device=torch.device(device)))
    return model, variables


def test_field_py_refuses_loudly_and_names_the_entry():
    pts = np.zeros((3, 3), np.float32)
    for entry, call in (('field.query', lambda m, v: field.query(m, v, pts)),
                        ('field.grid', lambda m, v: field.grid(m, v, (0, 0, 0), (2, 2, 2), step=1.0))):
        for kw, text in ((dict(dynamics=False), 'dynamics=False'), (dict(use_viewdirs=False), 'use_viewdirs=False'),
                         (dict(device='cpu'), 'device')):
            with pytest.raises(NotImplementedError, match=re.escape(entry)) as e:
                call(*_fake(**kw))
            assert text in str(e.value), (entry, kw, str(e.value))
    field._refuse(*_fake(K=0, dynamics=False), 'field.query')            # dynamics=False without boxes is the static model
    with pytest.raises(ValueError, match='step or axes'):
        field.grid(*_fake(), (0, 0, 0), (2, 2, 2))


def test_writers(tmp_path):
    g = dict(density=np.arange(24, dtype=np.float32).reshape(2, 3, 4), frame=dict(origin=[0, 0, 0], du=[1, 0, 0], dv=[0, 1, 0],
                                                                                 dw=[0, 0, 0.5], shape=[2, 3, 4]))
    field.write_density(str(tmp_path / 'density'), g)
    assert (np.load(tmp_path / 'density.npy') == g['density']).all()
    meta = json.load(open(tmp_path / 'density.json'))
    assert meta['shape'] == [2, 3, 4] and meta['dw'] == [0, 0, 0.5] and meta['file'] == 'density.npy'
    field.write_pgm(str(tmp_path / 'm.pgm'), np.array([[0.0, 0.5, np.nan], [1.0, 2.0, -1.0]]))
    blob = open(tmp_path / 'm.pgm', 'rb').read()
    assert blob.startswith(b'P5\n3 2\n255\n') and list(blob[-6:]) == [0, 128, 0, 255, 255, 0]
    field.write_ppm(str(tmp_path / 'm.ppm'), np.zeros((2, 3, 3), np.uint8))
    assert open(tmp_path / 'm.ppm', 'rb').read().startswith(b'P6\n3 2\n255\n')
    with pytest.raises(ValueError):
        field.write_pgm(str(tmp_path / 'x.pgm'), np.zeros((2, 2, 2)))
