"""libdurf_smooth.so on the device against tests/smooth_ref.py: the keys, both CSR structures, the vertex class, the census, steps,
Taubin and the normals in every bit of every output, on the smallest shapes at which they can go wrong; canaries round every
output and after offsets[V]; refusals that write nothing; and mesh.surface -> smooth.taubin as a pipeline."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from durf_amd import _lib, mesh, smooth
from tests import mesh_ref as M, smooth_ref as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
PAD = 64                                                                    # canary elements on either side of every output
FILL = {torch.int64: -7, torch.int32: -7, torch.uint8: 0xAB, torch.float32: -7.0}
_CACHE = {}


class Out:
    """an output with canaries round it: `t` is what the library is given"""
    def __init__(self, n, dtype, cuda):
        self.buf = torch.full((n + 2 * PAD,), FILL[dtype], dtype=dtype, device=cuda)
        self.t, self.n, self.fill = self.buf[PAD:PAD + n], n, FILL[dtype]

    def host(self, written=None):
        """the output on the host; everything outside its first `written` elements must still be the canary"""
        b = self.buf.cpu().numpy()
        w = self.n if written is None else written
        assert (b[:PAD] == self.fill).all() and (b[PAD + w:] == self.fill).all(), 'a canary was overwritten'
        return b[PAD:PAD + w].copy()

    def edges(self):
        """only the canaries on either side: what lies between is not looked at"""
        b = self.buf.cpu().numpy()
        assert (b[:PAD] == self.fill).all() and (b[PAD + self.n:] == self.fill).all(), 'a canary was overwritten'

    def untouched(self):
        return bool((self.buf == self.fill).all())


def _p(t):
    return None if t is None or t.numel() == 0 else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ok(rc):
    assert rc == 0, _lib.lib().durf_last_error().decode()


def _same(got, want, what):
    a, b = (S.bits(x) if x.dtype == np.float32 else np.ascontiguousarray(x) for x in (got, np.asarray(want)))
    assert a.shape == b.shape and np.array_equal(a, b), (what, a.shape, b.shape, np.argwhere(a != b)[:5])


def _device_adjacency(cuda, v, t, extra_cap=5):
    """every adjacency entry through the C ABI with canaries -> (dict of device views for the later calls, dict of host arrays)"""
    L = _lib.smooth_lib()
    V, T = v.shape[0], t.shape[0]
    dv = torch.as_tensor(np.ascontiguousarray(v, F32)).to(cuda).reshape(V, 3).contiguous()
    dt = torch.as_tensor(np.ascontiguousarray(t, np.int32)).to(cuda).reshape(T, 3).contiguous()
    ek, ck = Out(6 * T, torch.int64, cuda), Out(3 * T, torch.int64, cuda)
    _ok(L.durf_smooth_keys(_stream(), V, T, _p(dt), _p(ek.t), _p(ck.t)))
    h = dict(edge_keys=ek.host(), corner_keys=ck.host())
    eks, cks = torch.sort(ek.t).values.contiguous(), torch.sort(ck.t).values.contiguous()
    cap = 6 * T + extra_cap
    ws = torch.empty(max(int(L.durf_smooth_workspace_bytes(T)), 256), dtype=torch.uint8, device=cuda)
    off, nb, mu = Out(V + 1, torch.int32, cuda), Out(cap, torch.int32, cuda), Out(cap, torch.int32, cuda)
    coff, ct = Out(V + 1, torch.int32, cuda), Out(3 * T, torch.int32, cuda)
    _ok(L.durf_smooth_adjacency(_stream(), V, T, _p(eks), _p(cks), cap, ws.data_ptr(), ws.numel(), off.t.data_ptr(), _p(nb.t), _p(mu.t),
                                coff.t.data_ptr(), _p(ct.t)))
    h['offsets'], h['corner_offsets'] = off.host(), coff.host()
    U, Uc = int(h['offsets'][V]), int(h['corner_offsets'][V])
    assert 0 <= U <= 6 * T and 0 <= Uc <= 3 * T
    h['neighbours'], h['multiplicity'], h['corner_tri'] = nb.host(U), mu.host(U), ct.host(Uc)      # nothing written past offsets[V]
    cls = Out(V, torch.uint8, cuda)
    _ok(L.durf_smooth_classify(_stream(), V, off.t.data_ptr(), _p(mu.t), _p(cls.t)))
    h['vertex_class'] = cls.host()
    cen = Out(8, torch.int32, cuda)
    _ok(L.durf_smooth_census(_stream(), V, off.t.data_ptr(), _p(nb.t), _p(mu.t), coff.t.data_ptr(), _p(cls.t), cen.t.data_ptr()))
    h['census'] = cen.host()
    d = dict(V=V, T=T, vertices=dv, triangles=dt, offsets=off.t, neighbours=nb.t, multiplicity=mu.t, corner_offsets=coff.t, corner_tri=ct.t,
             vertex_class=cls.t, keep=(off, nb, mu, coff, ct, cls))
    return d, h


def _step(cuda, d, x, factor, boundary=0, fixed=None):
    out = Out(3 * d['V'], torch.float32, cuda)
    fx = None if fixed is None else torch.as_tensor(np.ascontiguousarray(fixed, np.uint8)).to(cuda)
    _ok(_lib.smooth_lib().durf_smooth_step(_stream(), d['V'], _p(x), d['offsets'].data_ptr(), _p(d['neighbours']), _p(d['multiplicity']),
                                           _p(d['vertex_class']), float(factor), boundary, _p(fx), _p(out.t)))
    return out.host().reshape(-1, 3)


def _taubin(cuda, d, x, iters, lam, mu, boundary=0, fixed=None):
    out, tmp = Out(3 * d['V'], torch.float32, cuda), Out(3 * d['V'], torch.float32, cuda)
    fx = None if fixed is None else torch.as_tensor(np.ascontiguousarray(fixed, np.uint8)).to(cuda)
    _ok(_lib.smooth_lib().durf_smooth_taubin(_stream(), d['V'], _p(x), d['offsets'].data_ptr(), _p(d['neighbours']), _p(d['multiplicity']),
                                             _p(d['vertex_class']), iters, float(lam), float(mu), boundary, _p(fx), _p(tmp.t), _p(out.t)))
    tmp.host()
    return out.host().reshape(-1, 3)


def _normals(cuda, d, x):
    out = Out(3 * d['V'], torch.float32, cuda)
    _ok(_lib.smooth_lib().durf_smooth_normals(_stream(), d['V'], d['T'], _p(x), _p(d['triangles']), d['corner_offsets'].data_ptr(),
                                              _p(d['corner_tri']), _p(out.t)))
    return out.host().reshape(-1, 3)


def _check_adjacency(h, a, what):
    for k in ('edge_keys', 'corner_keys', 'offsets', 'neighbours', 'multiplicity', 'corner_offsets', 'corner_tri', 'vertex_class'):
        _same(h[k], a[k], (what, k))
    _same(h['census'], S.census(a), (what, 'census'))


def _check_everything(cuda, v, t, what, fixed=None):
    """every output of every entry on one mesh against the oracle"""
    d, h = _device_adjacency(cuda, v, t)
    a = S.adjacency(v, t)
    _check_adjacency(h, a, what)
    x = d['vertices']
    for factor in (-1.0, 0.0, 1.0, 0.5):
        for boundary in (S.PIN, S.SLIDE):
            _same(_step(cuda, d, x, factor, boundary, fixed), S.step(a, v, factor, boundary, fixed), (what, 'step', factor, boundary))
    got = _taubin(cuda, d, x, 2, 0.5, -0.53, S.SLIDE, fixed)
    _same(got, S.taubin(a, v, 2, 0.5, -0.53, S.SLIDE, fixed), (what, 'taubin'))
    _same(_normals(cuda, d, x), S.normals(a, v), (what, 'normals'))
    gx = torch.as_tensor(got).to(cuda).contiguous()
    _same(_normals(cuda, d, gx), S.normals(a, got), (what, 'normals of the smoothed'))
    return d, h, a


def _grid_T(T, seed):
    """T triangles of a jittered 46 x 46 quad grid (4232 in all), chosen and ordered at random: holes, boundaries, interior"""
    key = ('grid', T, seed)
    if key not in _CACHE:
        v, t = S.quad_grid(46)
        rng = np.random.default_rng(seed)
        v = (v + rng.uniform(-0.3, 0.3, v.shape)).astype(F32)
        _CACHE[key] = (v, t[rng.permutation(t.shape[0])[:T]])
    return _CACHE[key]


# ---- small and awkward meshes -------------------------------------------------------------------------------------------------------
SMALL = dict(V0_T0=lambda: (np.zeros((0, 3), F32), np.zeros((0, 3), np.int32)), V1_T0=lambda: (np.ones((1, 3), F32), np.zeros((0, 3), np.int32)),
             V0_T1=lambda: (np.zeros((0, 3), F32), np.zeros((1, 3), np.int32)), V1_T1=lambda: (np.ones((1, 3), F32), np.zeros((1, 3), np.int32)),
             V3_T1=lambda: (S.quad()[0][:3], S.quad()[1][:1]), tetrahedron=S.tetrahedron, quad=S.quad, book=S.book, duplicate=S.duplicate,
             bad_indices=S.bad_indices, not_finite=S.not_finite, fan_300=S.fan, soup=lambda: S.soup(40, 300, 3),
             all_bad=lambda: (np.ones((4, 3), F32), np.asarray([[0, 0, 1], [-1, 2, 3], [1, 2, 4]], np.int32)))


@pytest.mark.parametrize('name', sorted(SMALL))
def test_every_output_equals_the_definition_on_small_and_awkward_meshes(cuda, name):
    v, t = SMALL[name]()
    d, h, a = _check_everything(cuda, v, t, name)
    if name == 'fan_300':
        assert h['offsets'][1] - h['offsets'][0] == 300 and h['vertex_class'][0] == S.INTERIOR and (h['vertex_class'][1:] == S.BOUNDARY).all()
    if name == 'not_finite':
        out = _step(cuda, d, d['vertices'], 0.5)
        assert np.array_equal(S.bits(out[[5, 17, 30]]), S.bits(v[[5, 17, 30]])) and np.isfinite(np.delete(out, [5, 17, 30], 0)).all()
    if name == 'bad_indices':
        assert h['census'][4] == t.shape[0] - 4


def test_fixed_masks_pin_their_vertices(cuda):
    v, t = S.noisy_icosphere(2, 4)
    fixed = (np.random.default_rng(0).random(v.shape[0]) < 0.3).astype(np.uint8)
    d, h, a = _check_everything(cuda, v, t, 'fixed', fixed)
    out = _taubin(cuda, d, d['vertices'], 3, 0.5, -0.53, 0, fixed)
    assert np.array_equal(S.bits(out[fixed != 0]), S.bits(v[fixed != 0])) and (S.bits(out[fixed == 0]) != S.bits(v[fixed == 0])).any(1).all()
    for mask in (np.ones_like(fixed), np.zeros_like(fixed), 7 * fixed):
        _same(_step(cuda, d, d['vertices'], 0.5, 0, mask), S.step(a, v, 0.5, S.PIN, mask), 'mask')


def test_boundary_pin_and_slide_on_an_open_patch(cuda):
    v, t = S.quad_grid(5)
    v = (v + np.random.default_rng(2).uniform(-0.2, 0.2, v.shape)).astype(F32)
    d, h, a = _check_everything(cuda, v, t, 'patch')
    edge = h['vertex_class'] == S.BOUNDARY
    assert edge.sum() == 20 and h['census'][6] == 20
    pin, slide = _step(cuda, d, d['vertices'], 0.5, S.PIN), _step(cuda, d, d['vertices'], 0.5, S.SLIDE)
    assert np.array_equal(S.bits(pin[edge]), S.bits(v[edge])) and (S.bits(slide[edge]) != S.bits(v[edge])).any(1).all()
    assert np.array_equal(S.bits(pin[~edge]), S.bits(slide[~edge]))


# ---- block edges, and the order of the triangles -----------------------------------------------------------------------------------
@pytest.mark.parametrize('T', [4095, 4096, 4097])
def test_block_edges_and_the_order_of_the_triangles(cuda, T):
    v, t = _grid_T(T, T)
    d, h, a = _check_everything(cuda, v, t, T)
    assert {S.INTERIOR, S.BOUNDARY} <= set(h['vertex_class'].tolist())
    perm = np.random.default_rng(T + 1).permutation(T)
    d2, h2 = _device_adjacency(cuda, v, t[perm])
    a2 = S.adjacency(v, t[perm])
    _check_adjacency(h2, a2, (T, 'permuted'))
    for k in ('offsets', 'neighbours', 'multiplicity', 'vertex_class', 'corner_offsets', 'census'):
        _same(h2[k], h[k], (T, 'the order of the triangles changed', k))
    assert not np.array_equal(h2['corner_tri'], h['corner_tri'])
    _same(_taubin(cuda, d2, d2['vertices'], 2, 0.5, -0.53, S.SLIDE), _taubin(cuda, d, d['vertices'], 2, 0.5, -0.53, S.SLIDE), (T, 'steps'))
    n2 = _normals(cuda, d2, d2['vertices'])
    _same(n2, S.normals(a2, v), (T, 'normals in the permuted order'))
    assert np.abs(n2 - _normals(cuda, d, d['vertices'])).max() < 1e-5        # (another order of the sum: close, not equal bits)


def test_an_icosphere_of_5120_triangles_taubin_is_its_steps_and_two_runs_agree(cuda):
    v, t = S.noisy_icosphere(4, 1)
    assert t.shape[0] == 5120
    d, h, a = _check_everything(cuda, v, t, 'icosphere')
    assert h['census'].tolist() == [0, v.shape[0], 0, 0, 5120, 7680, 0, 0]
    for iters in (0, 1, 2, 5):
        for mu in (-0.53, 0.0):
            got = _taubin(cuda, d, d['vertices'], iters, 0.5, mu)
            x = d['vertices']
            for k in range(iters * (2 if mu != 0 else 1)):
                x = torch.as_tensor(_step(cuda, d, x, mu if (mu != 0 and k % 2) else 0.5)).to(cuda).contiguous()
            _same(got, x.cpu().numpy(), ('taubin against its steps', iters, mu))
            _same(got, S.taubin(a, v, iters, 0.5, mu), ('taubin against the oracle', iters, mu))
            _same(_taubin(cuda, d, d['vertices'], iters, 0.5, mu), got, ('two runs', iters, mu))
    d2, h2 = _device_adjacency(cuda, v, t)
    for k in h:
        _same(h2[k], h[k], ('two runs', k))


# ---- the public interface -----------------------------------------------------------------------------------------------------------
def test_smooth_py_returns_what_the_library_computes_and_leaves_its_input_alone(cuda):
    v, t = S.noisy_icosphere(2, 7)
    a = S.adjacency(v, t)
    colour = np.random.default_rng(0).random((v.shape[0], 3)).astype(F32)
    m = dict(vertices=torch.as_tensor(v).to(cuda), triangles=torch.as_tensor(t).to(cuda), normals=torch.zeros(v.shape[0], 3, device=cuda),
             rgb=torch.as_tensor(colour).to(cuda), iso=1.5)
    before = {k: (x.clone() if torch.is_tensor(x) else x) for k, x in m.items()}
    adj = smooth.adjacency(m)
    U = int(a['offsets'][-1])
    for k in ('offsets', 'corner_offsets', 'vertex_class'):
        _same(adj[k].cpu().numpy(), a[k], k)
    for k in ('neighbours', 'multiplicity'):
        _same(adj[k].cpu().numpy()[:U], a[k], k)
    _same(adj['corner_tri'].cpu().numpy(), a['corner_tri'], 'corner_tri')
    c = smooth.census(adj)
    assert c['closed'] and c['euler'] == 2 and [c[k] for k in smooth.CENSUS_FIELDS] == S.census(a).tolist()
    fixed = np.zeros(v.shape[0], bool)
    fixed[::5] = True
    for out, want in ((smooth.taubin(m, 3, adj=adj), S.taubin(a, v, 3, 0.5, -0.53)), (smooth.taubin(m, 2), S.taubin(a, v, 2, 0.5, -0.53)),
                      (smooth.laplacian(m, 4, 0.25, adj=adj), S.taubin(a, v, 4, 0.25, 0.0)), (smooth.step(m, -0.5, adj=adj), S.step(a, v, -0.5)),
                      (smooth.taubin(m, 2, boundary='slide', fixed=fixed, adj=adj), S.taubin(a, v, 2, 0.5, -0.53, S.SLIDE, fixed)),
                      (smooth.taubin(dict(vertices=v, triangles=t, normals=v), 1), S.taubin(a, v, 1, 0.5, -0.53))):
        _same(out['vertices'].cpu().numpy(), want, 'vertices')
        _same(out['normals'].cpu().numpy(), S.normals(a, want), 'normals are recomputed')
        if 'rgb' in out:
            assert out['rgb'] is m['rgb'] and out['iso'] == 1.5 and out['triangles'] is m['triangles']
    assert 'normals' not in smooth.taubin(dict(vertices=m['vertices'], triangles=m['triangles']), 1, adj=adj)
    _same(smooth.normals(m, adj).cpu().numpy(), S.normals(a, v), 'normals')
    assert all(torch.equal(m[k], before[k]) if torch.is_tensor(m[k]) else m[k] == before[k] for k in before) and set(m) == set(before)
    e = smooth.adjacency(dict(vertices=np.zeros((2, 3), F32), triangles=np.zeros((0, 3), np.int32)))
    assert smooth.census(e)['isolated'] == 2 and smooth.census(e)['closed'] and smooth.taubin(dict(vertices=np.zeros((2, 3), F32), triangles=np.zeros((0, 3), np.int32)), 2)['vertices'].shape == (2, 3)


# ---- refusals write nothing ---------------------------------------------------------------------------------------------------------
def test_a_refused_call_writes_nothing(cuda):
    L = _lib.smooth_lib()
    v, t = S.tetrahedron()
    d, h = _device_adjacency(cuda, v, t)
    V, T = 4, 4
    err = lambda: _lib.lib().durf_last_error().decode()
    out, tmp = Out(3 * V, torch.float32, cuda), Out(3 * V, torch.float32, cuda)
    args = (d['offsets'].data_ptr(), _p(d['neighbours']), _p(d['multiplicity']), _p(d['vertex_class']))
    x = d['vertices']
    for call, text in ((lambda: L.durf_smooth_step(_stream(), V, _p(x), *args, float('nan'), 0, None, _p(out.t)), 'factor = nan'),
                       (lambda: L.durf_smooth_step(_stream(), V, _p(x), *args, 1.5, 0, None, _p(out.t)), 'factor = 1.5'),
                       (lambda: L.durf_smooth_step(_stream(), V, _p(x), *args, 0.5, 2, None, _p(out.t)), 'boundary = 2'),
                       (lambda: L.durf_smooth_step(_stream(), V, _p(out.t), *args, 0.5, 0, None, _p(out.t)), 'in != out'),
                       (lambda: L.durf_smooth_taubin(_stream(), V, _p(x), *args, -1, 0.5, -0.53, 0, None, _p(tmp.t), _p(out.t)), 'iters = -1'),
                       (lambda: L.durf_smooth_taubin(_stream(), V, _p(x), *args, 2, 0.5, -0.53, 0, None, None, _p(out.t)), 'tmp [V,3]'),
                       (lambda: L.durf_smooth_taubin(_stream(), V, _p(x), *args, 2, 0.5, float('inf'), 0, None, _p(tmp.t), _p(out.t)), 'mu = inf'),
                       (lambda: L.durf_smooth_normals(_stream(), V, -1, _p(x), _p(d['triangles']), d['corner_offsets'].data_ptr(), _p(d['corner_tri']), _p(out.t)), 'T = -1')):
        assert call() != 0 and text in err(), (text, err())
    kk, kc, cls, cen = Out(6 * T, torch.int64, cuda), Out(3 * T, torch.int64, cuda), Out(V, torch.uint8, cuda), Out(8, torch.int32, cuda)
    big = 357913942
    for call, text in ((lambda: L.durf_smooth_keys(_stream(), -1, T, _p(d['triangles']), _p(kk.t), _p(kc.t)), 'durf_smooth_keys: requirement failed: V >= 0, V = -1'),
                       (lambda: L.durf_smooth_keys(_stream(), V, big, _p(d['triangles']), _p(kk.t), _p(kc.t)), 'durf_smooth_keys: requirement failed: T in 0 .. DURF_SMOOTH_MAX_TRIANGLES - 1'),
                       (lambda: L.durf_smooth_keys(_stream(), V, T, None, _p(kk.t), _p(kc.t)), 'durf_smooth_keys: requirement failed: triangles for T = 4'),
                       (lambda: L.durf_smooth_keys(_stream(), V, T, _p(d['triangles']), _p(kk.t), None), 'edge_keys and corner_keys for T = 4'),
                       (lambda: L.durf_smooth_classify(_stream(), -1, args[0], args[2], _p(cls.t)), 'durf_smooth_classify: requirement failed: V >= 0, V = -1'),
                       (lambda: L.durf_smooth_classify(_stream(), V, None, args[2], _p(cls.t)), 'durf_smooth_classify: requirement failed: offsets [V+1]'),
                       (lambda: L.durf_smooth_census(_stream(), -1, args[0], args[1], args[2], d['corner_offsets'].data_ptr(), args[3], _p(cen.t)), 'durf_smooth_census: requirement failed: V >= 0'),
                       (lambda: L.durf_smooth_census(_stream(), V, args[0], args[1], args[2], None, args[3], _p(cen.t)), 'offsets, corner_offsets and census'),
                       (lambda: L.durf_smooth_census(_stream(), V, args[0], args[1], args[2], d['corner_offsets'].data_ptr(), None, _p(cen.t)), 'vertex_class for V = 4')):
        assert call() != 0 and text in err(), (text, err())
    ws = torch.empty(max(int(L.durf_smooth_workspace_bytes(T)), 256), dtype=torch.uint8, device=cuda)
    ek = torch.sort(torch.as_tensor(S.keys(t, V)[0]).to(cuda)).values.contiguous()
    ck = torch.sort(torch.as_tensor(S.keys(t, V)[1]).to(cuda)).values.contiguous()
    off, nb, mu, coff, ct = (Out(n, torch.int32, cuda) for n in (V + 1, 6 * T, 6 * T, V + 1, 3 * T))
    adj = lambda cap=6 * T, wsp=ws.data_ptr(), wb=ws.numel(): L.durf_smooth_adjacency(_stream(), V, T, _p(ek), _p(ck), cap, wsp, wb, off.t.data_ptr(), _p(nb.t),
                                                                                     _p(mu.t), coff.t.data_ptr(), _p(ct.t))
    for call, text in ((lambda: adj(cap=6 * T - 1), 'cap >= 6 T'), (lambda: adj(wb=ws.numel() // 2), 'durf_smooth_workspace_bytes(4)'),
                       (lambda: adj(wsp=ws.data_ptr() + 8), 'aligned to 256 bytes')):
        assert call() != 0 and text in err(), (text, err())
    torch.cuda.synchronize()
    assert all(o.untouched() for o in (out, tmp, off, nb, mu, coff, ct, kk, kc, cls, cen))
    assert adj() == 0
    _same(off.host(), h['offsets'], 'the accepted call')


# ---- the pipeline -------------------------------------------------------------------------------------------------------------------
def test_a_planted_sphere_is_extracted_smoothed_and_stays_closed(cuda):
    n = 24
    fr = M.unit_frame(4.0 / (n - 1), (-2.0, -2.0, -2.0))
    dens = torch.as_tensor(M.sphere_field(fr, (n, n, n), (0.03, -0.02, 0.01), 1.3)).to(cuda)
    m = mesh.surface(dict(density=dens, valid=None, frame=fr), 0.0)
    V = m['vertices'].shape[0]
    adj = smooth.adjacency(m)
    c = smooth.census(adj)
    assert c['closed'] and c['euler'] == 2 and c['interior'] == V > 1000 and c['triangles'] == m['triangles'].shape[0]
    s = smooth.taubin(m, adj=adj)
    assert torch.equal(s['triangles'], m['triangles']) and s['triangles'] is m['triangles'] and s['vertex_edge'] is m['vertex_edge']
    c2 = smooth.census(smooth.adjacency(s))
    assert c2 == c
    a = S.adjacency(m['vertices'].cpu().numpy(), m['triangles'].cpu().numpy())
    _same(s['vertices'].cpu().numpy(), S.taubin(a, m['vertices'].cpu().numpy(), 10, 0.5, -0.53), 'vertices')
    _same(s['normals'].cpu().numpy(), S.normals(a, s['vertices'].cpu().numpy()), 'normals')
    interior = adj['vertex_class'] == S.INTERIOR
    dots = (s['normals'] * m['normals']).sum(1)[interior]
    assert bool((dots > 0).all()), float(dots.min())
    r = torch.linalg.norm(s['vertices'] - torch.tensor([0.03, -0.02, 0.01], device=cuda), dim=1)
    r0 = torch.linalg.norm(m['vertices'] - torch.tensor([0.03, -0.02, 0.01], device=cuda), dim=1)
    print('radius: extracted %.5f +- %.5f, smoothed %.5f +- %.5f' % (float(r0.mean()), float(r0.std()), float(r.mean()), float(r.std())))


def test_extract_with_smooth_0_is_extract_and_with_smooth_it_smooths(cuda):
    from tests import test_gpu_mesh as TM
    s = TM._model_scene(cuda)
    kw = dict(ext=s['ext'], box_enable=s['en'])
    G = TM.GRID
    g = TM.field.grid(s['model'], s['variables'], G['origin'], G['shape'], step=G['step'], **kw)
    iso = float(g['density'][g['valid'] != 0].median())
    a = mesh.extract(s['model'], s['variables'], G['origin'], G['shape'], step=G['step'], iso=iso, **kw)
    b = mesh.extract(s['model'], s['variables'], G['origin'], G['shape'], step=G['step'], iso=iso, smooth=0, **kw)
    assert set(a) == set(b) and 'smooth' not in b and 'census' not in b
    for k in a:
        if torch.is_tensor(a[k]):
            assert a[k].dtype == b[k].dtype and a[k].cpu().numpy().tobytes() == b[k].cpu().numpy().tobytes(), k
    c = mesh.extract(s['model'], s['variables'], G['origin'], G['shape'], step=G['step'], iso=iso, smooth=3, **kw)
    assert torch.equal(c['triangles'], a['triangles']) and c['smooth'] == dict(iters=3, lam=0.5, mu=-0.53, boundary='pin')
    assert c['census']['triangles'] <= a['triangles'].shape[0]
    want = smooth.taubin(a, 3)
    assert torch.equal(TM._bits(c['vertices']), TM._bits(want['vertices'])) and torch.equal(TM._bits(c['normals']), TM._bits(want['normals']))
    q = TM.field.query(s['model'], s['variables'], c['vertices'], mesh.view_of_normals(c['normals']), **kw)
    assert torch.equal(TM._bits(q['rgb']), TM._bits(c['rgb'])), 'the colour is asked at the smoothed vertices with the fresh normals'


def test_keys_that_are_not_sorted_give_unspecified_arrays_inside_their_buffers(cuda):
    """the header's last rule: nothing is read or written outside the buffers (the workspace is zeroed here, so the run is the same every time)"""
    L = _lib.smooth_lib()
    v, t = S.noisy_icosphere(2, 3)
    V, T = v.shape[0], t.shape[0]
    ek, ck = (torch.as_tensor(k).to(cuda).flip(0).contiguous() for k in S.keys(t, V))       # descending, unsorted within a triangle too
    ws = torch.zeros(int(L.durf_smooth_workspace_bytes(T)), dtype=torch.uint8, device=cuda)
    off, nb, mu, coff, ct = (Out(n, torch.int32, cuda) for n in (V + 1, 6 * T, 6 * T, V + 1, 3 * T))
    _ok(L.durf_smooth_adjacency(_stream(), V, T, _p(ek), _p(ck), 6 * T, ws.data_ptr(), ws.numel(), off.t.data_ptr(), _p(nb.t), _p(mu.t),
                                coff.t.data_ptr(), _p(ct.t)))
    for o in (off, nb, mu, coff, ct):
        o.edges()                                                            # what lies between is unspecified
    h = off.host()
    assert ((h >= 0) & (h <= 6 * T)).all()


# ---- the commands -------------------------------------------------------------------------------------------------------------------
GIN = ['--gin_param', 'MipNerfModel.num_samples = 32', '--gin_param', 'MipNerfModel.no_pose_opt = True', '--gin_param', 'MipNerfModel.no_yaw_opt = True']
SMOOTH_FLAGS = ['--smooth', '2', '--smooth_lambda', '0.4', '--smooth_mu', '-0.42', '--smooth_boundary', 'slide']


def _command(module, argv, out, extra):
    p = subprocess.run([sys.executable, '-m', 'durf_amd.' + module] + argv + ['--eval_dir', out] + extra, cwd=ROOT, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=300)                 # a fresh child process
    assert p.returncode == 0, p.stdout.decode()[-3000:]
    return {n: open(os.path.join(out, n), 'rb').read() for n in sorted(os.listdir(out))}


@pytest.mark.parametrize('module,doc,argv', [
    ('extract_mesh', 'mesh.json', ['--synthetic', '--objects', '--iso', '0.001', '--grid=-2,-2,-1;16,16,8;0.25', '--gin_param', 'MipNerfModel.mlp_precision = \'f32\''] + GIN),
    ('fuse_tsdf', 'tsdf.json', ['--synthetic', '--objects', '--synthetic_boxes', '2', '--synthetic_size', '16', '24', '--frames', '2', '--grid=-2,-2,-1;12,12,12;0.35',
                                '--obj_step', '0.06'] + GIN)])
def test_the_commands_smooth_only_when_asked(cuda, tmp_path, module, doc, argv):
    plain = _command(module, argv, str(tmp_path / 'plain'), [])
    zero = _command(module, argv, str(tmp_path / 'zero'), ['--smooth', '0', '--smooth_lambda', '0.3'])
    assert plain == zero, 'without --smooth every file keeps its bytes'
    flagged = _command(module, argv, str(tmp_path / 'smooth'), SMOOTH_FLAGS)
    assert set(flagged) == set(plain)
    a, b = json.loads(plain[doc]), json.loads(flagged[doc])
    assert 'smooth' not in a and 'census' not in a['background'] and not any('census' in o for o in a['objects'])
    b_smooth = b.pop('smooth')
    assert b_smooth == dict(iters=2, lam=0.4, mu=-0.42, boundary='slide')
    records = [(a['background'], b['background'], 'background.ply')] + [(x, y, 'object_%02d.ply' % k) for k, (x, y) in enumerate(zip(a['objects'], b['objects']))]
    assert len(records) > 1
    moved = 0
    for x, y, name in records:
        c = y.pop('census')
        assert x == y, 'nothing else in the record changes'
        assert set(c) == set(smooth.CENSUS_FIELDS) | {'closed', 'euler'} and c['triangles'] <= x['triangles']
        p, q = mesh.read_ply(os.path.join(str(tmp_path / 'plain'), name)), mesh.read_ply(os.path.join(str(tmp_path / 'smooth'), name))
        assert np.array_equal(p['triangles'], q['triangles']) and p['vertices'].shape == q['vertices'].shape
        if c['triangles']:                                                   # the file against the library on the file's own mesh
            want = smooth.taubin(dict(vertices=p['vertices'], triangles=p['triangles'], normals=p['vertices']), 2, 0.4, -0.42, 'slide')
            _same(q['vertices'], want['vertices'].cpu().numpy(), name)
            moved += int((p['vertices'] != q['vertices']).any())
    print('%s: triangles per mesh %s, meshes with a moved vertex %d' % (module, [x['triangles'] for x, _, _ in records], moved))
    if module == 'extract_mesh':
        assert moved > 0, 'some mesh of the scene has a vertex that moves'
    else:
        # two frames of an untrained field may fuse into meshes without a vertex that is free to move: what the command applies to
        # tsdf.fuse_scene's meshes is held to the library here, on a mesh with the keys such a mesh carries
        v, t = S.noisy_icosphere(2, 5)
        m = dict(vertices=torch.as_tensor(v).to(cuda), triangles=torch.as_tensor(t).to(cuda), normals=torch.zeros(v.shape[0], 3, device=cuda),
                 rgb=torch.zeros(v.shape[0], 3, device=cuda), observed=7, cleaning=dict(kept=1))
        got = mesh.smoothed(m, dict(iters=2, lam=0.4, mu=-0.42, boundary='slide'))
        a_ = S.adjacency(v, t)
        want = S.taubin(a_, v, 2, 0.4, -0.42, S.SLIDE)
        _same(got['vertices'].cpu().numpy(), want, 'vertices'), _same(got['normals'].cpu().numpy(), S.normals(a_, want), 'normals')
        assert got['observed'] == 7 and got['rgb'] is m['rgb'] and got['census']['closed'] and got['smooth'] == b_smooth and mesh.smoothed(m, None) is m
