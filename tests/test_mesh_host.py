"""The iso-surface without a device: the three-way agreement of include/durf_mesh.h, durf_amd/_mesh_sigs.py and
libdurf_mesh.so's symbol table, every refusal of the entry points (they come before any launch), tests/mesh_ref.py against
closed forms -- combinatorial facts that hold exactly (every edge in two triangles, once in each direction; the Euler
characteristic) and the second-order convergence of the enclosed volume --, and the refusals and the PLY writer of
durf_amd/mesh.py."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest
import torch

from durf_amd import _lib, extract_mesh, mesh, ops, query_field
from tests import mesh_ref as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = {'durf_mesh_workspace_bytes', 'durf_mesh_count', 'durf_mesh_emit', 'durf_mesh_gather'}
FAKE = 4096              # a non-null, 256-byte aligned address no refused call may touch
CENTRE = (0.03, -0.02, 0.01)
_S = {}


def _err():
    return _lib.lib().durf_last_error().decode()


# ---- the binding ----------------------------------------------------------------------------------------------------------------
def test_header_sigs_and_symbol_table_agree():
    hdr = open(os.path.join(ROOT, 'include', 'durf_mesh.h')).read()
    assert ENTRY == set(_lib.mesh_symbols())           # (header == table == symbol table: tests/test_satellites_host.py)
    assert len(_lib.symbols()) == 118
    assert ops.MESH_BLOCK == 256                       # (the constants against the header: tests/test_headers_host.py)
    for rule in ('e + 1 = 4 di + 2 dj + dk', '(0,1,2), (0,2,1), (1,0,2), (1,2,0), (2,0,1), (2,1,0)', '(ab, ac, ad)',
                 '(ac, ad, bd) and (ac, bd, bc)', 'emitted as (x, z, y)'):
        assert rule in hdr, rule


def test_every_refusal_comes_before_a_launch():
    L = _lib.mesh_lib()
    big = 1 << 40
    cnt = lambda shape=(4, 4, 4), d=FAKE, iso=0.0, ws=FAKE, nb=big, c=FAKE: L.durf_mesh_count(None, *shape, d, None, iso, ws, nb, c)
    for kw, text in ((dict(shape=(1, 4, 4)), 'nu = 1, nv = 4, nw = 4'), (dict(shape=(4, 4, 0)), 'nw = 0'),
                     (dict(shape=(512, 512, 512)), '512 x 512 x 512'), (dict(iso=float('nan')), 'iso = nan'),
                     (dict(d=None), 'density and counts'), (dict(c=None), 'density and counts'), (dict(ws=None), 'workspace aligned'),
                     (dict(ws=FAKE + 8), 'workspace aligned')):
        assert cnt(**kw) != 0 and text in _err() and 'durf_mesh_count' in _err(), (kw, _err())
    need = L.durf_mesh_workspace_bytes(4, 4, 4)
    assert need == 256 * 4 and L.durf_mesh_workspace_bytes(1, 4, 4) == 0 and L.durf_mesh_workspace_bytes(512, 512, 512) == 0
    assert L.durf_mesh_workspace_bytes(511, 512, 512) > 9 * 511 * 512 * 512
    assert cnt(nb=need - 1) != 0
    assert 'workspace of %d bytes' % (need - 1) in _err() and 'durf_mesh_workspace_bytes(4, 4, 4) = %d' % need in _err()
    f3 = (C.c_float * 3)(1.0, 0.0, 0.0)
    f9 = (C.c_float * 9)(*([0.0] * 9))

    def emit(shape=(4, 4, 4), d=FAKE, iso=0.0, org=f3, A=f9, ws=FAKE, nb=big, mv=8, mt=8, vert=FAKE, nrm=FAKE, tri=FAKE):
        return L.durf_mesh_emit(None, *shape, d, None, iso, org, f3, f3, f3, A, 0, ws, nb, mv, mt, vert, nrm, None, None, tri)
    for kw, text in ((dict(shape=(4, 1, 4)), 'nv = 1'), (dict(shape=(1024, 1024, 128)), '1024 x 1024 x 128'),
                     (dict(iso=float('nan')), 'iso = nan'), (dict(d=None), 'density'), (dict(org=None), 'origin, du, dv and dw'),
                     (dict(A=None), 'normals need normal_xform'), (dict(mv=-1), 'max_vertices = -1'), (dict(mt=-3), 'max_triangles = -3'),
                     (dict(vert=None), 'vertices for max_vertices = 8'), (dict(tri=None), 'triangles for max_triangles = 8'),
                     (dict(ws=None), 'workspace aligned'), (dict(nb=need - 1), 'durf_mesh_workspace_bytes(4, 4, 4) = %d' % need)):
        assert emit(**kw) != 0 and text in _err() and 'durf_mesh_emit' in _err(), (kw, _err())
    assert emit(mv=0, mt=0, vert=None, tri=None, nrm=None, A=None) == 0                 # nothing to write: no launch

    def gather(shape=(4, 4, 4), c=FAKE, mv=8, ve=FAKE, Cn=3, af=FAKE, of=FAKE, ai=None, d=None, iso=0.0, oi=None):
        return L.durf_mesh_gather(None, *shape, c, mv, ve, FAKE, Cn, af, of, ai, d, None, iso, oi)
    for kw, text in ((dict(shape=(0, 4, 4)), 'nu = 0'), (dict(mv=-1), 'max_vertices = -1'), (dict(c=None), 'counts, vertex_edge and vertex_t'),
                     (dict(ve=None), 'counts, vertex_edge and vertex_t'), (dict(af=None), 'at least one attribute'),
                     (dict(of=None), 'attr_f needs out_f'), (dict(Cn=0), 'C = 0'), (dict(ai=FAKE, d=FAKE), 'attr_i needs out_i and density'),
                     (dict(ai=FAKE, oi=FAKE), 'attr_i needs out_i and density'),
                     (dict(ai=FAKE, oi=FAKE, d=FAKE, iso=float('nan')), 'iso = nan')):
        assert gather(**kw) != 0 and text in _err() and 'durf_mesh_gather' in _err(), (kw, _err())
    assert gather(mv=0) == 0


# ---- the oracle against closed forms ------------------------------------------------------------------------------------------
def _sphere(h):
    if h not in _S:
        n = int(round(4.0 / h)) + 1
        fr = M.unit_frame(h, (-2.0, -2.0, -2.0))
        _S[h] = (fr, M.surface(M.sphere_field(fr, (n, n, n), CENTRE, 1.3), None, 0.0, fr))
    return _S[h]


def test_a_sphere_is_a_closed_oriented_surface_of_genus_zero():
    _, m = _sphere(0.25)
    assert m['counts'][0] > 1000 and m['counts'][1] == m['triangles'].shape[0]
    assert M.is_closed(m['triangles']), 'every undirected edge is in exactly two triangles, once in each direction'
    assert M.euler(m['triangles']) == 2
    assert np.unique(m['triangles']).size == m['counts'][0], 'with a margin every vertex is referenced'
    assert M.signed_volume(m['vertices'], m['triangles']) > 0


def test_a_torus_and_two_spheres():
    fr = M.unit_frame(0.2, (-2.0, -2.0, -1.0))
    t = M.surface(M.torus_field(fr, (21, 21, 11), (0.01, 0.02, 0.03), 1.2, 0.45), None, 0.0, fr)
    assert M.is_closed(t['triangles']) and M.euler(t['triangles']) == 0
    assert M.signed_volume(t['vertices'], t['triangles']) > 0
    shape = (31, 16, 16)
    fr = M.unit_frame(0.2, (-3.0, -1.5, -1.5))
    d = np.maximum(M.sphere_field(fr, shape, (-1.5, 0.01, 0.02), 1.0), M.sphere_field(fr, shape, (1.5, -0.03, 0.0), 0.9))
    s = M.surface(d, None, 0.0, fr)
    assert M.is_closed(s['triangles']) and M.euler(s['triangles']) == 4
    assert M.signed_volume(s['vertices'], s['triangles']) > 0


def test_the_enclosed_volume_converges_at_second_order():
    """measured: error 1.714e-01 at h = 0.25 and 4.253e-02 at h = 0.125 (ratio 4.03) against 4/3 pi 1.3^3 = 9.2028"""
    true = 4.0 / 3.0 * np.pi * 1.3 ** 3
    err = [abs(M.signed_volume(_sphere(h)[1]['vertices'], _sphere(h)[1]['triangles']) - true) for h in (0.25, 0.125)]
    print('sphere volume error: %.3e at h, %.3e at h / 2 (ratio %.2f)' % (err[0], err[1], err[0] / err[1]))
    assert err[1] < 0.5 * err[0]


def test_normals_point_outward_and_the_twin_follows_the_oracle():
    fr, m = _sphere(0.25)
    X = m['vertices'] - np.asarray(CENTRE)
    assert (np.einsum('ij,ij->i', m['normals'], X) > 0).all()
    assert np.abs(np.linalg.norm(m['normals'], axis=1) - 1).max() < 1e-12
    n = 17
    d = M.sphere_field(fr, (n, n, n), CENTRE, 1.3)
    t32, X32, N32 = M.geometry(d, None, 0.0, fr, m['vertex_edge'], np.float32)
    assert X32.dtype == np.float32 and N32.dtype == np.float32 and t32.dtype == np.float32
    assert np.abs(X32 - m['vertices']).max() < 1e-5 and np.abs(N32 - m['normals']).max() < 1e-4
    assert (t32 >= 0).all() and (t32 <= 1).all()


def test_a_left_handed_frame_with_flip_gives_the_same_surface():
    h, n = 0.25, 17
    right = M.unit_frame(h, (-2.0, -2.0, -2.0))
    left = dict(origin=[-2.0, -2.0, -2.0], du=[h, 0.0, 0.0], dv=[0.0, 0.0, h], dw=[0.0, h, 0.0])
    assert M.host_frame(left)[5] < 0 < M.host_frame(right)[5] and mesh.host_frame(left)[5] and not mesh.host_frame(right)[5]
    a = M.surface(M.sphere_field(left, (n, n, n), CENTRE, 1.3), None, 0.0, left, flip=True)
    b = _sphere(h)[1]
    assert M.is_closed(a['triangles']) and M.euler(a['triangles']) == 2
    va, vb = M.signed_volume(a['vertices'], a['triangles']), M.signed_volume(b['vertices'], b['triangles'])
    assert va > 0 and abs(va - vb) < 2e-3 * vb, (va, vb)
    assert (np.einsum('ij,ij->i', a['normals'], a['vertices'] - np.asarray(CENTRE)) > 0).all()
    unflipped = M.surface(M.sphere_field(left, (n, n, n), CENTRE, 1.3), None, 0.0, left, flip=False)
    assert M.signed_volume(unflipped['vertices'], unflipped['triangles']) < 0


def test_the_winding_depends_on_the_case_and_the_parity_alone():
    even, odd = (0, 3, 4), (1, 2, 5)
    for cs in range(16):
        assert len({str(M.case_triangles(M.PERMS[t], cs)) for t in even}) == 1
        assert len({str(M.case_triangles(M.PERMS[t], cs)) for t in odd}) == 1
        assert len(M.case_triangles(M.PERMS[0], cs)) == (0 if cs in (0, 15) else 2 if bin(cs).count('1') == 2 else 1)
    assert any(M.case_triangles(M.PERMS[0], cs) != M.case_triangles(M.PERMS[1], cs) for cs in range(16))


def test_holes_leave_no_edge_in_more_than_two_triangles():
    fr = M.unit_frame(0.25, (-2.0, -2.0, -2.0))
    d = M.sphere_field(fr, (17, 17, 17), CENTRE, 1.3)
    v = np.ones(d.shape, np.uint8)
    v[8, 5:9, 10:15] = 0
    d[3:5, 8, 8] = np.nan
    m = M.surface(d, v, 0.0, fr)
    fwd, bwd, same = M.edge_census(m['triangles'])
    assert (fwd <= 1).all() and (bwd <= 1).all() and (same == 0).all() and ((fwd + bwd) == 1).any()
    # a lone usable pair among unusable points: its vertex exists and no tetrahedron can reference it
    d2 = np.full((3, 3, 3), np.nan, np.float32)
    d2[1, 1, 1], d2[1, 1, 2] = 1.0, -1.0
    lone = M.surface(d2, None, 0.0, M.unit_frame())
    assert lone['counts'] == (1, 0) and lone['vertex_edge'].tolist() == [[13, 0]] and lone['vertices'].tolist() == [[1.0, 1.0, 1.5]]


# ---- durf_amd/mesh.py -----------------------------------------------------------------------------------------------------------
def test_ply_round_trip(tmp_path):
    _, m = _sphere(0.25)
    g = np.random.default_rng(0)
    rgb = g.random((m['counts'][0], 3))
    path = str(tmp_path / 's.ply')
    mesh.write_ply(path, dict(vertices=m['vertices'], normals=m['normals'], triangles=m['triangles'], rgb=rgb))
    blob = open(path, 'rb').read()
    assert blob.startswith(b'ply\nformat binary_little_endian 1.0\n') and b'property list uchar int vertex_indices' in blob
    r = mesh.read_ply(path)
    assert (r['vertices'] == m['vertices'].astype(np.float32)).all() and (r['normals'] == m['normals'].astype(np.float32)).all()
    assert (r['triangles'] == m['triangles']).all() and r['triangles'].dtype == np.int32
    assert (r['rgb'] == np.rint(rgb * 255).astype(np.uint8)).all()
    mesh.write_ply(path, dict(vertices=np.zeros((0, 3)), triangles=np.zeros((0, 3), np.int32)))
    e = mesh.read_ply(path)
    assert e['vertices'].shape == (0, 3) and e['triangles'].shape == (0, 3)
    mesh.write_ply(path, dict(vertices=m['vertices'][:3], triangles=np.array([[0, 1, 2]]), normals=None, rgb=None))
    assert (mesh.read_ply(path)['rgb'] == 200).all() and (mesh.read_ply(path)['normals'] == 0).all()
    open(path, 'wb').write(blob[:-5])
    with pytest.raises(ValueError, match='header promises'):
        mesh.read_ply(path)


def _fake(K=2, use_viewdirs=True, dynamics=True, device='cuda'):
    model = types.SimpleNamespace(use_viewdirs=use_viewdirs, dynamics=dynamics)
    variables = types.SimpleNamespace(layout=types.SimpleNamespace(K=K, use_viewdirs=use_viewdirs),
                                      flat=types.SimpleNamespace(device=torch.device(device)))
    return model, variables


def test_mesh_py_refuses_loudly():
    for kw, text in ((dict(dynamics=False), 'dynamics=False'), (dict(use_viewdirs=False), 'use_viewdirs=False'), (dict(device='cpu'), 'device')):
        with pytest.raises(NotImplementedError, match=re.escape(text)):
            mesh.extract(*_fake(**kw), (0, 0, 0), (2, 2, 2), step=1.0, iso=1.0)
        with pytest.raises(NotImplementedError, match=re.escape('mesh.extract_object')):
            mesh.extract_object(*_fake(**kw), 0, np.ones((2, 3)), 0.1, 1.0)
    with pytest.raises(ValueError, match='step or axes'):
        mesh.extract(*_fake(), (0, 0, 0), (2, 2, 2), iso=1.0)
    for call in (lambda: mesh.extract(*_fake(), (0, 0, 0), (2, 2, 2), step=1.0), lambda: mesh.surface({}, None),
                 lambda: mesh.surface({}, float('nan')), lambda: mesh.extract_object(*_fake(), 0, np.ones((2, 3)), 0.1, None)):
        with pytest.raises(ValueError, match='no default'):
            call()
    with pytest.raises(ValueError, match='box 2 of K = 2'):
        mesh.extract_object(*_fake(), 2, np.ones((2, 3)), 0.1, 1.0)
    with pytest.raises(ValueError, match='colour'):
        mesh.extract(*_fake(), (0, 0, 0), (2, 2, 2), step=1.0, iso=1.0, colour='texture')
    for bad in (dict(origin=[0, 0, 0], du=[1, 0, 0], dv=[2, 0, 0], dw=[0, 0, 1]), dict(origin=[0, 0, 0], du=[1, 0, 0], dv=[0, 0, 0], dw=[0, 0, 1]),
                dict(origin=[0, 0, 0], du=[1, 1, 0], dv=[0, 1, 1], dw=[1, 2, 1])):
        with pytest.raises(ValueError, match='singular frame'):
            mesh.host_frame(bad)
    o, du, dv, dw, A, flip = mesh.host_frame(dict(origin=[1, 2, 3], du=[0.5, 0, 0], dv=[0, 0.25, 0], dw=[0, 0, 2]))
    assert not flip and A.dtype == np.float32 and A.tolist() == [2, 0, 0, 0, 4, 0, 0, 0, 0.5]
    with pytest.raises(ValueError, match='on the device'):
        mesh.surface(dict(density=torch.zeros(3, 3, 3), frame=M.unit_frame()), 0.5)


def test_the_object_lattice_stays_inside_the_padded_box():
    c, R = np.array([1.0, -2.0, 0.5]), mesh.aa2matrix([0.1, -0.2, 0.7])
    assert np.abs(R @ R.T - np.eye(3)).max() < 1e-9 and abs(np.linalg.det(R) - 1) < 1e-9
    ext = np.array([0.5, 0.3, 0.25])
    obj, world, shape = mesh.object_lattice(c, R, ext, 0.05, 0.05)
    for j, key in enumerate(('du', 'dv', 'dw')):
        far = obj['origin'][j] + (shape[j] - 1) * obj[key][j]
        assert abs(far + obj['origin'][j]) < 1e-12 and ext[j] * 1.05 - 0.05 / 2 - 1e-6 < far <= ext[j] * 1.05
    P = M.lattice_points(obj, shape).reshape(-1, 3)
    X = M.lattice_points(world, shape).reshape(-1, 3)
    assert np.abs((X - c) @ R.T - P).max() < 1e-12, 'P = R (X - c)'
    with pytest.raises(ValueError, match='lattice of'):
        mesh.object_lattice(c, R, ext, 0.4, 0.05)


def test_the_commands_default_iso_is_query_fields_threshold():
    ap = extract_mesh.build_parser()
    a = ap.parse_args(['--eval_dir', 'x', '--synthetic', '--objects'])
    assert a.iso == query_field.build_parser().get_default('threshold') == extract_mesh.default_iso()
    assert a.write_objects is True and a.synthetic_boxes == 3 and ap.parse_args(['--eval_dir', 'x']).write_objects is False
    for flag in ('--gin_file', '--grid', '--iso', '--ts', '--eval_dir', '--objects', '--synthetic', '--train_dir', '--data_dir'):
        assert flag in ap.format_help(), flag
