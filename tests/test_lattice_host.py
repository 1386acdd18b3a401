"""The lattice on the host (durf_amd/lattice.py, tests/lattice_ref.py): one definition behind field, mesh, parts,
tsdf and closest.

tests/golden/lattice_frames.json holds what the five modules' own frame builders returned, or refused with, before they shared
one: field.grid, tsdf.volume, closest.grid, mesh.host_frame and mesh.object_lattice on a scalar step, three steps, skewed,
left-handed and singular frames, wrong lengths, both or neither of step and axes, a shape with a 1 and a shape of 2^27 points.
The callers must reproduce it exactly: values, types and messages.  No device is touched: the library calls are stubbed."""
import json
import os

import numpy as np
import pytest

from durf_amd import closest, field, lattice, mesh, ops, tsdf
from tests import lattice_ref, mesh_ref, tsdf_ref

GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'lattice_frames.json')))
F32 = np.float32
# skewed, left-handed, no component a dyadic rational
SKEW = dict(origin=[0.3, -1.7, 2.1], du=[0.31, 0.02, -0.013], dv=[0.023, -0.011, 0.19], dw=[-0.017, 0.27, 0.041])


def _enc(v):
    """a result as the golden file holds it: arrays with their dtype, tuples marked, lists, dicts, floats, ints and bools as JSON's
    own -- and as one JSON string, in which 1, 1.0 and true differ"""
    def plain(v):
        if isinstance(v, np.ndarray):
            return {'array': str(v.dtype), 'values': [float(x) for x in v.reshape(-1)]}
        if isinstance(v, tuple):
            return {'tuple': [plain(x) for x in v]}
        if isinstance(v, list):
            return [plain(x) for x in v]
        if isinstance(v, dict):
            return {k: plain(x) for k, x in v.items()}
        assert type(v) in (float, int, bool, np.bool_), type(v)
        return bool(v) if isinstance(v, np.bool_) else v
    return json.dumps(plain(v))


def _run(fn, kw, monkeypatch):
    if fn == 'field.grid':
        monkeypatch.setattr(field, '_args', lambda *a, **k: (None, None))
        monkeypatch.setattr(ops, 'field_grid', lambda *a, **k: {})
        variables = type('V', (), {'flat': type('F', (), {'device': 'cpu'})()})()
        return field.grid(None, variables, **kw)['frame']
    if fn == 'tsdf.volume':
        return tsdf.volume(device='cpu', colour=False, **kw)['frame']
    if fn == 'closest.grid':
        monkeypatch.setattr(ops, 'closest_grid', lambda *a, **k: (None, None))
        return closest.grid(dict(ws=0, T=1), **kw)['frame']
    if fn == 'mesh.host_frame':
        return mesh.host_frame(**kw)
    assert fn == 'mesh.object_lattice', fn
    return mesh.object_lattice(np.asarray(kw['c'], np.float64), np.asarray(kw['R'], np.float64), kw['ext_k'], kw['step'], kw['pad'])


@pytest.mark.parametrize('case', GOLDEN, ids=['%02d-%s' % (i, c['fn']) for i, c in enumerate(GOLDEN)])
def test_the_callers_build_and_refuse_what_they_did(case, monkeypatch):
    if 'error' in case:
        with pytest.raises(ValueError) as e:
            _run(case['fn'], case['args'], monkeypatch)
        assert str(e.value) == case['error']
    else:
        assert _enc(_run(case['fn'], case['args'], monkeypatch)) == json.dumps(case['result'])


def test_the_golden_file_covers_what_it_says():
    fns = {c['fn'] for c in GOLDEN}
    assert fns == {'field.grid', 'tsdf.volume', 'closest.grid', 'mesh.host_frame', 'mesh.object_lattice'} and len(GOLDEN) >= 20
    errors = ' '.join(c.get('error', '') for c in GOLDEN)
    for text in ('give step or axes', 'three components each', 'a singular frame', '3 x 1 x 5 points', '512 x 512 x 512 points',
                 'one or three finite steps'):
        assert text in errors, text


def test_the_shape_rule():
    assert lattice.check_shape([2, 2, 2], 'x') == (2, 2, 2) and lattice.check_shape((512, 512, 511), 'x') == (512, 512, 511)
    for bad in ((1, 4, 5), (4, 5, 1), (512, 512, 512)):
        with pytest.raises(ValueError, match=r'x: a lattice of %d x %d x %d points \(each dimension >= 2, fewer than 2\^27 points\)' % bad):
            lattice.check_shape(bad, 'x')


def test_one_point_rule_behind_every_oracle():
    """lattice_ref.points in float32 is, bit for bit, what each library's oracle placed its points with before they shared it
    (restated here, in each one's own array layout), on a skewed frame with non-dyadic components"""
    shape = (3, 4, 5)
    P = lattice_ref.points(SKEW, shape, F32)
    assert P.dtype == F32 and P.shape == (60, 3)
    o, du, dv, dw = (np.asarray(SKEW[k], F32) for k in ('origin', 'du', 'dv', 'dw'))
    i, j, k = (a.reshape(-1).astype(F32) for a in np.meshgrid(np.arange(3), np.arange(4), np.arange(5), indexing='ij'))
    columns = np.stack([((o[c] + i * du[c]) + j * dv[c]) + k * dw[c] for c in range(3)], 1)        # field_ref, tsdf_ref
    rows = (((o + i[:, None] * du) + j[:, None] * dv) + k[:, None] * dw).astype(F32)                # closest_ref
    assert columns.dtype == F32 and P.tobytes() == columns.tobytes() == rows.tobytes()
    assert not np.array_equal(P, lattice_ref.points(SKEW, shape, np.float64).astype(F32)), 'the frame is awkward enough to tell'
    # the name the tsdf oracle keeps
    assert tsdf_ref.voxels(SKEW, shape, F32).tobytes() == P.tobytes()
    # the index and the edges: g = (i nv + j) nw + k, edge e ends at the point whose offset has the bits of e + 1
    g = np.arange(60)
    gi, gj, gk = lattice_ref.ijk(g, shape)
    assert np.array_equal((gi * 4 + gj) * 5 + gk, g) and gi.max() == 2 and gj.max() == 3 and gk.max() == 4
    assert [tuple(int(x) for x in lattice_ref.edge(np.int64(e))) for e in range(7)] == [(0, 0, 1), (0, 1, 0), (0, 1, 1), (1, 0, 0), (1, 0, 1), (1, 1, 0), (1, 1, 1)]
    assert lattice_ref.edge_end(7, 4, shape) == 7 + 20 + 1
    # mesh_ref places a vertex with the same rule at fractional coordinates
    half = lattice_ref.place(SKEW, [i + F32(0.5), j, k], F32)
    assert half.tobytes() == np.stack([((o[c] + (i + F32(0.5)) * du[c]) + j * dv[c]) + k * dw[c] for c in range(3)], 1).tobytes()


def test_the_host_frame_is_the_oracles():
    for frame in (SKEW, dict(SKEW, dv=SKEW['dw'], dw=SKEW['dv']), lattice_ref.frame_of([1.0, 2.0, 3.0], 0.23), mesh_ref.unit_frame(0.2, (-2.0, -2.0, -1.0))):
        got, want = lattice.host(frame, 'x'), lattice_ref.host_frame(frame)
        for a, b in zip(got[:5], want[:5]):
            assert a.dtype == F32 and a.tobytes() == np.asarray(b, F32).reshape(-1).tobytes()
        assert got[5] == (want[5] < 0)
        assert mesh.host_frame(frame)[4].tobytes() == got[4].tobytes()
        assert lattice_ref.inverse_of(frame).tobytes() == np.ascontiguousarray(got[4].reshape(3, 3).T).tobytes()
    assert lattice.host(SKEW, 'x')[5] and not lattice.host(dict(SKEW, dv=SKEW['dw'], dw=SKEW['dv']), 'x')[5]
    assert mesh_ref.unit_frame(0.25, (1, 2, 3)) == dict(origin=[1.0, 2.0, 3.0], du=[0.25, 0.0, 0.0], dv=[0.0, 0.25, 0.0], dw=[0.0, 0.0, 0.25])
