"""The triangle mesh on the host: what every mesh consumer refuses, replayed against tests/golden/trimesh_refusals.json
as the five entries gave it before durf_amd/trimesh.py held their checks (no device: a call that gets as far as the device is
recorded as such), and trimesh_ref's three rules on cases small enough to write out by hand.

    python -m tests.test_trimesh_host tests/golden/trimesh_refusals.json      # records the file from the tree it runs in"""
import inspect
import json
import os
import sys

import numpy as np
import pytest

from tests import trimesh_ref as M

GOLDEN = os.path.join(os.path.dirname(__file__), 'golden', 'trimesh_refusals.json')
DEVICE = 'accepted up to the first device call'
ENTRIES = ('raster.render_mesh', 'cast.build', 'geometry.sample_mesh', 'closest.points', 'shade.cameras')


class _Reached(Exception):
    pass


class _Shape:
    """an array too large to make: a shape and a dtype, nothing else"""

    def __init__(self, shape, dtype):
        self.shape, self.dtype = shape, np.dtype(dtype)


def cases():
    """name -> (mesh, keywords of raster.render_mesh)"""
    v, t = M.icosphere(0)
    V = v.shape[0]
    ok = dict(vertices=v, triangles=t)
    return {
        'well_formed': (ok, {}),
        'not_a_dict': ([v, t], {}),
        'none': (None, {}),
        'missing_triangles': (dict(vertices=v), {}),
        'vertices_none': (dict(vertices=None, triangles=t), {}),
        'vertices_V2': (dict(vertices=v[:, :2], triangles=t), {}),
        'triangles_T4': (dict(vertices=v, triangles=np.concatenate([t, t[:, :1]], 1)), {}),
        'one_dimensional': (dict(vertices=v.reshape(-1), triangles=t.reshape(-1)), {}),
        'attribute_short': (dict(ok, rgb=np.zeros((V - 1, 3), np.float32)), dict(attrs=('rgb',))),
        'label_short': (dict(ok, owner=np.zeros(V - 1, np.int32)), {}),
        'attribute_key_not_a_string': (dict(ok, rgb=np.zeros((V, 3), np.float32)), dict(attrs=('rgb', 3))),
        'attrs_a_string': (dict(ok, rgb=np.zeros((V, 3), np.float32)), dict(attrs='rgb')),
        'label_not_a_string': (ok, dict(label=5)),
        'T_at_the_cast_limit': (dict(vertices=v, triangles=_Shape((1 << 30, 3), np.int32)), {}),
        'T_at_2_31': (dict(vertices=v, triangles=_Shape((1 << 31, 3), np.int32)), {}),
        'V_at_2_31': (dict(vertices=_Shape((1 << 31, 3), np.float32), triangles=t), {}),
    }


def _call(entry, m, kw):
    from durf_amd import camera, cast, closest, geometry, raster, shade
    cams = camera.rows([np.eye(4, dtype=np.float32)], 8.0, (4.0, 3.0), 6, 8)
    if entry == 'raster.render_mesh':
        return raster.render_mesh(m, cams, **kw)
    if entry == 'cast.build':
        return cast.build(m)
    if entry == 'geometry.sample_mesh':
        return geometry.sample_mesh(m, 5)
    if entry == 'closest.points':
        return closest.points(m, np.zeros((2, 3), np.float32))
    return shade.cameras(m, cams)


def outcome(entry, m, kw, monkeypatch):
    """[exception type, message] of the call, or [DEVICE, ''] when it reaches the device (any durf_amd.ops function, or the
    choice of the current device) without a refusal"""
    import torch
    from durf_amd import ops

    def reached(*a, **k):
        raise _Reached()
    with monkeypatch.context() as mp:
        mp.setattr(torch.cuda, 'current_device', reached)
        for name, f in inspect.getmembers(ops, inspect.isfunction):
            if f.__module__ == ops.__name__ and not name.startswith('_'):
                mp.setattr(ops, name, reached)
        try:
            _call(entry, m, kw)
        except _Reached:
            return [DEVICE, '']
        except Exception as e:  # noqa: BLE001  (whatever the entry raises is what is recorded)
            return [type(e).__name__, str(e)]
    return ['returned', '']


def record(monkeypatch):
    return {name: {entry: outcome(entry, m, kw, monkeypatch) for entry in ENTRIES} for name, (m, kw) in cases().items()}


def test_every_entry_refuses_a_malformed_mesh_as_it_did(monkeypatch):
    want = json.load(open(GOLDEN))
    assert sorted(want) == sorted(cases()) and all(sorted(w) == sorted(ENTRIES) for w in want.values())
    got = record(monkeypatch)
    for name in want:
        for entry in ENTRIES:
            assert got[name][entry] == want[name][entry], (name, entry)
    kinds = {o[0] for w in want.values() for o in w.values()}
    assert DEVICE in kinds and 'ValueError' in kinds and 'returned' not in kinds


# ---- the three rules by hand --------------------------------------------------------------------------------------------------------
def test_valid_triangles_by_hand():
    nan = np.nan
    v = np.asarray([(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (nan, 0, 0)], np.float32)           # V = 5, vertex 4 is not finite
    t = np.asarray([(0, 1, 2), (0, -1, 2), (0, 1, 5), (1, 2, 4), (3, 2, 1), (0, 1, 2 ** 31 - 1)], np.int32)
    ok, P = M.valid_triangles(v, t)
    assert ok.tolist() == [True, False, False, False, True, False]         # a negative index, index == V, a NaN vertex, INT_MAX
    assert np.array_equal(P[0], v[[0, 1, 2]]) and np.array_equal(P[4], v[[3, 2, 1]]) and not P[~ok].any()
    ok, P = M.valid_triangles(np.zeros((0, 3), np.float32), np.zeros((2, 3), np.int32))
    assert ok.tolist() == [False, False] and P.shape == (2, 3, 3)


def test_interp32_by_hand():
    t = np.asarray([(0, 1, 2), (2, 1, 3), (0, 1, 4)], np.int32)           # T = 3; triangle 2 names vertex 4 == V
    attr = np.asarray([(1.0, 10.0), (2.0, 20.0), (4.0, 40.0), (8.0, 80.0)], np.float32)
    tri = np.asarray([0, 1, -1, -2, 3, 2], np.int32)                       # two hits, nothing, unusable, id == T, a bad index
    bary = np.asarray([(0.5, 0.25, 0.25), (0.0, 1.0, 0.0), (1, 1, 1), (nan := np.nan, nan, nan), (1, 0, 0), (1, 0, 0)], np.float32)
    got = M.interp32(t, tri, bary, attr)
    assert got.dtype == np.float32 and got.tolist() == [[2.0, 20.0], [2.0, 20.0], [0, 0], [0, 0], [0, 0], [0, 0]]
    # the order of the sum: (q0 a0 + q1 a1) + q2 a2, not q0 a0 + (q1 a1 + q2 a2)
    one, eps = np.float32(1.0), np.float32(2.0 ** -24)
    got = M.interp32([(0, 1, 2)], [0], [(1.0, 1.0, 1.0)], np.asarray([[one], [eps], [eps]], np.float32))
    assert got[0, 0] == (one + eps) + eps == one and one + (eps + eps) != one
    assert M.interp32(np.zeros((0, 3), np.int32), [0, -1], np.ones((2, 3), np.float32), attr).tolist() == [[0, 0], [0, 0]]


def test_u8_by_hand():
    x = np.asarray([0.5 / 255, 1.5 / 255, 2.5 / 255, np.nan, -1.0, 2.0, 0.0, 1.0, np.inf, -np.inf, 0.999], np.float32)
    # float32(k / 255) * 255 rounds to k exactly for these three: 0.5 -> 0, 1.5 -> 2 and 2.5 -> 2 by round-half-even
    assert M.u8(x).tolist() == [0, 2, 2, 0, 0, 255, 0, 255, 255, 0, 255]
    assert M.u8(x).dtype == np.uint8 and M.u8(x.reshape(1, -1, 1)).shape == (1, 11, 1)


def test_the_old_homes_hand_out_the_same_objects():
    from tests import cast_ref, closest_ref, shade_ref, tsdf_ref           # noqa: F401
    assert cast_ref.valid_triangles is M.valid_triangles and shade_ref.interp32 is M.interp32 and shade_ref.u8 is M.u8
    for name in ('icosphere', 'box_mesh', 'quad_grid', 'dirty_mesh', 'random_soup'):
        assert getattr(cast_ref, name) is getattr(M, name), name
    assert shade_ref.merge is M.merge and tsdf_ref.icosphere is M.icosphere


if __name__ == '__main__':
    mp = pytest.MonkeyPatch()
    json.dump(record(mp), open(sys.argv[1], 'w'), indent=1, sort_keys=True)
    mp.undo()
