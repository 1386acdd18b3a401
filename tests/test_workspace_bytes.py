"""The workspace sizes of the one-call entry points are part of what a host allocates by: every `*_workspace_bytes`
function must return what it returned before the carvers of csrc/forward.hip and csrc/train.hip were folded into
csrc/workspace.h.  tests/workspace_bytes_parent.json was recorded from the library built at the commit before that change
(inference shapes x n_rays 63 / 153600 x F 1 / 600, training shapes x flags 0 / 1 / 3 / 5: buffers on both sides of the
1 MB alignment switch).  Host arithmetic: no device."""
import json
import os

import pytest

from durf_amd import _lib

RECORDED = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'workspace_bytes_parent.json')))['values']
FUNCTIONS = ('durf_forward_workspace_bytes', 'durf_render_image_workspace_bytes', 'durf_render_layers_workspace_bytes',
             'durf_render_trajectory_workspace_bytes', 'durf_train_workspace_bytes', 'durf_train_workspace_bytes_flags')


def test_every_sizing_function_is_recorded():
    assert {r['fn'] for r in RECORDED} == set(FUNCTIONS)


@pytest.mark.parametrize('fn', FUNCTIONS)
def test_workspace_bytes_equal_the_parent(fn):
    f = getattr(_lib.lib(), fn)
    rows = [r for r in RECORDED if r['fn'] == fn]
    assert rows
    for r in rows:
        assert int(f(*r['args'])) == r['bytes'], (fn, r['args'])
