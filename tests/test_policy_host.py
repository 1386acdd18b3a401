"""The launch policy of a step's bf16 object work (durf_step_policy, csrc/policy.h) without a GPU: the library's answer and the
five readers in durf_amd/ops.py against a truth table written out here.

The table is what the code BEFORE the policy function did, read off its two statements of the rule (ops.py: _MODE /
overlap_mode / overlap_forward / overlap_backward / overlap_dw / obj_mix; csrc/mlp_fwd.hip: msplit_enabled / obj_msplit /
obj_mix), which factor as written below: the side bits depend on DURF_OVERLAP_OBJECTS and on which side of the threshold the
row count lies; the M-split and mix bits on DURF_OBJ_MSPLIT, DURF_OBJ_MIX and the same side; ops.obj_mix is the mix bit of a
step that runs on one stream.  Two cases differed between the languages then and are pinned here: modes '1' and '3' (the C
obj_mix ignored the mode, ops.obj_mix is False there -- both survive, as DURF_POLICY_MIX and as ops.obj_mix), and a change of
the environment after `import durf_amd.ops` (the Python side kept the value seen at import; now every reader follows it)."""
import itertools
import os
import re

import pytest

from durf_amd import _lib, _sigs, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = 2048 * 128
SIDE = {32: 'small', T - 32: 'small', T: 'large', 4096 * 128: 'large'}
# (DURF_OVERLAP_OBJECTS, side of the threshold) -> (overlap_mode, overlap_forward, overlap_backward, overlap_dw)
OVERLAP = {
    (None, 'small'): ('0', False, False, False), (None, 'large'): ('2', True, True, True),
    ('auto', 'small'): ('0', False, False, False), ('auto', 'large'): ('2', True, True, True),
    ('0', 'small'): ('0', False, False, False), ('0', 'large'): ('0', False, False, False),
    ('1', 'small'): ('1', True, False, False), ('1', 'large'): ('1', True, False, False),
    ('2', 'small'): ('2', True, True, True), ('2', 'large'): ('2', True, True, True),
    ('3', 'small'): ('3', True, True, False), ('3', 'large'): ('3', True, True, False),
}
# (DURF_OBJ_MSPLIT, DURF_OBJ_MIX, side of the threshold) -> (msplit, mix enabled)
MSPLIT_MIX = {
    (None, None, 'small'): (True, True), (None, None, 'large'): (False, False),
    (None, '0', 'small'): (True, False), (None, '0', 'large'): (False, False),
    ('0', None, 'small'): (False, False), ('0', None, 'large'): (False, False),
    ('0', '0', 'small'): (False, False), ('0', '0', 'large'): (False, False),
}
CASES = list(itertools.product([None, 'auto', '0', '1', '2', '3'], [None, '0'], [None, '0'], sorted(SIDE)))


def _set(monkeypatch, **env):
    for k, v in env.items():
        if v is None:
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, v)


def _bits():
    hdr = open(os.path.join(ROOT, 'include', 'durf_hip.h')).read()
    return {m.group(1): int(m.group(2), 16) for m in re.finditer(r'#define DURF_POLICY_(\w+) (0x[0-9a-fA-F]+)', hdr)}


def test_the_header_names_five_bits_and_one_threshold():
    assert _bits() == dict(SIDE_FWD=0x1, SIDE_BWD=0x2, SIDE_DW=0x4, MSPLIT=0x8, MIX=0x10)
    assert [1 << i for i in range(5)] == [_bits()[n] for n in ('SIDE_FWD', 'SIDE_BWD', 'SIDE_DW', 'MSPLIT', 'MIX')]
    assert ops.StepPolicy._fields == ('side_fwd', 'side_bwd', 'side_dw', 'msplit', 'mix_enabled')     # ops.step_policy: in bit order
    assert int(_lib.lib().durf_overlap_min_rows()) == T == ops.OVERLAP_MIN_ROWS
    for name in ('durf_step_policy', 'durf_overlap_min_rows'):
        assert name in _sigs.SIGS and name in _lib.symbols() and hasattr(_lib.lib(), name)
        assert name in open(os.path.join(ROOT, 'include', 'durf_ctypes_stub.py')).read()
        assert name in open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    assert _lib.lib().durf_version() == 41


@pytest.mark.parametrize('overlap,msplit,mix,rows', CASES)
def test_policy_truth_table(monkeypatch, overlap, msplit, mix, rows):
    _set(monkeypatch, DURF_OVERLAP_OBJECTS=overlap, DURF_OBJ_MSPLIT=msplit, DURF_OBJ_MIX=mix)
    mode, fwd, bwd, dw = OVERLAP[(overlap, SIDE[rows])]
    want_ms, want_mix = MSPLIT_MIX[(msplit, mix, SIDE[rows])]
    B = _bits()
    want = ((B['SIDE_FWD'] if fwd else 0) | (B['SIDE_BWD'] if bwd else 0) | (B['SIDE_DW'] if dw else 0) |
            (B['MSPLIT'] if want_ms else 0) | (B['MIX'] if want_mix else 0))
    assert int(_lib.lib().durf_step_policy(rows)) == want
    assert ops.step_policy(rows) == (fwd, bwd, dw, want_ms, want_mix)
    assert ops.overlap_mode(rows) == mode
    assert (ops.overlap_forward(rows), ops.overlap_backward(rows), ops.overlap_dw(rows)) == (fwd, bwd, dw)
    assert ops.obj_mix(rows) is (want_mix and mode == '0')


@pytest.mark.parametrize('mode', ['1', '3'])
def test_modes_1_and_3_keep_the_mix_bit_and_do_not_mix(monkeypatch, mode):
    _set(monkeypatch, DURF_OVERLAP_OBJECTS=mode, DURF_OBJ_MSPLIT=None, DURF_OBJ_MIX=None)
    assert int(_lib.lib().durf_step_policy(512 * 128)) & _bits()['MIX']      # as csrc/mlp_fwd.hip's obj_mix: the mode is not its business
    assert ops.step_policy(512 * 128).mix_enabled and not ops.step_policy(512 * 128).mix
    assert ops.obj_mix(512 * 128) is False                                   # as ops.obj_mix: a step with a side stream does not mix


def test_the_environment_is_followed_after_import(monkeypatch):
    rows = 512 * 128
    _set(monkeypatch, DURF_OVERLAP_OBJECTS=None, DURF_OBJ_MSPLIT=None, DURF_OBJ_MIX=None)
    assert ops.overlap_mode(rows) == '0' and ops.obj_mix(rows) and ops._MODE == 'auto'
    monkeypatch.setenv('DURF_OVERLAP_OBJECTS', '2')          # what tests/test_gpu_dist.py does: both orchestrations move
    assert ops.overlap_mode(rows) == '2' and ops.overlap_dw(rows) and not ops.obj_mix(rows) and ops._MODE == '2'
    assert int(_lib.lib().durf_step_policy(rows)) & 0x7 == 0x7
    monkeypatch.setenv('DURF_OBJ_MIX', '0')
    monkeypatch.setenv('DURF_OVERLAP_OBJECTS', '0')
    assert ops.overlap_mode(4096 * 128) == '0' and not ops.obj_mix(rows) and ops.step_policy(rows).msplit
    # set_overlap_mode writes the variable and nothing else; ops._MODE reads back what restores the present setting
    monkeypatch.setenv('DURF_OVERLAP_OBJECTS', '3')
    keep = ops._MODE
    ops.set_overlap_mode('auto')
    assert os.environ['DURF_OVERLAP_OBJECTS'] == 'auto' and ops.overlap_mode(rows) == '0' and ops.overlap_mode(T) == '2'
    ops.set_overlap_mode(keep)
    assert os.environ['DURF_OVERLAP_OBJECTS'] == '3' and ops.overlap_mode(rows) == '3' and '_MODE' not in vars(ops)
