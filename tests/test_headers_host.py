"""The generated tables (durf_amd/_sigs.py, durf_amd/_<name>_sigs.py: tools/gen_integration_stub.py) against the headers they
are generated from, with the C compiler as the judge: the value of every `#define DURF_*`, the size of every `durf_*` struct,
the offset of every field (and the size of every array field), and every function-like macro at sizes around its block
edges.  The generator reads the headers with regular expressions of its own; this test reads nothing but names."""
import ctypes as C
import importlib
import inspect
import itertools
import os
import re
import subprocess

import pytest

from durf_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MACRO_ARGS = (0, 1, 255, 256, 257, 4095, 4096, 4097, 1000003)
OPS_NAMES = dict(durf_loss_level='LossLevel', durf_forward_args='ForwardArgs', durf_step_timing='StepTiming',
                 durf_train_args='TrainArgs', durf_field_args='FieldArgs', DURF_LIDAR_COMPACT_SCRATCH='lidar_compact_scratch',
                 DURF_FLOW_POSE_FLOATS='flow_pose_floats', DURF_FLOW_CONS_SCRATCH='flow_cons_scratch',
                 DURF_FIELD_POSE_FLOATS='field_pose_floats')


def _table(name):
    mod = importlib.import_module('durf_amd._sigs' if name == 'hip' else 'durf_amd._%s_sigs' % name)
    own = {k: v for k, v in vars(mod).items() if k.lower().startswith('durf_')}
    consts = {k: v for k, v in own.items() if type(v) is int}
    macros = {k: v for k, v in own.items() if inspect.isfunction(v)}
    structs = {k: v for k, v in own.items() if inspect.isclass(v) and issubclass(v, C.Structure)}
    assert len(consts) + len(macros) + len(structs) == len(own), sorted(set(own) - set(consts) - set(macros) - set(structs))
    return consts, macros, structs


@pytest.mark.parametrize('name', ('hip',) + _lib.SATELLITES)
def test_generated_tables_match_the_compiled_header(name, tmp_path):
    consts, macros, structs = _table(name)
    # completeness, both ways: the names a plain search finds in the header are the names the table holds
    text = re.sub(r'/\*.*?\*/', ' ', open(os.path.join(ROOT, 'include', 'durf_%s.h' % name)).read(), flags=re.S)
    guards = set(re.findall(r'#\s*ifndef\s+(DURF_\w+_H)\b', text))
    defined = set(re.findall(r'#\s*define\s+(DURF_\w+)', text)) - guards
    assert defined == set(consts) | set(macros), defined ^ (set(consts) | set(macros))
    assert set(re.findall(r'\}\s*(durf_\w+)\s*;', text)) == set(structs)
    assert defined, 'no #define found in the header'

    ll = lambda what, expr: '  printf("%s %%lld\\n", (long long)(%s));' % (what, expr)
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "durf_%s.h"' % name, 'int main(void) {']
    want = {}
    for k, v in consts.items():
        lines.append(ll(k, k))
        want[k] = v
    for k, fn in macros.items():
        for args in itertools.product(MACRO_ARGS, repeat=len(inspect.signature(fn).parameters)):
            what = '%s(%s)' % (k, ','.join(map(str, args)))
            lines.append(ll(what, '%s(%s)' % (k, ', '.join('%dLL' % a for a in args))))
            want[what] = fn(*args)
    for k, cls in structs.items():
        lines.append(ll('sizeof:' + k, 'sizeof(%s)' % k))
        want['sizeof:' + k] = C.sizeof(cls)
        for field, ctype in cls._fields_:
            lines.append(ll('offsetof:%s.%s' % (k, field), 'offsetof(%s, %s)' % (k, field)))
            want['offsetof:%s.%s' % (k, field)] = getattr(cls, field).offset
            if issubclass(ctype, C.Array):
                lines.append(ll('sizeof:%s.%s' % (k, field), 'sizeof(((%s*)0)->%s)' % (k, field)))
                want['sizeof:%s.%s' % (k, field)] = C.sizeof(ctype)
    lines += ['  return 0;', '}']
    src, exe = tmp_path / 'probe.c', tmp_path / 'probe'
    src.write_text('\n'.join(lines) + '\n')
    subprocess.run(['gcc', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    got = {k: int(v) for k, v in (line.rsplit(' ', 1) for line in out.splitlines())}
    assert set(got) == set(want)
    wrong = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not wrong, 'compiled header against generated table: %s' % wrong
    # durf_amd/ops.py's public names are these very objects, not copies of them
    from durf_amd import ops
    assert all(getattr(ops, k[len('DURF_'):]) == v for k, v in consts.items() if k != 'DURF_OVERLAP_MIN_ROWS')
    assert 'OVERLAP_MIN_ROWS' not in vars(ops)                      # (launch policy: ops asks the library, tests/test_policy_host.py)
    assert all(getattr(ops, OPS_NAMES[k]) is v for k, v in {**structs, **macros}.items() if k in OPS_NAMES)
    assert set(structs) <= set(OPS_NAMES)
