"""The reference's side of a cross-check, stored: what the reference's own functions returned on the tests' seeded inputs,
kept in tests/golden/<name>.npz so that the cross-checks run without the reference tree.

    DURF_RECORD_REFERENCE=1 python -m pytest tests/<module>.py     # where the reference tree is: (re)writes the fixture

A record run calls the reference (through tests/ref_standin.py's stand-ins, as the tests always did) and stores every value
it returns; any other run reads the values back under the same keys.  The inputs are regenerated from the tests' seeds either
way, and the oracle side always runs live.  A fixture is data -- outputs of seeded runs -- no reference text."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
SEP = '|'


def recording():
    return os.environ.get('DURF_RECORD_REFERENCE', '0') != '0'


def _current_test():
    # "tests/test_x.py::test_name[param] (call)" -> "test_name[param]"
    return os.environ['PYTEST_CURRENT_TEST'].split('::', 1)[1].rsplit(' ', 1)[0]


def _flatten(value, key, out):
    if value is None:
        out[key + SEP + '~'] = np.zeros(0)
    elif isinstance(value, (list, tuple)):
        out[key + SEP + '#'] = np.array(len(value))
        for i, v in enumerate(value):
            _flatten(v, key + SEP + str(i), out)
    else:
        out[key] = np.array(value)            # (a copy: the caller may change its array afterwards)


def _unflatten(store, key):
    if key + SEP + '~' in store:
        return None
    if key + SEP + '#' in store:
        return [_unflatten(store, key + SEP + str(i)) for i in range(int(store[key + SEP + '#']))]
    if key not in store:
        raise KeyError('%s: not in the stored reference outputs -- re-record with DURF_RECORD_REFERENCE=1' % key)
    return store[key].copy()


class Recorder:
    """outputs(key, compute): compute() when recording (and stored), else the stored value -- nested tuples / lists read
    back as lists, arrays and numbers as numpy arrays.  calls(mods): `mods` (a namespace of modules) with every function call
    recorded under '<test>:<n>' -- the n-th reference call of the running test."""

    def __init__(self, name):
        self.path = os.path.join(GOLDEN, name + '.npz')
        self.store = {} if recording() else None        # (read at the first lookup, not when the test module is collected)
        self.counts = {}

    def outputs(self, key, compute):
        key = _current_test() + SEP + key
        if recording():             # (the live value goes on to the test, exactly as without the recorder)
            value = compute()
            _flatten(value, key, self.store)
            return value
        if self.store is None:
            self.store = dict(np.load(self.path))
        return _unflatten(self.store, key)

    def calls(self, mods):
        rec = self

        class Fn:
            def __init__(self, path):
                self.path = path

            def __getattr__(self, name):
                return Fn(self.path + (name,))

            def __call__(self, *a, **k):
                def compute():
                    f = mods
                    for p in self.path:
                        f = getattr(f, p)
                    return f(*a, **k)
                t = _current_test()
                n = rec.counts[t] = rec.counts.get(t, -1) + 1
                return rec.outputs('%s:%d' % ('.'.join(self.path), n), compute)
        return Fn(())

    def save(self):
        if recording():
            np.savez_compressed(self.path, **self.store)
