"""ctypes binding of libdurf_hip.so (C ABI in include/durf_hip.h).

The library is the product: there is no CPU or eager-PyTorch fallback.  If the shared
object is missing this module raises at import of any op (run `python -c "import
__graft_entry__ as g; g.build()"` or `make -C durf_amd/csrc`).
"""
import ctypes as C
import functools
import importlib
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# DURF_LIB_PATH: kernel-tuning A/B builds (tools/build_variant.sh); the default is the in-tree build
LIB_PATH = os.environ.get('DURF_LIB_PATH') or os.path.join(_HERE, 'libdurf_hip.so')

# the feature libraries built beside it, libdurf_<name>.so (include/durf_<name>.h): each links against libdurf_hip.so, reports
# errors through its durf_last_error, and keeps its own entry points.  One word here (and one in csrc/Makefile) adds one.
SATELLITES = ('overlay', 'lidar', 'flow', 'field', 'mesh', 'geom', 'parts', 'raster', 'tsdf', 'cast', 'closest', 'shade', 'smooth')

_lib = None
_satellites = {}

from ._sigs import SIGS as _SIGS       # generated from include/durf_hip.h (tools/gen_integration_stub.py)


def symbols():
    """Every symbol include/durf_hip.h declares (checked by the CPU test-suite)."""
    return sorted(_SIGS)


def _bind(L, sigs):
    for name, (res, args) in sigs.items():
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = args
    return L


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                'libdurf_hip.so not built (%s): the HIP extension is required, there is no '
                'fallback path.  Run __graft_entry__.build().' % LIB_PATH)
        # PyTorch first: the process must hold ONE HIP runtime -- the copy torch brings.  Loaded before torch, this library
        # would bind /opt/rocm's libamdhip64 and torch would then load its own next to it; launches from here then fail with
        # "no ROCm-capable device is detected" (seen with __graft_entry__.build() followed by smoke() in one process).
        import torch  # noqa: F401
        _lib = _bind(C.CDLL(LIB_PATH), _SIGS)
    return _lib


def satellite_path(name):
    return os.path.join(_HERE, 'libdurf_%s.so' % name)


def _satellite_sigs(name):
    """the table generated from include/durf_<name>.h, read on first use: importing this module needs none of them"""
    if name not in SATELLITES:
        raise KeyError('no satellite library %r (durf_amd._lib.SATELLITES)' % (name,))
    return importlib.import_module('._%s_sigs' % name, __package__).SIGS


def satellite_symbols(name):
    """Every symbol include/durf_<name>.h declares."""
    return sorted(_satellite_sigs(name))


def satellite(name):
    """libdurf_<name>.so, after libdurf_hip.so (it calls that library and reports errors through its durf_last_error): no fallback either"""
    if name not in _satellites:
        sigs = _satellite_sigs(name)
        lib()
        path = satellite_path(name)
        if not os.path.exists(path):
            raise RuntimeError('libdurf_%s.so not built (%s).  Run __graft_entry__.build().' % (name, path))
        _satellites[name] = _bind(C.CDLL(path), sigs)
    return _satellites[name]


def __getattr__(attr):
    """<name>_lib(), <name>_symbols() and <NAME>_LIB_PATH of every satellite, as ops.py and the tests spell them"""
    for name in SATELLITES:
        if attr == name + '_lib':
            return functools.partial(satellite, name)
        if attr == name + '_symbols':
            return functools.partial(satellite_symbols, name)
        if attr == name.upper() + '_LIB_PATH':
            return satellite_path(name)
    raise AttributeError('module %r has no attribute %r' % (__name__, attr))


class DurfError(RuntimeError):
    pass


def check(rc, what):
    if rc != 0:
        raise DurfError('%s failed (%d): %s' % (what, rc, lib().durf_last_error().decode()))
