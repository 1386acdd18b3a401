"""ctypes binding of libdurf_hip.so (C ABI in include/durf_hip.h).

The library is the product: there is no CPU or eager-PyTorch fallback.  If the shared
object is missing this module raises at import of any op (run `python -c "import
__graft_entry__ as g; g.build()"` or `make -C durf_amd/csrc`).
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# DURF_LIB_PATH: kernel-tuning A/B builds (tools/build_variant.sh); the default is the in-tree build
LIB_PATH = os.environ.get('DURF_LIB_PATH') or os.path.join(_HERE, 'libdurf_hip.so')

OVERLAY_LIB_PATH = os.path.join(_HERE, 'libdurf_overlay.so')        # the box overlay (include/durf_overlay.h), built beside it
LIDAR_LIB_PATH = os.path.join(_HERE, 'libdurf_lidar.so')            # LIDAR sweeps (include/durf_lidar.h), likewise
FLOW_LIB_PATH = os.path.join(_HERE, 'libdurf_flow.so')              # motion between frames (include/durf_flow.h), likewise
FIELD_LIB_PATH = os.path.join(_HERE, 'libdurf_field.so')            # the field at world points (include/durf_field.h), likewise
MESH_LIB_PATH = os.path.join(_HERE, 'libdurf_mesh.so')              # the iso-surface of a density lattice (include/durf_mesh.h), likewise
GEOM_LIB_PATH = os.path.join(_HERE, 'libdurf_geom.so')              # distances between point sets (include/durf_geom.h), likewise

_lib = None
_overlay = None
_lidar = None
_flow = None
_field = None
_mesh = None
_geom = None

from ._sigs import SIGS as _SIGS       # generated from include/durf_hip.h (tools/gen_integration_stub.py)
from ._overlay_sigs import SIGS as _OVERLAY_SIGS       # generated from include/durf_overlay.h
from ._lidar_sigs import SIGS as _LIDAR_SIGS       # generated from include/durf_lidar.h
from ._flow_sigs import SIGS as _FLOW_SIGS       # generated from include/durf_flow.h
from ._field_sigs import SIGS as _FIELD_SIGS       # generated from include/durf_field.h
from ._mesh_sigs import SIGS as _MESH_SIGS       # generated from include/durf_mesh.h
from ._geom_sigs import SIGS as _GEOM_SIGS       # generated from include/durf_geom.h


def symbols():
    """Every symbol include/durf_hip.h declares (checked by the CPU test-suite)."""
    return sorted(_SIGS)


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
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in _SIGS.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def overlay_symbols():
    """Every symbol include/durf_overlay.h declares."""
    return sorted(_OVERLAY_SIGS)


def overlay_lib():
    """libdurf_overlay.so, after libdurf_hip.so (it reports errors through that library's durf_last_error): no fallback either"""
    global _overlay
    if _overlay is None:
        lib()
        if not os.path.exists(OVERLAY_LIB_PATH):
            raise RuntimeError('libdurf_overlay.so not built (%s).  Run __graft_entry__.build().' % OVERLAY_LIB_PATH)
        L = C.CDLL(OVERLAY_LIB_PATH)
        for name, (res, args) in _OVERLAY_SIGS.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _overlay = L
    return _overlay


def lidar_symbols():
    """Every symbol include/durf_lidar.h declares."""
    return sorted(_LIDAR_SIGS)


def lidar_lib():
    """libdurf_lidar.so, after libdurf_hip.so (it calls that library and reports errors through its durf_last_error): no fallback either"""
    global _lidar
    if _lidar is None:
        lib()
        if not os.path.exists(LIDAR_LIB_PATH):
            raise RuntimeError('libdurf_lidar.so not built (%s).  Run __graft_entry__.build().' % LIDAR_LIB_PATH)
        L = C.CDLL(LIDAR_LIB_PATH)
        for name, (res, args) in _LIDAR_SIGS.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lidar = L
    return _lidar


def flow_symbols():
    """Every symbol include/durf_flow.h declares."""
    return sorted(_FLOW_SIGS)


def flow_lib():
    """libdurf_flow.so, after libdurf_hip.so (it calls that library and reports errors through its durf_last_error): no fallback either"""
    global _flow
    if _flow is None:
        lib()
        if not os.path.exists(FLOW_LIB_PATH):
            raise RuntimeError('libdurf_flow.so not built (%s).  Run __graft_entry__.build().' % FLOW_LIB_PATH)
        L = C.CDLL(FLOW_LIB_PATH)
        for name, (res, args) in _FLOW_SIGS.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _flow = L
    return _flow


def field_symbols():
    """Every symbol include/durf_field.h declares."""
    return sorted(_FIELD_SIGS)


def field_lib():
    """libdurf_field.so, after libdurf_hip.so (it calls that library and reports errors through its durf_last_error): no fallback either"""
    global _field
    if _field is None:
        lib()
        if not os.path.exists(FIELD_LIB_PATH):
            raise RuntimeError('libdurf_field.so not built (%s).  Run __graft_entry__.build().' % FIELD_LIB_PATH)
        L = C.CDLL(FIELD_LIB_PATH)
        for name, (res, args) in _FIELD_SIGS.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _field = L
    return _field


def mesh_symbols():
    """Every symbol include/durf_mesh.h declares."""
    return sorted(_MESH_SIGS)


def mesh_lib():
    """libdurf_mesh.so, after libdurf_hip.so (it reports errors through that library's durf_last_error): no fallback either"""
    global _mesh
    if _mesh is None:
        lib()
        if not os.path.exists(MESH_LIB_PATH):
            raise RuntimeError('libdurf_mesh.so not built (%s).  Run __graft_entry__.build().' % MESH_LIB_PATH)
        L = C.CDLL(MESH_LIB_PATH)
        for name, (res, args) in _MESH_SIGS.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _mesh = L
    return _mesh


def geom_symbols():
    """Every symbol include/durf_geom.h declares."""
    return sorted(_GEOM_SIGS)


def geom_lib():
    """libdurf_geom.so, after libdurf_hip.so (it reports errors through that library's durf_last_error): no fallback either"""
    global _geom
    if _geom is None:
        lib()
        if not os.path.exists(GEOM_LIB_PATH):
            raise RuntimeError('libdurf_geom.so not built (%s).  Run __graft_entry__.build().' % GEOM_LIB_PATH)
        L = C.CDLL(GEOM_LIB_PATH)
        for name, (res, args) in _GEOM_SIGS.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _geom = L
    return _geom


class DurfError(RuntimeError):
    pass


def check(rc, what):
    if rc != 0:
        raise DurfError('%s failed (%d): %s' % (what, rc, lib().durf_last_error().decode()))
