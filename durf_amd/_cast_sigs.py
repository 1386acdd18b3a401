"""Argument types of every entry point of libdurf_cast.so, and the constants, macros and structs of its header -- GENERATED from
include/durf_cast.h by tools/gen_integration_stub.py (do not edit; `--check` runs in the CPU test-suite)."""
import ctypes as C

vp, i32, f32, u64 = C.c_void_p, C.c_int, C.c_float, C.c_size_t

SIGS = {
    'durf_cast_workspace_bytes': (u64, [i32]),
    'durf_cast_keys': (i32, [vp, i32, i32, vp, vp, vp, vp]),
    'durf_cast_build': (i32, [vp, i32, i32, vp, vp, vp, vp, u64]),
    'durf_cast_rays': (i32, [vp, i32, vp, vp, vp, vp, f32, f32, i32, i32, vp, u64, vp, vp, vp]),
    'durf_cast_any': (i32, [vp, i32, vp, vp, vp, vp, f32, f32, i32, i32, vp, u64, vp]),
    'durf_cast_cameras': (i32, [vp, i32, i32, i32, vp, f32, f32, i32, i32, vp, u64, vp, vp, vp]),
}


DURF_CAST_LEAF = 4
DURF_CAST_BLOCK = 256
DURF_CAST_STACK = 32
DURF_CAST_TOP = 256
DURF_CAST_RECORD_FLOATS = 10
DURF_CAST_NODE_FLOATS = 8
DURF_CAST_KEY_BITS = 21
DURF_CAST_MAX_TRIANGLES = 1073741824          # (1 << 30)
