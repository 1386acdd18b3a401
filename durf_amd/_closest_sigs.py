"""Argument types of every entry point of libdurf_closest.so, and the constants, macros and structs of its header -- GENERATED from
include/durf_closest.h by tools/gen_integration_stub.py (do not edit; `--check` runs in the CPU test-suite)."""
import ctypes as C

vp, i32, f32, u64 = C.c_void_p, C.c_int, C.c_float, C.c_size_t

SIGS = {
    'durf_closest_points': (i32, [vp, i32, vp, f32, i32, vp, u64, vp, vp, vp, vp]),
    'durf_closest_grid': (i32, [vp, i32, i32, i32, vp, vp, vp, vp, f32, i32, vp, u64, vp, vp]),
}


DURF_CLOSEST_BLOCK = 256
DURF_CLOSEST_STACK = 32
DURF_CLOSEST_BRICK = 4
