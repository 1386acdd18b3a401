"""Argument types of every entry point of libdurf_smooth.so, and the constants, macros and structs of its header -- GENERATED from
include/durf_smooth.h by tools/gen_integration_stub.py (do not edit; `--check` runs in the CPU test-suite)."""
import ctypes as C

vp, i32, f32, u64 = C.c_void_p, C.c_int, C.c_float, C.c_size_t

SIGS = {
    'durf_smooth_keys': (i32, [vp, i32, i32, vp, vp, vp]),
    'durf_smooth_workspace_bytes': (u64, [i32]),
    'durf_smooth_adjacency': (i32, [vp, i32, i32, vp, vp, i32, vp, u64, vp, vp, vp, vp, vp]),
    'durf_smooth_classify': (i32, [vp, i32, vp, vp, vp]),
    'durf_smooth_census': (i32, [vp, i32, vp, vp, vp, vp, vp, vp]),
    'durf_smooth_step': (i32, [vp, i32, vp, vp, vp, vp, vp, f32, i32, vp, vp]),
    'durf_smooth_taubin': (i32, [vp, i32, vp, vp, vp, vp, vp, i32, f32, f32, i32, vp, vp, vp]),
    'durf_smooth_normals': (i32, [vp, i32, i32, vp, vp, vp, vp, vp]),
}


DURF_SMOOTH_BLOCK = 256
DURF_SMOOTH_MAX_TRIANGLES = 357913942
DURF_SMOOTH_CENSUS_INTS = 8
DURF_SMOOTH_ISOLATED = 0
DURF_SMOOTH_INTERIOR = 1
DURF_SMOOTH_BOUNDARY = 2
DURF_SMOOTH_NONMANIFOLD = 3
DURF_SMOOTH_PIN = 0
DURF_SMOOTH_SLIDE = 1
DURF_SMOOTH_NO_KEY = 0x7fffffffffffffff
