"""Argument types of every entry point of libdurf_geom.so, and the constants, macros and structs of its header -- GENERATED from
include/durf_geom.h by tools/gen_integration_stub.py (do not edit; `--check` runs in the CPU test-suite)."""
import ctypes as C

vp, i32, f32, u64 = C.c_void_p, C.c_int, C.c_float, C.c_size_t

SIGS = {
    'durf_geom_workspace_bytes': (u64, [i32, i32]),
    'durf_geom_keys': (i32, [vp, i32, vp, C.POINTER(f32), f32, i32, i32, i32, vp]),
    'durf_geom_nearest': (i32, [vp, i32, vp, i32, vp, vp, vp, C.POINTER(f32), f32, i32, i32, i32, f32, vp, vp]),
    'durf_geom_stats': (i32, [vp, i32, vp, vp, i32, C.POINTER(f32), vp, u64, vp]),
    'durf_geom_sample_mesh': (i32, [vp, i32, vp, i32, vp, i32, vp, u64, vp, vp, vp]),
}


DURF_GEOM_BLOCK = 256
DURF_GEOM_STAT_CHUNK = 1024
DURF_GEOM_MAX_CELLS = 2048
DURF_GEOM_MAX_THRESHOLDS = 8
DURF_GEOM_STAT_DOUBLES = 13
