"""Argument types of every entry point of libdurf_shade.so, and the constants, macros and structs of its header -- GENERATED from
include/durf_shade.h by tools/gen_integration_stub.py (do not edit; `--check` runs in the CPU test-suite)."""
import ctypes as C

vp, i32, f32, u64 = C.c_void_p, C.c_int, C.c_float, C.c_size_t

SIGS = {
    'durf_shade_surface': (i32, [vp, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp]),
    'durf_shade_occlusion': (i32, [vp, i32, vp, vp, i32, vp, f32, f32, i32, i32, vp, u64, vp, vp]),
    'durf_shade_compose': (i32, [vp, i32, vp, vp, vp, vp, vp, vp, vp, f32, vp, vp, vp]),
    'durf_shade_workspace_bytes': (u64, [i32, i32, i32]),
    'durf_shade_cameras': (i32, [vp, i32, i32, i32, vp, f32, f32, i32, i32, i32, vp, vp, vp, u64, i32, vp, f32, f32, vp, i32, f32, vp, vp, vp, u64, vp, vp, vp, vp, vp, vp, vp]),
}


DURF_SHADE_MAX_DIRS = 256
