"""Argument types of every entry point of libdurf_lidar.so, and the constants, macros and structs of its header -- GENERATED from
include/durf_lidar.h by tools/gen_integration_stub.py (do not edit; `--check` runs in the CPU test-suite)."""
import ctypes as C

vp, i32, f32, u64 = C.c_void_p, C.c_int, C.c_float, C.c_size_t

SIGS = {
    'durf_lidar_rays': (i32, [vp, C.POINTER(f32), vp, C.POINTER(f32), i32, i32, f32, f32, vp, vp, vp, vp, vp, vp]),
    'durf_lidar_returns': (i32, [vp, i32, i32, vp, vp, vp, vp, vp, C.POINTER(f32), f32, f32, f32, f32, f32, vp, vp, vp, vp, vp]),
    'durf_lidar_compact': (i32, [vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
    'durf_render_lidar_workspace_bytes': (u64, [i32, i32, i32, i32]),
    'durf_render_lidar': (i32, [vp, vp, vp, i32, C.POINTER(f32), vp, C.POINTER(f32), vp, f32, f32, i32, f32, f32, f32, f32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, u64]),
}


DURF_LIDAR_SENSOR_FLOATS = 6
DURF_LIDAR_SWEEP_FLOATS = 18
DURF_LIDAR_COMPACT_BLOCK = 256
DURF_LIDAR_POINT_FLOATS = 8


def DURF_LIDAR_COMPACT_SCRATCH(n):
    return (((n) + DURF_LIDAR_COMPACT_BLOCK - 1) // DURF_LIDAR_COMPACT_BLOCK + 1)
