"""Argument types of every entry point of libdurf_raster.so, and the constants, macros and structs of its header -- GENERATED from
include/durf_raster.h by tools/gen_integration_stub.py (do not edit; `--check` runs in the CPU test-suite)."""
import ctypes as C

vp, i32, f32, u64 = C.c_void_p, C.c_int, C.c_float, C.c_size_t

SIGS = {
    'durf_raster_workspace_bytes': (u64, [i32, i32, i32, i32]),
    'durf_raster_setup': (i32, [vp, i32, i32, i32, vp, i32, i32, vp, vp, f32, i32, vp, u64, vp]),
    'durf_raster_draw': (i32, [vp, i32, i32, i32, i32, vp, u64, vp, i32, vp, vp, vp]),
    'durf_raster_interp': (i32, [vp, i32, i32, i32, vp, vp, vp, i32, vp, vp, vp, i32, vp]),
    'durf_render_mesh': (i32, [vp, i32, i32, i32, vp, i32, i32, vp, vp, f32, i32, vp, u64, vp, i32, vp, vp, vp, vp, i32, vp, vp, vp, i32, vp]),
}


DURF_RASTER_SUBPIXEL = 256
DURF_RASTER_MAX_COORD = 536870912          # (1 << 29)
DURF_RASTER_TILE = 16
DURF_RASTER_BATCH = 256
DURF_RASTER_BLOCK = 256
DURF_RASTER_MAX_SIZE = 4096
DURF_RASTER_RECORD_INTS = 10
DURF_RASTER_COUNTS = 8
