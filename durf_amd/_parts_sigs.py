"""Argument types of every entry point of libdurf_parts.so, and the constants, macros and structs of its header -- GENERATED from
include/durf_parts.h by tools/gen_integration_stub.py (do not edit; `--check` runs in the CPU test-suite)."""
import ctypes as C

vp, i32, f32, u64 = C.c_void_p, C.c_int, C.c_float, C.c_size_t

SIGS = {
    'durf_parts_workspace_bytes': (u64, [i32, i32, i32]),
    'durf_parts_label': (i32, [vp, i32, i32, i32, vp, vp, f32, vp, u64, vp]),
    'durf_parts_number': (i32, [vp, i32, vp, vp, u64, vp, vp]),
    'durf_parts_stats': (i32, [vp, i32, i32, i32, vp, i32, vp, vp]),
    'durf_parts_select_mesh': (i32, [vp, vp, i32, i32, vp, vp, vp, i32, vp, u64, vp, vp, vp, vp]),
}


DURF_PARTS_TILE_I = 4
DURF_PARTS_TILE_J = 4
DURF_PARTS_TILE_K = 16
DURF_PARTS_TILE_POINTS = 256          # (DURF_PARTS_TILE_I * DURF_PARTS_TILE_J * DURF_PARTS_TILE_K)
DURF_PARTS_BLOCK = 256
