"""Argument types of every entry point of libdurf_overlay.so, and the constants, macros and structs of its header -- GENERATED from
include/durf_overlay.h by tools/gen_integration_stub.py (do not edit; `--check` runs in the CPU test-suite)."""
import ctypes as C

vp, i32, f32, u64 = C.c_void_p, C.c_int, C.c_float, C.c_size_t

SIGS = {
    'durf_project_boxes': (i32, [vp, i32, i32, vp, vp, vp, vp, f32, vp, vp]),
    'durf_draw_boxes': (i32, [vp, i32, i32, i32, i32, vp, vp, f32, f32, vp, vp, vp]),
}


DURF_BOX_EDGES = 12
DURF_BOX_RECT_FLOATS = 6
