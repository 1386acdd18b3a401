"""Argument types of every entry point of libdurf_flow.so, and the constants, macros and structs of its header -- GENERATED from
include/durf_flow.h by tools/gen_integration_stub.py (do not edit; `--check` runs in the CPU test-suite)."""
import ctypes as C

vp, i32, f32, u64 = C.c_void_p, C.c_int, C.c_float, C.c_size_t

SIGS = {
    'durf_flow_points': (i32, [vp, i32, i32, i32, vp, vp, vp, vp, vp, C.POINTER(f32), C.POINTER(f32), vp, vp, vp, i32, f32, f32, f32, vp, vp, vp, vp, vp, vp, vp, vp]),
    'durf_flow_warp': (i32, [vp, i32, i32, i32, i32, vp, vp, vp, vp, f32, f32, vp, vp]),
    'durf_flow_consistency': (i32, [vp, i32, i32, i32, vp, vp, vp, vp, vp]),
    'durf_flow_color': (i32, [vp, i32, vp, f32, vp, vp]),
    'durf_render_flow_workspace_bytes': (u64, [i32, i32]),
    'durf_render_flow': (i32, [vp, i32, i32, C.POINTER(f32), vp, vp, vp, vp, vp, i32, C.POINTER(i32), f32, f32, i32, i32, f32, f32, f32, vp, vp, vp, vp, vp, vp, vp, vp, u64]),
}


def DURF_FLOW_POSE_FLOATS(K):
    return (2 * (K) * 12)


DURF_FLOW_CONS_FLOATS = 4
DURF_FLOW_CONS_SPAN = 4096


def DURF_FLOW_CONS_GROUPS(m):
    return (((m) + DURF_FLOW_CONS_SPAN - 1) // DURF_FLOW_CONS_SPAN)


def DURF_FLOW_CONS_SCRATCH(P, m):
    return ((P) * DURF_FLOW_CONS_GROUPS(m) * 3)


DURF_FLOW_WHEEL = 55
