"""Argument types of every entry point of libdurf_field.so -- GENERATED from include/durf_field.h by
tools/gen_integration_stub.py (do not edit; `--check` runs in the CPU test-suite)."""
import ctypes as C

vp, i32, f32, u64 = C.c_void_p, C.c_int, C.c_float, C.c_size_t

SIGS = {
    'durf_field_classify': (i32, [vp, i32, vp, i32, vp, vp, vp, f32, vp, vp, vp]),
    'durf_field_lists': (i32, [vp, i32, i32, vp, vp, vp]),
    'durf_field_owned': (i32, [vp, i32, i32, vp, vp, vp, vp]),
    'durf_field_encode': (i32, [vp, i32, i32, vp, vp, vp, f32, i32, C.POINTER(f32), vp, vp]),
    'durf_field_activate': (i32, [vp, i32, i32, vp, vp, vp, vp, vp, vp, f32, vp, vp, vp, vp]),
    'durf_field_workspace_bytes': (u64, [i32, i32]),
    'durf_field_query': (i32, [vp, vp, i32, i32, vp, u64]),
    'durf_field_grid': (i32, [vp, vp, C.POINTER(f32), C.POINTER(f32), C.POINTER(f32), C.POINTER(f32), i32, i32, i32, i32, f32, f32, f32, i32, vp, u64, vp]),
    'durf_field_columns': (i32, [vp, i32, i32, i32, vp, vp, f32, f32, vp, vp, vp]),
}
