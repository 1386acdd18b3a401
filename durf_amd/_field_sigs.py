"""Argument types of every entry point of libdurf_field.so, and the constants, macros and structs of its header -- GENERATED from
include/durf_field.h by tools/gen_integration_stub.py (do not edit; `--check` runs in the CPU test-suite)."""
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


def DURF_FIELD_POSE_FLOATS(K):
    return ((K) * 12)


DURF_FIELD_ENC_BKGD = 60
DURF_FIELD_ENC_OBJ = 63


class durf_field_args(C.Structure):
    _fields_ = [
        ('K', i32),
        ('enc_flags', i32),
        ('sigma', f32),
        ('inside_tol', f32),
        ('density_bias', f32),
        ('barf_w', f32 * 10),
        ('bkgd_params', vp),
        ('obj_params', vp),
        ('param_stride', u64),
        ('bkgd_wstream', vp),
        ('obj_wstream', vp),
        ('const_trunk', vp),
        ('pose', vp),
        ('ext', vp),
        ('box_enable', vp),
        ('points', vp),
        ('viewdirs', vp),
        ('density', vp),
        ('rgb', vp),
        ('raw', vp),
        ('owner', vp),
        ('valid', vp),
    ]
