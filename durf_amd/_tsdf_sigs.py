"""Argument types of every entry point of libdurf_tsdf.so, and the constants, macros and structs of its header -- GENERATED from
include/durf_tsdf.h by tools/gen_integration_stub.py (do not edit; `--check` runs in the CPU test-suite)."""
import ctypes as C

vp, i32, f32, u64 = C.c_void_p, C.c_int, C.c_float, C.c_size_t

SIGS = {
    'durf_tsdf_integrate': (i32, [vp, i32, i32, i32, C.POINTER(f32), C.POINTER(f32), C.POINTER(f32), C.POINTER(f32), i32, i32, i32, vp, vp, vp, f32, vp, vp, i32, i32, vp, vp, f32, f32, f32, vp, vp, vp]),
    'durf_tsdf_lattice': (i32, [vp, i32, i32, i32, vp, vp, vp, f32, vp, vp, vp]),
    'durf_tsdf_sample': (i32, [vp, i32, i32, i32, C.POINTER(f32), C.POINTER(f32), vp, vp, vp, f32, f32, i32, vp, vp, vp, vp]),
}


DURF_TSDF_BLOCK = 256
DURF_TSDF_MAX_POINTS = 134217728          # (1 << 27)
DURF_TSDF_MAX_SIZE = 4096
DURF_TSDF_MAX_COORD = 1048576          # (1 << 20)
