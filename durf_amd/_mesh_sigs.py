"""Argument types of every entry point of libdurf_mesh.so, and the constants, macros and structs of its header -- GENERATED from
include/durf_mesh.h by tools/gen_integration_stub.py (do not edit; `--check` runs in the CPU test-suite)."""
import ctypes as C

vp, i32, f32, u64 = C.c_void_p, C.c_int, C.c_float, C.c_size_t

SIGS = {
    'durf_mesh_workspace_bytes': (u64, [i32, i32, i32]),
    'durf_mesh_count': (i32, [vp, i32, i32, i32, vp, vp, f32, vp, u64, vp]),
    'durf_mesh_emit': (i32, [vp, i32, i32, i32, vp, vp, f32, C.POINTER(f32), C.POINTER(f32), C.POINTER(f32), C.POINTER(f32), C.POINTER(f32), i32, vp, u64, i32, i32, vp, vp, vp, vp, vp]),
    'durf_mesh_gather': (i32, [vp, i32, i32, i32, vp, i32, vp, vp, i32, vp, vp, vp, vp, vp, f32, vp]),
}


DURF_MESH_BLOCK = 256
DURF_MESH_MAX_POINTS = 134217728          # (1 << 27)
