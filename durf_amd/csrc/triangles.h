// The triangle mesh every mesh library takes -- vertices [V,3] float32, triangles [T,3] int32 -- defined once for
// raster, geom, cast, closest and shade: which triangle is readable, the fetch of its vertices, the attribute interpolation, the
// three small vector operations with their operation order written out, and the launchers' refusal of a mesh.  The tree is built
// with -ffp-contract=off: each of these is the expression its callers wrote inline, in the same order.  Internal.
#pragma once
#include "durf_common.h"
#include "camera.h"                    // cam_finite

// (x0 y0 + x1 y1) + x2 y2
__device__ __forceinline__ float vec3_dot(const float* x, const float* y) { return (x[0] * y[0] + x[1] * y[1]) + x[2] * y[2]; }

__device__ __forceinline__ void vec3_sub(const float* x, const float* y, float* r) {
#pragma unroll
    for (int a = 0; a < 3; a++) r[a] = x[a] - y[a];
}

__device__ __forceinline__ void vec3_cross(const float* x, const float* y, float* r) {
    r[0] = x[1] * y[2] - x[2] * y[1];
    r[1] = x[2] * y[0] - x[0] * y[2];
    r[2] = x[0] * y[1] - x[1] * y[0];
}

// The readable triangle: t in 0 .. T-1 and its three indices, written to v, in 0 .. V-1.  ID = false for a caller whose t is in
// range by construction: the indices are read either way, so t must be.  v is written only when t is in range.
template <bool ID = true>
__device__ __forceinline__ bool tri_indices(int t, int V, int T, const int32_t* __restrict__ triangles, int* v /* [3] */) {
    if (ID && (t < 0 || t >= T)) return false;
    bool ok = true;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        v[c] = triangles[(size_t)t * 3 + c];
        ok = ok && v[c] >= 0 && v[c] < V;
    }
    return ok;
}

// a readable triangle's vertices; false too for a coordinate that is not finite
__device__ __forceinline__ bool tri_fetch(int t, int V, int T, const float* __restrict__ vertices, const int32_t* __restrict__ triangles,
                                          float* P /* [9] */) {
    int v[3];
    if (!tri_indices(t, V, T, triangles, v)) return false;
    bool ok = true;
#pragma unroll
    for (int c = 0; c < 3; c++)
#pragma unroll
        for (int a = 0; a < 3; a++) {
            P[3 * c + a] = vertices[(size_t)v[c] * 3 + a];
            ok = ok && cam_finite(P[3 * c + a]);
        }
    return ok;
}

// channel c of a per-vertex attribute [V,C] at the weights q of a readable triangle's vertices v: (q0 a0 + q1 a1) + q2 a2
__device__ __forceinline__ float tri_interp(const float* q, const int* v, const float* __restrict__ attr, int C, int c) {
    return (q[0] * attr[(size_t)v[0] * C + c] + q[1] * attr[(size_t)v[1] * C + c]) + q[2] * attr[(size_t)v[2] * C + c];
}

// ---- the launchers' refusal of a mesh: -> 0, or -1 with the refusal set ---------------------------------------------------------------
inline int check_mesh_triangles(const char* who, int T, const int32_t* triangles) {
    if (!(triangles || T == 0)) { durf_set_error("%s: requirement failed: triangles for T = %d", who, T); return -1; }
    return 0;
}

// V, then t_ok -- what the caller checks between, already evaluated: 0, or -1 with its own refusal set (the tree's limit on T; the
// rasteriser's znear, cull and cams) -- then the two arrays.  A refused V is reported first: durf_set_error replaces what t_ok set.
inline int check_mesh(const char* who, int V, int T, int t_ok, const float* vertices, const int32_t* triangles) {
    if (!(V >= 0)) { durf_set_error("%s: requirement failed: V >= 0, V = %d", who, V); return -1; }
    if (t_ok != 0) return -1;
    if (!(vertices || V == 0)) { durf_set_error("%s: requirement failed: vertices for V = %d", who, V); return -1; }
    return check_mesh_triangles(who, T, triangles);
}
