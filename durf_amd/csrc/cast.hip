// The nearest triangle of a mesh along arbitrary rays (include/durf_cast.h; libdurf_cast.so): Morton keys, an implicit complete
// binary tree of boxes over the caller's sorted order built level by level, and a per-ray walk with a short stack in LDS.  The
// header defines the result as a minimum over all triangles and proves that no tree can change it; the kernels follow it.  No
// atomics, nothing synchronises or copies to the host, no workgroup waits for another.
#include <climits>
#include "cast_query.h"

static_assert(DURF_CAST_KEY_BITS == 21, "three axes in 63 bits");

// ---- keys ---------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(CB)
k_cast_keys(int V, int T, const float* __restrict__ vertices, const int32_t* __restrict__ triangles, const float* __restrict__ bounds,
            long long* __restrict__ keys) {
    const int i = blockIdx.x * CB + threadIdx.x;
    if (i >= T) return;
    float P[9];
    if (!tri_fetch(i, V, T, vertices, triangles, P)) {
        keys[i] = LLONG_MAX;
        return;
    }
    unsigned long long key = 0;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const float lo = bounds[a], ext = bounds[3 + a] - lo;
        const float c = ((P[a] + P[3 + a]) + P[6 + a]) / 3.0f;
        const float x = ((c - lo) / ext) * 2097152.0f;
        const unsigned g = (!(ext > 0.0f) || !(x >= 0.0f)) ? 0u : x >= 2097151.0f ? 2097151u : (unsigned)(int)x;
        for (int b = 0; b < DURF_CAST_KEY_BITS; b++) key |= (unsigned long long)(g >> b & 1u) << (3 * b + (2 - a));
    }
    keys[i] = (long long)key;
}

// ---- build --------------------------------------------------------------------------------------------------------------------------
// one thread per leaf: its records and its box
__global__ void __launch_bounds__(CB)
k_cast_leaves(int V, int T, int n0, const float* __restrict__ vertices, const int32_t* __restrict__ triangles,
              const int32_t* __restrict__ order, float* __restrict__ records, float* __restrict__ nodes) {
    const int l = blockIdx.x * CB + threadIdx.x;
    if (l >= n0) return;
    CastBox B = cast_empty_box();
#pragma unroll
    for (int j = 0; j < CLEAF; j++) {
        const size_t s = (size_t)l * CLEAF + j;
        float P[9] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
        int id = s < (size_t)T ? order[s] : -1;
        if (tri_fetch(id, V, T, vertices, triangles, P)) {
            cast_union(B, cast_tri_box(P, P + 3, P + 6));
        } else {
            id = -1;
#pragma unroll
            for (int c = 0; c < 9; c++) P[c] = 0.0f;
        }
        float* r = records + s * CREC;
#pragma unroll
        for (int c = 0; c < 9; c++) r[c] = P[c];
        r[9] = __int_as_float(id);
    }
    cast_store_box(nodes, l, B);
}

// one thread per node of a level: the union of its two children on the level below (a missing sibling is empty)
__global__ void __launch_bounds__(CB)
k_cast_level(int n_below, int off_below, int n_here, int off_here, float* nodes) {
    const int j = blockIdx.x * CB + threadIdx.x;
    if (j >= n_here) return;
    CastBox B = cast_load_box(nodes, off_below + 2 * j);
    if (2 * j + 1 < n_below) cast_union(B, cast_load_box(nodes, off_below + 2 * j + 1));
    cast_store_box(nodes, off_here + j, B);
}

// one workgroup: every level from `first` (whose level below has at most 2 DURF_CAST_TOP nodes) up to the root
__global__ void __launch_bounds__(CB)
k_cast_top(const CastTree R, int first, float* nodes) {
    for (int k = first; k <= R.K; k++) {                                     // (uniform; at most DURF_CAST_STACK levels)
        const int j = threadIdx.x;
        if (j < R.n(k)) {
            CastBox B = cast_load_box(nodes, R.off[k - 1] + 2 * j);
            if (2 * j + 1 < R.n(k - 1)) cast_union(B, cast_load_box(nodes, R.off[k - 1] + 2 * j + 1));
            cast_store_box(nodes, R.off[k] + j, B);
        }
        __threadfence_block();
        __syncthreads();                                                     // the next level reads what this one wrote
    }
}

// ---- the walk -----------------------------------------------------------------------------------------------------------------------
// (the ray, its box and triangle rules, the two queries and the outputs of a hit: cast_query.h)
template <bool ANY>
__global__ void __launch_bounds__(CB)
k_cast_rays(const CastTree R, int n, const float* __restrict__ origins, const float* __restrict__ directions,
            const float* __restrict__ tmin_rays, const float* __restrict__ tmax_rays, float tmin, float tmax, int cull,
            const float* __restrict__ records, const float* __restrict__ nodes, int32_t* __restrict__ tri, float* __restrict__ t,
            float* __restrict__ bary) {
    __shared__ int s_stack[CSTACK * CB];
    __shared__ int s_off[CSTACK];
    cast_offsets_to_lds(R, s_off);
    const int i = blockIdx.x * CB + threadIdx.x;
    if (i >= n) return;                                                      // (no barrier below)
    CastRay r;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        r.o[a] = origins[(size_t)i * 3 + a];
        r.d[a] = directions[(size_t)i * 3 + a];
    }
    r.tmin = tmin_rays ? tmin_rays[i] : tmin;
    r.tmax = tmax_rays ? tmax_rays[i] : tmax;
    const bool usable = cast_ray_setup(r);
    CastHit hit{-1, 0.0f, 0.0f, 0.0f, 0.0f};
    if (usable) hit = cast_walk<ANY>(R, records, nodes, r, cull, s_stack + threadIdx.x, s_off);
    if (ANY) tri[i] = !usable ? -2 : hit.tri >= 0 ? 1 : 0;
    else cast_write(hit, usable, (size_t)i, tri, t, bary);
}

__global__ void __launch_bounds__(CB)
k_cast_cameras(const CastTree R, int F, int h, int w, const float* __restrict__ cams, float tmin, float tmax, int cull,
               const float* __restrict__ records, const float* __restrict__ nodes, int32_t* __restrict__ tri, float* __restrict__ depth,
               float* __restrict__ bary) {
    __shared__ int s_stack[CSTACK * CB];
    __shared__ int s_off[CSTACK];
    cast_offsets_to_lds(R, s_off);
    const unsigned i = blockIdx.x * (unsigned)CB + threadIdx.x;              // F h w < 2^31
    const unsigned hw = (unsigned)h * (unsigned)w;
    if (i >= (unsigned)F * hw) return;
    const int f = i / hw, p = i - (unsigned)f * hw;
    const float* cam = cams + (size_t)f * DURF_CAM_FLOATS;
    CastRay r;
    r.tmin = tmin;
    r.tmax = tmax;
    bool usable = (int)cam[DURF_CAM_H] == h && (int)cam[DURF_CAM_W] == w;    // (a NaN converts to some int: the row is not finite then)
    if (usable) {
        float view[3], radius, nr, fr;
        pinhole_ray(cam, p, tmin, tmax, 0, r.o, r.d, view, &radius, &nr, &fr);
        usable = cast_ray_setup(r);
    }
    CastHit hit{-1, 0.0f, 0.0f, 0.0f, 0.0f};
    if (usable) hit = cast_walk<false>(R, records, nodes, r, cull, s_stack + threadIdx.x, s_off);
    cast_write(hit, usable, (size_t)i, tri, depth, bary);
}

// ---- launchers ----------------------------------------------------------------------------------------------------------------------
namespace {

int check_cast_bounds(const char* who, bool scalar_tmin, bool scalar_tmax, float tmin, float tmax, int cull) {
    if (!(cull >= 0 && cull <= 2)) { durf_set_error("%s: requirement failed: cull in 0 .. 2, cull = %d", who, cull); return -1; }
    if (scalar_tmin && !(tmin >= 0.0f)) { durf_set_error("%s: requirement failed: tmin >= 0, tmin = %g", who, (double)tmin); return -1; }
    if (scalar_tmax && tmax != tmax) { durf_set_error("%s: requirement failed: tmax is a number, tmax = %g", who, (double)tmax); return -1; }
    return 0;
}

template <bool ANY>
int cast_rays(const char* who, void* stream, int n, const float* origins, const float* directions, const float* tmin_rays,
              const float* tmax_rays, float tmin, float tmax, int cull, int T, const void* workspace, size_t workspace_bytes,
              int32_t* tri, float* t, float* bary) {
    if (!(n >= 0)) { durf_set_error("%s: requirement failed: n >= 0, n = %d", who, n); return -1; }
    if (check_cast_t(who, T) != 0) return -1;
    if (check_cast_bounds(who, tmin_rays == nullptr, tmax_rays == nullptr, tmin, tmax, cull) != 0) return -1;
    if (!((origins && directions) || n == 0)) { durf_set_error("%s: requirement failed: origins and directions for n = %d", who, n); return -1; }
    if (!((tri && (ANY || t)) || n == 0)) { durf_set_error("%s: requirement failed: outputs for n = %d", who, n); return -1; }
    const CastTree R = cast_tree(T);
    CastWs ws;
    if (check_cast_ws(who, workspace, workspace_bytes, R, &ws) != 0) return -1;
    if (n == 0) return 0;
    hipLaunchKernelGGL(k_cast_rays<ANY>, dim3(durf_cdiv((size_t)n, CB)), dim3(CB), 0, (hipStream_t)stream, R, n, origins, directions,
                       tmin_rays, tmax_rays, tmin, tmax, cull, ws.records, ws.nodes, tri, t, bary);
    DURF_CHECK_LAUNCH(ANY ? "k_cast_rays<any>" : "k_cast_rays<nearest>");
    return 0;
}

}  // namespace

extern "C" {

size_t durf_cast_workspace_bytes(int T) {
    if (!cast_t_ok(T)) return 0;
    return cast_carve(nullptr, cast_tree(T)).total;
}

int durf_cast_keys(void* stream, int V, int T, const float* vertices, const int32_t* triangles, const float* bounds, int64_t* keys) {
    if (check_cast_mesh(__func__, V, T, vertices, triangles) != 0) return -1;
    if (!((bounds && keys) || T == 0)) { durf_set_error("%s: requirement failed: bounds and keys for T = %d", __func__, T); return -1; }
    if (T == 0) return 0;
    hipLaunchKernelGGL(k_cast_keys, dim3(durf_cdiv((size_t)T, CB)), dim3(CB), 0, (hipStream_t)stream, V, T, vertices, triangles, bounds,
                       (long long*)keys);
    DURF_CHECK_LAUNCH("k_cast_keys");
    return 0;
}

int durf_cast_build(void* stream, int V, int T, const float* vertices, const int32_t* triangles, const int32_t* order, void* workspace,
                    size_t workspace_bytes) {
    if (check_cast_mesh(__func__, V, T, vertices, triangles) != 0) return -1;
    if (!(order || T == 0)) { durf_set_error("%s: requirement failed: order for T = %d", __func__, T); return -1; }
    const CastTree R = cast_tree(T);
    CastWs ws;
    if (check_cast_ws(__func__, workspace, workspace_bytes, R, &ws) != 0) return -1;
    if (T == 0) return 0;
    const hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_cast_leaves, dim3(durf_cdiv((size_t)R.n0, CB)), dim3(CB), 0, s, V, T, R.n0, vertices, triangles, order,
                       ws.records, ws.nodes);
    DURF_CHECK_LAUNCH("k_cast_leaves");
    int k = 1;
    for (; k <= R.K && R.n(k) > DURF_CAST_TOP; k++) {
        hipLaunchKernelGGL(k_cast_level, dim3(durf_cdiv((size_t)R.n(k), CB)), dim3(CB), 0, s, R.n(k - 1), R.off[k - 1], R.n(k), R.off[k],
                           ws.nodes);
        DURF_CHECK_LAUNCH("k_cast_level");
    }
    if (k <= R.K) {
        hipLaunchKernelGGL(k_cast_top, dim3(1), dim3(CB), 0, s, R, k, ws.nodes);
        DURF_CHECK_LAUNCH("k_cast_top");
    }
    return 0;
}

int durf_cast_rays(void* stream, int n, const float* origins, const float* directions, const float* tmin_rays, const float* tmax_rays,
                   float tmin, float tmax, int cull, int T, const void* workspace, size_t workspace_bytes, int32_t* tri, float* t,
                   float* bary) {
    return cast_rays<false>(__func__, stream, n, origins, directions, tmin_rays, tmax_rays, tmin, tmax, cull, T, workspace,
                            workspace_bytes, tri, t, bary);
}

int durf_cast_any(void* stream, int n, const float* origins, const float* directions, const float* tmin_rays, const float* tmax_rays,
                  float tmin, float tmax, int cull, int T, const void* workspace, size_t workspace_bytes, int32_t* hit) {
    return cast_rays<true>(__func__, stream, n, origins, directions, tmin_rays, tmax_rays, tmin, tmax, cull, T, workspace, workspace_bytes,
                           hit, nullptr, nullptr);
}

int durf_cast_cameras(void* stream, int F, int h, int w, const float* cams_dev, float tmin, float tmax, int cull, int T,
                      const void* workspace, size_t workspace_bytes, int32_t* tri, float* depth, float* bary) {
    if (!(F >= 0 && h >= 1 && w >= 1)) {
        durf_set_error("%s: requirement failed: F >= 0, h >= 1, w >= 1, F = %d, h = %d, w = %d", __func__, F, h, w);
        return -1;
    }
    if (!((double)F * h * w < 2147483648.0)) {
        durf_set_error("%s: requirement failed: F h w < 2^31 pixels, F = %d, h = %d, w = %d", __func__, F, h, w);
        return -1;
    }
    if (check_cast_t(__func__, T) != 0) return -1;
    if (check_cast_bounds(__func__, true, true, tmin, tmax, cull) != 0) return -1;
    if (!((cams_dev && tri && depth) || F == 0)) { durf_set_error("%s: requirement failed: cams_dev, tri and depth for F = %d", __func__, F); return -1; }
    const CastTree R = cast_tree(T);
    CastWs ws;
    if (check_cast_ws(__func__, workspace, workspace_bytes, R, &ws) != 0) return -1;
    if (F == 0) return 0;
    hipLaunchKernelGGL(k_cast_cameras, dim3(durf_cdiv((size_t)F * h * w, CB)), dim3(CB), 0, (hipStream_t)stream, R, F, h, w, cams_dev, tmin,
                       tmax, cull, ws.records, ws.nodes, tri, depth, bary);
    DURF_CHECK_LAUNCH("k_cast_cameras");
    return 0;
}

}  // extern "C"
