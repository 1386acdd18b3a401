// Vertex adjacency, census, Laplacian / Taubin smoothing and vertex normals of a triangle mesh (include/durf_smooth.h;
// libdurf_smooth.so).  The first library that knows which vertices are neighbours: two CSR structures built from keys the caller
// sorted (head flags, scan.h's scan, a scatter of the heads, a binary search per vertex), then gathers over them, one thread per
// vertex.  It writes its outputs and its workspace, nothing else: the only atomics are the census counters' integer adds, nothing
// synchronises or copies to the host, no workgroup waits for another.
#include <cmath>
#include "triangles.h"
#include "scan.h"
#include "workspace.h"
#include "../../include/durf_smooth.h"

#define SB DURF_SMOOTH_BLOCK
#define SMOOTH_WAVES (SB / DURF_WAVE)

static_assert(SB % DURF_WAVE == 0, "whole waves");
static_assert(6ll * (DURF_SMOOTH_MAX_TRIANGLES - 1) < 2147483648ll && 6ll * DURF_SMOOTH_MAX_TRIANGLES >= 2147483648ll, "6 T < 2^31");
static_assert(DURF_SMOOTH_NO_KEY == INT64_MAX, "the sentinel sorts last");
static_assert(DURF_SMOOTH_CENSUS_INTS == 8, "four classes, triangles, edges, boundary and non-manifold edges");

namespace {

__device__ __forceinline__ int64_t smooth_key(int hi, int lo) { return (int64_t)(((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo); }

// ---- keys ---------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(SB)
k_smooth_keys(int V, int T, const int32_t* __restrict__ triangles, int64_t* __restrict__ edge_keys, int64_t* __restrict__ corner_keys) {
    const unsigned t = blockIdx.x * (unsigned)SB + threadIdx.x;              // T < 2^31
    if (t >= (unsigned)T) return;
    int v[3];
    const bool ok = tri_indices<false>((int)t, V, T, triangles, v) && v[0] != v[1] && v[1] != v[2] && v[2] != v[0];
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const int p = v[c], q = v[(c + 1) % 3];
        edge_keys[(size_t)t * 6 + 2 * c] = ok ? smooth_key(p, q) : DURF_SMOOTH_NO_KEY;
        edge_keys[(size_t)t * 6 + 2 * c + 1] = ok ? smooth_key(q, p) : DURF_SMOOTH_NO_KEY;
        corner_keys[(size_t)t * 3 + c] = ok ? smooth_key(p, (int)t) : DURF_SMOOTH_NO_KEY;
    }
}

// ---- the CSR of a sorted key array --------------------------------------------------------------------------------------------------
// key i is a HEAD when it is below the sentinel and differs from key i - 1: the first of a run of equal keys
__device__ __forceinline__ int smooth_head(int i, int n, const int64_t* __restrict__ keys) {
    if (i >= n) return 0;
    const int64_t k = keys[i];
    return k != DURF_SMOOTH_NO_KEY && (i == 0 || keys[i - 1] != k) ? 1 : 0;
}

__global__ void __launch_bounds__(SB)
k_smooth_heads(int n, const int64_t* __restrict__ keys, int32_t* __restrict__ sums) {
    __shared__ int s_w[SMOOTH_WAVES];
    const int i = blockIdx.x * SB + threadIdx.x;                             // n < 2^31, the grid covers n
    scan_wave_to_lds(smooth_head(i, n, keys), s_w);
    __syncthreads();
    if (threadIdx.x == 0) sums[blockIdx.x] = scan_block_sum<SMOOTH_WAVES>(s_w);
}

// starts[r] = the position of head r, for r = 0 .. U-1; starts[U] = the number of keys below the sentinel (where run U-1 ends)
__global__ void __launch_bounds__(SB)
k_smooth_starts(int n, const int64_t* __restrict__ keys, const int32_t* __restrict__ sums, int32_t* __restrict__ starts) {
    __shared__ int s_w[SMOOTH_WAVES];
    const int i = blockIdx.x * SB + threadIdx.x;
    const int c = smooth_head(i, n, keys);
    const int inc = scan_wave_to_lds(c, s_w);
    __syncthreads();
    if (i >= n) return;
    const int before = scan_before_wave<SMOOTH_WAVES>(sums[blockIdx.x], s_w) + (inc - c);     // heads before i: <= i
    if (c) starts[before] = i;
    const bool sentinel = keys[i] == DURF_SMOOTH_NO_KEY;
    if (sentinel && (i == 0 || keys[i - 1] != DURF_SMOOTH_NO_KEY)) starts[before] = i;      // the first sentinel: U == before
    if (!sentinel && i == n - 1) starts[before + c] = n;                      // no sentinel at all: U == before + c <= n
}

// the unique keys' low words and multiplicities, for r < U (U: the scan's total, read from the device)
__global__ void __launch_bounds__(SB)
k_smooth_unique(int n, const int64_t* __restrict__ keys, const int32_t* __restrict__ starts, const int32_t* __restrict__ total,
                int32_t* __restrict__ low, int32_t* __restrict__ mult) {
    const int r = blockIdx.x * SB + threadIdx.x;
    const int U = min(total[0], n);                                          // (== total[0]; a bound the loop below can rely on)
    if (r >= U) return;
    const int a = starts[r], b = starts[r + 1];
    if (a < 0 || a >= n) return;                                             // (keys that are not sorted: the header's last rule)
    low[r] = (int32_t)(uint32_t)(uint64_t)keys[a];
    if (mult) mult[r] = b - a;
}

// offsets[v], v = 0 .. V: the first r in 0 .. U whose unique key is >= (v << 32); 32 halvings cover U < 2^31
__global__ void __launch_bounds__(SB)
k_smooth_offsets(int V, int n, const int64_t* __restrict__ keys, const int32_t* __restrict__ starts, const int32_t* __restrict__ total,
                 int32_t* __restrict__ offsets) {
    const unsigned v = blockIdx.x * (unsigned)SB + threadIdx.x;
    if (v > (unsigned)V) return;
    const int U = min(total[0], n);
    const int64_t want = (int64_t)((uint64_t)v << 32);
    int lo = 0, hi = U;                                                      // the answer lies in [lo, hi]
    for (int it = 0; it < 32; it++) {
        if (lo >= hi) break;
        const int mid = lo + (hi - lo) / 2;
        const int a = starts[mid];
        const bool less = a >= 0 && a < n && keys[a] < want;
        if (less) lo = mid + 1; else hi = mid;
    }
    offsets[v] = lo;
}

// ---- vertex class -------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int smooth_class_of(int o0, int o1, const int32_t* __restrict__ multiplicity) {
    if (o1 <= o0) return DURF_SMOOTH_ISOLATED;
    bool open = false, many = false;
    for (int k = o0; k < o1; k++) {
        const int m = multiplicity[k];
        open = open || m == 1;
        many = many || m > 2;
    }
    return many ? DURF_SMOOTH_NONMANIFOLD : open ? DURF_SMOOTH_BOUNDARY : DURF_SMOOTH_INTERIOR;
}

__global__ void __launch_bounds__(SB)
k_smooth_classify(int V, const int32_t* __restrict__ offsets, const int32_t* __restrict__ multiplicity, uint8_t* __restrict__ vertex_class) {
    const unsigned i = blockIdx.x * (unsigned)SB + threadIdx.x;
    if (i >= (unsigned)V) return;
    vertex_class[i] = (uint8_t)smooth_class_of(offsets[i], offsets[i + 1], multiplicity);
}

// ---- census -------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int wave_sum_int(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__global__ void __launch_bounds__(SB)
k_smooth_census(int V, const int32_t* __restrict__ offsets, const int32_t* __restrict__ neighbours, const int32_t* __restrict__ multiplicity,
                const int32_t* __restrict__ corner_offsets, const uint8_t* __restrict__ vertex_class, int32_t* __restrict__ census) {
    const unsigned i = blockIdx.x * (unsigned)SB + threadIdx.x;
    int c[6] = {0, 0, 0, 0, 0, 0};                                            // the four classes, boundary edges, non-manifold edges
    if (i < (unsigned)V) {
        const int cls = vertex_class[i];
        if (cls >= 0 && cls < 4) c[cls] = 1;
        const int o0 = offsets[i], o1 = offsets[i + 1];
        for (int k = o0; k < o1; k++) {
            if (neighbours[k] > (int)i) {                                     // the undirected edge, once
                const int m = multiplicity[k];
                c[4] += m == 1 ? 1 : 0;
                c[5] += m > 2 ? 1 : 0;
            }
        }
    }
    const int lane = threadIdx.x & (DURF_WAVE - 1);
#pragma unroll
    for (int k = 0; k < 6; k++) {
        const int s = wave_sum_int(c[k]);
        if (lane == 0 && s != 0) atomicAdd(&census[k < 4 ? k : k + 2], s);
    }
    if (i == 0) {
        atomicAdd(&census[4], corner_offsets[V] / 3);
        atomicAdd(&census[5], offsets[V] / 2);
    }
}

// ---- one step -----------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(SB)
k_smooth_step(int V, const float* __restrict__ in, const int32_t* __restrict__ offsets, const int32_t* __restrict__ neighbours,
              const int32_t* __restrict__ multiplicity, const uint8_t* __restrict__ vertex_class, float factor, int boundary,
              const uint8_t* __restrict__ fixed, float* __restrict__ out) {
    const unsigned i = blockIdx.x * (unsigned)SB + threadIdx.x;
    if (i >= (unsigned)V) return;
    const uint32_t* in_bits = (const uint32_t*)in;
    uint32_t* out_bits = (uint32_t*)out;
    uint32_t xb[3];
    float x[3];
    bool finite = true;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        xb[a] = in_bits[(size_t)i * 3 + a];
        x[a] = __uint_as_float(xb[a]);
        finite = finite && cam_finite(x[a]);
    }
    const int cls = vertex_class[i];
    const bool interior = cls == DURF_SMOOTH_INTERIOR, slide = cls == DURF_SMOOTH_BOUNDARY && boundary == DURF_SMOOTH_SLIDE;
    const bool moves = finite && (interior || slide) && !(fixed && fixed[i] != 0);
    float s[3] = {0.0f, 0.0f, 0.0f};
    int n = 0;
    if (moves) {
        const int o0 = offsets[i], o1 = offsets[i + 1];                       // the row, read before its loop
        for (int k = o0; k < o1; k++) {
            const int j = neighbours[k];
            if (!(interior || multiplicity[k] == 1)) continue;
            float y[3];
            bool ok = true;
#pragma unroll
            for (int a = 0; a < 3; a++) {
                y[a] = in[(size_t)j * 3 + a];
                ok = ok && cam_finite(y[a]);
            }
            if (!ok) continue;
#pragma unroll
            for (int a = 0; a < 3; a++) s[a] = n == 0 ? y[a] : s[a] + y[a];
            n++;
        }
    }
    if (n == 0) {                                                            // PINNED: the bits as they are
#pragma unroll
        for (int a = 0; a < 3; a++) out_bits[(size_t)i * 3 + a] = xb[a];
        return;
    }
    const float fn = (float)n;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const float m = s[a] / fn;
        out[(size_t)i * 3 + a] = x[a] + factor * (m - x[a]);
    }
}

__global__ void __launch_bounds__(SB)
k_smooth_copy(size_t n, const uint32_t* __restrict__ in, uint32_t* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * SB + threadIdx.x;
    if (i < n) out[i] = in[i];
}

// ---- normals ------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(SB)
k_smooth_normals(int V, int T, const float* __restrict__ vertices, const int32_t* __restrict__ triangles, const int32_t* __restrict__ corner_offsets,
                 const int32_t* __restrict__ corner_tri, float* __restrict__ normals) {
    const unsigned i = blockIdx.x * (unsigned)SB + threadIdx.x;
    if (i >= (unsigned)V) return;
    const int o0 = corner_offsets[i], o1 = corner_offsets[i + 1];             // the row, read before its loop
    float S[3] = {0.0f, 0.0f, 0.0f};
    int n = 0;
    for (int k = o0; k < o1; k++) {
        float P[9], e1[3], e2[3], N[3];
        if (!tri_fetch(corner_tri[k], V, T, vertices, triangles, P)) continue;
        vec3_sub(P + 3, P, e1);
        vec3_sub(P + 6, P, e2);
        vec3_cross(e1, e2, N);
#pragma unroll
        for (int a = 0; a < 3; a++) S[a] = n == 0 ? N[a] : S[a] + N[a];
        n++;
    }
    const float len2 = vec3_dot(S, S);
    const bool flat = n == 0 || !(len2 > 0.0f) || !cam_finite(len2);
    const float inv = flat ? 0.0f : 1.0f / sqrtf(len2);
#pragma unroll
    for (int a = 0; a < 3; a++) normals[(size_t)i * 3 + a] = flat ? 0.0f : S[a] * inv;
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------
bool smooth_t_ok(int T) { return T >= 0 && T < DURF_SMOOTH_MAX_TRIANGLES; }

int check_smooth_t(const char* who, int T) {
    if (smooth_t_ok(T)) return 0;
    durf_set_error("%s: requirement failed: T in 0 .. DURF_SMOOTH_MAX_TRIANGLES - 1 = %d, T = %d", who, DURF_SMOOTH_MAX_TRIANGLES - 1, T);
    return -1;
}

int check_smooth_sizes(const char* who, int V, int T) {
    if (!(V >= 0)) { durf_set_error("%s: requirement failed: V >= 0, V = %d", who, V); return -1; }
    return check_smooth_t(who, T);
}

int check_smooth_factor(const char* who, const char* name, float f) {
    if (!(std::isfinite(f) && f >= -1.0f && f <= 1.0f)) {
        durf_set_error("%s: requirement failed: %s finite and in [-1, 1], %s = %g", who, name, name, (double)f);
        return -1;
    }
    return 0;
}

// what the CSR build keeps between its launches, for n keys: the block sums and their total, the heads' positions
struct SmoothWs {
    int32_t *sums, *total, *starts;
    int nb;
    size_t bytes;
};

SmoothWs carve_smooth(void* base, size_t n) {
    durf::Carver c{(char*)base, 0};
    SmoothWs w{};
    w.nb = (int)durf_cdiv(n, SB);
    w.sums = (int32_t*)c.take(((size_t)w.nb + 1) * 4);
    w.total = (int32_t*)c.take(4);
    w.starts = (int32_t*)c.take((n + 1) * 4);
    w.bytes = c.total() > 256 ? c.total() : 256;
    return w;
}

// the one CSR routine: n sorted keys -> offsets [V+1], low [<= n], mult [<= n] (nullable)
int smooth_csr(hipStream_t s, int V, int n, const int64_t* keys, void* workspace, int32_t* offsets, int32_t* low, int32_t* mult) {
    const SmoothWs w = carve_smooth(workspace, (size_t)n);
    hipLaunchKernelGGL(k_smooth_heads, dim3(w.nb), dim3(SB), 0, s, n, keys, w.sums);
    DURF_CHECK_LAUNCH("k_smooth_heads");
    hipLaunchKernelGGL((k_scan_block_sums<int32_t, 1>), dim3(1), dim3(SCAN_THREADS), 0, s, w.nb, w.sums, w.total);
    DURF_CHECK_LAUNCH("k_scan_block_sums<int32_t, 1>");
    hipLaunchKernelGGL(k_smooth_starts, dim3(w.nb), dim3(SB), 0, s, n, keys, w.sums, w.starts);
    DURF_CHECK_LAUNCH("k_smooth_starts");
    hipLaunchKernelGGL(k_smooth_unique, dim3(w.nb), dim3(SB), 0, s, n, keys, w.starts, w.total, low, mult);
    DURF_CHECK_LAUNCH("k_smooth_unique");
    hipLaunchKernelGGL(k_smooth_offsets, dim3(durf_cdiv((size_t)V + 1, SB)), dim3(SB), 0, s, V, n, keys, w.starts, w.total, offsets);
    DURF_CHECK_LAUNCH("k_smooth_offsets");
    return 0;
}

int check_smooth_rows(const char* who, int V, const float* in, const int32_t* offsets, const uint8_t* vertex_class, int boundary, const float* out) {
    if (!(boundary == DURF_SMOOTH_PIN || boundary == DURF_SMOOTH_SLIDE)) {
        durf_set_error("%s: requirement failed: boundary in 0 .. 1 (DURF_SMOOTH_PIN, DURF_SMOOTH_SLIDE), boundary = %d", who, boundary);
        return -1;
    }
    if (in == out && in != nullptr) { durf_set_error("%s: requirement failed: in != out (a step reads its neighbours' old positions)", who); return -1; }
    if (!offsets) { durf_set_error("%s: requirement failed: offsets [V+1]", who); return -1; }
    if (!((in && out && vertex_class) || V == 0)) { durf_set_error("%s: requirement failed: in, out and vertex_class for V = %d", who, V); return -1; }
    return 0;
}

void launch_step(hipStream_t s, int V, const float* in, const int32_t* offsets, const int32_t* neighbours, const int32_t* multiplicity,
                 const uint8_t* vertex_class, float factor, int boundary, const uint8_t* fixed, float* out) {
    hipLaunchKernelGGL(k_smooth_step, dim3(durf_cdiv((size_t)V, SB)), dim3(SB), 0, s, V, in, offsets, neighbours, multiplicity, vertex_class, factor,
                       boundary, fixed, out);
}

}  // namespace

extern "C" {

int durf_smooth_keys(void* stream, int V, int T, const int32_t* triangles, int64_t* edge_keys, int64_t* corner_keys) {
    if (check_smooth_sizes(__func__, V, T) != 0) return -1;
    if (check_mesh_triangles(__func__, T, triangles) != 0) return -1;
    if (!((edge_keys && corner_keys) || T == 0)) { durf_set_error("%s: requirement failed: edge_keys and corner_keys for T = %d", __func__, T); return -1; }
    if (T == 0) return 0;
    hipLaunchKernelGGL(k_smooth_keys, dim3(durf_cdiv((size_t)T, SB)), dim3(SB), 0, (hipStream_t)stream, V, T, triangles, edge_keys, corner_keys);
    DURF_CHECK_LAUNCH("k_smooth_keys");
    return 0;
}

size_t durf_smooth_workspace_bytes(int T) {
    if (!smooth_t_ok(T)) return 0;
    return carve_smooth(nullptr, (size_t)T * 6).bytes;
}

int durf_smooth_adjacency(void* stream, int V, int T, const int64_t* edge_keys, const int64_t* corner_keys, int cap, void* workspace,
                          size_t workspace_bytes, int32_t* offsets, int32_t* neighbours, int32_t* multiplicity, int32_t* corner_offsets,
                          int32_t* corner_tri) {
    if (check_smooth_sizes(__func__, V, T) != 0) return -1;
    if (!((long long)cap >= 6ll * T)) { durf_set_error("%s: requirement failed: cap >= 6 T, cap = %d, T = %d", __func__, cap, T); return -1; }
    if (!((edge_keys && corner_keys && corner_tri) || T == 0)) {
        durf_set_error("%s: requirement failed: edge_keys, corner_keys and corner_tri for T = %d", __func__, T);
        return -1;
    }
    if (!((neighbours && multiplicity) || T == 0)) { durf_set_error("%s: requirement failed: neighbours and multiplicity for T = %d", __func__, T); return -1; }
    if (!(offsets && corner_offsets)) { durf_set_error("%s: requirement failed: offsets and corner_offsets [V+1]", __func__); return -1; }
    if (durf::check_workspace_aligned(__func__, workspace) != 0) return -1;
    if (durf::check_workspace(__func__, workspace_bytes, carve_smooth(nullptr, (size_t)T * 6).bytes, "durf_smooth_workspace_bytes(%d)", T) != 0) return -1;
    const hipStream_t s = (hipStream_t)stream;
    if (T == 0) {
        if (hipMemsetAsync(offsets, 0, ((size_t)V + 1) * 4, s) != hipSuccess || hipMemsetAsync(corner_offsets, 0, ((size_t)V + 1) * 4, s) != hipSuccess) {
            durf_set_error("%s: hipMemsetAsync of the offsets failed", __func__);
            return -1;
        }
        return 0;
    }
    int rc = smooth_csr(s, V, 6 * T, edge_keys, workspace, offsets, neighbours, multiplicity);
    if (rc != 0) return rc;
    return smooth_csr(s, V, 3 * T, corner_keys, workspace, corner_offsets, corner_tri, nullptr);
}

int durf_smooth_classify(void* stream, int V, const int32_t* offsets, const int32_t* multiplicity, uint8_t* vertex_class) {
    if (!(V >= 0)) { durf_set_error("%s: requirement failed: V >= 0, V = %d", __func__, V); return -1; }
    if (!offsets) { durf_set_error("%s: requirement failed: offsets [V+1]", __func__); return -1; }
    if (!(vertex_class || V == 0)) { durf_set_error("%s: requirement failed: vertex_class for V = %d", __func__, V); return -1; }
    if (V == 0) return 0;
    hipLaunchKernelGGL(k_smooth_classify, dim3(durf_cdiv((size_t)V, SB)), dim3(SB), 0, (hipStream_t)stream, V, offsets, multiplicity, vertex_class);
    DURF_CHECK_LAUNCH("k_smooth_classify");
    return 0;
}

int durf_smooth_census(void* stream, int V, const int32_t* offsets, const int32_t* neighbours, const int32_t* multiplicity,
                       const int32_t* corner_offsets, const uint8_t* vertex_class, int32_t* census) {
    if (!(V >= 0)) { durf_set_error("%s: requirement failed: V >= 0, V = %d", __func__, V); return -1; }
    if (!(offsets && corner_offsets && census)) { durf_set_error("%s: requirement failed: offsets, corner_offsets and census", __func__); return -1; }
    if (!(vertex_class || V == 0)) { durf_set_error("%s: requirement failed: vertex_class for V = %d", __func__, V); return -1; }
    const hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(census, 0, DURF_SMOOTH_CENSUS_INTS * 4, s) != hipSuccess) { durf_set_error("%s: hipMemsetAsync of the census failed", __func__); return -1; }
    hipLaunchKernelGGL(k_smooth_census, dim3(V > 0 ? durf_cdiv((size_t)V, SB) : 1), dim3(SB), 0, s, V, offsets, neighbours, multiplicity, corner_offsets,
                       vertex_class, census);
    DURF_CHECK_LAUNCH("k_smooth_census");
    return 0;
}

int durf_smooth_step(void* stream, int V, const float* in, const int32_t* offsets, const int32_t* neighbours, const int32_t* multiplicity,
                     const uint8_t* vertex_class, float factor, int boundary, const uint8_t* fixed, float* out) {
    if (!(V >= 0)) { durf_set_error("%s: requirement failed: V >= 0, V = %d", __func__, V); return -1; }
    if (check_smooth_factor(__func__, "factor", factor) != 0) return -1;
    if (check_smooth_rows(__func__, V, in, offsets, vertex_class, boundary, out) != 0) return -1;
    if (V == 0) return 0;
    launch_step((hipStream_t)stream, V, in, offsets, neighbours, multiplicity, vertex_class, factor, boundary, fixed, out);
    DURF_CHECK_LAUNCH("k_smooth_step");
    return 0;
}

int durf_smooth_taubin(void* stream, int V, const float* in, const int32_t* offsets, const int32_t* neighbours, const int32_t* multiplicity,
                       const uint8_t* vertex_class, int iters, float lambda, float mu, int boundary, const uint8_t* fixed, float* tmp, float* out) {
    if (!(V >= 0)) { durf_set_error("%s: requirement failed: V >= 0, V = %d", __func__, V); return -1; }
    if (!(iters >= 0 && iters < (1 << 30))) { durf_set_error("%s: requirement failed: iters in 0 .. 2^30 - 1, iters = %d", __func__, iters); return -1; }
    if (check_smooth_factor(__func__, "lambda", lambda) != 0 || check_smooth_factor(__func__, "mu", mu) != 0) return -1;
    if (check_smooth_rows(__func__, V, in, offsets, vertex_class, boundary, out) != 0) return -1;
    const int steps = mu == 0.0f ? iters : 2 * iters;
    if (steps >= 2 && V > 0 && !(tmp && tmp != in && tmp != out)) {
        durf_set_error("%s: requirement failed: tmp [V,3] that is neither in nor out, for %d steps", __func__, steps);
        return -1;
    }
    if (V == 0) return 0;
    const hipStream_t s = (hipStream_t)stream;
    if (steps == 0) {
        const size_t n = (size_t)V * 3;
        hipLaunchKernelGGL(k_smooth_copy, dim3(durf_cdiv(n, SB)), dim3(SB), 0, s, n, (const uint32_t*)in, (uint32_t*)out);
        DURF_CHECK_LAUNCH("k_smooth_copy");
        return 0;
    }
    const float* src = in;
    for (int k = 0; k < steps; k++) {
        float* dst = (steps - 1 - k) % 2 == 0 ? out : tmp;                   // the last step writes out
        const float factor = mu == 0.0f || k % 2 == 0 ? lambda : mu;
        launch_step(s, V, src, offsets, neighbours, multiplicity, vertex_class, factor, boundary, fixed, dst);
        DURF_CHECK_LAUNCH("k_smooth_step");
        src = dst;
    }
    return 0;
}

int durf_smooth_normals(void* stream, int V, int T, const float* vertices, const int32_t* triangles, const int32_t* corner_offsets,
                        const int32_t* corner_tri, float* normals) {
    if (check_mesh(__func__, V, T, check_smooth_t(__func__, T), vertices, triangles) != 0) return -1;
    if (!(corner_tri || T == 0)) { durf_set_error("%s: requirement failed: corner_tri for T = %d", __func__, T); return -1; }
    if (!corner_offsets) { durf_set_error("%s: requirement failed: corner_offsets [V+1]", __func__); return -1; }
    if (!(normals || V == 0)) { durf_set_error("%s: requirement failed: normals for V = %d", __func__, V); return -1; }
    if (V == 0) return 0;
    hipLaunchKernelGGL(k_smooth_normals, dim3(durf_cdiv((size_t)V, SB)), dim3(SB), 0, (hipStream_t)stream, V, T, vertices, triangles, corner_offsets,
                       corner_tri, normals);
    DURF_CHECK_LAUNCH("k_smooth_normals");
    return 0;
}

}  // extern "C"
