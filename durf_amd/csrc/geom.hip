// Distances between unordered point sets (include/durf_geom.h; libdurf_geom.so): cell keys (k_geom_keys), the nearest point
// within a radius over a cell-sorted reference set (k_geom_nearest: nine binary-searched key ranges per query, no cell table),
// the two-level float64 statistics of the distances (k_geom_stats_partial, k_geom_stats_final) and area-uniform mesh samples
// (k_geom_areas, k_scan_block_sums, k_geom_offsets -- the three plain passes of scan.h, in float64 -- and k_geom_sample).
// One thread per point, plain fp32 in the order the header states; no atomics, nothing synchronises or copies to the host.
#include <cmath>
#include "workspace.h"
#include "scan.h"
#include "triangles.h"
#include "../../include/durf_geom.h"

#define GEOM_B DURF_GEOM_BLOCK
#define GEOM_WAVES (GEOM_B / DURF_WAVE)
#define GEOM_NS DURF_GEOM_STAT_DOUBLES

struct GeomGrid {
    float o[3], inv_cell;
    int n[3];
};

// the cell coordinate of x on axis a as a float (floorf of the header's t); NaN stays NaN
__device__ __forceinline__ float geom_cell(const GeomGrid& G, int a, float x) { return floorf((x - G.o[a]) * G.inv_cell); }

// ---- cell keys -----------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(GEOM_B)
k_geom_keys(int n, const float* __restrict__ points, const GeomGrid G, int64_t* __restrict__ keys) {
    const int i = blockIdx.x * GEOM_B + threadIdx.x;
    if (i >= n) return;
    float c[3];
    bool in = true;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        c[a] = geom_cell(G, a, points[(size_t)i * 3 + a]);
        in = in && c[a] >= 0.0f && c[a] < (float)G.n[a];                    // (false for NaN and the infinities)
    }
    keys[i] = in ? ((int64_t)(int)c[0] * G.n[1] + (int)c[1]) * G.n[2] + (int)c[2] : (int64_t)-1;
}

// ---- nearest point within max_dist --------------------------------------------------------------------------------------------
// the first position in keys [0, m) whose key is >= k
__device__ __forceinline__ int geom_lower_bound(const int64_t* __restrict__ keys, int lo, int m, int64_t k) {
    int hi = m;
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        if (keys[mid] < k) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__global__ void __launch_bounds__(GEOM_B)
k_geom_nearest(int q, const float* __restrict__ query, int m, const float* __restrict__ ref, const int64_t* __restrict__ keys,
               const int32_t* __restrict__ ref_index, const GeomGrid G, float max_dist, float md2, float* __restrict__ dist,
               int32_t* __restrict__ index) {
    const int i = blockIdx.x * GEOM_B + threadIdx.x;
    if (i >= q) return;
    const float qx = query[(size_t)i * 3], qy = query[(size_t)i * 3 + 1], qz = query[(size_t)i * 3 + 2];
    const float fx = geom_cell(G, 0, qx), fy = geom_cell(G, 1, qy), fz = geom_cell(G, 2, qz);
    const bool usable = fx >= -1.0f && fx <= (float)G.n[0] && fy >= -1.0f && fy <= (float)G.n[1] && fz >= -1.0f && fz <= (float)G.n[2] &&
                        fabsf(qx) <= 3.0e38f && fabsf(qy) <= 3.0e38f && fabsf(qz) <= 3.0e38f;
    if (!usable) {
        dist[i] = nanf("");
        index[i] = -2;
        return;
    }
    const int cx = (int)fx, cy = (int)fy, cz = (int)fz;
    const int zlo = max(cz - 1, 0), zhi = min(cz + 1, G.n[2] - 1);           // (cz in [-1, nz]: zlo <= zhi)
    float best = 0.0f;
    int who = -1;
    for (int a = -1; a <= 1; a++) {
        const int X = cx + a;
        if (X < 0 || X >= G.n[0]) continue;
        for (int b = -1; b <= 1; b++) {
            const int Y = cy + b;
            if (Y < 0 || Y >= G.n[1]) continue;
            const int64_t base = ((int64_t)X * G.n[1] + Y) * G.n[2];
            const int lo = geom_lower_bound(keys, 0, m, base + zlo);
            const int hi = geom_lower_bound(keys, lo, m, base + zhi + 1);
            for (int j = lo; j < hi; j++) {                                  // (lo <= hi <= m)
                const float dx = qx - ref[(size_t)j * 3], dy = qy - ref[(size_t)j * 3 + 1], dz = qz - ref[(size_t)j * 3 + 2];
                const float d2 = (dx * dx + dy * dy) + dz * dz;
                if (!(d2 <= md2)) continue;
                const int id = ref_index[j];
                if (who < 0 || d2 < best || (d2 == best && id < who)) { best = d2; who = id; }
            }
        }
    }
    dist[i] = who >= 0 ? sqrtf(best) : max_dist;
    index[i] = who >= 0 ? who : -1;
}

// ---- statistics -----------------------------------------------------------------------------------------------------------------
struct GeomThresholds {
    float t[DURF_GEOM_MAX_THRESHOLDS];
    int n;
};

// the workgroup's 256 rows of GEOM_NS values folded pairwise, stride 128, 64, ... 1; thread 0 writes the result
__device__ __forceinline__ void geom_fold(double* acc, double (*s)[GEOM_B], double* __restrict__ out) {
    const int t = threadIdx.x;
#pragma unroll
    for (int k = 0; k < GEOM_NS; k++) s[k][t] = acc[k];
    __syncthreads();
    for (int stride = GEOM_B / 2; stride >= 1; stride >>= 1) {
        if (t < stride) {
#pragma unroll
            for (int k = 0; k < GEOM_NS; k++) s[k][t] = s[k][t] + s[k][t + stride];
        }
        __syncthreads();
    }
    if (t == 0) {
#pragma unroll
        for (int k = 0; k < GEOM_NS; k++) out[k] = s[k][0];
    }
}

__global__ void __launch_bounds__(GEOM_B)
k_geom_stats_partial(int q, const float* __restrict__ dist, const int32_t* __restrict__ index, const GeomThresholds T,
                     double* __restrict__ partials) {
    __shared__ double s[GEOM_NS][GEOM_B];
    double acc[GEOM_NS];
#pragma unroll
    for (int k = 0; k < GEOM_NS; k++) acc[k] = 0.0;
    const size_t base = (size_t)blockIdx.x * DURF_GEOM_STAT_CHUNK;
    for (int r = 0; r < DURF_GEOM_STAT_CHUNK / GEOM_B; r++) {
        const size_t i = base + (size_t)r * GEOM_B + threadIdx.x;
        if (i >= (size_t)q) continue;
        const int id = index[i];
        if (id == -2) continue;
        const float d = dist[i];
        acc[0] += 1.0;
        acc[4] += (double)d;
        if (id >= 0) {
            acc[1] += 1.0;
            acc[2] += (double)d;
            acc[3] += (double)d * (double)d;
#pragma unroll
            for (int k = 0; k < DURF_GEOM_MAX_THRESHOLDS; k++)
                if (k < T.n && d <= T.t[k]) acc[5 + k] += 1.0;
        }
    }
    geom_fold(acc, s, partials + (size_t)blockIdx.x * GEOM_NS);
}

__global__ void __launch_bounds__(GEOM_B)
k_geom_stats_final(int nb, const double* __restrict__ partials, double* __restrict__ stats) {
    __shared__ double s[GEOM_NS][GEOM_B];
    double acc[GEOM_NS];
#pragma unroll
    for (int k = 0; k < GEOM_NS; k++) acc[k] = 0.0;
    for (int w = threadIdx.x; w < nb; w += GEOM_B) {
#pragma unroll
        for (int k = 0; k < GEOM_NS; k++) acc[k] += partials[(size_t)w * GEOM_NS + k];
    }
    geom_fold(acc, s, stats);
}

// ---- points on a mesh -------------------------------------------------------------------------------------------------------------
// pass 1: the area of every triangle (into cum) and the sum of every workgroup's 256
__global__ void __launch_bounds__(GEOM_B)
k_geom_areas(int V, const float* __restrict__ vert, int T, const int32_t* __restrict__ tri, double* __restrict__ cum,
             double* __restrict__ sums) {
    __shared__ double s_a[GEOM_WAVES];
    const int t = threadIdx.x, g = blockIdx.x * GEOM_B + t;
    double area = 0.0;
    if (g < T) {
        int v[3];
        if (tri_indices<false>(g, V, T, tri, v)) {                          // (not tri_fetch: what is not finite fails the area test)
            const float* A = vert + (size_t)v[0] * 3;
            float e1[3], e2[3], c[3];
            vec3_sub(vert + (size_t)v[1] * 3, A, e1);
            vec3_sub(vert + (size_t)v[2] * 3, A, e2);
            vec3_cross(e1, e2, c);
            const float a = 0.5f * sqrtf(vec3_dot(c, c));
            if (fabsf(a) <= 3.0e38f) area = (double)a;                      // (false for NaN and the infinities)
        }
        cum[g] = area;
    }
    scan_wave_to_lds(area, s_a);
    __syncthreads();
    if (t == 0) sums[blockIdx.x] = scan_block_sum<GEOM_WAVES>(s_a);
}

// pass 2: k_scan_block_sums<double, 1> (scan.h); the total goes to sums[nb] and *total

// pass 3: the areas in cum become their inclusive prefix sums
__global__ void __launch_bounds__(GEOM_B)
k_geom_offsets(int T, double* __restrict__ cum, const double* __restrict__ sums) {
    __shared__ double s_a[GEOM_WAVES];
    const int g = blockIdx.x * GEOM_B + threadIdx.x;
    const double a = g < T ? cum[g] : 0.0;
    const double ia = scan_wave_to_lds(a, s_a);
    __syncthreads();
    if (g >= T) return;
    cum[g] = scan_before_wave<GEOM_WAVES>(sums[blockIdx.x], s_a) + ia;
}

__global__ void __launch_bounds__(GEOM_B)
k_geom_sample(int V, const float* __restrict__ vert, int T, const int32_t* __restrict__ tri, const double* __restrict__ cum,
              const double* __restrict__ total, int n, float* __restrict__ points, int32_t* __restrict__ tri_out) {
    const int s = blockIdx.x * GEOM_B + threadIdx.x;
    if (s >= n) return;
    const double tot = T > 0 ? *total : 0.0;
    float* P = points + (size_t)s * 3;
    if (!(tot > 0.0)) {
        P[0] = P[1] = P[2] = nanf("");
        tri_out[s] = -1;
        return;
    }
    const double target = (((double)s + 0.5) * tot) / (double)n;
    int lo = 0, hi = T;                                                     // the first i with cum[i] > target
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        if (cum[mid] > target) hi = mid; else lo = mid + 1;
    }
    const int g = min(lo, T - 1);
    double u = 0.5 + (double)s * 0.7548776662466927, v = 0.5 + (double)s * 0.5698402909980532;
    u = u - floor(u);
    v = v - floor(v);
    if (u + v > 1.0) { u = 1.0 - u; v = 1.0 - v; }
    const float uf = (float)u, vf = (float)v;
    int iv[3];
    const bool readable = tri_indices<false>(g, V, T, tri, iv);             // (0 <= g < T: tot > 0 means T > 0)
    tri_out[s] = g;
    if (!readable) {                                                        // (an area-0 triangle is never chosen: a guard)
        P[0] = P[1] = P[2] = nanf("");
        return;
    }
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const float a = vert[(size_t)iv[0] * 3 + c], b = vert[(size_t)iv[1] * 3 + c], cc = vert[(size_t)iv[2] * 3 + c];
        P[c] = a + (uf * (b - a) + vf * (cc - a));                          // (its own order: a + (u e1 + v e2), not tri_interp's)
    }
}

// ---- launchers ------------------------------------------------------------------------------------------------------------------
namespace {

struct GeomWs {
    double *partials, *cum, *sums;
    int nbq, nbt;
    size_t total;
};

GeomWs carve_geom(void* base, int q, int T) {
    durf::Carver c{(char*)base, 0};
    GeomWs w{};
    w.nbq = (int)durf_cdiv((size_t)q, DURF_GEOM_STAT_CHUNK);
    w.nbt = (int)durf_cdiv((size_t)T, GEOM_B);
    w.partials = (double*)c.take((size_t)w.nbq * GEOM_NS * 8);
    w.cum = (double*)c.take((size_t)T * 8);
    w.sums = (double*)c.take((size_t)(w.nbt + 1) * 8);
    w.total = c.total();
    return w;
}

// -> 0, or -1 with the refusal set
int check_geom_grid(const char* who, const float* origin_host, float inv_cell, int nx, int ny, int nz, GeomGrid* G) {
    if (!origin_host) {
        durf_set_error("%s: requirement failed: origin", who);
        return -1;
    }
    if (!(nx >= 1 && ny >= 1 && nz >= 1 && nx <= DURF_GEOM_MAX_CELLS && ny <= DURF_GEOM_MAX_CELLS && nz <= DURF_GEOM_MAX_CELLS)) {
        durf_set_error("%s: requirement failed: 1 .. %d cells per axis (at most %d cells per axis), nx = %d, ny = %d, nz = %d", who,
                       DURF_GEOM_MAX_CELLS, DURF_GEOM_MAX_CELLS, nx, ny, nz);
        return -1;
    }
    if (!(inv_cell > 0.0f && inv_cell <= 3.0e38f)) {
        durf_set_error("%s: requirement failed: inv_cell is a positive finite number, inv_cell = %g", who, (double)inv_cell);
        return -1;
    }
    for (int a = 0; a < 3; a++) G->o[a] = origin_host[a];
    G->inv_cell = inv_cell;
    G->n[0] = nx; G->n[1] = ny; G->n[2] = nz;
    return 0;
}

}  // namespace

extern "C" {

size_t durf_geom_workspace_bytes(int n_queries, int n_triangles) {
    if (n_queries < 0 || n_triangles < 0) return 0;
    return carve_geom(nullptr, n_queries, n_triangles).total;
}

int durf_geom_keys(void* stream, int n, const float* points, const float* origin_host, float inv_cell, int nx, int ny, int nz,
                   int64_t* keys) {
    DURF_REQUIREF(n >= 0, "n >= 0, n = %d", n);
    DURF_REQUIREF(n == 0 || (points && keys), "points and keys for n = %d", n);
    GeomGrid G{};
    if (check_geom_grid(__func__, origin_host, inv_cell, nx, ny, nz, &G) != 0) return -1;
    if (n == 0) return 0;
    hipLaunchKernelGGL(k_geom_keys, dim3(durf_cdiv((size_t)n, GEOM_B)), dim3(GEOM_B), 0, (hipStream_t)stream, n, points, G, keys);
    DURF_CHECK_LAUNCH("k_geom_keys");
    return 0;
}

int durf_geom_nearest(void* stream, int q, const float* query, int m, const float* ref_sorted, const int64_t* ref_keys,
                      const int32_t* ref_index, const float* origin_host, float inv_cell, int nx, int ny, int nz, float max_dist,
                      float* dist, int32_t* index) {
    DURF_REQUIREF(q >= 0 && m >= 0, "q >= 0 and m >= 0, q = %d, m = %d", q, m);
    DURF_REQUIREF(q == 0 || (query && dist && index), "query, dist and index for q = %d", q);
    DURF_REQUIREF(m == 0 || (ref_sorted && ref_keys && ref_index), "ref_sorted, ref_keys and ref_index for m = %d", m);
    DURF_REQUIREF(max_dist >= 1e-18f && max_dist <= 1e18f, "1e-18 <= max_dist <= 1e18, max_dist = %g", (double)max_dist);
    GeomGrid G{};
    if (check_geom_grid(__func__, origin_host, inv_cell, nx, ny, nz, &G) != 0) return -1;
    const double rule = (double)inv_cell * (double)max_dist * (1.0 + 1.0 / 1024.0);
    DURF_REQUIREF(rule <= 1.0 + 1.0 / 4194304.0,
                 "the grid rule inv_cell * max_dist * (1 + 2^-10) <= 1 + 2^-22 (a cell is max_dist (1 + 2^-10) or more), inv_cell = %.9g, "
                 "max_dist = %.9g", (double)inv_cell, (double)max_dist);
    if (q == 0) return 0;
    const float md2 = max_dist * max_dist;
    hipLaunchKernelGGL(k_geom_nearest, dim3(durf_cdiv((size_t)q, GEOM_B)), dim3(GEOM_B), 0, (hipStream_t)stream, q, query, m, ref_sorted,
                       ref_keys, ref_index, G, max_dist, md2, dist, index);
    DURF_CHECK_LAUNCH("k_geom_nearest");
    return 0;
}

int durf_geom_stats(void* stream, int q, const float* dist, const int32_t* index, int n_thresholds, const float* thresholds_host,
                    void* workspace, size_t workspace_bytes, double* stats) {
    DURF_REQUIREF(q >= 0, "q >= 0, q = %d", q);
    DURF_REQUIREF(q == 0 || (dist && index), "dist and index for q = %d", q);
    DURF_REQUIREF(n_thresholds >= 0 && n_thresholds <= DURF_GEOM_MAX_THRESHOLDS, "0 .. %d thresholds, n_thresholds = %d",
                 DURF_GEOM_MAX_THRESHOLDS, n_thresholds);
    DURF_REQUIREF(n_thresholds == 0 || thresholds_host, "thresholds for n_thresholds = %d", n_thresholds);
    GeomThresholds T{};
    T.n = n_thresholds;
    for (int k = 0; k < n_thresholds; k++) {
        DURF_REQUIREF(thresholds_host[k] == thresholds_host[k], "thresholds are numbers, thresholds[%d] = %g", k, (double)thresholds_host[k]);
        T.t[k] = thresholds_host[k];
    }
    DURF_REQUIREF(stats != nullptr, "stats");
    DURF_REQUIREF(workspace != nullptr && ((size_t)workspace & 255) == 0, "workspace aligned to 256 bytes");
    const GeomWs w = carve_geom(workspace, q, 0);
    int rc = durf::check_workspace(__func__, workspace_bytes, w.total, "durf_geom_workspace_bytes(%d, 0)", q);
    if (rc != 0) return rc;
    if (w.nbq > 0) {
        hipLaunchKernelGGL(k_geom_stats_partial, dim3(w.nbq), dim3(GEOM_B), 0, (hipStream_t)stream, q, dist, index, T, w.partials);
        DURF_CHECK_LAUNCH("k_geom_stats_partial");
    }
    hipLaunchKernelGGL(k_geom_stats_final, dim3(1), dim3(GEOM_B), 0, (hipStream_t)stream, w.nbq, w.partials, stats);
    DURF_CHECK_LAUNCH("k_geom_stats_final");
    return 0;
}

int durf_geom_sample_mesh(void* stream, int n_vertices, const float* vertices, int n_triangles, const int32_t* triangles, int n,
                          void* workspace, size_t workspace_bytes, float* points, int32_t* tri, double* total_area) {
    DURF_REQUIREF(n >= 0 && n_vertices >= 0 && n_triangles >= 0, "n, n_vertices and n_triangles >= 0, n = %d, n_vertices = %d, n_triangles = %d",
                 n, n_vertices, n_triangles);
    // (not triangles.h's check_mesh: this entry's arguments are called n_vertices and n_triangles, and its messages say so)
    DURF_REQUIREF(n_vertices == 0 || vertices, "vertices for n_vertices = %d", n_vertices);
    DURF_REQUIREF(n_triangles == 0 || triangles, "triangles for n_triangles = %d", n_triangles);
    DURF_REQUIREF(n == 0 || (points && tri), "points and tri for n = %d", n);
    DURF_REQUIREF(total_area != nullptr, "total_area");
    DURF_REQUIREF(workspace != nullptr && ((size_t)workspace & 255) == 0, "workspace aligned to 256 bytes");
    const GeomWs w = carve_geom(workspace, 0, n_triangles);
    int rc = durf::check_workspace(__func__, workspace_bytes, w.total, "durf_geom_workspace_bytes(0, %d)", n_triangles);
    if (rc != 0) return rc;
    if (w.nbt > 0) {
        hipLaunchKernelGGL(k_geom_areas, dim3(w.nbt), dim3(GEOM_B), 0, (hipStream_t)stream, n_vertices, vertices, n_triangles, triangles,
                           w.cum, w.sums);
        DURF_CHECK_LAUNCH("k_geom_areas");
    }
    hipLaunchKernelGGL((k_scan_block_sums<double, 1>), dim3(1), dim3(SCAN_THREADS), 0, (hipStream_t)stream, w.nbt, w.sums, total_area);
    DURF_CHECK_LAUNCH("k_scan_block_sums<double, 1>");
    if (w.nbt > 0) {
        hipLaunchKernelGGL(k_geom_offsets, dim3(w.nbt), dim3(GEOM_B), 0, (hipStream_t)stream, n_triangles, w.cum, w.sums);
        DURF_CHECK_LAUNCH("k_geom_offsets");
    }
    if (n > 0) {
        hipLaunchKernelGGL(k_geom_sample, dim3(durf_cdiv((size_t)n, GEOM_B)), dim3(GEOM_B), 0, (hipStream_t)stream, n_vertices, vertices,
                           n_triangles, triangles, w.cum, total_area, n, points, tri);
        DURF_CHECK_LAUNCH("k_geom_sample");
    }
    return 0;
}

}  // extern "C"
