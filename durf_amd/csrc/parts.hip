// The connected components of a density lattice's IN points under the 14-neighbour adjacency of the Kuhn tetrahedra
// (include/durf_parts.h; libdurf_parts.so): label (a union-find by minimum index: tile pass in LDS, border unions with
// atomicMin, flatten), number (the scan of scan.h over the roots, one gather), sizes and index bounds (integer atomics, folded
// per wave first), and the compaction of a mesh to the components a caller keeps.  Integers throughout; nothing synchronises
// or copies to the host; no workgroup waits for another.
#include <climits>
#include "workspace.h"
#include "scan.h"
#include "lattice.h"
#include "../../include/durf_mesh.h"
#include "../../include/durf_parts.h"

#define PARTS_B DURF_PARTS_BLOCK
#define PARTS_WAVES (PARTS_B / DURF_WAVE)
#define TI DURF_PARTS_TILE_I
#define TJ DURF_PARTS_TILE_J
#define TK DURF_PARTS_TILE_K
#define TPOINTS DURF_PARTS_TILE_POINTS
static_assert(TPOINTS == 256 && TPOINTS % DURF_WAVE == 0 && DURF_WAVE % TK == 0, "one workgroup of whole waves, lanes along k");

struct PartsTiles { int tu, tv, tw; };  // tiles along each axis

__device__ __forceinline__ bool parts_in(const float* __restrict__ density, const uint8_t* __restrict__ valid, float iso, int g) {
    float d;
    return lattice_usable(density, valid, g, &d) && d >= iso;
}

// L is read while other workgroups change it: a relaxed load at agent scope (served past this unit's L1)
__device__ __forceinline__ int parts_load(const int32_t* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- (a) the tile pass -----------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(TPOINTS)
k_parts_tile(const LatticeDims D, const PartsTiles B, const float* __restrict__ density, const uint8_t* __restrict__ valid, float iso,
             int32_t* __restrict__ L) {
    __shared__ int s_lab[TPOINTS];
    const LatticeDims T{TI, TJ, TK, TPOINTS};                                 // the tile is a lattice of its own, in LDS
    const int l = threadIdx.x;
    int li, lj, lk;
    lattice_ijk(T, l, li, lj, lk);
    const int b = blockIdx.x;
    const int bk = b % B.tw, bj = b / B.tw % B.tv, bi = b / (B.tw * B.tv);
    const int i = bi * TI + li, j = bj * TJ + lj, k = bk * TK + lk;
    const bool inside = i < D.nu && j < D.nv && k < D.nw;
    const int g = inside ? lattice_index(D, i, j, k) : 0;
    const bool in = inside && parts_in(density, valid, iso, g);
    int mine = in ? l : -1;
    s_lab[l] = mine;
    __syncthreads();
    // the adjacent points inside the tile: bit e the end of owned edge e, bit 7 + e the point that owns edge e towards this one
    unsigned adj = 0;
    if (in) {
#pragma unroll
        for (int e = 0; e < 7; e++) {
            int di, dj, dk;
            lattice_edge(e, di, dj, dk);
            const int o = lattice_edge_offset(T, e);
            if (li + di < TI && lj + dj < TJ && lk + dk < TK && s_lab[l + o] >= 0) adj |= 1u << e;
            if (li - di >= 0 && lj - dj >= 0 && lk - dk >= 0 && s_lab[l - o] >= 0) adj |= 1u << (7 + e);
        }
    }
    // every value in s_lab is the local index of an IN point of the same component, no larger than the point's own
    for (int round = 0; round < TPOINTS; round++) {
        int m = mine;
        if (adj) {
#pragma unroll
            for (int e = 0; e < 7; e++) {
                const int o = lattice_edge_offset(T, e);
                if (adj >> e & 1u) m = min(m, s_lab[l + o]);
                if (adj >> (7 + e) & 1u) m = min(m, s_lab[l - o]);
            }
            m = s_lab[m];                                                     // one jump (m is IN: s_lab[m] is in 0 .. m)
        }
        __syncthreads();                                                      // every read of this round is done
        const bool changed = m < mine;
        if (changed) {
            mine = m;
            s_lab[l] = m;
        }
        if (!__syncthreads_or(changed)) break;                                // (uniform over the workgroup)
    }
    if (inside) {
        int out = -1;
        if (in) {
            int ri, rj, rk;
            lattice_ijk(T, mine, ri, rj, rk);
            out = lattice_index(D, bi * TI + ri, bj * TJ + rj, bk * TK + rk);
        }
        L[g] = out;
    }
}

// ---- (b) the border pass ---------------------------------------------------------------------------------------------------------
// the end of x's chain of links: strictly decreasing indices, at most n steps (x is IN: L[x] is in 0 .. x)
__device__ __forceinline__ int parts_find(const int32_t* L, int x) {
    for (;;) {
        const int p = parts_load(L + x);
        if (p >= x || p < 0) return x;                                        // the root (p == x); anything else cannot be
        x = p;
    }
}

// links only ever go under a smaller index; the larger of the pair strictly decreases from one retry to the next
__device__ __forceinline__ void parts_unite(int32_t* L, int a, int b) {
    while (a != b) {
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(L + a, b);
        if (old == a || old < 0) break;                                       // a was a root and hangs under b now
        a = old;                                                              // old < a: (old, b) are still to be united
    }
}

__global__ void __launch_bounds__(PARTS_B)
k_parts_border(const LatticeDims D, int32_t* L) {
    const int g = blockIdx.x * PARTS_B + threadIdx.x;
    if (g >= D.n) return;
    int i, j, k;
    lattice_ijk(D, g, i, j, k);
    const bool ei = i % TI == TI - 1 && i + 1 < D.nu, ej = j % TJ == TJ - 1 && j + 1 < D.nv, ek = k % TK == TK - 1 && k + 1 < D.nw;
    if (!(ei || ej || ek)) return;                                            // every owned edge stays inside the tile
    if (parts_load(L + g) < 0) return;                                        // not IN (-1 is never changed)
    int a = -1;
#pragma unroll
    for (int e = 0; e < 7; e++) {
        int di, dj, dk;
        lattice_edge(e, di, dj, dk);
        if (!((di && ei) || (dj && ej) || (dk && ek))) continue;              // stays inside the tile (or leaves the lattice)
        if (i + di >= D.nu || j + dj >= D.nv || k + dk >= D.nw) continue;
        const int q = g + lattice_index(D, di, dj, dk);
        if (parts_load(L + q) < 0) continue;
        if (a < 0) a = parts_find(L, g);
        parts_unite(L, a, parts_find(L, q));
    }
}

// ---- (c) flatten ------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(PARTS_B)
k_parts_flatten(int n, const int32_t* __restrict__ L, int32_t* __restrict__ labels) {
    const int g = blockIdx.x * PARTS_B + threadIdx.x;
    if (g >= n) return;
    int x = L[g];
    if (x >= 0) {
        for (;;) {                                                            // L is constant here: plain loads
            const int p = L[x];
            if (p >= x || p < 0) break;
            x = p;
        }
    }
    labels[g] = x;
}

// ---- number -----------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(PARTS_B)
k_parts_roots(int n, const int32_t* __restrict__ labels, int32_t* __restrict__ sums) {
    __shared__ int s_w[PARTS_WAVES];
    const int g = blockIdx.x * PARTS_B + threadIdx.x;
    const int c = g < n && labels[g] == g ? 1 : 0;
    scan_wave_to_lds(c, s_w);
    __syncthreads();
    if (threadIdx.x == 0) sums[blockIdx.x] = scan_block_sum<PARTS_WAVES>(s_w);
}

__global__ void __launch_bounds__(PARTS_B)
k_parts_rank(int n, const int32_t* __restrict__ labels, const int32_t* __restrict__ sums, int32_t* __restrict__ rank) {
    __shared__ int s_w[PARTS_WAVES];
    const int g = blockIdx.x * PARTS_B + threadIdx.x;
    const int c = g < n && labels[g] == g ? 1 : 0;
    const int inc = scan_wave_to_lds(c, s_w);
    __syncthreads();
    if (g < n) rank[g] = scan_before_wave<PARTS_WAVES>(sums[blockIdx.x], s_w) + (inc - c);
}

__global__ void __launch_bounds__(PARTS_B)
k_parts_number(int n, const int32_t* __restrict__ labels, const int32_t* __restrict__ rank, int32_t* __restrict__ comp) {
    const int g = blockIdx.x * PARTS_B + threadIdx.x;
    if (g >= n) return;
    const int l = labels[g];
    comp[g] = l >= 0 && l < n ? rank[l] : -1;
}

// ---- stats ------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(PARTS_B)
k_parts_stats_init(int max_components, int32_t* __restrict__ size, int32_t* __restrict__ bbox) {
    const int c = blockIdx.x * PARTS_B + threadIdx.x;
    if (c >= max_components) return;
    size[c] = 0;
#pragma unroll
    for (int x = 0; x < 3; x++) {
        bbox[(size_t)c * 6 + x] = INT_MAX;
        bbox[(size_t)c * 6 + 3 + x] = -1;
    }
}

__device__ __forceinline__ int wave_min(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
    return v;
}

// where the sums of one component go: the bounds only move one way, so a value read earlier that is already as good (a stale
// one is never better than the current one) means the atomic would change nothing
__device__ __forceinline__ void parts_stats_add(int32_t* size, int32_t* bbox, int c, int cnt, const int* lo, const int* hi) {
    atomicAdd(size + c, cnt);
    int32_t* row = bbox + (size_t)c * 6;
#pragma unroll
    for (int x = 0; x < 3; x++) {
        if (parts_load(row + x) > lo[x]) atomicMin(row + x, lo[x]);
        if (parts_load(row + 3 + x) < hi[x]) atomicMax(row + 3 + x, hi[x]);
    }
}

#define STATS_CHUNKS 8                 // a workgroup walks this many runs of PARTS_B points
#define STATS_SLOTS 16                 // and collects this many components in LDS before it adds them to global memory

// One thread per lattice point and chunk.  A wave folds the lanes that share a component (lanes lie along k, so a wave usually
// holds a few components; the loop retires at least one lane per turn: at most 64 turns); the fold's leader adds the result to
// the workgroup's small LDS table, found with at most STATS_SLOTS probes, or straight to global memory when the table is full;
// at the end the table's entries are added to global memory.  So one component of millions of points sends a few thousand
// atomics to its seven addresses, not millions.
__global__ void __launch_bounds__(PARTS_B)
k_parts_stats(const LatticeDims D, const int32_t* __restrict__ comp, int max_components, int32_t* size, int32_t* bbox) {
    __shared__ int s_key[STATS_SLOTS], s_cnt[STATS_SLOTS], s_lo[STATS_SLOTS][3], s_hi[STATS_SLOTS][3];
    const int lane = threadIdx.x & (DURF_WAVE - 1);
    if (threadIdx.x < STATS_SLOTS) {
        s_key[threadIdx.x] = -1;
        s_cnt[threadIdx.x] = 0;
#pragma unroll
        for (int x = 0; x < 3; x++) { s_lo[threadIdx.x][x] = INT_MAX; s_hi[threadIdx.x][x] = -1; }
    }
    __syncthreads();
    for (int chunk = 0; chunk < STATS_CHUNKS; chunk++) {
        const int g = (blockIdx.x * STATS_CHUNKS + chunk) * PARTS_B + threadIdx.x;       // < n + STATS_CHUNKS PARTS_B < 2^28
        int c = -1, i = 0, j = 0, k = 0;
        if (g < D.n) {
            c = comp[g];
            lattice_ijk(D, g, i, j, k);
        }
        bool todo = c >= 0 && c < max_components;
        for (int turn = 0; turn < DURF_WAVE; turn++) {
            const unsigned long long open = __ballot(todo);
            if (open == 0) break;                                             // (uniform over the wave)
            const int lead = __ffsll((long long)open) - 1;
            const int cl = __shfl(c, lead, 64);
            const bool member = todo && c == cl;
            const int cnt = __popcll(__ballot(member));
            const int lo[3] = {wave_min(member ? i : INT_MAX), wave_min(member ? j : INT_MAX), wave_min(member ? k : INT_MAX)};
            const int hi[3] = {-wave_min(member ? -i : INT_MAX), -wave_min(member ? -j : INT_MAX), -wave_min(member ? -k : INT_MAX)};
            if (lane == lead) {
                int slot = -1;
                for (int probe = 0; probe < STATS_SLOTS; probe++) {
                    const int h = (cl + probe) & (STATS_SLOTS - 1);
                    const int old = atomicCAS(&s_key[h], -1, cl);
                    if (old == -1 || old == cl) { slot = h; break; }
                }
                if (slot >= 0) {
                    atomicAdd(&s_cnt[slot], cnt);
#pragma unroll
                    for (int x = 0; x < 3; x++) {
                        atomicMin(&s_lo[slot][x], lo[x]);
                        atomicMax(&s_hi[slot][x], hi[x]);
                    }
                } else {
                    parts_stats_add(size, bbox, cl, cnt, lo, hi);
                }
            }
            if (member) todo = false;
        }
    }
    __syncthreads();
    if (threadIdx.x < STATS_SLOTS && s_key[threadIdx.x] >= 0)
        parts_stats_add(size, bbox, s_key[threadIdx.x], s_cnt[threadIdx.x], s_lo[threadIdx.x], s_hi[threadIdx.x]);
}

// ---- keep some components of a mesh ------------------------------------------------------------------------------------------------
struct PartsSelect {
    const int32_t* counts;
    int max_vertices, max_triangles;
    const int32_t* vertex_comp;
    const int32_t* triangles;
    const uint8_t* keep;
    int n_components;
};

__device__ __forceinline__ bool select_vertex(const PartsSelect& S, int V, int v) {
    if (v < 0 || v >= V) return false;
    const int c = S.vertex_comp[v];
    return c >= 0 && c < S.n_components && S.keep[c] != 0;
}

__device__ __forceinline__ bool select_triangle(const PartsSelect& S, int V, int T, int t) {
    return t < T && select_vertex(S, V, S.triangles[(size_t)t * 3]);
}

// row 0 of the block sums counts kept vertices, row 1 kept triangles: element x of block b is vertex x and triangle x
__global__ void __launch_bounds__(PARTS_B)
k_parts_select_sums(const PartsSelect S, int32_t* __restrict__ sums_v, int32_t* __restrict__ sums_t) {
    __shared__ int s_v[PARTS_WAVES], s_t[PARTS_WAVES];
    const int x = blockIdx.x * PARTS_B + threadIdx.x;
    const int V = min(S.counts[0], S.max_vertices), T = min(S.counts[1], S.max_triangles);
    scan_wave_to_lds(select_vertex(S, V, x) ? 1 : 0, s_v);
    scan_wave_to_lds(select_triangle(S, V, T, x) ? 1 : 0, s_t);
    __syncthreads();
    if (threadIdx.x == 0) {
        sums_v[blockIdx.x] = scan_block_sum<PARTS_WAVES>(s_v);
        sums_t[blockIdx.x] = scan_block_sum<PARTS_WAVES>(s_t);
    }
}

__global__ void __launch_bounds__(PARTS_B)
k_parts_select_vertices(const PartsSelect S, const int32_t* __restrict__ sums_v, int32_t* __restrict__ vertex_map,
                        int32_t* __restrict__ vertex_src) {
    __shared__ int s_v[PARTS_WAVES];
    const int v = blockIdx.x * PARTS_B + threadIdx.x;
    const int V = min(S.counts[0], S.max_vertices);
    const int c = select_vertex(S, V, v) ? 1 : 0;
    const int inc = scan_wave_to_lds(c, s_v);
    __syncthreads();
    if (v >= S.max_vertices) return;
    const int id = scan_before_wave<PARTS_WAVES>(sums_v[blockIdx.x], s_v) + (inc - c);       // id <= v < max_vertices
    vertex_map[v] = c ? id : -1;
    if (c) vertex_src[id] = v;
}

__global__ void __launch_bounds__(PARTS_B)
k_parts_select_triangles(const PartsSelect S, const int32_t* __restrict__ sums_t, const int32_t* __restrict__ vertex_map,
                         int32_t* __restrict__ triangles_out) {
    __shared__ int s_t[PARTS_WAVES];
    const int t = blockIdx.x * PARTS_B + threadIdx.x;
    const int V = min(S.counts[0], S.max_vertices), T = min(S.counts[1], S.max_triangles);
    const int c = select_triangle(S, V, T, t) ? 1 : 0;
    const int inc = scan_wave_to_lds(c, s_t);
    __syncthreads();
    if (!c) return;
    const int id = scan_before_wave<PARTS_WAVES>(sums_t[blockIdx.x], s_t) + (inc - c);       // id <= t < max_triangles
#pragma unroll
    for (int x = 0; x < 3; x++) {
        const int v = S.triangles[(size_t)t * 3 + x];
        triangles_out[(size_t)id * 3 + x] = v >= 0 && v < V ? vertex_map[v] : -1;
    }
}

// ---- launchers --------------------------------------------------------------------------------------------------------------------
namespace {

struct PartsWs {
    int32_t *link, *sums;
    int nb;
    size_t total;
};

PartsWs carve_parts(void* base, int n) {
    durf::Carver c{(char*)base, 0};
    PartsWs w{};
    w.nb = (int)durf_cdiv((size_t)n, PARTS_B);
    w.link = (int32_t*)c.take((size_t)n * 4);
    w.sums = (int32_t*)c.take((size_t)(w.nb + 1) * 4);
    w.total = c.total();
    return w;
}

}  // namespace

extern "C" {

size_t durf_parts_workspace_bytes(int nu, int nv, int nw) {
    if (!lattice_shape_ok(nu, nv, nw, DURF_MESH_MAX_POINTS)) return 0;
    return carve_parts(nullptr, nu * nv * nw).total;
}

int durf_parts_label(void* stream, int nu, int nv, int nw, const float* density, const uint8_t* valid, float iso, void* workspace,
                     size_t workspace_bytes, int32_t* labels) {
    const int n = check_lattice_shape(__func__, nu, nv, nw, DURF_MESH_MAX_POINTS);
    if (n < 0) return -1;
    DURF_REQUIREF(iso == iso, "iso is a number, iso = %g", (double)iso);
    DURF_REQUIREF(density && labels, "density and labels");
    if (durf::check_workspace_aligned(__func__, workspace) != 0) return -1;
    const PartsWs w = carve_parts(workspace, n);
    int rc = durf::check_workspace(__func__, workspace_bytes, w.total, "durf_parts_workspace_bytes(%d, %d, %d)", nu, nv, nw);
    if (rc != 0) return rc;
    const LatticeDims D{nu, nv, nw, n};
    const PartsTiles B{(int)durf_cdiv(nu, TI), (int)durf_cdiv(nv, TJ), (int)durf_cdiv(nw, TK)};
    const hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_parts_tile, dim3((unsigned)B.tu * B.tv * B.tw), dim3(TPOINTS), 0, s, D, B, density, valid, iso, w.link);
    DURF_CHECK_LAUNCH("k_parts_tile");
    hipLaunchKernelGGL(k_parts_border, dim3(w.nb), dim3(PARTS_B), 0, s, D, w.link);
    DURF_CHECK_LAUNCH("k_parts_border");
    hipLaunchKernelGGL(k_parts_flatten, dim3(w.nb), dim3(PARTS_B), 0, s, n, w.link, labels);
    DURF_CHECK_LAUNCH("k_parts_flatten");
    return 0;
}

int durf_parts_number(void* stream, int n, const int32_t* labels, void* workspace, size_t workspace_bytes, int32_t* comp,
                      int32_t* count) {
    DURF_REQUIREF(n >= 1 && n < DURF_MESH_MAX_POINTS, "1 <= n < 2^27, n = %d", n);
    DURF_REQUIREF(labels && comp && count, "labels, comp and count");
    if (durf::check_workspace_aligned(__func__, workspace) != 0) return -1;
    const PartsWs w = carve_parts(workspace, n);
    int rc = durf::check_workspace(__func__, workspace_bytes, w.total, "the workspace of n = %d points", n);
    if (rc != 0) return rc;
    const hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_parts_roots, dim3(w.nb), dim3(PARTS_B), 0, s, n, labels, w.sums);
    DURF_CHECK_LAUNCH("k_parts_roots");
    hipLaunchKernelGGL((k_scan_block_sums<int32_t, 1>), dim3(1), dim3(SCAN_THREADS), 0, s, w.nb, w.sums, count);
    DURF_CHECK_LAUNCH("k_scan_block_sums<int32_t, 1>");
    hipLaunchKernelGGL(k_parts_rank, dim3(w.nb), dim3(PARTS_B), 0, s, n, labels, w.sums, w.link);
    DURF_CHECK_LAUNCH("k_parts_rank");
    hipLaunchKernelGGL(k_parts_number, dim3(w.nb), dim3(PARTS_B), 0, s, n, labels, w.link, comp);
    DURF_CHECK_LAUNCH("k_parts_number");
    return 0;
}

int durf_parts_stats(void* stream, int nu, int nv, int nw, const int32_t* comp, int max_components, int32_t* size, int32_t* bbox) {
    const int n = check_lattice_shape(__func__, nu, nv, nw, DURF_MESH_MAX_POINTS);
    if (n < 0) return -1;
    DURF_REQUIREF(max_components >= 0, "max_components >= 0, max_components = %d", max_components);
    DURF_REQUIREF(comp != nullptr, "comp");
    DURF_REQUIREF((size && bbox) || max_components == 0, "size and bbox for max_components = %d", max_components);
    if (max_components == 0) return 0;
    const LatticeDims D{nu, nv, nw, n};
    const hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_parts_stats_init, dim3(durf_cdiv((size_t)max_components, PARTS_B)), dim3(PARTS_B), 0, s, max_components, size, bbox);
    DURF_CHECK_LAUNCH("k_parts_stats_init");
    hipLaunchKernelGGL(k_parts_stats, dim3(durf_cdiv((size_t)n, (size_t)PARTS_B * STATS_CHUNKS)), dim3(PARTS_B), 0, s, D, comp, max_components, size, bbox);
    DURF_CHECK_LAUNCH("k_parts_stats");
    return 0;
}

int durf_parts_select_mesh(void* stream, const int32_t* counts, int max_vertices, int max_triangles, const int32_t* vertex_comp,
                           const int32_t* triangles, const uint8_t* keep, int n_components, void* workspace, size_t workspace_bytes,
                           int32_t* vertex_map, int32_t* vertex_src, int32_t* triangles_out, int32_t* counts_out) {
    DURF_REQUIREF(max_vertices >= 0 && max_triangles >= 0, "capacities >= 0, max_vertices = %d, max_triangles = %d", max_vertices,
                 max_triangles);
    DURF_REQUIREF(n_components >= 0, "n_components >= 0, n_components = %d", n_components);
    DURF_REQUIREF(counts && counts_out, "counts and counts_out");
    DURF_REQUIREF((vertex_comp && vertex_map && vertex_src) || max_vertices == 0, "vertex_comp, vertex_map and vertex_src for max_vertices = %d",
                 max_vertices);
    DURF_REQUIREF((triangles && triangles_out) || max_triangles == 0, "triangles and triangles_out for max_triangles = %d", max_triangles);
    DURF_REQUIREF(keep || n_components == 0, "keep for n_components = %d", n_components);
    if (durf::check_workspace_aligned(__func__, workspace) != 0) return -1;
    const int nm = (int)durf_cdiv((size_t)(max_vertices > max_triangles ? max_vertices : max_triangles), PARTS_B);
    const size_t need = ((size_t)2 * (nm + 1) * 4 + 255) & ~(size_t)255;
    int rc = durf::check_workspace(__func__, workspace_bytes, need, "the block sums of %d vertices and %d triangles", max_vertices,
                                   max_triangles);
    if (rc != 0) return rc;
    int32_t* sums_v = (int32_t*)workspace;
    int32_t* sums_t = sums_v + (nm + 1);
    const PartsSelect S{counts, max_vertices, max_triangles, vertex_comp, triangles, keep, n_components};
    const hipStream_t s = (hipStream_t)stream;
    if (nm > 0) {
        hipLaunchKernelGGL(k_parts_select_sums, dim3(nm), dim3(PARTS_B), 0, s, S, sums_v, sums_t);
        DURF_CHECK_LAUNCH("k_parts_select_sums");
    }
    hipLaunchKernelGGL((k_scan_block_sums<int32_t, 2>), dim3(1), dim3(SCAN_THREADS), 0, s, nm, sums_v, counts_out);
    DURF_CHECK_LAUNCH("k_scan_block_sums<int32_t, 2>");
    if (max_vertices > 0) {
        hipLaunchKernelGGL(k_parts_select_vertices, dim3(durf_cdiv((size_t)max_vertices, PARTS_B)), dim3(PARTS_B), 0, s, S, sums_v, vertex_map,
                           vertex_src);
        DURF_CHECK_LAUNCH("k_parts_select_vertices");
    }
    if (max_triangles > 0) {
        hipLaunchKernelGGL(k_parts_select_triangles, dim3(durf_cdiv((size_t)max_triangles, PARTS_B)), dim3(PARTS_B), 0, s, S, sums_t, vertex_map,
                           triangles_out);
        DURF_CHECK_LAUNCH("k_parts_select_triangles");
    }
    return 0;
}

}  // extern "C"
