// A triangle mesh through pinhole cameras (include/durf_raster.h; libdurf_raster.so): project, cull and snap every (frame,
// triangle) pair into a record, count the pairs per 16 x 16 tile, scan, bin, and let one workgroup per tile gather the
// nearest covering triangle of each of its pixels with exact int64 edge functions; then a per-pixel attribute gather.  The only
// atomics are integer adds on counters; the picture is a minimum over a set and does not depend on their order.  Nothing
// synchronises or copies to the host; no workgroup waits for another.
#include <climits>
#include "workspace.h"
#include "scan.h"
#include "triangles.h"
#include "../../include/durf_raster.h"

#define RB DURF_RASTER_BLOCK
#define RWAVES (RB / DURF_WAVE)
#define RTILE DURF_RASTER_TILE
#define RBATCH DURF_RASTER_BATCH
#define RINTS DURF_RASTER_RECORD_INTS
#define REC_EMPTY 1                    // tx0 = 1 > tx1 = 0: a pair that draws nothing
static_assert(RTILE * RTILE == 256 && RBATCH == 256 && RB == 256, "one pixel, one record of a batch and one element per thread");
static_assert(DURF_RASTER_MAX_SIZE / RTILE <= 256, "a tile coordinate fits 8 bits");
static_assert(DURF_RASTER_COUNTS == 8 && RINTS == 10, "the layouts the header states");

typedef long long i64;

struct RasterDims {
    int F, T, h, w;
    int th, tw, tpf;                   // tiles down, across and per frame
    int n_tiles;                       // F tpf
};

// ---- steps 1 and 2 ---------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(RB)
k_raster_clear(int n_tiles, int32_t* __restrict__ tile_count, int32_t* __restrict__ counts) {
    const int i = blockIdx.x * RB + threadIdx.x;
    if (i < n_tiles) tile_count[i] = 0;
    if (i < DURF_RASTER_COUNTS) counts[i] = 0;
}

// the pixels whose centres lie in [lo, hi] (snapped units): ceil(lo / 256) .. floor(hi / 256); >> floors for negatives too
__device__ __forceinline__ int raster_px_lo(int lo) { return (lo + (DURF_RASTER_SUBPIXEL - 1)) >> 8; }
__device__ __forceinline__ int raster_px_hi(int hi) { return hi >> 8; }

__global__ void __launch_bounds__(RB)
k_raster_setup(const RasterDims D, const float* __restrict__ cams, int V, const float* __restrict__ vertices,
               const int32_t* __restrict__ triangles, float znear, int cull, int32_t* __restrict__ records, int32_t* tile_count,
               int32_t* counts) {
    __shared__ int s_tally[DURF_RASTER_COUNTS];
    if (threadIdx.x < DURF_RASTER_COUNTS) s_tally[threadIdx.x] = 0;
    __syncthreads();
    const unsigned i = blockIdx.x * (unsigned)RB + threadIdx.x;              // F T < 2^31
    const bool live = i < (unsigned)D.F * (unsigned)D.T;
    int why = 0;                                                             // the index into counts: 1 drawn, 2 .. 7 the culls
    int X[3] = {0, 0, 0}, Y[3] = {0, 0, 0};
    float iz[3] = {0.0f, 0.0f, 0.0f};
    int packed = REC_EMPTY;
    if (live) {
        const int f = i / (unsigned)D.T, t = i - (unsigned)f * (unsigned)D.T;
        const float* cam = cams + (size_t)f * DURF_CAM_FLOATS;
        float x[3], y[3], z[3];
        int v[3];
        bool valid = tri_indices<false>(t, V, D.T, triangles, v);            // (t < T by construction; finiteness is tested in camera space below)
        if (valid) {
#pragma unroll
            for (int c = 0; c < 3; c++) {
                const float* P = vertices + (size_t)v[c] * 3;
                const float P0 = P[0], P1 = P[1], P2 = P[2];
                float pc[3];
                cam_to_camera(cam, P0, P1, P2, pc);
                valid = valid && cam_finite(P0) && cam_finite(P1) && cam_finite(P2) && cam_finite(pc[0]) && cam_finite(pc[1]) &&
                        cam_finite(pc[2]);
                z[c] = -pc[2];
                cam_pixel(cam, pc[0], pc[1], z[c], x[c], y[c]);
            }
        }
        const float lim = (float)DURF_RASTER_MAX_COORD;
        if (!valid) {
            why = 2;
        } else {
            const int n_near = (z[0] < znear) + (z[1] < znear) + (z[2] < znear);
            bool range = false;
#pragma unroll
            for (int c = 0; c < 3; c++)
                range = range || !(fabsf(256.0f * x[c]) <= lim) || !(fabsf(256.0f * y[c]) <= lim);
            if (n_near == 3) {
                why = 3;
            } else if (n_near > 0) {
                why = 4;
            } else if (range) {
                why = 5;
            } else {
#pragma unroll
                for (int c = 0; c < 3; c++) {
                    X[c] = (int)rintf(256.0f * x[c]);
                    Y[c] = (int)rintf(256.0f * y[c]);
                    iz[c] = 1.0f / z[c];
                }
                const i64 A2 = (i64)(X[1] - X[0]) * (Y[2] - Y[0]) - (i64)(Y[1] - Y[0]) * (X[2] - X[0]);
                if (A2 == 0) why = 6;
                else if ((cull == 1 && A2 > 0) || (cull == 2 && A2 < 0)) why = 7;
                else why = 1;
            }
        }
        if (why == 1) {
            const int x0 = max(raster_px_lo(min(X[0], min(X[1], X[2]))), 0), x1 = min(raster_px_hi(max(X[0], max(X[1], X[2]))), D.w - 1);
            const int y0 = max(raster_px_lo(min(Y[0], min(Y[1], Y[2]))), 0), y1 = min(raster_px_hi(max(Y[0], max(Y[1], Y[2]))), D.h - 1);
            if (x0 <= x1 && y0 <= y1) {
                const int tx0 = x0 / RTILE, tx1 = x1 / RTILE, ty0 = y0 / RTILE, ty1 = y1 / RTILE;     // < 256 each
                packed = tx0 | tx1 << 8 | ty0 << 16 | (int)((unsigned)ty1 << 24);
                int32_t* row = tile_count + (size_t)f * D.tpf;
                for (int ty = ty0; ty <= ty1; ty++)
                    for (int tx = tx0; tx <= tx1; tx++) atomicAdd(row + ty * D.tw + tx, 1);
            }
        }
        int32_t* r = records + (size_t)i * RINTS;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            r[2 * c] = X[c];
            r[2 * c + 1] = Y[c];
            r[6 + c] = __float_as_int(iz[c]);
        }
        r[9] = packed;
    }
    // the tallies: a wave's lanes per reason, then the workgroup's in LDS, then one add per reason that occurred
#pragma unroll
    for (int c = 1; c < DURF_RASTER_COUNTS; c++) {
        const int cnt = __popcll(__ballot(why == c));
        if ((threadIdx.x & (DURF_WAVE - 1)) == 0 && cnt) atomicAdd(&s_tally[c], cnt);
    }
    __syncthreads();
    if (threadIdx.x >= 1 && threadIdx.x < DURF_RASTER_COUNTS && s_tally[threadIdx.x]) atomicAdd(counts + threadIdx.x, s_tally[threadIdx.x]);
}

__global__ void __launch_bounds__(RB)
k_raster_sums(int n_tiles, const int32_t* __restrict__ tile_count, i64* __restrict__ sums) {
    __shared__ i64 s_w[RWAVES];
    const int g = blockIdx.x * RB + threadIdx.x;
    scan_wave_to_lds<i64>(g < n_tiles ? tile_count[g] : 0, s_w);
    __syncthreads();
    if (threadIdx.x == 0) sums[blockIdx.x] = scan_block_sum<RWAVES>(s_w);
}

__global__ void __launch_bounds__(RB)
k_raster_offsets(int n_tiles, const int32_t* __restrict__ tile_count, const i64* __restrict__ sums, const i64* __restrict__ grand,
                 i64* __restrict__ tile_start, int32_t* __restrict__ counts) {
    __shared__ i64 s_w[RWAVES];
    const int g = blockIdx.x * RB + threadIdx.x;
    const i64 c = g < n_tiles ? tile_count[g] : 0;
    const i64 inc = scan_wave_to_lds<i64>(c, s_w);
    __syncthreads();
    if (g < n_tiles) tile_start[g] = scan_before_wave<RWAVES>(sums[blockIdx.x], s_w) + (inc - c);
    if (g == 0) {
        const i64 total = *grand;
        counts[0] = total > (i64)INT_MAX ? INT_MAX : (int)total;
    }
}

// ---- steps 3 and 4 ---------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(RB)
k_raster_begin(int n_tiles, int32_t* __restrict__ cursor) {
    const int i = blockIdx.x * RB + threadIdx.x;
    if (i < n_tiles) cursor[i] = 0;
}

__global__ void __launch_bounds__(RB)
k_raster_fill(const RasterDims D, const int32_t* __restrict__ records, const i64* __restrict__ tile_start, const i64* __restrict__ total,
              int32_t* cursor, int32_t* __restrict__ pairs, int max_pairs) {
    const unsigned i = blockIdx.x * (unsigned)RB + threadIdx.x;
    if (i >= (unsigned)D.F * (unsigned)D.T) return;
    if (*total > (i64)max_pairs) return;                                     // nothing is drawn: nothing is written
    const unsigned packed = (unsigned)records[(size_t)i * RINTS + 9];
    const int tx0 = packed & 255, tx1 = packed >> 8 & 255, ty0 = packed >> 16 & 255, ty1 = packed >> 24;
    if (tx0 > tx1 || tx1 >= D.tw || ty1 >= D.th) return;
    const int f = i / (unsigned)D.T;
    for (int ty = ty0; ty <= ty1; ty++)
        for (int tx = tx0; tx <= tx1; tx++) {
            const int tile = f * D.tpf + ty * D.tw + tx;
            const i64 pos = tile_start[tile] + atomicAdd(cursor + tile, 1);
            if (pos >= 0 && pos < (i64)max_pairs) pairs[pos] = (int)i;       // (always, while the total fits: the range is exact)
        }
}

// a record as the pixels of a tile want it: vertices 1 and 2 exchanged where A2 < 0, |A2| as a float, the bounds inside the tile
struct TileRec {
    int X[3], Y[3];
    float iz[3];
    float area;
    int t;                             // the triangle id, bit 31: exchanged
    int box;                           // lx0 | lx1 << 4 | ly0 << 8 | ly1 << 12 inside the tile, bit 16 + i: E_i == 0 counts as covered
};

__global__ void __launch_bounds__(RTILE * RTILE)
k_raster_tile(const RasterDims D, const int32_t* __restrict__ records, const int32_t* __restrict__ tile_count,
              const i64* __restrict__ tile_start, const i64* __restrict__ total, const int32_t* __restrict__ pairs, int max_pairs,
              int32_t* __restrict__ tri, float* __restrict__ depth, float* __restrict__ bary) {
    __shared__ TileRec s_rec[RBATCH];
    const int tile = blockIdx.x;
    const int f = tile / D.tpf, r = tile - f * D.tpf, ty = r / D.tw, tx = r - ty * D.tw;
    const int lx = threadIdx.x & (RTILE - 1), ly = threadIdx.x / RTILE;
    const int px = tx * RTILE + lx, py = ty * RTILE + ly;
    const bool inside = px < D.w && py < D.h;
    const size_t p = ((size_t)f * D.h + (inside ? py : 0)) * D.w + (inside ? px : 0);
    if (*total > (i64)max_pairs) {                                           // (uniform over the launch)
        if (inside) {
            const float nan = __builtin_nanf("");
            tri[p] = -2;
            depth[p] = nan;
            if (bary) bary[p * 3] = bary[p * 3 + 1] = bary[p * 3 + 2] = nan;
        }
        return;
    }
    const int n = tile_count[tile];
    const i64 start = tile_start[tile];
    unsigned long long best = ~0ull;
    float bq[3] = {0.0f, 0.0f, 0.0f};
    const int cx = px * DURF_RASTER_SUBPIXEL, cy = py * DURF_RASTER_SUBPIXEL;
    for (int base = 0; base < n; base += RBATCH) {                           // (uniform over the workgroup)
        const int m = min(RBATCH, n - base);
        if ((int)threadIdx.x < m) {
            const i64 pos = start + base + threadIdx.x;
            TileRec R;
            R.t = 0;
            R.box = 1;                                                       // lx0 = 1 > lx1 = 0: no pixel
            const unsigned id = pos >= 0 && pos < (i64)max_pairs ? (unsigned)pairs[pos] : ~0u;
            if (id < (unsigned)D.F * (unsigned)D.T) {
                const int32_t* g = records + (size_t)id * RINTS;
                int X[3], Y[3];
                float iz[3];
#pragma unroll
                for (int c = 0; c < 3; c++) {
                    X[c] = g[2 * c];
                    Y[c] = g[2 * c + 1];
                    iz[c] = __int_as_float(g[6 + c]);
                }
                i64 A2 = (i64)(X[1] - X[0]) * (Y[2] - Y[0]) - (i64)(Y[1] - Y[0]) * (X[2] - X[0]);
                const bool ex = A2 < 0;
                if (ex) {
                    int ti = X[1]; X[1] = X[2]; X[2] = ti;
                    ti = Y[1]; Y[1] = Y[2]; Y[2] = ti;
                    const float tf = iz[1]; iz[1] = iz[2]; iz[2] = tf;
                    A2 = -A2;
                }
                const int x0 = max(raster_px_lo(min(X[0], min(X[1], X[2]))), tx * RTILE) - tx * RTILE;
                const int x1 = min(raster_px_hi(max(X[0], max(X[1], X[2]))), tx * RTILE + RTILE - 1) - tx * RTILE;
                const int y0 = max(raster_px_lo(min(Y[0], min(Y[1], Y[2]))), ty * RTILE) - ty * RTILE;
                const int y1 = min(raster_px_hi(max(Y[0], max(Y[1], Y[2]))), ty * RTILE + RTILE - 1) - ty * RTILE;
                if (A2 > 0 && x0 <= x1 && y0 <= y1) {
                    int box = x0 | x1 << 4 | y0 << 8 | y1 << 12;
#pragma unroll
                    for (int e = 0; e < 3; e++) {
                        const int a = (e + 1) % 3, b = (e + 2) % 3;
                        const int dX = X[b] - X[a], dY = Y[b] - Y[a];
                        if (dY > 0 || (dY == 0 && dX < 0)) box |= 1 << (16 + e);
                    }
                    R.box = box;
                    R.t = (int)(id - (unsigned)f * (unsigned)D.T) | (ex ? INT_MIN : 0);
                    R.area = (float)A2;
#pragma unroll
                    for (int c = 0; c < 3; c++) {
                        R.X[c] = X[c];
                        R.Y[c] = Y[c];
                        R.iz[c] = iz[c];
                    }
                }
            }
            s_rec[threadIdx.x] = R;
        }
        __syncthreads();
        if (inside) {
            for (int j = 0; j < m; j++) {
                const int box = s_rec[j].box;
                if (lx < (box & 15) || lx > (box >> 4 & 15) || ly < (box >> 8 & 15) || ly > (box >> 12 & 15)) continue;
                const TileRec& R = s_rec[j];
                i64 E[3];
                bool covered = true;
#pragma unroll
                for (int e = 0; e < 3; e++) {
                    const int a = (e + 1) % 3, b = (e + 2) % 3;
                    E[e] = (i64)(R.X[b] - R.X[a]) * (cy - R.Y[a]) - (i64)(R.Y[b] - R.Y[a]) * (cx - R.X[a]);
                    covered = covered && (E[e] > 0 || (E[e] == 0 && (box >> (16 + e) & 1)));
                }
                if (!covered) continue;
                float wz[3];
#pragma unroll
                for (int e = 0; e < 3; e++) wz[e] = ((float)E[e] / R.area) * R.iz[e];
                const float s = (wz[0] + wz[1]) + wz[2];
                const float dep = 1.0f / s;
                const unsigned long long key = (unsigned long long)__float_as_uint(dep) << 32 | (unsigned)(R.t & INT_MAX);
                if (key < best) {
                    best = key;
                    const bool ex = R.t < 0;                                 // q goes back to the mesh's own vertex order
                    const float q1 = wz[1] * dep, q2 = wz[2] * dep;
                    bq[0] = wz[0] * dep;
                    bq[1] = ex ? q2 : q1;
                    bq[2] = ex ? q1 : q2;
                }
            }
        }
        __syncthreads();                                                      // s_rec is rewritten by the next batch
    }
    if (inside) {
        const bool hit = best != ~0ull;
        tri[p] = hit ? (int)(best & 0xffffffffull) : -1;
        depth[p] = hit ? __uint_as_float((unsigned)(best >> 32)) : 0.0f;
        if (bary) {
            bary[p * 3] = bq[0];
            bary[p * 3 + 1] = bq[1];
            bary[p * 3 + 2] = bq[2];
        }
    }
}

// ---- step 5 ------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(RB)
k_raster_interp(int n_pixels, int V, int T, const int32_t* __restrict__ triangles, const int32_t* __restrict__ tri,
                const float* __restrict__ bary, int C, const float* __restrict__ attr_f, float* __restrict__ out_f,
                const int32_t* __restrict__ attr_i, int fill, int32_t* __restrict__ out_i) {
    const int p = blockIdx.x * RB + threadIdx.x;
    if (p >= n_pixels) return;
    const int t = tri[p];
    int v[3] = {-1, -1, -1};
    const bool hit = tri_indices(t, V, T, triangles, v);
    if (out_i) out_i[p] = hit ? attr_i[v[0]] : fill;
    if (out_f) {
        float q[3] = {0.0f, 0.0f, 0.0f};
        if (hit) {
#pragma unroll
            for (int c = 0; c < 3; c++) q[c] = bary[(size_t)p * 3 + c];
        }
        for (int c = 0; c < C; c++) out_f[(size_t)p * C + c] = hit ? tri_interp(q, v, attr_f, C, c) : 0.0f;
    }
}

// ---- launchers --------------------------------------------------------------------------------------------------------------------
namespace {

struct RasterWs {
    int32_t *records, *tile_count, *cursor;
    i64 *tile_start, *sums, *grand;    // grand: the total number of (tile, pair) entries
    int nb;
    size_t total;
};

bool raster_shape_ok(int F, int T, int h, int w) {
    return F >= 0 && T >= 0 && h >= 1 && w >= 1 && h <= DURF_RASTER_MAX_SIZE && w <= DURF_RASTER_MAX_SIZE &&
           (double)F * T < 2147483648.0 && (double)F * h * w < 2147483648.0;
}

RasterDims raster_dims(int F, int T, int h, int w) {
    RasterDims D{F, T, h, w, (int)durf_cdiv(h, RTILE), (int)durf_cdiv(w, RTILE), 0, 0};
    D.tpf = D.th * D.tw;
    D.n_tiles = F * D.tpf;                                                   // <= F h w
    return D;
}

RasterWs carve_raster(void* base, const RasterDims& D) {
    durf::Carver c{(char*)base, 0};
    RasterWs w{};
    w.nb = (int)durf_cdiv((size_t)D.n_tiles, RB);
    w.records = (int32_t*)c.take((size_t)D.F * D.T * RINTS * 4);
    w.tile_count = (int32_t*)c.take((size_t)D.n_tiles * 4);
    w.cursor = (int32_t*)c.take((size_t)D.n_tiles * 4);
    w.tile_start = (i64*)c.take((size_t)D.n_tiles * 8);
    w.sums = (i64*)c.take((size_t)(w.nb + 2) * 8);                           // [nb + 1] and the scan's `totals` slot
    w.grand = w.sums + w.nb + 1;
    w.total = c.total();
    return w;
}

int check_raster_shape(const char* who, int F, int T, int h, int w) {
    if (!(F >= 0 && T >= 0)) {
        durf_set_error("%s: requirement failed: F >= 0 and T >= 0, F = %d, T = %d", who, F, T);
        return -1;
    }
    if (!(h >= 1 && w >= 1 && h <= DURF_RASTER_MAX_SIZE && w <= DURF_RASTER_MAX_SIZE)) {
        durf_set_error("%s: requirement failed: 1 <= h, w <= %d, h = %d, w = %d", who, DURF_RASTER_MAX_SIZE, h, w);
        return -1;
    }
    if (!((double)F * T < 2147483648.0)) {
        durf_set_error("%s: requirement failed: F T < 2^31 pairs, F = %d, T = %d", who, F, T);
        return -1;
    }
    if (!((double)F * h * w < 2147483648.0)) {
        durf_set_error("%s: requirement failed: F h w < 2^31 pixels, F = %d, h = %d, w = %d", who, F, h, w);
        return -1;
    }
    return 0;
}

int check_raster_ws(const char* who, const void* workspace, size_t workspace_bytes, const RasterDims& D, RasterWs* ws) {
    if (workspace == nullptr || ((size_t)workspace & 255) != 0) {
        durf_set_error("%s: requirement failed: workspace aligned to 256 bytes", who);
        return -1;
    }
    *ws = carve_raster((void*)workspace, D);
    return durf::check_workspace(who, workspace_bytes, ws->total, "durf_raster_workspace_bytes(%d, %d, %d, %d)", D.F, D.T, D.h, D.w);
}

int check_setup_view(const char* who, int F, const float* cams, float znear, int cull) {
    if (!(znear >= FLT_MIN)) { durf_set_error("%s: requirement failed: znear > 0 (a normal float), znear = %g", who, (double)znear); return -1; }
    if (!(cull >= 0 && cull <= 2)) { durf_set_error("%s: requirement failed: cull in 0 .. 2, cull = %d", who, cull); return -1; }
    if (!(cams || F == 0)) { durf_set_error("%s: requirement failed: cams_dev for F = %d", who, F); return -1; }
    return 0;
}

int check_setup_args(const char* who, int F, const float* cams, int V, int T, const float* vertices, const int32_t* triangles,
                     float znear, int cull, const int32_t* counts) {
    if (check_mesh(who, V, T, check_setup_view(who, F, cams, znear, cull), vertices, triangles) != 0) return -1;
    if (!counts) { durf_set_error("%s: requirement failed: counts", who); return -1; }
    return 0;
}

int check_draw_args(const char* who, int F, const int32_t* pairs, int max_pairs, const int32_t* tri, const float* depth) {
    if (!(max_pairs >= 0)) { durf_set_error("%s: requirement failed: 0 <= max_pairs < 2^31, max_pairs = %d", who, max_pairs); return -1; }
    if (!(pairs || max_pairs == 0)) { durf_set_error("%s: requirement failed: pairs for max_pairs = %d", who, max_pairs); return -1; }
    if (!((tri && depth) || F == 0)) { durf_set_error("%s: requirement failed: tri and depth for F = %d", who, F); return -1; }
    return 0;
}

int check_interp_args(const char* who, int n_pixels, int V, int T, const int32_t* triangles, const int32_t* tri, const float* bary, int C,
                      const float* attr_f, const float* out_f, const int32_t* attr_i, const int32_t* out_i) {
    if (!(n_pixels >= 0 && V >= 0 && T >= 0)) {
        durf_set_error("%s: requirement failed: n_pixels, V, T >= 0, n_pixels = %d, V = %d, T = %d", who, n_pixels, V, T);
        return -1;
    }
    if (!(attr_f || attr_i)) { durf_set_error("%s: requirement failed: attr_f or attr_i", who); return -1; }
    if (attr_f && !(out_f && bary)) { durf_set_error("%s: requirement failed: out_f and bary with attr_f", who); return -1; }
    if (attr_f && !(C >= 1)) { durf_set_error("%s: requirement failed: C >= 1, C = %d", who, C); return -1; }
    if (attr_i && !out_i) { durf_set_error("%s: requirement failed: out_i with attr_i", who); return -1; }
    if (!(tri || n_pixels == 0)) { durf_set_error("%s: requirement failed: tri for n_pixels = %d", who, n_pixels); return -1; }
    return check_mesh_triangles(who, T, triangles);
}

int launch_setup(hipStream_t s, const RasterDims& D, const RasterWs& w, const float* cams, int V, const float* vertices,
                 const int32_t* triangles, float znear, int cull, int32_t* counts) {
    const size_t ft = (size_t)D.F * D.T;
    hipLaunchKernelGGL(k_raster_clear, dim3(w.nb > 0 ? w.nb : 1), dim3(RB), 0, s, D.n_tiles, w.tile_count, counts);
    DURF_CHECK_LAUNCH("k_raster_clear");
    if (ft > 0) {
        hipLaunchKernelGGL(k_raster_setup, dim3(durf_cdiv(ft, RB)), dim3(RB), 0, s, D, cams, V, vertices, triangles, znear, cull, w.records,
                           w.tile_count, counts);
        DURF_CHECK_LAUNCH("k_raster_setup");
    }
    if (w.nb > 0) {
        hipLaunchKernelGGL(k_raster_sums, dim3(w.nb), dim3(RB), 0, s, D.n_tiles, w.tile_count, w.sums);
        DURF_CHECK_LAUNCH("k_raster_sums");
    }
    hipLaunchKernelGGL((k_scan_block_sums<i64, 1>), dim3(1), dim3(SCAN_THREADS), 0, s, w.nb, w.sums, w.grand);
    DURF_CHECK_LAUNCH("k_scan_block_sums<int64, 1>");
    hipLaunchKernelGGL(k_raster_offsets, dim3(w.nb > 0 ? w.nb : 1), dim3(RB), 0, s, D.n_tiles, w.tile_count, w.sums, w.grand, w.tile_start,
                       counts);
    DURF_CHECK_LAUNCH("k_raster_offsets");
    return 0;
}

int launch_draw(hipStream_t s, const RasterDims& D, const RasterWs& w, int32_t* pairs, int max_pairs, int32_t* tri, float* depth,
                float* bary) {
    if (D.n_tiles == 0) return 0;
    const size_t ft = (size_t)D.F * D.T;
    hipLaunchKernelGGL(k_raster_begin, dim3(w.nb), dim3(RB), 0, s, D.n_tiles, w.cursor);
    DURF_CHECK_LAUNCH("k_raster_begin");
    if (ft > 0) {
        hipLaunchKernelGGL(k_raster_fill, dim3(durf_cdiv(ft, RB)), dim3(RB), 0, s, D, w.records, w.tile_start, w.grand, w.cursor, pairs,
                           max_pairs);
        DURF_CHECK_LAUNCH("k_raster_fill");
    }
    hipLaunchKernelGGL(k_raster_tile, dim3(D.n_tiles), dim3(RTILE * RTILE), 0, s, D, w.records, w.tile_count, w.tile_start, w.grand, pairs,
                       max_pairs, tri, depth, bary);
    DURF_CHECK_LAUNCH("k_raster_tile");
    return 0;
}

int launch_interp(hipStream_t s, int n_pixels, int V, int T, const int32_t* triangles, const int32_t* tri, const float* bary, int C,
                  const float* attr_f, float* out_f, const int32_t* attr_i, int fill, int32_t* out_i) {
    if (n_pixels == 0) return 0;
    hipLaunchKernelGGL(k_raster_interp, dim3(durf_cdiv((size_t)n_pixels, RB)), dim3(RB), 0, s, n_pixels, V, T, triangles, tri, bary, C, attr_f,
                       attr_f ? out_f : nullptr, attr_i, fill, attr_i ? out_i : nullptr);
    DURF_CHECK_LAUNCH("k_raster_interp");
    return 0;
}

}  // namespace

extern "C" {

size_t durf_raster_workspace_bytes(int F, int T, int h, int w) {
    if (!raster_shape_ok(F, T, h, w)) return 0;
    return carve_raster(nullptr, raster_dims(F, T, h, w)).total;
}

int durf_raster_setup(void* stream, int F, int h, int w, const float* cams_dev, int V, int T, const float* vertices,
                      const int32_t* triangles, float znear, int cull, void* workspace, size_t workspace_bytes, int32_t* counts) {
    if (check_raster_shape(__func__, F, T, h, w) != 0) return -1;
    if (check_setup_args(__func__, F, cams_dev, V, T, vertices, triangles, znear, cull, counts) != 0) return -1;
    const RasterDims D = raster_dims(F, T, h, w);
    RasterWs ws;
    if (check_raster_ws(__func__, workspace, workspace_bytes, D, &ws) != 0) return -1;
    return launch_setup((hipStream_t)stream, D, ws, cams_dev, V, vertices, triangles, znear, cull, counts);
}

int durf_raster_draw(void* stream, int F, int T, int h, int w, const void* workspace, size_t workspace_bytes, int32_t* pairs,
                     int max_pairs, int32_t* tri, float* depth, float* bary) {
    if (check_raster_shape(__func__, F, T, h, w) != 0) return -1;
    if (check_draw_args(__func__, F, pairs, max_pairs, tri, depth) != 0) return -1;
    const RasterDims D = raster_dims(F, T, h, w);
    RasterWs ws;
    if (check_raster_ws(__func__, workspace, workspace_bytes, D, &ws) != 0) return -1;
    return launch_draw((hipStream_t)stream, D, ws, pairs, max_pairs, tri, depth, bary);
}

int durf_raster_interp(void* stream, int n_pixels, int V, int T, const int32_t* triangles, const int32_t* tri, const float* bary, int C,
                       const float* attr_f, float* out_f, const int32_t* attr_i, int fill, int32_t* out_i) {
    if (check_interp_args(__func__, n_pixels, V, T, triangles, tri, bary, C, attr_f, out_f, attr_i, out_i) != 0) return -1;
    return launch_interp((hipStream_t)stream, n_pixels, V, T, triangles, tri, bary, C, attr_f, out_f, attr_i, fill, out_i);
}

int durf_render_mesh(void* stream, int F, int h, int w, const float* cams_dev, int V, int T, const float* vertices,
                     const int32_t* triangles, float znear, int cull, void* workspace, size_t workspace_bytes, int32_t* pairs,
                     int max_pairs, int32_t* counts, int32_t* tri, float* depth, float* bary, int C, const float* attr_f, float* out_f,
                     const int32_t* attr_i, int fill, int32_t* out_i) {
    if (check_raster_shape(__func__, F, T, h, w) != 0) return -1;
    if (check_setup_args(__func__, F, cams_dev, V, T, vertices, triangles, znear, cull, counts) != 0) return -1;
    if (check_draw_args(__func__, F, pairs, max_pairs, tri, depth) != 0) return -1;
    const bool interp = attr_f || attr_i;
    const int n_pixels = F * h * w;
    if (interp && check_interp_args(__func__, n_pixels, V, T, triangles, tri, bary, C, attr_f, out_f, attr_i, out_i) != 0) return -1;
    const RasterDims D = raster_dims(F, T, h, w);
    RasterWs ws;
    if (check_raster_ws(__func__, workspace, workspace_bytes, D, &ws) != 0) return -1;
    const hipStream_t s = (hipStream_t)stream;
    int rc = launch_setup(s, D, ws, cams_dev, V, vertices, triangles, znear, cull, counts);
    if (rc == 0) rc = launch_draw(s, D, ws, pairs, max_pairs, tri, depth, bary);
    if (rc == 0 && interp) rc = launch_interp(s, n_pixels, V, T, triangles, tri, bary, C, attr_f, out_f, attr_i, fill, out_i);
    return rc;
}

}  // extern "C"
