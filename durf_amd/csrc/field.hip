// The field at world points (include/durf_field.h; libdurf_field.so): which box a point lies in and the point in that box's
// frame (k_field_poses, k_field_classify), ordered lists per owner (k_field_lists, k_field_owned), the two encodings of a
// point's isotropic Gaussian as fp32 rows (k_field_encode, on the device bodies of gauss.h and enc_lane.h), the merge rule and
// the compositor's activations (k_field_activate), grid points (k_field_grid_points) and the top-down column map
// (k_field_columns); durf_field_query walks n points in chunks through these and the exact-fp32 MLP entries of
// libdurf_hip.so.  Streaming kernels, plain fp32 in the order the header states; no atomics, nothing synchronises or copies to
// the host.
#include "workspace.h"
#include "lattice.h"
#include "aa2matrix.h"
#include "enc_lane.h"
#include "loss_common.h"
#include "../../include/durf_field.h"

#define FIELD_THREADS 256
#define FIELD_LIST_THREADS 1024
#define FIELD_LIST_WAVES (FIELD_LIST_THREADS / DURF_WAVE)

// ---- which box ----------------------------------------------------------------------------------------------------------------
// one wave: thread k turns pose k into its row of the table
__global__ void __launch_bounds__(64)
k_field_poses(int K, const float* __restrict__ pose, float* __restrict__ table) {
    const int k = threadIdx.x;
    if (k >= K) return;
    pose_row_fill(pose + k * 6, table + k * DURF_POSE_ROW);          // k < K: inside DURF_FIELD_POSE_FLOATS(K)
}

// one thread per point; the box loop runs over k, the same in every lane, so the table and the extents are read at
// wave-uniform addresses and no lane's arithmetic depends on which points share its wave
__global__ void __launch_bounds__(FIELD_THREADS)
k_field_classify(int n, const float* __restrict__ points, int K, const float* __restrict__ table, const float* __restrict__ ext,
                 const int32_t* __restrict__ enable, float inside_tol, int32_t* __restrict__ owner, float* __restrict__ local) {
    const int i = blockIdx.x * FIELD_THREADS + threadIdx.x;
    if (i >= n) return;
    const size_t r = (size_t)i;
    const float X0 = points[r * 3 + 0], X1 = points[r * 3 + 1], X2 = points[r * 3 + 2];
    float L0 = X0, L1 = X1, L2 = X2;
    int nin = 0, own = -1;
    const float grow = 1.0f + inside_tol;
    for (int k = 0; k < K; k++) {
        if (enable && enable[k] == 0) continue;      // (uniform)
        float P[3];
        pose_to_box(table + k * DURF_POSE_ROW, X0, X1, X2, P);
        const bool in = fabsf(P[0]) <= ext[k * 3 + 0] * grow && fabsf(P[1]) <= ext[k * 3 + 1] * grow &&
                        fabsf(P[2]) <= ext[k * 3 + 2] * grow;
        if (in) { nin++; own = k; L0 = P[0]; L1 = P[1]; L2 = P[2]; }
    }
    if (nin > 1) { own = -2; L0 = X0; L1 = X1; L2 = X2; }
    owner[r] = own;
    local[r * 3 + 0] = L0; local[r * 3 + 1] = L1; local[r * 3 + 2] = L2;
}

// ---- lists --------------------------------------------------------------------------------------------------------------------
// workgroup c compacts the points of owner c (c == K: owner -1) in ascending order: per round of FIELD_LIST_THREADS points a
// ballot per wave, the waves' counts through LDS, a running base carried in a register of every thread
__global__ void __launch_bounds__(FIELD_LIST_THREADS)
k_field_lists(int n, int K, const int32_t* __restrict__ owner, int32_t* __restrict__ idx, int32_t* __restrict__ count) {
    __shared__ int s_wave[2][FIELD_LIST_WAVES];
    const int c = blockIdx.x, want = c < K ? c : -1;
    const int t = threadIdx.x, lane = t & (DURF_WAVE - 1), wave = t / DURF_WAVE;
    int32_t* out = idx + (size_t)c * n;
    int base = 0, round = 0;
    for (int i0 = 0; i0 < n; i0 += FIELD_LIST_THREADS, round ^= 1) {
        const int i = i0 + t;
        const bool v = i < n && owner[i] == want;
        const unsigned long long m = __ballot(v);
        if (lane == 0) s_wave[round][wave] = __popcll(m);
        __syncthreads();                               // (the two buffers alternate: one barrier per round is enough)
        int before = 0, total = 0;
#pragma unroll
        for (int u = 0; u < FIELD_LIST_WAVES; u++) {
            const int cu = s_wave[round][u];
            before += u < wave ? cu : 0;
            total += cu;
        }
        // base + before + rank < base + total <= the points seen so far <= n: inside list c's n slots
        if (v) out[base + before + __popcll(m & ((1ull << lane) - 1ull))] = i;
        base += total;
    }
    if (t == 0) count[c] = base;
}

// a device count as a loop bound: never beyond the n slots of its list
__device__ __forceinline__ int field_count(const int32_t* count, int c, int n) {
    const int v = count[c];
    return v < 0 ? 0 : (v > n ? n : v);
}

// the rows of lists 0 .. c-1
__device__ __forceinline__ int field_offset(const int32_t* count, int c, int n) {
    int off = 0;
    for (int u = 0; u < c; u++) off += field_count(count, u, n);
    return off;
}

__global__ void __launch_bounds__(FIELD_THREADS)
k_field_owned(int n, int K, const int32_t* __restrict__ idx, const int32_t* __restrict__ count, int32_t* __restrict__ owned,
              int32_t* __restrict__ owned_count) {
    const int c = blockIdx.y, r = blockIdx.x * FIELD_THREADS + threadIdx.x;
    if (c == 0 && r == 0) {
        const int tot = field_offset(count, K, n);
        *owned_count = tot > n ? n : tot;
    }
    if (r >= field_count(count, c, n)) return;
    const int at = field_offset(count, c, n) + r;
    if (at < n) owned[at] = idx[(size_t)c * n + r];
}

// ---- encodings ----------------------------------------------------------------------------------------------------------------
// thread = (row, 8-feature vector): eight lanes per row, so a wave stores eight consecutive rows; blockIdx.y = box (OBJ)
template <bool OBJ>
__global__ void __launch_bounds__(FIELD_THREADS)
k_field_encode(int n, int c0, const float* __restrict__ pts, const int32_t* __restrict__ idx, const int32_t* __restrict__ count,
               float var, int flags, BarfW barf_w, float* __restrict__ enc) {
    constexpr int DIM = OBJ ? DURF_FIELD_ENC_OBJ : DURF_FIELD_ENC_BKGD;
    const int c = c0 + blockIdx.y;
    const size_t gid = (size_t)blockIdx.x * FIELD_THREADS + threadIdx.x;
    const size_t r = gid >> 3;
    const int q = (int)(gid & 7);
    if (r >= (size_t)field_count(count, c, n)) return;
    const int i = idx[(size_t)c * n + r];
    if (i < 0 || i >= n) return;
    Gauss g;
#pragma unroll
    for (int j = 0; j < 3; j++) { g.x[j] = pts[(size_t)i * 3 + j]; g.var[j] = var; }
    float* row = enc + ((size_t)blockIdx.y * n + r) * DIM;        // r < n: inside this box's (or the background's) n rows
    if (OBJ) {
        float v[8];
        obj_features8(g, barf_w, q, v);
#pragma unroll
        for (int e = 0; e < 8; e++)
            if (q * 8 + e < DIM) row[q * 8 + e] = v[e];
    } else {
        if (flags & DURF_ENC_CONTRACT) contract_gaussian(g);
#pragma unroll
        for (int e = 0; e < 8; e++) {
            const int p = q * 8 + e;
            if (p < DIM) row[p] = ipe_feature(g, p);
        }
    }
}

// ---- merge + activations ------------------------------------------------------------------------------------------------------
// blockIdx.y = c: a list (c <= K; thread = its row) or (c == K + 1; thread = point) the multi-owner points
__global__ void __launch_bounds__(FIELD_THREADS)
k_field_activate(int n, int K, const int32_t* __restrict__ idx, const int32_t* __restrict__ count, const float* __restrict__ raw_bkgd,
                 const float* __restrict__ raw_obj, const float* __restrict__ raw_const, const int32_t* __restrict__ owner,
                 float density_bias, float* __restrict__ density, float* __restrict__ rgb, float* __restrict__ raw,
                 uint8_t* __restrict__ valid) {
    const int c = blockIdx.y, r = blockIdx.x * FIELD_THREADS + threadIdx.x;
    if (r >= n) return;
    int i;
    float m[4];
    bool ok = true;
    if (c == K + 1) {
        if (owner[r] != -2) return;
        i = r;
        ok = false;
        m[0] = m[1] = m[2] = m[3] = __builtin_nanf("");
    } else {
        if (r >= field_count(count, c, n)) return;
        i = idx[(size_t)c * n + r];
        if (i < 0 || i >= n) return;
        if (c == K) {
            const f32x4 b = *(const f32x4*)(raw_bkgd + (size_t)r * 4);
            m[0] = b[0]; m[1] = b[1]; m[2] = b[2]; m[3] = b[3];
        } else {
            const int at = field_offset(count, c, n) + r;
            if (at >= n) return;
            const f32x4 o = *(const f32x4*)(raw_obj + ((size_t)c * n + r) * 4);
            const f32x4 k = *(const f32x4*)(raw_const + (size_t)at * 4);
            m[0] = k[0] + o[0]; m[1] = k[1] + o[1]; m[2] = k[2] + o[2]; m[3] = k[3] + o[3];
        }
    }
    const size_t p = (size_t)i;
    density[p] = ok ? softplusf_(m[3] + density_bias) : m[3];
    if (rgb) {
#pragma unroll
        for (int q = 0; q < 3; q++) rgb[p * 3 + q] = ok ? sigmoidf_(m[q]) : m[q];
    }
    if (raw) {
#pragma unroll
        for (int q = 0; q < 4; q++) raw[p * 4 + q] = m[q];
    }
    valid[p] = ok ? 1 : 0;
}

// ---- grids --------------------------------------------------------------------------------------------------------------------

__global__ void __launch_bounds__(FIELD_THREADS)
k_field_grid_points(int m, int first, const LatticeDims D, const LatticeFrame F, float* __restrict__ pts, float* __restrict__ points_out) {
    const int t = blockIdx.x * FIELD_THREADS + threadIdx.x;
    if (t >= m) return;
    const int g = first + t;                                                 // nu nv nw < 2^31
    int i, j, k;
    lattice_ijk(D, g, i, j, k);
    float P[3];
    lattice_point(F, (float)i, (float)j, (float)k, P);
#pragma unroll
    for (int c = 0; c < 3; c++) {
        pts[(size_t)t * 3 + c] = P[c];
        if (points_out) points_out[(size_t)g * 3 + c] = P[c];
    }
}

__global__ void __launch_bounds__(FIELD_THREADS)
k_field_columns(int ncol, int nw, const float* __restrict__ density, const uint8_t* __restrict__ valid, float step, float threshold,
                float* __restrict__ col_max, float* __restrict__ col_opacity, int32_t* __restrict__ col_first) {
    const int col = blockIdx.x * FIELD_THREADS + threadIdx.x;
    if (col >= ncol) return;
    const size_t base = (size_t)col * nw;
    float mx = __builtin_nanf(""), s = 0.0f;
    int first = -1;
    bool any = false;
    for (int k = 0; k < nw; k++) {
        const float d = density[base + k];
        if (valid[base + k] == 0 || d != d) continue;
        mx = any ? fmaxf(mx, d) : d;
        any = true;
        s += d;
        if (first < 0 && d >= threshold) first = k;
    }
    if (col_max) col_max[col] = mx;
    if (col_opacity) col_opacity[col] = 1.0f - expf(-(step * s));
    if (col_first) col_first[col] = first;
}

// ---- launchers and the one-call walk ------------------------------------------------------------------------------------------
namespace {

int check_field_K(const char* who, int n, int K) {
    if (!(n >= 0 && n < (1 << 27))) {
        durf_set_error("%s: requirement failed: 0 <= n < 2^27 points per call, n = %d", who, n);
        return -1;
    }
    if (!(K >= 0 && K <= DURF_MAX_OBJ)) {
        durf_set_error("%s: requirement failed: 0 <= K <= DURF_MAX_OBJ (%d), K = %d", who, DURF_MAX_OBJ, K);
        return -1;
    }
    return 0;
}

struct FieldWs {
    float *pts, *local, *table, *enc_b, *enc_o, *view3, *view27, *raw_b, *raw_o, *raw_c, *density;
    int32_t *owner, *idx, *count, *owned, *owned_count;
    uint8_t* valid;
    size_t total;
};

FieldWs carve_field(void* base, int chunk, int K) {
    durf::Carver c{(char*)base, 0};
    FieldWs w{};
    const size_t B = chunk > 0 ? chunk : 0, Kc = K > 0 ? K : 0;
    w.pts = (float*)c.take(B * 3 * 4);
    w.local = (float*)c.take(B * 3 * 4);
    w.owner = (int32_t*)c.take(B * 4);
    w.table = (float*)c.take((size_t)DURF_FIELD_POSE_FLOATS(Kc ? Kc : 1) * 4);
    w.idx = (int32_t*)c.take((Kc + 1) * B * 4);
    w.count = (int32_t*)c.take((Kc + 1) * 4);
    w.owned = (int32_t*)c.take(B * 4);
    w.owned_count = (int32_t*)c.take(4);
    w.enc_b = (float*)c.take(B * DURF_FIELD_ENC_BKGD * 4);
    w.enc_o = (float*)c.take(Kc * B * DURF_FIELD_ENC_OBJ * 4);
    w.view3 = (float*)c.take(B * 3 * 4);
    w.view27 = (float*)c.take(B * 27 * 4);
    w.raw_b = (float*)c.take(B * 4 * 4);
    w.raw_o = (float*)c.take(Kc * B * 4 * 4);
    w.raw_c = (float*)c.take(B * 4 * 4);
    w.valid = (uint8_t*)c.take(B);
    w.total = c.total();
    return w;
}

int check_field_args(const char* who, const durf_field_args* a, int n, int chunk, bool grid) {
    if (!a) { durf_set_error("%s: requirement failed: arguments", who); return -1; }
    int rc = check_field_K(who, 0, a->K);
    if (rc != 0) return rc;
    const char* bad = nullptr;
    if (!(n >= 0)) bad = "n >= 0";
    else if (!(chunk > 0 && chunk < (1 << 27))) bad = "0 < chunk < 2^27";
    else if (!(a->sigma >= 0.0f)) bad = "sigma >= 0";
    else if (!(a->inside_tol >= 0.0f)) bad = "inside_tol >= 0";
    else if (a->enc_flags & ~DURF_ENC_CONTRACT) bad = "enc_flags is 0 or DURF_ENC_CONTRACT";
    else if (!(a->bkgd_params && a->bkgd_wstream)) bad = "bkgd_params and bkgd_wstream";
    else if (a->K > 0 && !(a->obj_params && a->obj_wstream && a->const_trunk && a->pose && a->ext))
        bad = "obj_params, obj_wstream, const_trunk, pose and ext for K > 0";
    else if (n > 0 && !a->density) bad = "the density output";
    else if (!grid && n > 0 && !a->points) bad = "points";
    else if (!grid && a->rgb && !a->viewdirs) bad = "rgb needs viewdirs (viewdirs == NULL is a density-only query)";
    if (bad) {
        durf_set_error("%s: requirement failed: %s (n = %d, chunk = %d, K = %d, sigma = %g, inside_tol = %g, enc_flags = %d)", who, bad,
                       n, chunk, a->K, (double)a->sigma, (double)a->inside_tol, a->enc_flags);
        return -1;
    }
    return 0;
}

int launch_encode(void* stream, int n, int K, const float* pts, const int32_t* idx, const int32_t* count, float sigma, int flags,
                  const float* barf_w, float* enc_bkgd, float* enc_obj) {
    const float var = sigma * sigma;
    const dim3 grid(durf_cdiv((size_t)n * 8, FIELD_THREADS));
    BarfW w{};
    if (enc_bkgd) {
        hipLaunchKernelGGL(k_field_encode<false>, grid, dim3(FIELD_THREADS), 0, (hipStream_t)stream, n, K, pts, idx, count, var, flags, w,
                           enc_bkgd);
        DURF_CHECK_LAUNCH("k_field_encode<bkgd>");
    }
    if (enc_obj && K > 0) {
        for (int i = 0; i < 10; i++) w.w[i] = barf_w[i];
        hipLaunchKernelGGL(k_field_encode<true>, dim3(grid.x, K), dim3(FIELD_THREADS), 0, (hipStream_t)stream, n, 0, pts, idx, count, var,
                           flags, w, enc_obj);
        DURF_CHECK_LAUNCH("k_field_encode<obj>");
    }
    return 0;
}

// one chunk of B points that lie at `pts` (device); view27: B rows; outputs at the chunk's offset
int field_chunk(void* stream, const durf_field_args* a, const FieldWs& w, int B, const float* pts, const float* view27, float* density,
                float* rgb, float* raw, int32_t* owner, uint8_t* valid) {
    const int K = a->K;
    int32_t* own = owner ? owner : w.owner;
    int rc = durf_field_classify(stream, B, pts, K, a->pose, a->ext, a->box_enable, a->inside_tol, w.table, own, w.local);
    if (rc != 0) return rc;
    if ((rc = durf_field_lists(stream, B, K, own, w.idx, w.count)) != 0) return rc;
    if ((rc = launch_encode(stream, B, K, w.local, w.idx, w.count, a->sigma, a->enc_flags, a->barf_w, w.enc_b, w.enc_o)) != 0) return rc;
    rc = durf_mlp_fwd_f32(stream, DURF_W_BKGD, DURF_FIELD_ENC_BKGD, (size_t)B, 1, w.enc_b, view27, w.idx + (size_t)K * B, w.count + K,
                          a->bkgd_params, a->bkgd_wstream, w.raw_b, nullptr);
    if (rc != 0) return rc;
    if (K > 0) {
        if ((rc = durf_field_owned(stream, B, K, w.idx, w.count, w.owned, w.owned_count)) != 0) return rc;
        rc = durf_objf32_fwd_batch(stream, K, B, 1, w.idx, w.count, w.enc_o, view27, a->obj_params, a->param_stride, a->obj_wstream,
                                   w.raw_o, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0);
        if (rc != 0) return rc;
        rc = durf_bkgd_hit_rays_f32(stream, B, view27, a->bkgd_params, w.owned, w.owned_count, a->const_trunk, w.raw_c);
        if (rc != 0) return rc;
    }
    return durf_field_activate(stream, B, K, w.idx, w.count, w.raw_b, w.raw_o, w.raw_c, own, a->density_bias, density, rgb, raw,
                               valid ? valid : w.valid);
}

}  // namespace

extern "C" {

int durf_field_classify(void* stream, int n, const float* points, int K, const float* pose, const float* ext, const int32_t* box_enable,
                        float inside_tol, float* pose_scratch, int32_t* owner, float* local) {
    int rc = check_field_K(__func__, n, K);
    if (rc != 0) return rc;
    DURF_REQUIREF(inside_tol >= 0.0f, "inside_tol >= 0, inside_tol = %g", (double)inside_tol);
    if (n == 0) return 0;
    DURF_REQUIREF(points && owner && local, "points, owner and local");
    DURF_REQUIREF(K == 0 || (pose && ext && pose_scratch), "pose, ext and pose_scratch for K = %d", K);
    if (K > 0) {
        hipLaunchKernelGGL(k_field_poses, dim3(1), dim3(64), 0, (hipStream_t)stream, K, pose, pose_scratch);
        DURF_CHECK_LAUNCH("k_field_poses");
    }
    hipLaunchKernelGGL(k_field_classify, dim3(durf_cdiv(n, FIELD_THREADS)), dim3(FIELD_THREADS), 0, (hipStream_t)stream, n, points, K,
                       pose_scratch, ext, box_enable, inside_tol, owner, local);
    DURF_CHECK_LAUNCH("k_field_classify");
    return 0;
}

int durf_field_lists(void* stream, int n, int K, const int32_t* owner, int32_t* idx, int32_t* count) {
    int rc = check_field_K(__func__, n, K);
    if (rc != 0) return rc;
    if (n == 0) return 0;
    DURF_REQUIREF(owner && idx && count, "owner, idx and count");
    hipLaunchKernelGGL(k_field_lists, dim3(K + 1), dim3(FIELD_LIST_THREADS), 0, (hipStream_t)stream, n, K, owner, idx, count);
    DURF_CHECK_LAUNCH("k_field_lists");
    return 0;
}

int durf_field_owned(void* stream, int n, int K, const int32_t* idx, const int32_t* count, int32_t* owned, int32_t* owned_count) {
    int rc = check_field_K(__func__, n, K);
    if (rc != 0) return rc;
    if (n == 0 || K == 0) return 0;
    DURF_REQUIREF(idx && count && owned && owned_count, "idx, count, owned and owned_count");
    hipLaunchKernelGGL(k_field_owned, dim3(durf_cdiv(n, FIELD_THREADS), K), dim3(FIELD_THREADS), 0, (hipStream_t)stream, n, K, idx, count,
                       owned, owned_count);
    DURF_CHECK_LAUNCH("k_field_owned");
    return 0;
}

int durf_field_encode(void* stream, int n, int K, const float* points_or_local, const int32_t* idx, const int32_t* count, float sigma,
                      int enc_flags, const float* barf_w, float* enc_bkgd, float* enc_obj) {
    int rc = check_field_K(__func__, n, K);
    if (rc != 0) return rc;
    DURF_REQUIREF(sigma >= 0.0f, "sigma >= 0, sigma = %g", (double)sigma);
    DURF_REQUIREF((enc_flags & ~DURF_ENC_CONTRACT) == 0, "enc_flags is 0 or DURF_ENC_CONTRACT, enc_flags = %d", enc_flags);
    if (n == 0) return 0;
    DURF_REQUIREF(points_or_local && idx && count, "points_or_local, idx and count");
    DURF_REQUIREF(enc_bkgd || enc_obj, "at least one output");
    DURF_REQUIREF(!(enc_obj && K > 0) || barf_w, "barf_w for the object rows");
    return launch_encode(stream, n, K, points_or_local, idx, count, sigma, enc_flags, barf_w, enc_bkgd, enc_obj);
}

int durf_field_activate(void* stream, int n, int K, const int32_t* idx, const int32_t* count, const float* raw_bkgd, const float* raw_obj,
                        const float* raw_const, const int32_t* owner, float density_bias, float* density, float* rgb, float* raw,
                        uint8_t* valid) {
    int rc = check_field_K(__func__, n, K);
    if (rc != 0) return rc;
    if (n == 0) return 0;
    DURF_REQUIREF(idx && count && raw_bkgd && owner && density && valid, "idx, count, raw_bkgd, owner, density and valid");
    DURF_REQUIREF(K == 0 || (raw_obj && raw_const), "raw_obj and raw_const for K = %d", K);
    DURF_REQUIREF((((size_t)raw_bkgd | (size_t)raw_obj | (size_t)raw_const) & 15) == 0, "the raw inputs are 16-byte aligned");
    hipLaunchKernelGGL(k_field_activate, dim3(durf_cdiv(n, FIELD_THREADS), K + 2), dim3(FIELD_THREADS), 0, (hipStream_t)stream, n, K, idx,
                       count, raw_bkgd, raw_obj, raw_const, owner, density_bias, density, rgb, raw, valid);
    DURF_CHECK_LAUNCH("k_field_activate");
    return 0;
}

size_t durf_field_workspace_bytes(int chunk, int K) { return carve_field(nullptr, chunk, K).total; }

int durf_field_query(void* stream, const durf_field_args* a, int n, int chunk, void* workspace, size_t workspace_bytes) {
    int rc = check_field_args(__func__, a, n, chunk, false);
    if (rc != 0) return rc;
    if (n == 0) return 0;
    if (durf::check_workspace_aligned(__func__, workspace) != 0) return -1;
    const FieldWs w = carve_field(workspace, chunk, a->K);
    rc = durf::check_workspace("durf_field_query", workspace_bytes, w.total, "durf_field_workspace_bytes(%d, %d)", chunk, a->K);
    if (rc != 0) return rc;
    if (!a->viewdirs && hipMemsetAsync(w.view27, 0, (size_t)(n < chunk ? n : chunk) * 27 * 4, (hipStream_t)stream) != hipSuccess) {
        durf_set_error("durf_field_query: clearing the view rows failed");
        return -1;
    }
    for (size_t i = 0; i < (size_t)n; i += (size_t)chunk) {
        const int B = (int)((size_t)n - i < (size_t)chunk ? (size_t)n - i : (size_t)chunk);
        if (a->viewdirs && (rc = durf_view_enc(stream, B, a->viewdirs + i * 3, nullptr, w.view27)) != 0) return rc;
        rc = field_chunk(stream, a, w, B, a->points + i * 3, w.view27, a->density + i, a->rgb ? a->rgb + i * 3 : nullptr,
                         a->raw ? a->raw + i * 4 : nullptr, a->owner ? a->owner + i : nullptr, a->valid ? a->valid + i : nullptr);
        if (rc != 0) return rc;
    }
    return 0;
}

int durf_field_grid(void* stream, const durf_field_args* a, const float* origin_host, const float* du_host, const float* dv_host,
                    const float* dw_host, int nu, int nv, int nw, int has_view, float view_x, float view_y, float view_z, int chunk,
                    void* workspace, size_t workspace_bytes, float* points_out) {
    DURF_REQUIREF(nu >= 1 && nv >= 1 && nw >= 1 && nu <= (1 << 24) && nv <= (1 << 24) && nw <= (1 << 24),
                  "1 <= nu, nv, nw <= 2^24, nu = %d, nv = %d, nw = %d", nu, nv, nw);
    const long long total = (long long)nu * nv * nw;
    DURF_REQUIREF((double)nu * nv * nw < 2147483648.0, "nu nv nw < 2^31, nu = %d, nv = %d, nw = %d", nu, nv, nw);
    int rc = check_field_args(__func__, a, (int)total, chunk, true);
    if (rc != 0) return rc;
    DURF_REQUIREF(origin_host && du_host && dv_host && dw_host, "origin, du, dv and dw");
    DURF_REQUIREF(has_view || !a->rgb, "rgb needs a view direction (has_view == 0 is a density-only query)");
    if (durf::check_workspace_aligned(__func__, workspace) != 0) return -1;
    const FieldWs w = carve_field(workspace, chunk, a->K);
    rc = durf::check_workspace("durf_field_grid", workspace_bytes, w.total, "durf_field_workspace_bytes(%d, %d)", chunk, a->K);
    if (rc != 0) return rc;
    const LatticeDims D{nu, nv, nw, (int)total};
    const LatticeFrame G = lattice_frame(origin_host, du_host, dv_host, dw_host);
    // the grid's one view direction as a chunk of view rows: durf_view_enc of `first` copies of it, once
    const int first = (int)(total < chunk ? total : (long long)chunk);
    if (has_view) {
        LatticeFrame V{};
        V.o[0] = view_x; V.o[1] = view_y; V.o[2] = view_z;       // steps of 0: every "grid point" is the view direction
        hipLaunchKernelGGL(k_field_grid_points, dim3(durf_cdiv(first, FIELD_THREADS)), dim3(FIELD_THREADS), 0, (hipStream_t)stream, first,
                           0, D, V, w.view3, (float*)nullptr);
        DURF_CHECK_LAUNCH("k_field_grid_points(view)");
        if ((rc = durf_view_enc(stream, first, w.view3, nullptr, w.view27)) != 0) return rc;
    } else if (hipMemsetAsync(w.view27, 0, (size_t)first * 27 * 4, (hipStream_t)stream) != hipSuccess) {
        durf_set_error("durf_field_grid: clearing the view rows failed");
        return -1;
    }
    for (long long i = 0; i < total; i += chunk) {
        const int B = (int)(total - i < chunk ? total - i : (long long)chunk);
        hipLaunchKernelGGL(k_field_grid_points, dim3(durf_cdiv(B, FIELD_THREADS)), dim3(FIELD_THREADS), 0, (hipStream_t)stream, B, (int)i, D,
                           G, w.pts, points_out);
        DURF_CHECK_LAUNCH("k_field_grid_points");
        rc = field_chunk(stream, a, w, B, w.pts, w.view27, a->density + i, a->rgb ? a->rgb + i * 3 : nullptr,
                         a->raw ? a->raw + i * 4 : nullptr, a->owner ? a->owner + i : nullptr, a->valid ? a->valid + i : nullptr);
        if (rc != 0) return rc;
    }
    return 0;
}

int durf_field_columns(void* stream, int nu, int nv, int nw, const float* density, const uint8_t* valid, float step, float threshold,
                       float* col_max, float* col_opacity, int32_t* col_first) {
    DURF_REQUIREF(nu >= 1 && nv >= 1 && nw >= 1 && (double)nu * nv * nw < 2147483648.0, "nu, nv, nw >= 1 and nu nv nw < 2^31, %d x %d x %d",
                  nu, nv, nw);
    DURF_REQUIREF(step >= 0.0f, "step >= 0, step = %g", (double)step);
    DURF_REQUIREF(density && valid, "density and valid");
    DURF_REQUIREF(col_max || col_opacity || col_first, "at least one output");
    const int ncol = nu * nv;
    hipLaunchKernelGGL(k_field_columns, dim3(durf_cdiv(ncol, FIELD_THREADS)), dim3(FIELD_THREADS), 0, (hipStream_t)stream, ncol, nw, density,
                       valid, step, threshold, col_max, col_opacity, col_first);
    DURF_CHECK_LAUNCH("k_field_columns");
    return 0;
}

}  // extern "C"
