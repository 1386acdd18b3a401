// The evaluation loop's metrics on the device (notebooks/render_eval_durf.ipynb; train_boxpose.py:535-575): MSE,
// PSNR and SSIM of F rendered frames against their ground truth, the object PSNR under a mask and the depth error against the
// LIDAR plane, as ONE record of DURF_EVAL_FLOATS floats per frame (include/durf_hip.h).  Two launches for any F: k_eval_tiles
// -- a workgroup per 32 x 32 pixels stages them and their 10-pixel SSIM halo in LDS once per channel, blurs the five moment
// planes along W then along H (fp32, as k_ssim does), and sums the tile's error terms in fp64 -- and k_eval_finish, one
// workgroup per frame that adds the tile records in tile order.  No atomics, no fences, nothing read back: every order is
// fixed, so a frame's record is bit-reproducible and does not depend on the frames beside it.
#include "durf_common.h"
#include <math.h>

#define EV_TILE 32                      // output pixels per workgroup and axis
#define EV_WIN 11                       // the reference's window (math.py:66 filter_size)
#define EV_HALO (EV_WIN - 1)
#define EV_STAGE (EV_TILE + EV_HALO)    // staged pixels per axis
#define EV_THREADS 256
// the fp64 partial sums of a tile, in this order: squared error, mask * squared error, mask, LIDAR returns, |depth error|,
// depth error^2, non-finite rgb elements, SSIM terms
#define EV_PART 8

struct EvWindow { float w[EV_WIN]; };   // the normalised 1-D Gaussian (math.py:96-100), by value in the kernarg segment

// the 256 lanes' values in a binary tree: the same order whatever the data
__device__ __forceinline__ double ev_block_sum(double v, double* red) {
    __syncthreads();
    red[threadIdx.x] = v;
    __syncthreads();
    for (int s = EV_THREADS / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    return red[0];
}

// grid (tiles x, tiles y, F).  The tile owns the pixels [y0, y0 + 32) x [x0, x0 + 32) and the SSIM outputs whose window STARTS
// there: output (y, x) reads the pixels [y, y + 10] x [x, x + 10], so the halo lies to the right and below.
__global__ void __launch_bounds__(EV_THREADS)
k_eval_tiles(int H, int W, EvWindow win, float c1, float c2, const float* __restrict__ rgb, const float* __restrict__ gt,
             const float* __restrict__ distance, const float* __restrict__ gt_depth, const float* __restrict__ obj_mask,
             double* __restrict__ part) {
    __shared__ float sa[EV_STAGE][EV_STAGE], sb[EV_STAGE][EV_STAGE];
    __shared__ float hz[5][EV_STAGE][EV_TILE];            // the five moment planes after the pass along W
    __shared__ double red[EV_THREADS];
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * EV_TILE, y0 = blockIdx.y * EV_TILE;
    const size_t hw = (size_t)H * W, f = blockIdx.z;
    const float* a_img = rgb + f * hw * 3;
    const float* b_img = gt + f * hw * 3;
    const int Ho = H - EV_HALO, Wo = W - EV_HALO;          // the 'valid' region
    double se = 0.0, sm = 0.0, mcount = 0.0, dcount = 0.0, dabs = 0.0, dsq = 0.0, bad = 0.0, ss = 0.0;

    // the planes: the tile's own pixels, once
    for (int i = tid; i < EV_TILE * EV_TILE; i += EV_THREADS) {
        const int gy = y0 + i / EV_TILE, gx = x0 + i % EV_TILE;
        if (gy >= H || gx >= W) continue;
        const size_t p = f * hw + (size_t)gy * W + gx;
        if (obj_mask) mcount += (double)obj_mask[p];
        if (gt_depth) {
            const float g = gt_depth[p];
            if (g > 0.0f) {
                const double e = (double)distance[p] - (double)g;
                dcount += 1.0;
                dabs += fabs(e);
                dsq += e * e;
            }
        }
    }

    for (int c = 0; c < 3; c++) {
        // stage the channel: tile + halo, zero outside the image (no output that counts reads a zero)
        for (int i = tid; i < EV_STAGE * EV_STAGE; i += EV_THREADS) {
            const int r = i / EV_STAGE, col = i % EV_STAGE;
            const int gy = y0 + r, gx = x0 + col;
            float a = 0.0f, b = 0.0f;
            if (gy < H && gx < W) {
                const size_t p = (size_t)gy * W + gx;
                a = a_img[p * 3 + c];
                b = b_img[p * 3 + c];
                if (r < EV_TILE && col < EV_TILE) {
                    const double d = (double)a - (double)b;
                    const double d2 = d * d;
                    se += d2;
                    if (obj_mask) sm += (double)obj_mask[f * hw + p] * d2;
                    if (!(fabsf(a) <= 3.4028234663852886e+38f)) bad += 1.0;
                }
            }
            sa[r][col] = a;
            sb[r][col] = b;
        }
        __syncthreads();
        // along W (math.py:112 filt_fn2): k_ssim's sequence of multiplies and adds
        for (int i = tid; i < EV_STAGE * EV_TILE; i += EV_THREADS) {
            const int r = i / EV_TILE, xo = i % EV_TILE;
            float r0 = 0.f, r1 = 0.f, r00 = 0.f, r11 = 0.f, r01 = 0.f;
#pragma unroll
            for (int k = 0; k < EV_WIN; k++) {
                const float w = win.w[EV_WIN - 1 - k], p = sa[r][xo + k], q = sb[r][xo + k];
                r0 += w * p; r1 += w * q; r00 += w * (p * p); r11 += w * (q * q); r01 += w * (p * q);
            }
            hz[0][r][xo] = r0; hz[1][r][xo] = r1; hz[2][r][xo] = r00; hz[3][r][xo] = r11; hz[4][r][xo] = r01;
        }
        __syncthreads();
        // along H (math.py:113 filt_fn1), then the SSIM term (:116-135)
        for (int i = tid; i < EV_TILE * EV_TILE; i += EV_THREADS) {
            const int yo = i / EV_TILE, xo = i % EV_TILE;
            if (y0 + yo >= Ho || x0 + xo >= Wo) continue;
            float m0 = 0.f, m1 = 0.f, s00 = 0.f, s11 = 0.f, s01 = 0.f;
#pragma unroll
            for (int k = 0; k < EV_WIN; k++) {
                const float g = win.w[EV_WIN - 1 - k];
                m0 += g * hz[0][yo + k][xo]; m1 += g * hz[1][yo + k][xo]; s00 += g * hz[2][yo + k][xo];
                s11 += g * hz[3][yo + k][xo]; s01 += g * hz[4][yo + k][xo];
            }
            const float mu00 = m0 * m0, mu11 = m1 * m1, mu01 = m0 * m1;
            const float v00 = fmaxf(0.0f, s00 - mu00), v11 = fmaxf(0.0f, s11 - mu11);
            float v01 = s01 - mu01;
            const float lim = sqrtf(v00 * v11);
            const float av = fminf(lim, fabsf(v01));
            // sign(v01) * min(lim, |v01|); a NaN covariance stays NaN (sign(NaN) is NaN in the reference)
            v01 = v01 > 0.0f ? av : (v01 < 0.0f ? -av : (v01 != v01 ? v01 : 0.0f));
            ss += (double)(((2.0f * mu01 + c1) * (2.0f * v01 + c2)) / ((mu00 + mu11 + c1) * (v00 + v11 + c2)));
        }
        __syncthreads();
    }

    se = ev_block_sum(se, red);
    sm = ev_block_sum(sm, red);
    mcount = ev_block_sum(mcount, red);
    dcount = ev_block_sum(dcount, red);
    dabs = ev_block_sum(dabs, red);
    dsq = ev_block_sum(dsq, red);
    bad = ev_block_sum(bad, red);
    ss = ev_block_sum(ss, red);
    if (tid == 0) {
        const size_t tile = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
        double* o = part + (f * ((size_t)gridDim.x * gridDim.y) + tile) * EV_PART;
        o[0] = se; o[1] = sm; o[2] = mcount; o[3] = dcount; o[4] = dabs; o[5] = dsq; o[6] = bad; o[7] = ss;
    }
}

__device__ __forceinline__ double ev_psnr(double mse) { return -10.0 / log(10.0) * log(mse); }

// one workgroup per frame: lane j < EV_PART adds partial sum j of the frame's tiles in tile order, lane 0 forms the record
__global__ void __launch_bounds__(64)
k_eval_finish(int H, int W, int tiles, int have_depth, int have_mask, const double* __restrict__ part, float* __restrict__ metrics) {
    __shared__ double tot[EV_PART];
    const size_t f = blockIdx.x;
    if (threadIdx.x < EV_PART) {
        const double* p = part + f * (size_t)tiles * EV_PART + threadIdx.x;
        double s = 0.0;
        for (int t = 0; t < tiles; t++) s += p[(size_t)t * EV_PART];
        tot[threadIdx.x] = s;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    const float nanf_ = __builtin_nanf("");
    float* o = metrics + f * DURF_EVAL_FLOATS;
    const double mse = tot[0] / ((double)H * W * 3.0);
    o[DURF_EVAL_MSE] = (float)mse;
    o[DURF_EVAL_PSNR] = (float)ev_psnr(mse);
    o[DURF_EVAL_SSIM] = (float)(tot[7] / ((double)(H - EV_HALO) * (W - EV_HALO) * 3.0));
    if (have_mask) {
        const double omse = tot[1] / tot[2];                  // 0 / 0 = NaN: no object in the frame
        o[DURF_EVAL_OBJ_COUNT] = (float)tot[2];
        o[DURF_EVAL_OBJ_MSE] = (float)omse;
        o[DURF_EVAL_OBJ_PSNR] = (float)ev_psnr(omse);
    } else {
        o[DURF_EVAL_OBJ_COUNT] = 0.0f;
        o[DURF_EVAL_OBJ_MSE] = nanf_;
        o[DURF_EVAL_OBJ_PSNR] = nanf_;
    }
    if (have_depth) {
        const double n = tot[3] > 1.0 ? tot[3] : 1.0;
        o[DURF_EVAL_DEPTH_COUNT] = (float)tot[3];
        o[DURF_EVAL_DEPTH_ABS] = (float)(tot[4] / n);
        o[DURF_EVAL_DEPTH_RMSE] = (float)sqrt(tot[5] / n);
    } else {
        o[DURF_EVAL_DEPTH_COUNT] = 0.0f;
        o[DURF_EVAL_DEPTH_ABS] = nanf_;
        o[DURF_EVAL_DEPTH_RMSE] = nanf_;
    }
    o[DURF_EVAL_NONFINITE] = (float)tot[6];
}

static size_t ev_tiles(int H, int W) { return (size_t)durf_cdiv(H, EV_TILE) * durf_cdiv(W, EV_TILE); }

extern "C" {

size_t durf_eval_scratch_bytes(int F, int H, int W) {
    if (F <= 0 || H <= 0 || W <= 0) return 0;
    return (size_t)F * ev_tiles(H, W) * EV_PART * sizeof(double);
}

int durf_eval_frames(void* stream, int F, int H, int W, const float* rgb, const float* gt_rgb, const float* distance,
                     const float* gt_depth, const float* obj_mask, float* metrics, void* scratch, size_t scratch_bytes) {
    DURF_REQUIRE(H >= EV_WIN && W >= EV_WIN, "image smaller than the window");
    DURF_REQUIRE(F >= 0 && (size_t)H * W <= 0x7fffffffu, "F >= 0, H * W < 2^31");
    DURF_REQUIRE((distance != nullptr) == (gt_depth != nullptr), "distance and gt_depth are given together or not at all");
    if (F == 0) return 0;
    const size_t need = durf_eval_scratch_bytes(F, H, W);
    if (scratch_bytes < need) {
        durf_set_error("durf_eval_frames: scratch of %zu bytes, durf_eval_scratch_bytes(%d, %d, %d) = %zu", scratch_bytes, F, H, W, need);
        return -1;
    }
    DURF_REQUIRE(rgb && gt_rgb && metrics && scratch, "rgb, gt_rgb, metrics and scratch are given");
    DURF_REQUIRE(((size_t)scratch & 7) == 0, "scratch is 8-byte aligned");
    const unsigned tx = durf_cdiv(W, EV_TILE), ty = durf_cdiv(H, EV_TILE);
    DURF_REQUIRE(F <= 65535 && ty <= 65535, "F <= 65535 (the frame is the grid's z), H <= 65535 * 32");
    // the window of math.py:96-100 in double, rounded once, as metrics.compute_ssim makes it
    EvWindow win;
    double g[EV_WIN], sum = 0.0;
    for (int i = 0; i < EV_WIN; i++) {
        const double x = ((double)i - EV_WIN / 2) / 1.5;
        g[i] = exp(-0.5 * (x * x));
        sum += g[i];
    }
    for (int i = 0; i < EV_WIN; i++) win.w[i] = (float)(g[i] / sum);
    const float k1 = 0.01f, k2 = 0.03f, max_val = 1.0f;
    const float c1 = (k1 * max_val) * (k1 * max_val), c2 = (k2 * max_val) * (k2 * max_val);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_eval_tiles, dim3(tx, ty, F), dim3(EV_THREADS), 0, s, H, W, win, c1, c2, rgb, gt_rgb, distance, gt_depth,
                       obj_mask, (double*)scratch);
    hipLaunchKernelGGL(k_eval_finish, dim3(F), dim3(64), 0, s, H, W, (int)(tx * ty), distance ? 1 : 0, obj_mask ? 1 : 0,
                       (const double*)scratch, metrics);
    DURF_CHECK_LAUNCH("durf_eval_frames");
    return 0;
}

}  // extern "C"
