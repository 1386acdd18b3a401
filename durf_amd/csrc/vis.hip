// Depth visualisations on the device (internal/vis.py): the three pictures the reference's evaluation block
// logs beside PSNR and SSIM -- depth through a colour map, depth modulo a period through the sinebow, fake normals of the
// depth plane -- for F frames at once.  Elementwise kernels (four pixels per lane, 16-byte loads and stores where the
// pointers allow it) and one two-pass reduction; plain fp32 in the reference's order of operations, fp64 only in the sums
// of the statistics.  Nothing here synchronises or copies to the host.
#include "durf_common.h"
#include <float.h>

#define DURF_TURBO_LUT_DECL __device__ const float k_turbo_lut[256 * 3]
#include "turbo_lut.h"
#undef DURF_TURBO_LUT_DECL
#define DURF_TURBO_LUT_DECL static const float h_turbo_lut[256 * 3]
#include "turbo_lut.h"
#undef DURF_TURBO_LUT_DECL

// ---- statistics: near / far / normal scale of every frame ---------------------------------------------------------------
// Pass 1 (grid G x F): count, sum x, sum y, sum d, min, max over the non-NaN pixels and whether any pixel is NaN, one record
// per workgroup.  Pass 2 (same grid): every workgroup adds the G records of its frame in index order -- all of them get the
// same means, bit for bit -- and sums the squared deviations of its pixels.  k_vis_stats_final adds those in index order.
// Every sum is fp64 and every order is fixed: thread t takes pixels t, t + 256, .. of its workgroup's range, the 256 lanes
// meet in a binary tree.
#define VIS_P1 8        // doubles of a pass-1 record: n, sx, sy, sd, min, max, any_nan, (pad)
#define VIS_P2 4        // doubles of a pass-2 record: qx, qy, qd, (pad)
#define VIS_WG_PIXELS 4096
#define VIS_MAX_WGS 64

static int vis_wgs(int H, int W) {
    const size_t hw = (size_t)H * W;
    const size_t g = (hw + VIS_WG_PIXELS - 1) / VIS_WG_PIXELS;
    return (int)(g < 1 ? 1 : (g > VIS_MAX_WGS ? VIS_MAX_WGS : g));
}

__device__ __forceinline__ double block_sum(double v, double* red) {
    __syncthreads();
    red[threadIdx.x] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    return red[0];
}
// min / max of the lanes' values, NaN = "no value" (fmin / fmax return the other operand)
__device__ __forceinline__ double block_minmax(double v, double* red, bool want_max) {
    __syncthreads();
    red[threadIdx.x] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s)
            red[threadIdx.x] = want_max ? fmax(red[threadIdx.x], red[threadIdx.x + s]) : fmin(red[threadIdx.x], red[threadIdx.x + s]);
        __syncthreads();
    }
    return red[0];
}

// the pixels of workgroup g of G: [lo, hi)
__device__ __forceinline__ void wg_range(int hw, int& lo, int& hi) {
    const int per = (hw + (int)gridDim.x - 1) / (int)gridDim.x;
    lo = (int)blockIdx.x * per;
    hi = lo + per < hw ? lo + per : hw;
}

__global__ void __launch_bounds__(256)
k_vis_stats_p1(int H, int W, const float* __restrict__ depth, double* __restrict__ part1) {
    __shared__ double red[256];
    const int hw = H * W;
    const float* d = depth + (size_t)blockIdx.y * hw;
    int lo, hi;
    wg_range(hw, lo, hi);
    const double nan = __builtin_nan("");
    double n = 0.0, sx = 0.0, sy = 0.0, sd = 0.0, mn = nan, mx = nan, bad = 0.0;
    for (int i = lo + (int)threadIdx.x; i < hi; i += 256) {
        const float v = d[i];
        if (v != v) { bad = 1.0; continue; }
        n += 1.0;
        sx += (double)(i % W);
        sy += (double)(i / W);
        sd += (double)v;
        mn = fmin(mn, (double)v);
        mx = fmax(mx, (double)v);
    }
    n = block_sum(n, red);
    sx = block_sum(sx, red);
    sy = block_sum(sy, red);
    sd = block_sum(sd, red);
    bad = block_sum(bad, red);
    mn = block_minmax(mn, red, false);
    mx = block_minmax(mx, red, true);
    if (threadIdx.x == 0) {
        double* o = part1 + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * VIS_P1;
        o[0] = n; o[1] = sx; o[2] = sy; o[3] = sd; o[4] = mn; o[5] = mx; o[6] = bad; o[7] = 0.0;
    }
}

struct VisSums { double n, sx, sy, sd, mn, mx, bad; };
__device__ __forceinline__ VisSums add_part1(const double* __restrict__ part1, int G) {
    VisSums s = {0.0, 0.0, 0.0, 0.0, __builtin_nan(""), __builtin_nan(""), 0.0};
    for (int g = 0; g < G; g++) {
        const double* p = part1 + (size_t)g * VIS_P1;
        s.n += p[0]; s.sx += p[1]; s.sy += p[2]; s.sd += p[3];
        s.mn = fmin(s.mn, p[4]); s.mx = fmax(s.mx, p[5]); s.bad += p[6];
    }
    return s;
}

__global__ void __launch_bounds__(256)
k_vis_stats_p2(int H, int W, const float* __restrict__ depth, const double* __restrict__ part1, double* __restrict__ part2) {
    __shared__ double red[256];
    const int hw = H * W;
    const float* d = depth + (size_t)blockIdx.y * hw;
    const VisSums s = add_part1(part1 + (size_t)blockIdx.y * gridDim.x * VIS_P1, (int)gridDim.x);
    const double mx = s.sx / s.n, my = s.sy / s.n, md = s.sd / s.n;
    int lo, hi;
    wg_range(hw, lo, hi);
    double qx = 0.0, qy = 0.0, qd = 0.0;
    for (int i = lo + (int)threadIdx.x; i < hi; i += 256) {
        const float v = d[i];
        if (v != v) continue;
        const double ex = (double)(i % W) - mx, ey = (double)(i / W) - my, ed = (double)v - md;
        qx += ex * ex; qy += ey * ey; qd += ed * ed;
    }
    qx = block_sum(qx, red);
    qy = block_sum(qy, red);
    qd = block_sum(qd, red);
    if (threadIdx.x == 0) {
        double* o = part2 + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * VIS_P2;
        o[0] = qx; o[1] = qy; o[2] = qd; o[3] = 0.0;
    }
}

// one thread per frame: the record {near_auto, far_auto, normal_scale, count, var x, var y, var depth, mean depth}
__global__ void __launch_bounds__(64)
k_vis_stats_final(int F, int G, const double* __restrict__ part1, const double* __restrict__ part2, float* __restrict__ stats) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= F) return;
    const VisSums s = add_part1(part1 + (size_t)f * G * VIS_P1, G);
    double qx = 0.0, qy = 0.0, qd = 0.0;
    for (int g = 0; g < G; g++) {
        const double* p = part2 + ((size_t)f * G + g) * VIS_P2;
        qx += p[0]; qy += p[1]; qd += p[2];
    }
    const double vx = qx / s.n, vy = qy / s.n, vd = qd / s.n;       // n == 0: 0 / 0 = NaN, the variance of nothing
    // the depth plane sorted ascending, NaNs last: its first element is the least non-NaN depth (NaN if there is none), its
    // last element is a NaN as soon as the plane holds one (vis.py:79-91 keeps it)
    const float first = (float)s.mn;
    const float last = s.bad > 0.0 ? __builtin_nanf("") : (float)s.mx;
    float* o = stats + (size_t)f * DURF_VIS_STATS_FLOATS;
    o[0] = first - FLT_EPSILON;
    o[1] = last + FLT_EPSILON;
    o[2] = (float)sqrt(((vx + vy) / 2.0) / vd);
    o[3] = (float)s.n;
    o[4] = (float)vx; o[5] = (float)vy; o[6] = (float)vd; o[7] = (float)(s.sd / s.n);
}

// ---- four pixels per lane ------------------------------------------------------------------------------------------------
struct VisU32x3 { unsigned a, b, c; };

// c[12] = the colours of pixels [p0, p0 + cnt), cnt <= 4: 16-byte float stores / one 12-byte store of the bytes (durf_common.h's
// rgb8 per value) when the group is whole and the pointers are aligned (wave-uniform but for the last group), element by element
// otherwise
__device__ __forceinline__ void store_pixels(size_t p0, int cnt, const float* c, float* __restrict__ rgb, uint8_t* __restrict__ out8) {
    if (rgb) {
        if (cnt == 4 && (((size_t)rgb & 15) == 0)) {
            f32x4* dst = (f32x4*)(rgb + p0 * 3);
            dst[0] = f32x4{c[0], c[1], c[2], c[3]};
            dst[1] = f32x4{c[4], c[5], c[6], c[7]};
            dst[2] = f32x4{c[8], c[9], c[10], c[11]};
        } else {
            for (int j = 0; j < cnt * 3; j++) rgb[p0 * 3 + j] = c[j];
        }
    }
    if (out8) {
        if (cnt == 4 && (((size_t)out8 & 3) == 0)) {
            VisU32x3 o;
            o.a = rgb8(c[0]) | (rgb8(c[1]) << 8) | (rgb8(c[2]) << 16) | (rgb8(c[3]) << 24);
            o.b = rgb8(c[4]) | (rgb8(c[5]) << 8) | (rgb8(c[6]) << 16) | (rgb8(c[7]) << 24);
            o.c = rgb8(c[8]) | (rgb8(c[9]) << 8) | (rgb8(c[10]) << 16) | (rgb8(c[11]) << 24);
            *(VisU32x3*)(out8 + p0 * 3) = o;
        } else {
            for (int j = 0; j < cnt * 3; j++) out8[p0 * 3 + j] = (uint8_t)rgb8(c[j]);
        }
    }
}

// v[4] = src[p0 .. p0 + cnt) (one 16-byte load when whole and aligned); src == NULL: ones
__device__ __forceinline__ void load_pixels(const float* __restrict__ src, size_t p0, int cnt, float* v) {
    v[0] = v[1] = v[2] = v[3] = 1.0f;
    if (!src) return;
    if (cnt == 4 && (((size_t)src & 15) == 0)) {
        const f32x4 q = *(const f32x4*)(src + p0);
        v[0] = q[0]; v[1] = q[1]; v[2] = q[2]; v[3] = q[3];
    } else {
        for (int j = 0; j < cnt; j++) v[j] = src[p0 + j];
    }
}

// ---- visualize_depth -----------------------------------------------------------------------------------------------------
__device__ __forceinline__ float vis_curve(int curve, float x) {
    if (curve == DURF_VIS_CURVE_IDENTITY) return x;
    if (curve == DURF_VIS_CURVE_INVERSE) return 1.0f / (x + FLT_EPSILON);
    return -logf(x + FLT_EPSILON);
}

// vis.sinebow (vis.py:23-26): sin(pi (k / 6 - h))^2 for k = 3, 5, 7
__device__ __forceinline__ void sinebow3(float h, float* c) {
    const float PI_F = 3.14159274101257324f;
    const float s0 = sinf(PI_F * (3.0f / 6.0f - h)), s1 = sinf(PI_F * (5.0f / 6.0f - h)), s2 = sinf(PI_F * (7.0f / 6.0f - h));
    c[0] = s0 * s0; c[1] = s1 * s1; c[2] = s2 * s2;
}

// a row of a 256 x 3 table for value in [0, 1] (matplotlib's call of a 256-entry map); NaN -> its 'bad' colour, black
__device__ __forceinline__ void lut_row(const float* lut, float value, float* c) {
    if (value != value) { c[0] = c[1] = c[2] = 0.0f; return; }
    int k = (int)(value * 256.0f);
    k = k < 0 ? 0 : (k > 255 ? 255 : k);
    c[0] = lut[k * 3]; c[1] = lut[k * 3 + 1]; c[2] = lut[k * 3 + 2];
}

template <bool MOD>
__global__ void __launch_bounds__(256)
k_vis_depth(size_t total, int hw, const float* __restrict__ depth, const float* __restrict__ acc, const float* __restrict__ range,
            int range_stride, int curve, float modulus, const float* __restrict__ lut, int use_lut, float* __restrict__ rgb,
            uint8_t* __restrict__ rgb8) {
    __shared__ float s_lut[256 * 3];
    if (use_lut) {
        const float* src = lut ? lut : k_turbo_lut;
        for (int j = threadIdx.x; j < 256 * 3; j += 256) s_lut[j] = src[j];
        __syncthreads();
    }
    const size_t p0 = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (p0 >= total) return;
    const int cnt = total - p0 < 4 ? (int)(total - p0) : 4;
    float d[4], a[4], c[12];
    load_pixels(depth, p0, cnt, d);
    load_pixels(acc, p0, cnt, a);
    size_t f = p0 / (size_t)hw;                  // (one 64-bit division per lane: the group's frame, stepped below)
    int i = (int)(p0 - f * hw);
    for (int j = 0; j < cnt; j++, i++) {
        while (i >= hw) { i -= hw; f++; }
        const float x = vis_curve(curve, d[j]);
        float value;
        if (MOD) {
            // jnp.mod: the remainder takes the divisor's sign
            float m = fmodf(x, modulus);
            if (m != 0.0f && ((m < 0.0f) != (modulus < 0.0f))) m += modulus;
            value = m / modulus;
        } else {
            const float n = vis_curve(curve, range[f * range_stride]), fr = vis_curve(curve, range[f * range_stride + 1]);
            const float v = (x - nan_min(n, fr)) / fabsf(fr - n);
            value = (v != v) ? 0.0f : fminf(fmaxf(v, 0.0f), 1.0f);        // nan_to_num(clip(v, 0, 1)); a NaN passes the clip
        }
        float* cj = c + j * 3;
        if (use_lut) lut_row(s_lut, value, cj);
        else sinebow3(value, cj);
        const float w = (d[j] != d[j]) ? 0.0f : a[j];
        const float rest = 1.0f - w;
        cj[0] = cj[0] * w + rest; cj[1] = cj[1] * w + rest; cj[2] = cj[2] * w + rest;
    }
    store_pixels(p0, cnt, c, rgb, rgb8);
}

// ---- visualize_normals / depth_to_normals --------------------------------------------------------------------------------
// scipy-style true convolution, mode 'same', zero padding, of s = scale * depth with
//   k_y[a][b] = edge[a] blur[b],  k_x[a][b] = blur[a] edge[b],  edge = (-1, 0, 1) / 2, blur = (1, 2, 1) / 4:
//   out[y][x] = sum_ab k[a][b] s[y + 1 - a][x + 1 - b].
// Every tap is multiplied, the zero ones too: 0 * NaN and 0 * inf are NaN and reach the pixel as they do in the reference.
__device__ __forceinline__ void normal_of(const float* __restrict__ d, float scale, int H, int W, int y, int x, float* n) {
    const float edge[3] = {-0.5f, 0.0f, 0.5f}, blur[3] = {0.25f, 0.5f, 0.25f};
    float dy = 0.0f, dx = 0.0f;
#pragma unroll
    for (int a = 0; a < 3; a++) {
#pragma unroll
        for (int b = 0; b < 3; b++) {
            const int yy = y + 1 - a, xx = x + 1 - b;
            if (yy < 0 || yy >= H || xx < 0 || xx >= W) continue;
            const float s = scale * d[(size_t)yy * W + xx];
            dy += (edge[a] * blur[b]) * s;
            dx += (blur[a] * edge[b]) * s;
        }
    }
    const float inv = 1.0f / sqrtf(1.0f + dx * dx + dy * dy);
    n[0] = dx * inv; n[1] = dy * inv; n[2] = inv;
}

__global__ void __launch_bounds__(256)
k_vis_normals(size_t total, int H, int W, const float* __restrict__ depth, const float* __restrict__ acc,
              const float* __restrict__ scale, int scale_stride, int raw, float* __restrict__ rgb, uint8_t* __restrict__ rgb8) {
    const size_t p0 = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (p0 >= total) return;
    const int cnt = total - p0 < 4 ? (int)(total - p0) : 4;
    const int hw = H * W;
    float a[4], c[12];
    load_pixels(acc, p0, cnt, a);
    size_t f = p0 / (size_t)hw;
    int i = (int)(p0 - f * hw);
    for (int j = 0; j < cnt; j++, i++) {
        while (i >= hw) { i -= hw; f++; }
        float* cj = c + j * 3;
        normal_of(depth + f * hw, scale ? scale[f * scale_stride] : 1.0f, H, W, i / W, i % W, cj);
        if (raw) continue;
        for (int k = 0; k < 3; k++) {
            // isnan(n) + nan_to_num((n + 1) / 2)
            const float h = (cj[k] + 1.0f) / 2.0f;
            float v = (cj[k] != cj[k]) ? 1.0f : 0.0f;
            v += nan_to_num(h);
            if (acc) v = v * a[j] + (1.0f - a[j]);
            cj[k] = v;
        }
    }
    store_pixels(p0, cnt, c, rgb, rgb8);
}

__global__ void __launch_bounds__(256)
k_vis_sinebow(size_t total, const float* __restrict__ h, float* __restrict__ rgb, uint8_t* __restrict__ rgb8) {
    const size_t p0 = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (p0 >= total) return;
    const int cnt = total - p0 < 4 ? (int)(total - p0) : 4;
    float v[4], c[12];
    load_pixels(h, p0, cnt, v);
    for (int j = 0; j < cnt; j++) sinebow3(v[j], c + j * 3);
    store_pixels(p0, cnt, c, rgb, rgb8);
}

extern "C" {

size_t durf_vis_scratch_bytes(int F, int H, int W) {
    if (F <= 0 || H <= 0 || W <= 0) return 0;
    return (size_t)F * vis_wgs(H, W) * (VIS_P1 + VIS_P2) * sizeof(double);
}

#define VIS_REQUIRE_PLANE()                                                                               \
    DURF_REQUIRE(F >= 0 && H >= 1 && W >= 1 && (size_t)H * W <= 0x7fffffffu, "F >= 0, H, W >= 1, H * W < 2^31"); \
    if (F == 0) return 0

int durf_vis_stats(void* stream, int F, int H, int W, const float* depth, float* stats, void* scratch, size_t scratch_bytes) {
    VIS_REQUIRE_PLANE();
    DURF_REQUIRE(depth && stats && scratch, "depth, stats and scratch are given");
    DURF_REQUIRE(((size_t)scratch & 7) == 0, "scratch is 8-byte aligned");
    const size_t need = durf_vis_scratch_bytes(F, H, W);
    if (scratch_bytes < need) {
        durf_set_error("durf_vis_stats: scratch of %zu bytes, durf_vis_scratch_bytes(%d, %d, %d) = %zu", scratch_bytes, F, H, W, need);
        return -1;
    }
    DURF_REQUIRE(F <= 65535, "F <= 65535 (the frame is the grid's y)");
    const int G = vis_wgs(H, W);
    double* part1 = (double*)scratch;
    double* part2 = part1 + (size_t)F * G * VIS_P1;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_vis_stats_p1, dim3(G, F), dim3(256), 0, s, H, W, depth, part1);
    hipLaunchKernelGGL(k_vis_stats_p2, dim3(G, F), dim3(256), 0, s, H, W, depth, part1, part2);
    hipLaunchKernelGGL(k_vis_stats_final, dim3(durf_cdiv(F, 64)), dim3(64), 0, s, F, G, part1, part2, stats);
    DURF_CHECK_LAUNCH("durf_vis_stats");
    return 0;
}

int durf_vis_depth(void* stream, int F, int H, int W, const float* depth, const float* acc, const float* range, int range_stride,
                   int curve, float modulus, const float* lut, float* rgb, uint8_t* rgb8) {
    VIS_REQUIRE_PLANE();
    DURF_REQUIRE(depth && (rgb || rgb8), "depth and at least one output are given");
    DURF_REQUIRE(curve == DURF_VIS_CURVE_NEGLOG || curve == DURF_VIS_CURVE_IDENTITY || curve == DURF_VIS_CURVE_INVERSE,
                 "curve is one of DURF_VIS_CURVE_*");
    const bool mod = modulus > 0.0f;
    DURF_REQUIRE(mod || (range && range_stride >= 2), "modulus == 0 takes a range of range_stride >= 2 floats per frame");
    const size_t total = (size_t)F * H * W;
    const unsigned grid = durf_cdiv(durf_cdiv(total, 4), 256);
    const int use_lut = (!mod || lut) ? 1 : 0;          // colormap or (sinebow if modulus > 0 else turbo), vis.py:99,104
    hipStream_t s = (hipStream_t)stream;
    if (mod)
        hipLaunchKernelGGL(k_vis_depth<true>, dim3(grid), dim3(256), 0, s, total, H * W, depth, acc, range, range_stride, curve, modulus,
                           lut, use_lut, rgb, rgb8);
    else
        hipLaunchKernelGGL(k_vis_depth<false>, dim3(grid), dim3(256), 0, s, total, H * W, depth, acc, range, range_stride, curve, modulus,
                           lut, use_lut, rgb, rgb8);
    DURF_CHECK_LAUNCH("durf_vis_depth");
    return 0;
}

int durf_vis_normals(void* stream, int F, int H, int W, const float* depth, const float* acc, const float* scale, int scale_stride,
                     int flags, float* rgb, uint8_t* rgb8) {
    VIS_REQUIRE_PLANE();
    DURF_REQUIRE(depth && (rgb || rgb8), "depth and at least one output are given");
    DURF_REQUIRE((flags & ~DURF_VIS_NORMALS_RAW) == 0, "flags: DURF_VIS_NORMALS_RAW or 0");
    DURF_REQUIRE(!scale || scale_stride >= 1, "scale_stride >= 1");
    const size_t total = (size_t)F * H * W;
    hipLaunchKernelGGL(k_vis_normals, dim3(durf_cdiv(durf_cdiv(total, 4), 256)), dim3(256), 0, (hipStream_t)stream, total, H, W, depth,
                       acc, scale, scale_stride, flags & DURF_VIS_NORMALS_RAW, rgb, rgb8);
    DURF_CHECK_LAUNCH("durf_vis_normals");
    return 0;
}

int durf_vis_sinebow(void* stream, size_t n, const float* h, float* rgb, uint8_t* rgb8) {
    DURF_REQUIRE(n == 0 || (h && (rgb || rgb8)), "h and at least one output are given");
    if (n == 0) return 0;
    hipLaunchKernelGGL(k_vis_sinebow, dim3(durf_cdiv(durf_cdiv(n, 4), 256)), dim3(256), 0, (hipStream_t)stream, n, h, rgb, rgb8);
    DURF_CHECK_LAUNCH("durf_vis_sinebow");
    return 0;
}

int durf_vis_turbo_lut(void* lut_host) {
    DURF_REQUIRE(lut_host, "a host buffer of 256 * 3 floats is given");
    float* o = (float*)lut_host;
    for (int j = 0; j < 256 * 3; j++) o[j] = h_turbo_lut[j];
    return 0;
}

}  // extern "C"
