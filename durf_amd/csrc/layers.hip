// Scene layers of a rendered image (durf_render_layers, csrc/forward.hip): which box every pixel shows, the image with the
// boxes taken out, the objects on their own.  Elementwise / compaction kernels only -- the rendering itself is the forward
// launch sequence, run a second time over the box-hit rays alone with K = 0.  Everything here is index bookkeeping and
// copies except one expression: obj_rgb = rgb - bg * (1 - acc), the composite with its background colour taken back out
// (render.hip composite_store adds bg * (1 - acc)).
#include "durf_common.h"

// ---------------------------------------------------------------------------
// per chunk, behind its composite: instance[b] = k if ray b hits exactly box k, -1 none, -2 several (hit: the prologue's
// [B,K], disabled boxes already 0); bg_* pre-filled with the composite (the second pass overwrites the box-hit rays);
// obj_rgba.  One thread per ray.
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
k_layer_chunk(int B, int K, const int32_t* __restrict__ hit, const float* __restrict__ rgb, const float* __restrict__ dist,
              const float* __restrict__ acc, int bkgd_mode, int32_t* __restrict__ instance, float* __restrict__ bg_rgb,
              float* __restrict__ bg_dist, float* __restrict__ bg_acc, float* __restrict__ obj_rgba) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    int nh = 0, which = -1;
    for (int k = 0; k < K; k++)
        if (hit[b * K + k] != 0) { nh++; which = k; }
    const int inst = nh == 0 ? -1 : (nh == 1 ? which : -2);
    instance[b] = inst;
    if (!bg_rgb && !obj_rgba) return;
    const float r0 = rgb[b * 3 + 0], r1 = rgb[b * 3 + 1], r2 = rgb[b * 3 + 2], a = acc[b];
    if (bg_rgb) {
        bg_rgb[b * 3 + 0] = r0; bg_rgb[b * 3 + 1] = r1; bg_rgb[b * 3 + 2] = r2;
        bg_dist[b] = dist[b];
        bg_acc[b] = a;
    }
    if (obj_rgba) {
        f32x4 o = {0.0f, 0.0f, 0.0f, 0.0f};
        if (inst != -1) {
            const float bg = bkgd_mode == 0 ? 0.5f : (bkgd_mode == 1 ? 1.0f : 0.0f);
            const float back = bg * (1.0f - a);
            o[0] = r0 - back; o[1] = r1 - back; o[2] = r2 - back; o[3] = a;
        }
        *(f32x4*)(obj_rgba + (size_t)b * 4) = o;
    }
}

// ---------------------------------------------------------------------------
// image-wide ordered compaction of the rays with instance != -1 (the model: compact_hits_block, rays.hip): idx[j] = the
// j-th such ray in ray order, count[0] = their number.  One workgroup; every thread takes 4 consecutive rays per round,
// so positions follow ray order whatever the scheduling.  Integer arithmetic only: the same result on every run.
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(1024)
k_layer_compact(int n, const int32_t* __restrict__ instance, int32_t* __restrict__ idx, int32_t* __restrict__ count) {
    __shared__ int wave_tot[16];
    __shared__ int base_s;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x == 0) base_s = 0;
    __syncthreads();
    for (int b0 = 0; b0 < n; b0 += 4096) {
        const int e = b0 + (int)threadIdx.x * 4;
        int h[4], c = 0;
#pragma unroll
        for (int j = 0; j < 4; j++) { h[j] = (e + j < n) && instance[e + j] != -1; c += h[j]; }
        int incl = c;                                     // inclusive scan of c over the wave
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) { const int t = __shfl_up(incl, d, 64); if (lane >= d) incl += t; }
        if (lane == 63) wave_tot[wave] = incl;
        __syncthreads();
        int woff = 0, tot = 0;
        for (int w = 0; w < 16; w++) { const int t = wave_tot[w]; if (w < wave) woff += t; tot += t; }
        int pos = base_s + woff + incl - c;
#pragma unroll
        for (int j = 0; j < 4; j++) if (h[j]) idx[pos++] = e + j;
        __syncthreads();
        if (threadIdx.x == 0) base_s += tot;
        __syncthreads();
    }
    if (threadIdx.x == 0) count[0] = base_s;
}

// the six Rays fields of rays idx[0..count) into dense buffers (12 floats per ray: one thread each)
struct RayFields { const float *origins, *directions, *viewdirs, *radii, *near, *far; };
struct RayFieldsOut { float *origins, *directions, *viewdirs, *radii, *near, *far; };

__global__ void __launch_bounds__(256)
k_layer_gather(int count, const int32_t* __restrict__ idx, RayFields src, RayFieldsOut dst) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count * 12) return;
    const int j = i / 12, c = i % 12;
    const size_t b = (size_t)idx[j];
    if (c < 3) dst.origins[j * 3 + c] = src.origins[b * 3 + c];
    else if (c < 6) dst.directions[j * 3 + c - 3] = src.directions[b * 3 + c - 3];
    else if (c < 9) dst.viewdirs[j * 3 + c - 6] = src.viewdirs[b * 3 + c - 6];
    else if (c == 9) dst.radii[j] = src.radii[b];
    else if (c == 10) dst.near[j] = src.near[b];
    else dst.far[j] = src.far[b];
}

// ... and the second pass's rgb / distance / acc of dense ray j into the image planes at ray idx[j]
__global__ void __launch_bounds__(256)
k_layer_scatter(int count, const int32_t* __restrict__ idx, const float* __restrict__ rgb, const float* __restrict__ dist,
                const float* __restrict__ acc, float* __restrict__ bg_rgb, float* __restrict__ bg_dist,
                float* __restrict__ bg_acc) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count * 5) return;
    const int j = i / 5, c = i % 5;
    const size_t b = (size_t)idx[j];
    if (c < 3) bg_rgb[b * 3 + c] = rgb[j * 3 + c];
    else if (c == 3) bg_dist[b] = dist[j];
    else bg_acc[b] = acc[j];
}

namespace durf {

int launch_layer_chunk(void* stream, int B, int K, const int32_t* hit, const float* rgb, const float* dist, const float* acc,
                       int bkgd_mode, int32_t* instance, float* bg_rgb, float* bg_dist, float* bg_acc, float* obj_rgba) {
    if (B <= 0) return 0;
    hipLaunchKernelGGL(k_layer_chunk, dim3(durf_cdiv(B, 256)), dim3(256), 0, (hipStream_t)stream, B, K, hit, rgb, dist, acc,
                       bkgd_mode, instance, bg_rgb, bg_dist, bg_acc, obj_rgba);
    DURF_CHECK_LAUNCH("durf_render_layers: layer_chunk");
    note_dispatch(DURF_LAYERLOG_SELECT);
    return 0;
}

int launch_layer_compact(void* stream, int n, const int32_t* instance, int32_t* idx, int32_t* count) {
    hipLaunchKernelGGL(k_layer_compact, dim3(1), dim3(1024), 0, (hipStream_t)stream, n, instance, idx, count);
    DURF_CHECK_LAUNCH("durf_render_layers: layer_compact");
    note_dispatch(DURF_LAYERLOG_SELECT);
    return 0;
}

int launch_layer_gather(void* stream, int count, const int32_t* idx, const float* const* src, float* const* dst) {
    if (count <= 0) return 0;
    const RayFields s{src[0], src[1], src[2], src[3], src[4], src[5]};
    const RayFieldsOut d{dst[0], dst[1], dst[2], dst[3], dst[4], dst[5]};
    hipLaunchKernelGGL(k_layer_gather, dim3(durf_cdiv((size_t)count * 12, 256)), dim3(256), 0, (hipStream_t)stream, count, idx, s, d);
    DURF_CHECK_LAUNCH("durf_render_layers: layer_gather");
    note_dispatch(DURF_LAYERLOG_PASS2);
    return 0;
}

int launch_layer_scatter(void* stream, int count, const int32_t* idx, const float* rgb, const float* dist, const float* acc,
                         float* bg_rgb, float* bg_dist, float* bg_acc) {
    if (count <= 0) return 0;
    hipLaunchKernelGGL(k_layer_scatter, dim3(durf_cdiv((size_t)count * 5, 256)), dim3(256), 0, (hipStream_t)stream, count, idx, rgb,
                       dist, acc, bg_rgb, bg_dist, bg_acc);
    DURF_CHECK_LAUNCH("durf_render_layers: layer_scatter");
    note_dispatch(DURF_LAYERLOG_PASS2);
    return 0;
}

}  // namespace durf
