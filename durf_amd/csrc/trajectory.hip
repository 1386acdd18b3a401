// A camera trajectory in one call (durf_render_trajectory, csrc/forward.hip; the reference's notebooks/durf_render_traj.ipynb
// loop): the three kernels around the per-chunk forward launch sequence.  No rendering maths here -- a chunk's rays are the
// pinhole generator of durf_gen_batch (csrc/camera.h), the boxes between two labelled timesteps are a lerp with the angles
// taken along the shorter arc, and the 8-bit frame is one multiply and a round per channel.
#include "durf_common.h"
#include "camera.h"

// the rays of pixels [first, first + count) of one camera into slots [0, count): one thread per ray
__global__ void __launch_bounds__(256)
k_camera_rays(int count, CamRow cam, int first, float near, float far, float* __restrict__ origins, float* __restrict__ dirs,
              float* __restrict__ viewdirs, float* __restrict__ radii, float* __restrict__ near_o, float* __restrict__ far_o) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    pinhole_ray(cam.v, first + i, near, far, i, origins, dirs, viewdirs, radii, near_o, far_o);
}

// d onto [-pi, pi): d - 2 pi floor((d + pi) / 2 pi), 2 pi subtracted as a float pair (hi exact in n for the few turns
// an angle difference holds; the pair carries 2 pi to ~1e-14)
__device__ __forceinline__ float wrap_pi(float d) {
    const float PI_F = 3.14159274101257324f, TWO_PI_HI = 6.28318548202514648f, TWO_PI_LO = -1.74845553146951715e-7f;
    const float n = floorf((d + PI_F) / TWO_PI_HI);
    return (d - n * TWO_PI_HI) - n * TWO_PI_LO;
}

// poses [F,K,6] of frames [f0, f0 + gridDim.y) from box_centers [T,K,6] (device: the head of the flat parameters, read
// here so that a trajectory can follow a training step without a host copy).  t = i + w: position p_i + w (p_{i+1} - p_i),
// angle a_i + w wrap(a_{i+1} - a_i); w == 0 copies row i and never reads row i + 1 (t = T - 1 is legal).
// blockIdx.y = frame (its time is a scalar read of the by-value table), threadIdx = element of the [K,6] row.
#define DURF_TRAJ_TIMES 512
struct TimeTable { float t[DURF_TRAJ_TIMES]; };

__global__ void __launch_bounds__(64)
k_pose_interp(int K6, TimeTable times, int f0, const float* __restrict__ box_centers, float* __restrict__ poses) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= K6) return;
    const float t = times.t[blockIdx.y];
    const float fl = floorf(t);
    const int i = (int)fl;
    const float w = t - fl;
    const float* row = box_centers + (size_t)i * K6;
    float* out = poses + (size_t)(f0 + blockIdx.y) * K6;
    const float a = row[e];
    if (w == 0.0f) { out[e] = a; return; }
    const float d = row[K6 + e] - a;
    out[e] = a + w * ((e % 6) < 3 ? d : wrap_pi(d));
}

struct U32x3 { unsigned a, b, c; };

// the chunk epilogue of an 8-bit output (durf_common.h's rgb8 per value): every lane packs 4 whole pixels -- three 16-byte loads,
// one 12-byte store -- when both pointers allow it (wave-uniform), and byte by byte otherwise or on the last partial group
__global__ void __launch_bounds__(256)
k_frame_pack(int count, const float* __restrict__ rgb, uint8_t* __restrict__ out8) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    const int p0 = g * 4;
    if (p0 >= count) return;
    const bool aligned = (((size_t)rgb & 15) == 0) && (((size_t)out8 & 3) == 0);
    if (aligned && p0 + 4 <= count) {
        const f32x4* src = (const f32x4*)(rgb + (size_t)p0 * 3);
        const f32x4 v0 = src[0], v1 = src[1], v2 = src[2];
        U32x3 o;
        o.a = rgb8(v0[0]) | (rgb8(v0[1]) << 8) | (rgb8(v0[2]) << 16) | (rgb8(v0[3]) << 24);
        o.b = rgb8(v1[0]) | (rgb8(v1[1]) << 8) | (rgb8(v1[2]) << 16) | (rgb8(v1[3]) << 24);
        o.c = rgb8(v2[0]) | (rgb8(v2[1]) << 8) | (rgb8(v2[2]) << 16) | (rgb8(v2[3]) << 24);
        *(U32x3*)(out8 + (size_t)p0 * 3) = o;
        return;
    }
    const int p1 = p0 + 4 < count ? p0 + 4 : count;
    for (int j = p0 * 3; j < p1 * 3; j++) out8[j] = (uint8_t)rgb8(rgb[j]);
}

namespace durf {

int launch_camera_rays(void* stream, const float* cam_host, int first, int count, float near, float far, float* const* rays) {
    if (count <= 0) return 0;
    hipLaunchKernelGGL(k_camera_rays, dim3(durf_cdiv(count, 256)), dim3(256), 0, (hipStream_t)stream, count, cam_row(cam_host), first, near, far,
                       rays[0], rays[1], rays[2], rays[3], rays[4], rays[5]);
    DURF_CHECK_LAUNCH("k_camera_rays");
    note_dispatch(DURF_LAYERLOG_TRAJ_RAYS);
    return 0;
}

// (one launch for trajectories of up to DURF_TRAJ_TIMES frames; longer ones take one launch per table)
int launch_pose_interp(void* stream, int F, int K, const float* times_host, const float* box_centers, float* poses) {
    if (K <= 0) return 0;
    for (int f0 = 0; f0 < F; f0 += DURF_TRAJ_TIMES) {
        const int nf = F - f0 < DURF_TRAJ_TIMES ? F - f0 : DURF_TRAJ_TIMES;
        TimeTable t{};
        for (int j = 0; j < nf; j++) t.t[j] = times_host[f0 + j];
        hipLaunchKernelGGL(k_pose_interp, dim3(durf_cdiv((size_t)K * 6, 64), nf), dim3(64), 0, (hipStream_t)stream, K * 6, t, f0,
                           box_centers, poses);
        DURF_CHECK_LAUNCH("k_pose_interp");
    }
    note_dispatch(DURF_LAYERLOG_TRAJ_POSE);
    return 0;
}

int launch_frame_pack(void* stream, int count, const float* rgb, uint8_t* rgb8) {
    if (count <= 0) return 0;
    hipLaunchKernelGGL(k_frame_pack, dim3(durf_cdiv(durf_cdiv(count, 4), 256)), dim3(256), 0, (hipStream_t)stream, count, rgb, rgb8);
    DURF_CHECK_LAUNCH("k_frame_pack");
    note_dispatch(DURF_LAYERLOG_TRAJ_PACK);
    return 0;
}

}  // namespace durf
