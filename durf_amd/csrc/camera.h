// The camera row (include/durf_hip.h, THE CAMERA ROW: c2w [3,4] row-major, then the DURF_CAM_* slots) and the two ways through
// it: pixel -> ray (k_gen_batch, k_camera_rays) and world point -> pixel (overlay, flow, raster, tsdf).  The one place either is
// written, so that every library places a point with the same bits; plain fp32 in the order written.  Every function takes the
// row as a pointer and works alike on a register copy, a by-value kernel argument and a wave-uniform global pointer.  Internal.
#pragma once
#include <cfloat>
#include "../../include/durf_hip.h"

// a row passed to a kernel by value
struct CamRow { float v[DURF_CAM_FLOATS]; };

inline CamRow cam_row(const float* host) {
    CamRow c;
    for (int j = 0; j < DURF_CAM_FLOATS; j++) c.v[j] = host[j];
    return c;
}

__device__ __forceinline__ bool cam_finite(float x) { return fabsf(x) <= FLT_MAX; }          // false for NaN

// camera space of a world point: pc = R_c^T (P - o), R_c[a][j] = cam[4 a + j], o[a] = cam[4 a + 3]
__device__ __forceinline__ void cam_to_camera(const float* cam, float P0, float P1, float P2, float* pc) {
    const float d0 = P0 - cam[3], d1 = P1 - cam[7], d2 = P2 - cam[11];
#pragma unroll
    for (int j = 0; j < 3; j++) pc[j] = (cam[j] * d0 + cam[4 + j] * d1) + cam[8 + j] * d2;
}

// the picture-space position of a camera-space point at depth z = -pc[2] (or at the near plane it was clipped to)
__device__ __forceinline__ void cam_pixel(const float* cam, float pcx, float pcy, float z, float& x, float& y) {
    const float focal = cam[DURF_CAM_FOCAL];
    x = cam[DURF_CAM_PPX] + (focal * pcx) / z;
    y = cam[DURF_CAM_PPY] - (focal * pcy) / z;
}

// The pinhole ray of one pixel (obbpose_dataset.py:1868-1916), shared by k_gen_batch (csrc/data.hip: a timestep's batch) and
// k_camera_rays (csrc/trajectory.hip: a free camera), so that both write the same bits for the same camera row.
__device__ __forceinline__ void pinhole_ray(const float* cam, int p /* pixel of the camera, row-major */, float near, float far,
                                            int i /* output slot */, float* __restrict__ origins, float* __restrict__ dirs,
                                            float* __restrict__ viewdirs, float* __restrict__ radii,
                                            float* __restrict__ near_o, float* __restrict__ far_o) {
    const int w = (int)cam[DURF_CAM_W], h = (int)cam[DURF_CAM_H];
    const int y = p / w, x = p - y * w;
    auto dir = [&](int yy, float* d) {           // :1882-1889: d = sum_j cam_dirs_j * R[:, j], in that order
        const float cd[3] = {((float)x - cam[DURF_CAM_PPX]) / cam[DURF_CAM_FOCAL],
                             -((float)yy - cam[DURF_CAM_PPY]) / cam[DURF_CAM_FOCAL], -1.0f};
#pragma unroll
        for (int a = 0; a < 3; a++) d[a] = (cd[0] * cam[4 * a] + cd[1] * cam[4 * a + 1]) + cd[2] * cam[4 * a + 2];
    };
    float d[3], dn[3];
    dir(y, d);
    // radius: distance to the next row's direction; the last row repeats the previous one (:1896-1902)
    const int y0 = (y < h - 1) ? y : h - 2;
    float d0[3];
    dir(y0, d0);
    dir(y0 + 1, dn);
    const float dx = sqrtf(((d0[0] - dn[0]) * (d0[0] - dn[0]) + (d0[1] - dn[1]) * (d0[1] - dn[1])) +
                           (d0[2] - dn[2]) * (d0[2] - dn[2]));
    const float nrm = sqrtf((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
#pragma unroll
    for (int a = 0; a < 3; a++) {
        origins[i * 3 + a] = cam[4 * a + 3];
        dirs[i * 3 + a] = d[a];
        viewdirs[i * 3 + a] = d[a] / nrm;
    }
    radii[i] = dx * 2.0f / 3.4641016151377544f;       // 2 / sqrt(12)
    near_o[i] = near;
    far_o[i] = far;
}
