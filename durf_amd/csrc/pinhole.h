// The pinhole ray of one pixel (obbpose_dataset.py:1868-1916), shared by k_gen_batch (csrc/data.hip: a timestep's batch) and
// k_camera_rays (csrc/trajectory.hip: a free camera), so that both write the same bits for the same camera row.
// cam: 17 floats -- c2w [3,4] row-major, focal, principal point x / y, height, width.
#pragma once

__device__ __forceinline__ void pinhole_ray(const float* cam, int p /* pixel of the camera, row-major */, float near, float far,
                                            int i /* output slot */, float* __restrict__ origins, float* __restrict__ dirs,
                                            float* __restrict__ viewdirs, float* __restrict__ radii,
                                            float* __restrict__ near_o, float* __restrict__ far_o) {
    const int w = (int)cam[16], h = (int)cam[15];
    const int y = p / w, x = p - y * w;
    auto dir = [&](int yy, float* d) {           // :1882-1889: d = sum_j cam_dirs_j * R[:, j], in that order
        const float cd[3] = {((float)x - cam[13]) / cam[12], -((float)yy - cam[14]) / cam[12], -1.0f};
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
