// The rotation of a box pose, shared by the box overlay (overlay.hip) and the flow library (flow.hip) so that both place a box
// with the same bits.  Internal.
#pragma once

// box_helpers.aa2matrix (:148-167) as k_ray_setup has it (csrc/rays.hip): the same safe_norm clamp, the same +1e-12, the same
// skew product.  R is the world->object matrix.
__device__ __forceinline__ void overlay_aa2matrix(float rx, float ry, float rz, float* R) {
    float s = rx * rx + ry * ry + rz * rz;
    s = (s < 1e-12f) ? 1e-12f : s;                    // math.safe_norm (:27-32)
    const float th = sqrtf(s) + 1e-12f;
    const float a = sinf(th) / th;
    const float b = (1.0f - cosf(th)) / (th * th);
    const float S[9] = {0.f, -rz, ry, rz, 0.f, -rx, -ry, rx, 0.f};
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) {
            float s2 = S[i * 3 + 0] * S[0 * 3 + j] + S[i * 3 + 1] * S[1 * 3 + j] + S[i * 3 + 2] * S[2 * 3 + j];
            R[i * 3 + j] = ((i == j) ? 1.0f : 0.0f) + a * S[i * 3 + j] + b * s2;
        }
}
