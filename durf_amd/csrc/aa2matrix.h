// The frame of a box pose, shared by the box overlay (overlay.hip), the flow library (flow.hip) and the field library (field.hip)
// so that all place a box with the same bits.  Internal.
#pragma once

#define DURF_POSE_ROW 12            // one box of a pose table: R row-major, then the centre

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

// a 6-float pose (centre, then axis-angle) -> its row of a pose table
__device__ __forceinline__ void pose_row_fill(const float* __restrict__ p, float* __restrict__ row) {
    float R[9];
    overlay_aa2matrix(p[3], p[4], p[5], R);
#pragma unroll
    for (int i = 0; i < 9; i++) row[i] = R[i];
    row[9] = p[0]; row[10] = p[1]; row[11] = p[2];
}

// world -> box: R (X - c) of one row
__device__ __forceinline__ void pose_to_box(const float* row, float X0, float X1, float X2, float* P) {
    const float d0 = X0 - row[9], d1 = X1 - row[10], d2 = X2 - row[11];
#pragma unroll
    for (int j = 0; j < 3; j++) P[j] = (row[j * 3] * d0 + row[j * 3 + 1] * d1) + row[j * 3 + 2] * d2;
}

// box -> world: c + R^T P of one row
__device__ __forceinline__ void pose_to_world(const float* row, float P0, float P1, float P2, float* X) {
#pragma unroll
    for (int j = 0; j < 3; j++) X[j] = row[9 + j] + ((row[j] * P0 + row[3 + j] * P1) + row[6 + j] * P2);
}
