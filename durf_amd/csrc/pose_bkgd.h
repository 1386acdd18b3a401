// Box-pose gradient through the BACKGROUND encoding (MipNerfModel.dynamics = False; included by pose.hip, which owns
// POSE_ROWS, pose_rows and the row reduction).
//
// With dynamics=False the boxes own no network (obbpose_model.py:116-122,229-236): a box-hit ray's (o', d') in box
// coordinates is what the background encoder sees.  d(loss)/d(enc) of the 60 background features -> integrated_pos_enc
// (mip.py:226-282: no BARF weights, no identity features) -> mip360.new_space when contracting -> the Gaussian -> (o', d')
// -> the 21 pose rows (pose_rows).  A ray that hits several boxes feeds the SUMS of their (o', d') (:121-122): every box
// it hits takes the whole d(o_s), d(d_s).  d_s reaches the loss one other way, delta = t_dists |d_s| (mip.py:305):
// d(loss)/d|d_s| = sum_n density_n d(loss)/d(density_n) / |d_s|, with density = softplus(raw + bias) and
// draw = d(loss)/d(raw) = sigmoid(raw + bias) d(loss)/d(density) -- zero after the normalisation's backward for a ray in
// one box (|d'| = 1), the whole term for a ray in several.
//
// Same structure as k_encode_obj_bwd: one workgroup per (hit ray, box), the four waves split the 60 features, lanes take
// the samples, fixed-order reductions (run-to-run bit-identical, no atomics).  libm exp / sin / cos only: the path runs
// behind exact-fp32 d(enc) in both precisions (the box-hit rays' background evaluation is fp32 under mlp_precision='bf16').
// raw, draw: the full [B*N, 4] rows of the level (row b*N + n), nullable together (no |d_s| term); d_enc: [rows, 64] with
// row denc_slot[b]*N + n (the fp32 evaluation of the box-hit rays only), or b*N + n when denc_slot is null.
#pragma once

template <int P>
__global__ void __launch_bounds__(256)
k_encode_bkgd_bwd(int B, int N, const int32_t* __restrict__ idx, const int32_t* __restrict__ count,
                  const float* __restrict__ d_enc, const int32_t* __restrict__ denc_slot, const float* __restrict__ t_vals,
                  const float* __restrict__ origins_s, const float* __restrict__ dirs_s, const float* __restrict__ radii,
                  const float* __restrict__ origins, const float* __restrict__ dirs, const float* __restrict__ pose,
                  const float* __restrict__ raw, const float* __restrict__ draw, float density_bias,
                  float* __restrict__ rows_out, int enc_flags) {
    const bool cyl = (enc_flags & DURF_ENC_CYLINDER) != 0, noint = (enc_flags & DURF_ENC_NO_INTEGRATION) != 0;
    const bool con = (enc_flags & DURF_ENC_CONTRACT) != 0;
    __shared__ float part[4][6];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int kb = blockIdx.y;                      // box
    idx += (size_t)kb * B; count += kb; rows_out += (size_t)kb * POSE_ROWS * B;
    const int nj = *count < B ? *count : B;
    for (int j = blockIdx.x; j < nj; j += gridDim.x) {
    const int b = idx[j];
    const float o[3] = {origins_s[b * 3], origins_s[b * 3 + 1], origins_s[b * 3 + 2]};
    const float d[3] = {dirs_s[b * 3], dirs_s[b * 3 + 1], dirs_s[b * 3 + 2]};
    const float radius = radii[b];
    const float dsum = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
    const float m = fmaxf(1e-10f, dsum);
    float go[3] = {0.f, 0.f, 0.f}, gd[3] = {0.f, 0.f, 0.f}, gnorm = 0.0f;
#pragma unroll
    for (int p = 0; p < P; p++) {
        const int n = lane * P + p;
        if (n >= N) continue;
        const size_t row = (size_t)b * N + n;
        const float t0 = t_vals[(size_t)b * (N + 1) + n], t1 = t_vals[(size_t)b * (N + 1) + n + 1];
        // the forward's Gaussian (gauss.h) and its contraction (enc_lane.h): the values the features were made from
        Gauss g = frustum_gaussian(t0, t1, o, d, radius, cyl);
        if (noint) g.var[0] = g.var[1] = g.var[2] = 0.0f;
        Gauss gc = g;
        if (con) contract_gaussian(gc);
        // IPE backward: d(loss)/d(x'), d(loss)/d(var') from this wave's 15 features
        const float* ge = d_enc + ((size_t)(denc_slot ? denc_slot[b] : b) * N + n) * DURF_ENC_DIM;
        float gxc[3] = {0.f, 0.f, 0.f}, gvc[3] = {0.f, 0.f, 0.f};
        for (int f = 15 * wv; f < 15 * wv + 15; f++) {
            const int c = f / 30, r = f - c * 30, deg = r / 3, i = r - deg * 3;
            const float sc = (float)(1 << deg);
            const float xi = i == 0 ? gc.x[0] : (i == 1 ? gc.x[1] : gc.x[2]);
            const float vi = i == 0 ? gc.var[0] : (i == 1 ? gc.var[1] : gc.var[2]);
            float z = xi * sc;
            if (c) z = z + 1.5707963705062866f;
            const float t = 314.15927124023438f;                          // safe_sin wrap (math.py:35-46)
            if (!(fabsf(z) < t)) { float q = fmodf(z, t); if (q != 0.0f && q < 0.0f) q += t; z = q; }
            const float e = expf(-0.5f * (vi * sc * sc));
            const float cz = cosf(z), sz = sinf(z);
            const float gf = ge[f];
            const float gxf = gf * e * sc * cz, gvf = noint ? 0.0f : gf * (-0.5f * sc * sc) * e * sz;
            if (i == 0) { gxc[0] += gxf; gvc[0] += gvf; }
            else if (i == 1) { gxc[1] += gxf; gvc[1] += gvf; }
            else { gxc[2] += gxf; gvc[2] += gvf; }
        }
        // mip360.new_space backward (linear in gxc, gvc: the per-wave partials add up).  Above the 0.1 threshold
        // x'_j = a x_j and v_j = a + c x_j S, with n = |x|, S = x_0 + x_1 + x_2, a = 2/n - 1/n^2, c = 2/n^4 - 2/n^3 = a'/n;
        // var'_j = var_j v_j^2, so d/dx also runs through v (the Hessian of contract applied to (1,1,1)).  At or below it
        // the identity (contract_gaussian's x_smaller branch: the reference's threshold quirk).
        float gx[3], gv[3];
        const float s0 = g.x[0] * g.x[0] + g.x[1] * g.x[1] + g.x[2] * g.x[2];
        const float nx = sqrtf(s0 < 1e-12f ? 1e-12f : s0);
        if (con && nx > 0.1f) {
            const float in1 = 1.0f / nx, in2 = in1 * in1, in3 = in2 * in1, in4 = in2 * in2;
            const float a = 2.0f * in1 - in2, cc = 2.0f * in4 - 2.0f * in3;
            const float ap = -2.0f * in2 + 2.0f * in3, cp = -8.0f * in4 * in1 + 6.0f * in4;     // da/dn, dc/dn
            const float S = g.x[0] + g.x[1] + g.x[2];
            float gvv[3], xg = 0.0f, vx = 0.0f, G = 0.0f;
#pragma unroll
            for (int i = 0; i < 3; i++) {
                const float v = a + cc * g.x[i] * S;
                gv[i] = gvc[i] * v * v;
                gvv[i] = gvc[i] * 2.0f * g.var[i] * v;                    // d(loss)/d(v_i)
                xg += gxc[i] * g.x[i];
                vx += gvv[i] * g.x[i];
                G += gvv[i];
            }
            const float radial = (ap * G + cp * S * vx) * in1;
#pragma unroll
            for (int i = 0; i < 3; i++)
                gx[i] = a * gxc[i] + cc * g.x[i] * xg + g.x[i] * radial + cc * (S * gvv[i] + vx);
        } else {
#pragma unroll
            for (int i = 0; i < 3; i++) { gx[i] = gxc[i]; gv[i] = gvc[i]; }
        }
        // x_i = o_i + d_i t_mean ; var_i = t_var d_i^2 + r_var (1 - d_i^2 / m)   (k_encode_obj_bwd's chain)
        const Moments mo = frustum_moments(t0, t1, radius, cyl);
        const float t_mean = mo.t_mean, t_var = mo.t_var, r_var = mo.r_var;
        if (noint) { gv[0] = gv[1] = gv[2] = 0.0f; }
        float s_gv = 0.0f;
#pragma unroll
        for (int i = 0; i < 3; i++) s_gv += gv[i] * r_var * (d[i] * d[i]) / (m * m);
#pragma unroll
        for (int i = 0; i < 3; i++) {
            go[i] += gx[i];
            float gg = gx[i] * t_mean + gv[i] * (2.0f * t_var * d[i]) - gv[i] * r_var * (2.0f * d[i] / m);
            if (dsum > 1e-10f) gg += s_gv * 2.0f * d[i];                  // through m = max(1e-10, |d|^2)
            gd[i] += gg;
        }
        if (wv == 0 && raw) {          // the |d_s| term: density_n d(loss)/d(density_n) = draw_n softplus(x) / sigmoid(x)
            const float x = raw[row * 4 + 3] + density_bias;
            const float ratio = x < -15.0f ? 1.0f : (x > 20.0f ? x : log1pf(expf(x))) * (1.0f + expf(-x));
            gnorm += draw[row * 4 + 3] * ratio;
        }
    }
    if (wv == 0 && raw && dsum > 0.0f) {
#pragma unroll
        for (int i = 0; i < 3; i++) gd[i] += gnorm * d[i] / dsum;     // d|d|/dd = d / |d|, times d(loss)/d|d| = gnorm / |d|
    }
#pragma unroll
    for (int i = 0; i < 3; i++) { go[i] = wave_sum(go[i]); gd[i] = wave_sum(gd[i]); }
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < 3; i++) { part[wv][i] = go[i]; part[wv][3 + i] = gd[i]; }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int i = 0; i < 3; i++) {
            go[i] = ((part[0][i] + part[1][i]) + part[2][i]) + part[3][i];
            gd[i] = ((part[0][3 + i] + part[1][3 + i]) + part[2][3 + i]) + part[3][3 + i];
        }
        pose_rows(pose + kb * 6, origins + b * 3, dirs + b * 3, go, gd, rows_out + j, B);
    }
    __syncthreads();                                // part[] is reused by the next ray
    }   // rays
}
