// Depth frames fused into a truncated signed distance volume (include/durf_tsdf.h; libdurf_tsdf.so): one thread per voxel walks
// the F frames of a call with the voxel's state in registers, projects the voxel into each camera, looks the nearest pixel's
// depth up and takes the running weighted mean.  A gather: no atomics, no counts, nothing that depends on a schedule; the
// volume is read once and written once per call.  Then the lattice durf_mesh_count takes and a trilinear sampler.  Nothing
// synchronises or copies to the host; no workgroup waits for another.
#include <cmath>
#include "durf_common.h"
#include "camera.h"
#include "lattice.h"
#include "../../include/durf_mesh.h"
#include "../../include/durf_tsdf.h"

#define TB DURF_TSDF_BLOCK
static_assert(TB == 256, "one voxel per thread, 256 per workgroup");
static_assert(DURF_TSDF_MAX_POINTS == DURF_MESH_MAX_POINTS, "the lattice goes on to durf_mesh_count");

struct TsdfFrames {
    int F, h, w;
    const float* cams;                 // [F,DURF_CAM_FLOATS]
    const float* depth;                // [F,h,w]
    const float* acc;                  // nullable
    const float* rgb;                  // nullable
    const int32_t* label;              // nullable
    const float* xform;                // nullable
    const float* frame_weight;         // nullable
    float min_acc, trunc, max_weight, znear;
    int select, other_mode;
};

// ---- integrate -------------------------------------------------------------------------------------------------------------------
// f, and with it every camera, xform and weight address, is the same for all lanes: the compiler reads those rows with scalar
// loads (camera.h's functions take the row's pointer, never a per-lane copy).  cam_finite (camera.h) is the library's one
// finite-and-not-NaN test: it guards depth, weights and lattice coordinates here as well as camera space.  The per-lane state is D, W, the
// four colour floats and the voxel's position.
__global__ void __launch_bounds__(TB)
k_tsdf_integrate(const LatticeDims L, const LatticeFrame G, const TsdfFrames A, float* __restrict__ tsdf, float* __restrict__ weight, float* __restrict__ colour) {
    const int g = blockIdx.x * TB + threadIdx.x;                             // n < 2^27
    if (g >= L.n) return;
    int i, j, k;
    lattice_ijk(L, g, i, j, k);
    float P[3];
    lattice_point(G, (float)i, (float)j, (float)k, P);
    float D = tsdf[g], W = weight[g];
    const bool keep_colour = colour != nullptr && A.rgb != nullptr;
    float C0 = 0.0f, C1 = 0.0f, C2 = 0.0f, Wc = 0.0f;
    if (keep_colour) {
        const float4 c4 = *reinterpret_cast<const float4*>(colour + (size_t)g * 4);
        C0 = c4.x, C1 = c4.y, C2 = c4.z, Wc = c4.w;
    }
    bool touched = false, coloured = false;
    const float lim = (float)DURF_TSDF_MAX_COORD;
    for (int f = 0; f < A.F; f++) {
        const float* __restrict__ cam = A.cams + (size_t)f * DURF_CAM_FLOATS;
        float X[3] = {P[0], P[1], P[2]};
        if (A.xform) {
            const float* __restrict__ M = A.xform + (size_t)f * 12;
#pragma unroll
            for (int c = 0; c < 3; c++) X[c] = ((M[4 * c] * P[0] + M[4 * c + 1] * P[1]) + M[4 * c + 2] * P[2]) + M[4 * c + 3];
        }
        float pc[3];
        cam_to_camera(cam, X[0], X[1], X[2], pc);
        if (!(cam_finite(X[0]) && cam_finite(X[1]) && cam_finite(X[2]) && cam_finite(pc[0]) && cam_finite(pc[1]) && cam_finite(pc[2])))
            continue;                                                        // 1 INVALID
        const float z = -pc[2];
        if (!(z >= A.znear)) continue;                                       // 2 BEHIND
        float x, y;
        cam_pixel(cam, pc[0], pc[1], z, x, y);
        if (!(fabsf(x) <= lim) || !(fabsf(y) <= lim)) continue;              // 3 RANGE
        const int px = (int)rintf(x), py = (int)rintf(y);
        if (px < 0 || px >= A.w || py < 0 || py >= A.h) continue;            // 4 OUTSIDE
        const size_t p = ((size_t)f * A.h + py) * A.w + px;                  // F h w < 2^31
        const float dep = A.depth[p];
        if (!cam_finite(dep) || !(dep > 0.0f)) continue;                    // 5 HOLE
        if (A.acc && !(A.acc[p] >= A.min_acc)) continue;                     // 6 FAINT
        const float sdf = dep - z;
        if (sdf < -A.trunc) continue;                                        // 7 OCCLUDED
        bool mine = true;
        if (A.label) {
            mine = A.label[p] == A.select;
            if (!mine && (A.other_mode == 0 || !(sdf >= A.trunc))) continue; // 8 OTHER
        }
        const float wf = A.frame_weight ? A.frame_weight[f] : 1.0f;
        if (!cam_finite(wf) || !(wf > 0.0f)) continue;                      // 9 WEIGHT
        const float dn = fminf(sdf / A.trunc, 1.0f);
        const float Wn = W + wf;
        D = (W * D + wf * dn) / Wn;
        W = fminf(Wn, A.max_weight);
        touched = true;
        if (keep_colour && mine && sdf <= A.trunc) {
            const float* __restrict__ q = A.rgb + p * 3;
            const float Wcn = Wc + wf;
            C0 = (Wc * C0 + wf * q[0]) / Wcn;
            C1 = (Wc * C1 + wf * q[1]) / Wcn;
            C2 = (Wc * C2 + wf * q[2]) / Wcn;
            Wc = fminf(Wcn, A.max_weight);
            coloured = true;
        }
    }
    if (touched) {
        tsdf[g] = D;
        weight[g] = W;
    }
    if (coloured) *reinterpret_cast<float4*>(colour + (size_t)g * 4) = make_float4(C0, C1, C2, Wc);
}

// ---- the lattice for durf_mesh_count -------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(TB)
k_tsdf_lattice(int n, const float* __restrict__ tsdf, const float* __restrict__ weight, const float* __restrict__ colour, float min_weight,
               float* __restrict__ density, uint8_t* __restrict__ valid, float* __restrict__ rgb_out) {
    const int g = blockIdx.x * TB + threadIdx.x;
    if (g >= n) return;
    density[g] = -tsdf[g];
    valid[g] = weight[g] >= min_weight ? 1 : 0;
    if (rgb_out) {
        const float4 c4 = *reinterpret_cast<const float4*>(colour + (size_t)g * 4);
        const bool has = c4.w > 0.0f;
        rgb_out[(size_t)g * 3] = has ? c4.x : 0.0f;
        rgb_out[(size_t)g * 3 + 1] = has ? c4.y : 0.0f;
        rgb_out[(size_t)g * 3 + 2] = has ? c4.z : 0.0f;
    }
}

// ---- the signed distance at points --------------------------------------------------------------------------------------------------
struct TsdfInverse {
    float origin[3], inv[9];
};

__device__ __forceinline__ float tsdf_lerp(float a, float b, float t) { return a + t * (b - a); }

__global__ void __launch_bounds__(TB)
k_tsdf_sample(int nu, int nv, int nw, const TsdfInverse Q, const float* __restrict__ tsdf, const float* __restrict__ weight,
              const float* __restrict__ colour, float trunc, float min_weight, int m, const float* __restrict__ points,
              float* __restrict__ sdf, uint8_t* __restrict__ ok, float* __restrict__ rgb_out) {
    const int r = blockIdx.x * TB + threadIdx.x;
    if (r >= m) return;
    const float e0 = points[(size_t)r * 3] - Q.origin[0], e1 = points[(size_t)r * 3 + 1] - Q.origin[1], e2 = points[(size_t)r * 3 + 2] - Q.origin[2];
    float q[3];
#pragma unroll
    for (int c = 0; c < 3; c++) q[c] = (Q.inv[3 * c] * e0 + Q.inv[3 * c + 1] * e1) + Q.inv[3 * c + 2] * e2;
    const int dims[3] = {nu, nv, nw};
    bool inside = true;
#pragma unroll
    for (int c = 0; c < 3; c++) inside = inside && cam_finite(q[c]) && q[c] >= 0.0f && q[c] <= (float)(dims[c] - 1);
    float v = __builtin_nanf("");
    float col[3] = {0.0f, 0.0f, 0.0f};
    bool good = false;
    if (inside) {                                                            // only then is a cell index inside the lattice
        int cell[3];
        float t[3];
#pragma unroll
        for (int c = 0; c < 3; c++) {
            cell[c] = min((int)floorf(q[c]), dims[c] - 2);
            t[c] = q[c] - (float)cell[c];
        }
        size_t idx[8];
#pragma unroll
        for (int a = 0; a < 8; a++)
            idx[a] = ((size_t)(cell[0] + (a >> 2)) * nv + (cell[1] + ((a >> 1) & 1))) * nw + (cell[2] + (a & 1));
        good = true;
        float d[8];
#pragma unroll
        for (int a = 0; a < 8; a++) {
            good = good && weight[idx[a]] >= min_weight;
            d[a] = tsdf[idx[a]];
        }
        if (good) {
            const float v00 = tsdf_lerp(d[0], d[1], t[2]), v01 = tsdf_lerp(d[2], d[3], t[2]);
            const float v10 = tsdf_lerp(d[4], d[5], t[2]), v11 = tsdf_lerp(d[6], d[7], t[2]);
            v = tsdf_lerp(tsdf_lerp(v00, v01, t[1]), tsdf_lerp(v10, v11, t[1]), t[0]) * trunc;
        }
        if (rgb_out) {
            float4 c4[8];
            bool has = true;
#pragma unroll
            for (int a = 0; a < 8; a++) {
                c4[a] = *reinterpret_cast<const float4*>(colour + idx[a] * 4);
                has = has && c4[a].w > 0.0f;
            }
            if (has) {
#pragma unroll
                for (int c = 0; c < 3; c++) {
                    float s[8];
#pragma unroll
                    for (int a = 0; a < 8; a++) s[a] = c == 0 ? c4[a].x : c == 1 ? c4[a].y : c4[a].z;
                    const float v00 = tsdf_lerp(s[0], s[1], t[2]), v01 = tsdf_lerp(s[2], s[3], t[2]);
                    const float v10 = tsdf_lerp(s[4], s[5], t[2]), v11 = tsdf_lerp(s[6], s[7], t[2]);
                    col[c] = tsdf_lerp(tsdf_lerp(v00, v01, t[1]), tsdf_lerp(v10, v11, t[1]), t[0]);
                }
            }
        }
    }
    sdf[r] = v;
    ok[r] = good ? 1 : 0;
    if (rgb_out) {
#pragma unroll
        for (int c = 0; c < 3; c++) rgb_out[(size_t)r * 3 + c] = col[c];
    }
}

namespace {

// colour is read and written as float4 rows: the header asks for 16-byte alignment
bool tsdf_aligned16(const void* p) { return ((size_t)p & 15) == 0; }

}  // namespace

extern "C" {

int durf_tsdf_integrate(void* stream, int nu, int nv, int nw, const float* origin_host, const float* du_host, const float* dv_host,
                        const float* dw_host, int F, int h, int w, const float* cams_dev, const float* depth, const float* acc,
                        float min_acc, const float* rgb, const int32_t* label, int select, int other_mode, const float* xform,
                        const float* frame_weight, float trunc, float max_weight, float znear, float* tsdf, float* weight, float* colour) {
    const int n = check_lattice_shape(__func__, nu, nv, nw, DURF_TSDF_MAX_POINTS);
    if (n < 0) return -1;
    DURF_REQUIREF(F >= 0, "F >= 0, F = %d", F);
    DURF_REQUIREF(h >= 1 && w >= 1 && h <= DURF_TSDF_MAX_SIZE && w <= DURF_TSDF_MAX_SIZE, "1 <= h, w <= %d, h = %d, w = %d",
                  DURF_TSDF_MAX_SIZE, h, w);
    DURF_REQUIREF((double)F * h * w < 2147483648.0, "F h w < 2^31 pixels, F = %d, h = %d, w = %d", F, h, w);
    DURF_REQUIREF(trunc > 0.0f && trunc <= FLT_MAX, "trunc > 0 and finite, trunc = %g", (double)trunc);
    DURF_REQUIREF(max_weight > 0.0f, "max_weight > 0, max_weight = %g", (double)max_weight);
    DURF_REQUIREF(znear >= FLT_MIN, "znear > 0 (a normal float), znear = %g", (double)znear);
    DURF_REQUIREF(!acc || min_acc == min_acc, "min_acc is a number with acc, min_acc = %g", (double)min_acc);
    DURF_REQUIREF(other_mode >= 0 && other_mode <= 1, "other_mode in 0 .. 1, other_mode = %d", other_mode);
    DURF_REQUIRE(label || other_mode == 0, "label with other_mode == 1");
    DURF_REQUIRE(origin_host, "origin_host");
    DURF_REQUIRE(du_host, "du_host");
    DURF_REQUIRE(dv_host, "dv_host");
    DURF_REQUIRE(dw_host, "dw_host");
    DURF_REQUIRE(tsdf, "tsdf");
    DURF_REQUIRE(weight, "weight");
    DURF_REQUIRE(tsdf_aligned16(colour), "colour aligned to 16 bytes");
    DURF_REQUIREF(cams_dev || F == 0, "cams_dev for F = %d", F);
    DURF_REQUIREF(depth || F == 0, "depth for F = %d", F);
    if (F == 0) return 0;
    const LatticeDims L{nu, nv, nw, n};
    const LatticeFrame G = lattice_frame(origin_host, du_host, dv_host, dw_host);
    TsdfFrames A;
    A.F = F, A.h = h, A.w = w;
    A.cams = cams_dev, A.depth = depth, A.acc = acc, A.rgb = rgb, A.label = label, A.xform = xform, A.frame_weight = frame_weight;
    A.min_acc = min_acc, A.trunc = trunc, A.max_weight = max_weight, A.znear = znear;
    A.select = select, A.other_mode = other_mode;
    hipLaunchKernelGGL(k_tsdf_integrate, dim3(durf_cdiv((size_t)n, TB)), dim3(TB), 0, (hipStream_t)stream, L, G, A, tsdf, weight, colour);
    DURF_CHECK_LAUNCH("k_tsdf_integrate");
    return 0;
}

int durf_tsdf_lattice(void* stream, int nu, int nv, int nw, const float* tsdf, const float* weight, const float* colour, float min_weight,
                      float* density, uint8_t* valid, float* rgb_out) {
    const int n = check_lattice_shape(__func__, nu, nv, nw, DURF_TSDF_MAX_POINTS);
    if (n < 0) return -1;
    DURF_REQUIREF(min_weight == min_weight, "min_weight is a number, min_weight = %g", (double)min_weight);
    DURF_REQUIRE(tsdf, "tsdf");
    DURF_REQUIRE(weight, "weight");
    DURF_REQUIRE(density, "density");
    DURF_REQUIRE(valid, "valid");
    DURF_REQUIRE(colour || !rgb_out, "colour with rgb_out");
    DURF_REQUIRE(tsdf_aligned16(colour), "colour aligned to 16 bytes");
    hipLaunchKernelGGL(k_tsdf_lattice, dim3(durf_cdiv((size_t)n, TB)), dim3(TB), 0, (hipStream_t)stream, n, tsdf, weight, colour, min_weight,
                       density, valid, rgb_out);
    DURF_CHECK_LAUNCH("k_tsdf_lattice");
    return 0;
}

int durf_tsdf_sample(void* stream, int nu, int nv, int nw, const float* origin_host, const float* inv_host, const float* tsdf,
                     const float* weight, const float* colour, float trunc, float min_weight, int m, const float* points, float* sdf,
                     uint8_t* ok, float* rgb_out) {
    const int n = check_lattice_shape(__func__, nu, nv, nw, DURF_TSDF_MAX_POINTS);
    if (n < 0) return -1;
    DURF_REQUIREF(m >= 0, "m >= 0, m = %d", m);
    DURF_REQUIREF(trunc > 0.0f && trunc <= FLT_MAX, "trunc > 0 and finite, trunc = %g", (double)trunc);
    DURF_REQUIREF(min_weight == min_weight, "min_weight is a number, min_weight = %g", (double)min_weight);
    DURF_REQUIRE(origin_host, "origin_host");
    DURF_REQUIRE(inv_host, "inv_host");
    DURF_REQUIRE(tsdf, "tsdf");
    DURF_REQUIRE(weight, "weight");
    DURF_REQUIREF(points || m == 0, "points for m = %d", m);
    DURF_REQUIREF((sdf && ok) || m == 0, "sdf and ok for m = %d", m);
    DURF_REQUIRE(colour || !rgb_out, "colour with rgb_out");
    DURF_REQUIRE(tsdf_aligned16(colour), "colour aligned to 16 bytes");
    if (m == 0) return 0;
    TsdfInverse Q;
    for (int c = 0; c < 3; c++) Q.origin[c] = origin_host[c];
    for (int c = 0; c < 9; c++) Q.inv[c] = inv_host[c];
    hipLaunchKernelGGL(k_tsdf_sample, dim3(durf_cdiv((size_t)m, TB)), dim3(TB), 0, (hipStream_t)stream, nu, nv, nw, Q, tsdf, weight, colour,
                       trunc, min_weight, m, points, sdf, ok, rgb_out);
    DURF_CHECK_LAUNCH("k_tsdf_sample");
    return 0;
}

}  // extern "C"
