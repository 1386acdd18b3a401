// How the scene moves between two frames (include/durf_flow.h; libdurf_flow.so): where every pixel of a rendered frame lands in
// another frame and how far it travels in the world (k_flow_poses, k_flow_points), that other frame warped back with an occlusion
// test (k_flow_warp), a deterministic two-pass consistency reduction (k_flow_cons_partial, k_flow_cons_final), the Middlebury flow
// picture (k_flow_color), and durf_render_flow, which walks P pairs of frames in chunks through durf_camera_rays and
// durf_ray_setup_masked of libdurf_hip.so.  Five streaming kernels, one thread per pixel, plain fp32 in the order the header
// states; nothing here synchronises or copies to the host.
#include "workspace.h"
#include "aa2matrix.h"
#include "camera.h"
#include "../../include/durf_flow.h"

#define FLOW_THREADS 256

// ---- where a pixel goes -----------------------------------------------------------------------------------------------------
struct FlowCams {
    CamRow a, b;
};

struct FlowOut {
    float *flow, *scene_flow, *xyz, *target, *zcam;
    int32_t *moving, *valid;
};

// one wave: thread s K + k turns pose s (0: a, 1: b) of box k into its row of the table
__global__ void __launch_bounds__(64)
k_flow_poses(int K, const float* __restrict__ pose_a, const float* __restrict__ pose_b, float* __restrict__ table) {
    const int j = threadIdx.x;
    if (j >= 2 * K) return;
    const int s = j / K, k = j - s * K;
    pose_row_fill((s ? pose_b : pose_a) + k * 6, table + j * DURF_POSE_ROW);        // j < 2 K: inside DURF_FLOW_POSE_FLOATS(K)
}

// one thread per pixel: consecutive lanes read and write consecutive pixels.  The box loop runs over k, the same in every lane,
// and enters a box only where a lane of the wave hit it, so the table is read at wave-uniform addresses; which lanes share a
// wave changes no lane's arithmetic.  Multi-hit and invalid pixels go through the same projection and are replaced at the end.
__global__ void __launch_bounds__(FLOW_THREADS)
k_flow_points(int n, int first, int w, int K, const float* __restrict__ origins_s, const float* __restrict__ dirs_s,
              const int32_t* __restrict__ hit, const float* __restrict__ t, const float* __restrict__ acc, FlowCams cams,
              const float* __restrict__ table, const float* __restrict__ ext, int normalise, float min_acc, float znear,
              float inside_tol, FlowOut out) {
    const int i = blockIdx.x * FLOW_THREADS + threadIdx.x;
    const bool live = i < n;
    const size_t r = live ? (size_t)i : 0;           // (n >= 1 where this is launched: row 0 exists)
    const float ac = acc[r];
    const float tt = normalise ? t[r] / ac : t[r];
    const float P0 = origins_s[r * 3 + 0] + tt * dirs_s[r * 3 + 0];
    const float P1 = origins_s[r * 3 + 1] + tt * dirs_s[r * 3 + 1];
    const float P2 = origins_s[r * 3 + 2] + tt * dirs_s[r * 3 + 2];
    float Xa[3] = {P0, P1, P2}, Xb[3] = {P0, P1, P2};
    int nh = 0, mv = -1;
    const float grow = 1.0f + inside_tol;
    for (int k = 0; k < K; k++) {
        const bool h = live && hit[r * K + k] != 0;
        if (__ballot(h) != 0ull) {                   // (uniform over the wave)
            float A[3], B[3];
            pose_to_world(table + k * DURF_POSE_ROW, P0, P1, P2, A);
            pose_to_world(table + (K + k) * DURF_POSE_ROW, P0, P1, P2, B);
            const bool in = fabsf(P0) <= ext[k * 3 + 0] * grow && fabsf(P1) <= ext[k * 3 + 1] * grow &&
                            fabsf(P2) <= ext[k * 3 + 2] * grow;
#pragma unroll
            for (int j = 0; j < 3; j++) {
                Xa[j] = h ? A[j] : Xa[j];
                Xb[j] = h ? (in ? B[j] : A[j]) : Xb[j];
            }
            mv = h ? (in ? k : -1) : mv;
        }
        nh += h ? 1 : 0;
    }
    if (!live) return;
    const int p = first + i;                         // < h w < 2^31 (checked by the caller)
    const int y = p / w, x = p - y * w;
    float pa[3], pb[3], xa, ya, xb, yb;
    cam_to_camera(cams.a.v, Xa[0], Xa[1], Xa[2], pa);
    const float za = -pa[2];
    cam_pixel(cams.a.v, pa[0], pa[1], za, xa, ya);
    cam_to_camera(cams.b.v, Xb[0], Xb[1], Xb[2], pb);
    const float zb = -pb[2];
    cam_pixel(cams.b.v, pb[0], pb[1], zb, xb, yb);
    const bool ok = ac >= min_acc && nh <= 1 && isfinite(tt) && zb >= znear;
    const float nan = __builtin_nanf("");
    if (out.flow) *(f32x2*)(out.flow + r * 2) = f32x2{ok ? xb - (float)x : nan, ok ? yb - (float)y : nan};
    if (out.scene_flow) {
#pragma unroll
        for (int j = 0; j < 3; j++) out.scene_flow[r * 3 + j] = ok ? Xb[j] - Xa[j] : nan;
    }
    if (out.xyz) {
#pragma unroll
        for (int j = 0; j < 3; j++) out.xyz[r * 3 + j] = ok ? Xa[j] : nan;
    }
    if (out.target) {
        out.target[r * 3 + 0] = ok ? xb : nan;
        out.target[r * 3 + 1] = ok ? yb : nan;
        out.target[r * 3 + 2] = ok ? zb : nan;
    }
    if (out.zcam) out.zcam[r] = ok ? za : nan;
    if (out.moving) out.moving[r] = ok ? mv : -2;
    if (out.valid) out.valid[r] = ok ? 1 : 0;
}

static int launch_flow_poses(void* stream, int K, const float* pose_a, const float* pose_b, float* table) {
    if (K == 0) return 0;
    hipLaunchKernelGGL(k_flow_poses, dim3(1), dim3(64), 0, (hipStream_t)stream, K, pose_a, pose_b, table);
    DURF_CHECK_LAUNCH("k_flow_poses");
    return 0;
}

static int launch_flow_points(void* stream, int n, int first, int K, const float* origins_s, const float* dirs_s, const int32_t* hit,
                              const float* t, const float* acc, const FlowCams& cams, const float* table, const float* ext,
                              int normalise, float min_acc, float znear, float inside_tol, const FlowOut& out) {
    hipLaunchKernelGGL(k_flow_points, dim3(durf_cdiv(n, FLOW_THREADS)), dim3(FLOW_THREADS), 0, (hipStream_t)stream, n, first,
                       (int)cams.a.v[DURF_CAM_W], K, origins_s, dirs_s, hit, t, acc, cams, table, ext, normalise, min_acc, znear, inside_tol, out);
    DURF_CHECK_LAUNCH("k_flow_points");
    return 0;
}

// ---- backward warp ------------------------------------------------------------------------------------------------------------
template <int C>
__global__ void __launch_bounds__(FLOW_THREADS)
k_flow_warp(int n, int h, int w, const float* __restrict__ target, const int32_t* __restrict__ valid, const float* __restrict__ img,
            const float* __restrict__ zc, float occ_rel, float occ_abs, float* __restrict__ warped, int32_t* __restrict__ mask) {
    const int i = blockIdx.x * FLOW_THREADS + threadIdx.x;
    if (i >= n) return;
    const size_t r = (size_t)i;
    const float xp = target[r * 3 + 0], yp = target[r * 3 + 1], zb = target[r * 3 + 2];
    const bool inframe = xp >= 0.0f && xp <= (float)(w - 1) && yp >= 0.0f && yp <= (float)(h - 1);
    const float xs = inframe ? xp : 0.0f, ys = inframe ? yp : 0.0f;      // every index below is inside the picture
    const int x0 = max(min((int)floorf(xs), w - 2), 0), x1 = min(x0 + 1, w - 1);
    const int y0 = max(min((int)floorf(ys), h - 2), 0), y1 = min(y0 + 1, h - 1);
    const float fx = w == 1 ? 0.0f : xs - (float)x0, fy = h == 1 ? 0.0f : ys - (float)y0;
    const int xr = (int)rintf(xs), yr = (int)rintf(ys);                  // in [0, w - 1], [0, h - 1]
    const float zs = zc[(size_t)yr * w + xr];
    const bool vis = valid[r] != 0 && inframe && isfinite(zs) && zb <= zs * (1.0f + occ_rel) + occ_abs;
    if (mask) mask[r] = vis ? 1 : 0;
    if (!warped) return;
    const float* r0 = img + (size_t)y0 * w * C;
    const float* r1 = img + (size_t)y1 * w * C;
    const float nan = __builtin_nanf("");
#pragma unroll
    for (int c = 0; c < C; c++) {
        const float v00 = r0[(size_t)x0 * C + c], v10 = r0[(size_t)x1 * C + c];
        const float v01 = r1[(size_t)x0 * C + c], v11 = r1[(size_t)x1 * C + c];
        const float v = (1.0f - fy) * ((1.0f - fx) * v00 + fx * v10) + fy * ((1.0f - fx) * v01 + fx * v11);
        warped[r * C + c] = vis ? v : nan;
    }
}

// ---- temporal consistency -----------------------------------------------------------------------------------------------------
#define FLOW_WAVES (FLOW_THREADS / DURF_WAVE)

// pass 1: workgroup g of pair p sums its span of DURF_FLOW_CONS_SPAN pixels into one triple
template <int C>
__global__ void __launch_bounds__(FLOW_THREADS)
k_flow_cons_partial(int m, int G, const float* __restrict__ warped, const float* __restrict__ img_a, const int32_t* __restrict__ mask,
                    float* __restrict__ scratch) {
    __shared__ float s_part[3][FLOW_WAVES];
    const int t = threadIdx.x, g = blockIdx.x, p = blockIdx.y;
    const size_t base = (size_t)p * m;
    const long long lo = (long long)g * DURF_FLOW_CONS_SPAN;
    const long long hi = lo + DURF_FLOW_CONS_SPAN < (long long)m ? lo + DURF_FLOW_CONS_SPAN : (long long)m;
    float cnt = 0.0f, sse = 0.0f, sae = 0.0f;
    for (long long q = lo + t; q < hi; q += FLOW_THREADS) {
        const size_t at = base + (size_t)q;
        if (mask[at] != 0) {
#pragma unroll
            for (int c = 0; c < C; c++) {
                const float d = warped[at * C + c] - img_a[at * C + c];
                sse += d * d;
                sae += fabsf(d);
            }
            cnt += 1.0f;
        }
    }
    cnt = wave_sum(cnt); sse = wave_sum(sse); sae = wave_sum(sae);
    if ((t & (DURF_WAVE - 1)) == 0) {
        s_part[0][t / DURF_WAVE] = cnt; s_part[1][t / DURF_WAVE] = sse; s_part[2][t / DURF_WAVE] = sae;
    }
    __syncthreads();
    if (t < 3) scratch[((size_t)p * G + g) * 3 + t] = (s_part[t][0] + s_part[t][1]) + (s_part[t][2] + s_part[t][3]);
}

// pass 2: one workgroup per pair; lane q < 3 adds quantity q of the pair's G triples in index order, in double
__global__ void __launch_bounds__(DURF_WAVE)
k_flow_cons_final(int G, int C, const float* __restrict__ scratch, float* __restrict__ out) {
    __shared__ double s_sum[3];
    const int t = threadIdx.x, p = blockIdx.x;
    if (t < 3) {
        double a = 0.0;
        for (int g = 0; g < G; g++) a += (double)scratch[((size_t)p * G + g) * 3 + t];
        s_sum[t] = a;
    }
    __syncthreads();
    if (t != 0) return;
    const double cnt = s_sum[0], sse = s_sum[1], sae = s_sum[2];
    double psnr;
    if (cnt == 0.0) psnr = (double)__builtin_nanf("");
    else if (sse == 0.0) psnr = (double)__builtin_inff();
    else psnr = -10.0 * log10(sse / (cnt * (double)C));
    float* o = out + (size_t)p * DURF_FLOW_CONS_FLOATS;
    o[0] = (float)cnt; o[1] = (float)sse; o[2] = (float)sae; o[3] = (float)psnr;
}

// ---- the flow picture ---------------------------------------------------------------------------------------------------------
struct FlowWheel {
    unsigned char v[DURF_FLOW_WHEEL][3];
};

// the Middlebury colour wheel, built at compile time from its description: six ramps between the primaries and secondaries
constexpr FlowWheel flow_make_wheel() {
    FlowWheel W{};
    int k = 0;
    for (int i = 0; i < 15; i++, k++) { W.v[k][0] = 255; W.v[k][1] = (unsigned char)(255 * i / 15); W.v[k][2] = 0; }          // red -> yellow
    for (int i = 0; i < 6; i++, k++) { W.v[k][0] = (unsigned char)(255 - 255 * i / 6); W.v[k][1] = 255; W.v[k][2] = 0; }      // yellow -> green
    for (int i = 0; i < 4; i++, k++) { W.v[k][0] = 0; W.v[k][1] = 255; W.v[k][2] = (unsigned char)(255 * i / 4); }            // green -> cyan
    for (int i = 0; i < 11; i++, k++) { W.v[k][0] = 0; W.v[k][1] = (unsigned char)(255 - 255 * i / 11); W.v[k][2] = 255; }    // cyan -> blue
    for (int i = 0; i < 13; i++, k++) { W.v[k][0] = (unsigned char)(255 * i / 13); W.v[k][1] = 0; W.v[k][2] = 255; }          // blue -> magenta
    for (int i = 0; i < 6; i++, k++) { W.v[k][0] = 255; W.v[k][1] = 0; W.v[k][2] = (unsigned char)(255 - 255 * i / 6); }      // magenta -> red
    return W;
}
constexpr FlowWheel FLOW_WHEEL = flow_make_wheel();
static_assert(15 + 6 + 4 + 11 + 13 + 6 == DURF_FLOW_WHEEL, "the six ramps fill the wheel");
static_assert(FLOW_WHEEL.v[0][0] == 255 && FLOW_WHEEL.v[0][1] == 0 && FLOW_WHEEL.v[0][2] == 0, "the wheel starts at pure red");
static_assert(FLOW_WHEEL.v[54][0] == 255 && FLOW_WHEEL.v[54][1] == 0 && FLOW_WHEEL.v[54][2] == 43, "and ends one step before it");
__constant__ FlowWheel c_flow_wheel = FLOW_WHEEL;

__global__ void __launch_bounds__(FLOW_THREADS)
k_flow_color(int n, const float* __restrict__ flow, float max_mag, float* __restrict__ rgb, uint8_t* __restrict__ rgb8) {
    const int i = blockIdx.x * FLOW_THREADS + threadIdx.x;
    if (i >= n) return;
    const size_t r = (size_t)i;
    const f32x2 uv = *(const f32x2*)(flow + r * 2);
    const float u = uv[0], v = uv[1];
    const bool ok = isfinite(u) && isfinite(v);
    const float us = ok ? u : 0.0f, vs = ok ? v : 0.0f;
    const float rad = sqrtf(us * us + vs * vs) / max_mag;
    const float a = atan2f(-vs, -us) / 3.14159265358979323846f;
    const float fk = ((a + 1.0f) / 2.0f) * (float)(DURF_FLOW_WHEEL - 1);
    const int k0 = max(min((int)fk, DURF_FLOW_WHEEL - 1), 0);
    const int k1 = k0 + 1 == DURF_FLOW_WHEEL ? 0 : k0 + 1;
    const float f = fk - (float)k0;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const float c0 = (float)c_flow_wheel.v[k0][c] / 255.0f, c1 = (float)c_flow_wheel.v[k1][c] / 255.0f;
        float col = (1.0f - f) * c0 + f * c1;
        col = rad <= 1.0f ? 1.0f - rad * (1.0f - col) : col * 0.75f;
        col = ok ? col : 0.0f;
        if (rgb) rgb[r * 3 + c] = col;
        if (rgb8) rgb8[r * 3 + c] = (uint8_t)rintf(col * 255.0f);
    }
}

// ---- P pairs in one call ------------------------------------------------------------------------------------------------------
namespace {
struct FlowWs {
    float* rays[6];
    float *o_s, *d_s, *zo, *table;
    int32_t* hit;
    size_t total;
};

FlowWs carve_flow(void* base, int chunk, int K) {
    durf::Carver c{(char*)base, 0};
    FlowWs w{};
    const size_t B = chunk > 0 ? chunk : 0, Kc = K > 0 ? K : 1;
    for (int i = 0; i < 6; i++) w.rays[i] = (float*)c.take(B * (i < 3 ? 3 : 1) * 4);
    w.o_s = (float*)c.take(B * 3 * 4);
    w.d_s = (float*)c.take(B * 3 * 4);
    w.hit = (int32_t*)c.take(B * Kc * 4);
    w.zo = (float*)c.take(B * 4);
    w.table = (float*)c.take((size_t)DURF_FLOW_POSE_FLOATS(Kc) * 4);
    w.total = c.total();
    return w;
}

// the refusals durf_flow_points and durf_render_flow share
int check_flow_scalars(const char* who, int K, float znear, float inside_tol) {
    if (!(K >= 0 && K <= DURF_MAX_OBJ)) {
        durf_set_error("%s: requirement failed: 0 <= K <= DURF_MAX_OBJ (%d), K = %d", who, DURF_MAX_OBJ, K);
        return -1;
    }
    if (!(znear > 0.0f)) {
        durf_set_error("%s: requirement failed: znear > 0, znear = %g", who, (double)znear);
        return -1;
    }
    if (!(inside_tol >= 0.0f)) {
        durf_set_error("%s: requirement failed: inside_tol >= 0, inside_tol = %g", who, (double)inside_tol);
        return -1;
    }
    return 0;
}
}  // namespace

extern "C" {

int durf_flow_points(void* stream, int n, int first, int K, const float* origins_s, const float* dirs_s, const int32_t* hit,
                     const float* t, const float* acc, const float* cam_a_host, const float* cam_b_host, const float* pose_a,
                     const float* pose_b, const float* ext, int normalise, float min_acc, float znear, float inside_tol,
                     float* pose_scratch, float* flow, float* scene_flow, float* xyz, float* target, float* zcam, int32_t* moving,
                     int32_t* valid) {
    DURF_REQUIREF(n >= 0 && first >= 0, "n >= 0 and first >= 0, n = %d, first = %d", n, first);
    int rc = check_flow_scalars(__func__, K, znear, inside_tol);
    if (rc != 0) return rc;
    DURF_REQUIREF(cam_a_host && cam_b_host, "the two camera rows");
    const float ha = cam_a_host[DURF_CAM_H], wa = cam_a_host[DURF_CAM_W];
    DURF_REQUIREF(ha >= 1.0f && wa >= 1.0f && (double)ha * wa < 2147483648.0, "an image of h >= 1, w >= 1, h w < 2^31, h = %g, w = %g",
                 (double)ha, (double)wa);
    const long long hw = (long long)(int)ha * (int)wa;
    DURF_REQUIREF((long long)first + n <= hw, "pixels [first, first + n) inside the image, first = %d, n = %d, h w = %lld", first, n, hw);
    if (n == 0) return 0;
    DURF_REQUIREF(flow || scene_flow || xyz || target || zcam || moving || valid, "at least one output");
    DURF_REQUIREF(origins_s && dirs_s && t && acc, "origins_s, dirs_s, t and acc");
    DURF_REQUIREF(K == 0 || (hit && pose_a && pose_b && ext && pose_scratch), "hit, pose_a, pose_b, ext and pose_scratch for K = %d", K);
    DURF_REQUIREF(((size_t)flow & 7) == 0, "flow is 8-byte aligned");
    const FlowCams cams{cam_row(cam_a_host), cam_row(cam_b_host)};
    if ((rc = launch_flow_poses(stream, K, pose_a, pose_b, pose_scratch)) != 0) return rc;
    const FlowOut out{flow, scene_flow, xyz, target, zcam, moving, valid};
    return launch_flow_points(stream, n, first, K, origins_s, dirs_s, hit, t, acc, cams, pose_scratch, ext, normalise, min_acc, znear,
                              inside_tol, out);
}

int durf_flow_warp(void* stream, int n, int h, int w, int C, const float* target, const int32_t* valid, const float* img_b,
                   const float* zcam_b, float occ_rel, float occ_abs, float* warped, int32_t* mask) {
    DURF_REQUIREF(n >= 0, "n >= 0, n = %d", n);
    DURF_REQUIREF(h >= 1 && w >= 1 && (long long)h * w < 2147483648ll, "h >= 1, w >= 1, h w < 2^31, h = %d, w = %d", h, w);
    DURF_REQUIREF(C == 1 || C == 3, "C is 1 or 3, C = %d", C);
    DURF_REQUIREF(occ_rel >= 0.0f && occ_abs >= 0.0f, "occ_rel >= 0 and occ_abs >= 0, occ_rel = %g, occ_abs = %g", (double)occ_rel,
                 (double)occ_abs);
    if (n == 0) return 0;
    DURF_REQUIREF(warped || mask, "at least one output");
    DURF_REQUIREF(target && valid && img_b && zcam_b, "target, valid, img_b and zcam_b");
    const dim3 grid(durf_cdiv(n, FLOW_THREADS)), block(FLOW_THREADS);
    if (C == 1)
        hipLaunchKernelGGL(k_flow_warp<1>, grid, block, 0, (hipStream_t)stream, n, h, w, target, valid, img_b, zcam_b, occ_rel, occ_abs,
                           warped, mask);
    else
        hipLaunchKernelGGL(k_flow_warp<3>, grid, block, 0, (hipStream_t)stream, n, h, w, target, valid, img_b, zcam_b, occ_rel, occ_abs,
                           warped, mask);
    DURF_CHECK_LAUNCH("k_flow_warp");
    return 0;
}

int durf_flow_consistency(void* stream, int P, int m, int C, const float* warped, const float* img_a, const int32_t* mask, float* out,
                          float* scratch) {
    DURF_REQUIREF(P >= 0 && P <= 65535, "0 <= P <= 65535 (the pair is the grid's y), P = %d", P);
    DURF_REQUIREF(m >= 1, "m >= 1 pixels, m = %d", m);
    DURF_REQUIREF(C == 1 || C == 3, "C is 1 or 3, C = %d", C);
    if (P == 0) return 0;
    DURF_REQUIREF(warped && img_a && mask && out && scratch, "warped, img_a, mask, out and scratch");
    const int G = DURF_FLOW_CONS_GROUPS(m);
    const dim3 grid(G, P), block(FLOW_THREADS);
    if (C == 1)
        hipLaunchKernelGGL(k_flow_cons_partial<1>, grid, block, 0, (hipStream_t)stream, m, G, warped, img_a, mask, scratch);
    else
        hipLaunchKernelGGL(k_flow_cons_partial<3>, grid, block, 0, (hipStream_t)stream, m, G, warped, img_a, mask, scratch);
    DURF_CHECK_LAUNCH("k_flow_cons_partial");
    hipLaunchKernelGGL(k_flow_cons_final, dim3(P), dim3(DURF_WAVE), 0, (hipStream_t)stream, G, C, scratch, out);
    DURF_CHECK_LAUNCH("k_flow_cons_final");
    return 0;
}

int durf_flow_color(void* stream, int n, const float* flow, float max_mag, float* rgb, uint8_t* rgb8) {
    DURF_REQUIREF(n >= 0, "n >= 0, n = %d", n);
    DURF_REQUIREF(max_mag > 0.0f, "max_mag > 0, max_mag = %g", (double)max_mag);
    if (n == 0) return 0;
    DURF_REQUIREF(rgb || rgb8, "at least one output");
    DURF_REQUIREF(flow != nullptr && ((size_t)flow & 7) == 0, "flow is given and 8-byte aligned");
    hipLaunchKernelGGL(k_flow_color, dim3(durf_cdiv(n, FLOW_THREADS)), dim3(FLOW_THREADS), 0, (hipStream_t)stream, n, flow, max_mag, rgb,
                       rgb8);
    DURF_CHECK_LAUNCH("k_flow_color");
    return 0;
}

size_t durf_render_flow_workspace_bytes(int chunk, int K) { return carve_flow(nullptr, chunk, K).total; }

int durf_render_flow(void* stream, int F, int K, const float* cams_host, const float* poses, const float* ext, const int32_t* box_enable,
                     const float* distance, const float* acc, int P, const int* pairs_host, float near, float far, int chunk,
                     int normalise, float min_acc, float znear, float inside_tol, float* flow, float* scene_flow, float* xyz,
                     float* target, float* zcam, int32_t* moving, int32_t* valid, void* workspace, size_t workspace_bytes) {
    DURF_REQUIREF(F > 0, "F > 0 frames, F = %d", F);
    DURF_REQUIREF(P > 0, "P > 0 pairs, P = %d", P);
    int rc = check_flow_scalars(__func__, K, znear, inside_tol);
    if (rc != 0) return rc;
    DURF_REQUIREF(chunk > 0, "chunk > 0, chunk = %d", chunk);
    DURF_REQUIREF(flow || scene_flow || xyz || target || zcam || moving || valid, "at least one output");
    DURF_REQUIREF(cams_host && pairs_host, "the camera rows and the pairs");
    for (int p = 0; p < P; p++)
        for (int s = 0; s < 2; s++) {
            const int f = pairs_host[p * 2 + s];
            DURF_REQUIREF(f >= 0 && f < F, "pair %d names frame %d outside [0, %d)", p, f, F);
        }
    const float hf = cams_host[DURF_CAM_H], wf = cams_host[DURF_CAM_W];
    DURF_REQUIREF(hf >= 2.0f && wf >= 1.0f && (double)hf * wf < 134217728.0, "frames of h >= 2, w >= 1, h w < 2^27, h = %g, w = %g",
                 (double)hf, (double)wf);
    for (int f = 1; f < F; f++) {
        const float* cam = cams_host + (size_t)f * DURF_CAM_FLOATS;
        DURF_REQUIREF(cam[DURF_CAM_H] == hf && cam[DURF_CAM_W] == wf, "frames of different sizes: frame %d is %g x %g, frame 0 is %g x %g",
                     f, (double)cam[DURF_CAM_H], (double)cam[DURF_CAM_W], (double)hf, (double)wf);
    }
    DURF_REQUIREF(distance && acc && (K == 0 || (poses && ext)), "distance, acc, and the box poses and extents for K = %d", K);
    DURF_REQUIREF(((size_t)flow & 7) == 0, "flow is 8-byte aligned");
    DURF_REQUIREF(workspace != nullptr && ((size_t)workspace & 255) == 0, "workspace aligned to 256 bytes");
    const FlowWs w = carve_flow(workspace, chunk, K);
    rc = durf::check_workspace("durf_render_flow", workspace_bytes, w.total, "durf_render_flow_workspace_bytes(%d, %d)", chunk, K);
    if (rc != 0) return rc;
    const size_t n = (size_t)(int)hf * (int)wf;
    for (int p = 0; p < P; p++) {
        const int fa = pairs_host[p * 2], fb = pairs_host[p * 2 + 1];
        const float* cam_a = cams_host + (size_t)fa * DURF_CAM_FLOATS;
        const float* pose_a = K > 0 ? poses + (size_t)fa * K * 6 : nullptr;
        const FlowCams cams{cam_row(cam_a), cam_row(cams_host + (size_t)fb * DURF_CAM_FLOATS)};
        if ((rc = launch_flow_poses(stream, K, pose_a, K > 0 ? poses + (size_t)fb * K * 6 : nullptr, w.table)) != 0) return rc;
        for (size_t i = 0; i < n; i += (size_t)chunk) {
            const int B = (int)(n - i < (size_t)chunk ? n - i : (size_t)chunk);
            rc = durf_camera_rays(stream, cam_a, (int)i, B, near, far, w.rays[0], w.rays[1], w.rays[2], w.rays[3], w.rays[4], w.rays[5]);
            if (rc != 0) return rc;
            rc = durf_ray_setup_masked(stream, B, K, w.rays[0], w.rays[1], pose_a, ext, box_enable, w.o_s, w.d_s, w.hit, w.zo);
            if (rc != 0) return rc;
            const size_t at = (size_t)p * n + i;
            const FlowOut out{flow ? flow + at * 2 : nullptr, scene_flow ? scene_flow + at * 3 : nullptr, xyz ? xyz + at * 3 : nullptr,
                              target ? target + at * 3 : nullptr, zcam ? zcam + at : nullptr, moving ? moving + at : nullptr,
                              valid ? valid + at : nullptr};
            rc = launch_flow_points(stream, B, (int)i, K, w.o_s, w.d_s, w.hit, distance + (size_t)fa * n + i, acc + (size_t)fa * n + i,
                                    cams, w.table, ext, normalise, min_acc, znear, inside_tol, out);
            if (rc != 0) return rc;
        }
    }
    return 0;
}

}  // extern "C"
