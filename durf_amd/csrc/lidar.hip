// LIDAR sweeps (include/durf_lidar.h; libdurf_lidar.so): the rays of a spinning multi-beam sensor in front of the renderer
// (k_lidar_rays), the return model behind it -- quantiles of every ray's weight distribution out of one wave scan
// (k_lidar_returns) --, the valid returns compacted into a point cloud in three plain passes (k_lidar_count, k_scan_block_sums
// of scan.h, k_lidar_scatter), and durf_render_lidar, which walks F sweeps in chunks through durf_forward_masked of
// libdurf_hip.so.  Plain fp32 in the order the header states; nothing here synchronises or copies to the host.
#include "workspace.h"
#include "scan.h"
#include "../../include/durf_lidar.h"

// ---- the sensor ----------------------------------------------------------------------------------------------------------
struct LidarSweep {
    int H, W;
    float az0, az_span, radius, near, far;
    float R[9], p[3], om[3], dp[3];
};

// one thread per ray: r = first + i, consecutive lanes write consecutive rays
__global__ void __launch_bounds__(256)
k_lidar_rays(LidarSweep S, const float* __restrict__ incl, int first, int count, float* __restrict__ origins,
             float* __restrict__ directions, float* __restrict__ viewdirs, float* __restrict__ radii, float* __restrict__ near_out,
             float* __restrict__ far_out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const int r = first + i;
    const int h = r / S.W, w = r - h * S.W;
    const float s = ((float)w + 0.5f) / (float)S.W;
    const float phi = S.az0 + s * S.az_span;
    const float th = incl[h];
    const float ct = cosf(th), st = sinf(th);
    const float d0 = ct * cosf(phi), d1 = ct * sinf(phi), d2 = st;
    const float v0 = s * S.om[0], v1 = s * S.om[1], v2 = s * S.om[2];
    const float t2 = (v0 * v0 + v1 * v1) + v2 * v2;
    float a = 1.0f, b = 0.5f;
    if (!(t2 < 1e-12f)) {
        const float t = sqrtf(t2);
        const float sh = sinf(0.5f * t);
        a = sinf(t) / t;
        b = ((2.0f * sh) * sh) / t2;
    }
    const float c0 = v1 * d2 - v2 * d1, c1 = v2 * d0 - v0 * d2, c2 = v0 * d1 - v1 * d0;          // v x d
    const float e0 = v1 * c2 - v2 * c1, e1 = v2 * c0 - v0 * c2, e2 = v0 * c1 - v1 * c0;          // v x (v x d)
    const float q0 = (d0 + a * c0) + b * e0, q1 = (d1 + a * c1) + b * e1, q2 = (d2 + a * c2) + b * e2;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const float dk = (S.R[k * 3 + 0] * q0 + S.R[k * 3 + 1] * q1) + S.R[k * 3 + 2] * q2;
        directions[(size_t)i * 3 + k] = dk;
        viewdirs[(size_t)i * 3 + k] = dk;
        origins[(size_t)i * 3 + k] = S.p[k] + s * S.dp[k];
    }
    radii[i] = S.radius;
    near_out[i] = S.near;
    far_out[i] = S.far;
}

// the sensor row and one sweep row -> the kernel's argument block; the refusals of both callers
static int lidar_sweep_args(const float* sensor, const float* sweep, float near, float far, LidarSweep* S) {
    DURF_REQUIRE(sensor != nullptr, "the sensor row");
    DURF_REQUIRE(sensor[0] >= 1.0f && sensor[0] < 65536.0f, "H > 0 beams (and < 65536)");
    DURF_REQUIRE(sensor[1] >= 1.0f && sensor[1] < 16777216.0f, "W > 0 azimuth columns (and < 2^24)");
    S->H = (int)sensor[0]; S->W = (int)sensor[1];
    DURF_REQUIRE((size_t)S->H * S->W < ((size_t)1 << 27), "H * W < 2^27");
    S->az0 = sensor[2]; S->az_span = sensor[3];
    S->radius = (float)((double)sensor[4] * fabs((double)sensor[3]) / (double)S->W * 2.0 / sqrt(12.0));
    S->near = near; S->far = far;
    if (sweep) {
        for (int i = 0; i < 3; i++) {
            for (int j = 0; j < 3; j++) S->R[i * 3 + j] = sweep[i * 4 + j];
            S->p[i] = sweep[i * 4 + 3];
            S->om[i] = sweep[12 + i];
            S->dp[i] = sweep[15 + i];
        }
    }
    return 0;
}

static int launch_lidar_rays(void* stream, const LidarSweep& S, const float* incl, int first, int count, float* const rays[6]) {
    hipLaunchKernelGGL(k_lidar_rays, dim3(durf_cdiv(count, 256)), dim3(256), 0, (hipStream_t)stream, S, incl, first, count, rays[0],
                       rays[1], rays[2], rays[3], rays[4], rays[5]);
    DURF_CHECK_LAUNCH("k_lidar_rays");
    return 0;
}

// ---- the return model -------------------------------------------------------------------------------------------------------
#define LIDAR_RET_WAVES 4               // rays per workgroup: one wavefront each
#define LIDAR_MAX_PER_LANE 4            // N <= 256 samples over 64 lanes

struct LidarReturns {
    float q[3];                         // q, q_lo, q_hi
    float min_acc, max_range;
    int to_sensor;
    float M[12];
};

__global__ void __launch_bounds__(LIDAR_RET_WAVES * DURF_WAVE)
k_lidar_returns(int n, int N, const float* __restrict__ weights, const float* __restrict__ t_vals, const float* __restrict__ acc,
                const float* __restrict__ origins, const float* __restrict__ directions, LidarReturns A, float* __restrict__ range_q,
                float* __restrict__ range_mean, int32_t* __restrict__ valid, float* __restrict__ xyz, float* __restrict__ spread) {
    const int lane = threadIdx.x & (DURF_WAVE - 1);
    const int ray = blockIdx.x * LIDAR_RET_WAVES + threadIdx.x / DURF_WAVE;
    if (ray >= n) return;                                     // (uniform over the wave)
    // lane l owns samples [lo, lo + cnt): contiguous, so a wave reads the ray's rows once, front to back
    const int lo = lane * N / DURF_WAVE, cnt = (lane + 1) * N / DURF_WAVE - lo;
    const float* wr = weights + (size_t)ray * N + lo;
    const float* tr = t_vals + (size_t)ray * (N + 1) + lo;     // lo + cnt <= N: t[cnt] is inside the row
    float w[LIDAR_MAX_PER_LANE], t[LIDAR_MAX_PER_LANE + 1];
#pragma unroll
    for (int i = 0; i < LIDAR_MAX_PER_LANE; i++) w[i] = i < cnt ? wr[i] : 0.0f;
#pragma unroll
    for (int i = 0; i <= LIDAR_MAX_PER_LANE; i++) t[i] = i <= cnt ? tr[i] : 0.0f;
    float s = 0.0f, m = 0.0f;
#pragma unroll
    for (int i = 0; i < LIDAR_MAX_PER_LANE; i++)
        if (i < cnt) {
            s += w[i];
            m += w[i] * (0.5f * (t[i] + t[i + 1]));
        }
    const float incl = wave_incl_scan(s, lane);              // c at the lane's last sample
    float excl = __shfl_up(incl, 1, DURF_WAVE);              // c before its first
    if (lane == 0) excl = 0.0f;
    const float W = __shfl(incl, DURF_WAVE - 1, DURF_WAVE);
    const float msum = wave_sum(m);
    const unsigned long long some = __ballot(s > 0.0f);      // lanes that own a positive weight
    float rq[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const float tau = A.q[k] * W;
        // the crossing lane: the first that owns a positive weight and ends at or beyond tau.  The scan's sums are rounded
        // lane by lane, so beside q -> 1 no lane may reach tau: the last lane with a positive weight then takes it.
        const unsigned long long cross = __ballot(s > 0.0f && incl >= tau);
        const int src = cross ? __ffsll((long long)cross) - 1 : (some ? 63 - __clzll((long long)some) : 0);
        float r = 0.0f;
        if (lane == src && s > 0.0f) {
            float c = excl;
            bool found = false;
#pragma unroll
            for (int i = 0; i < LIDAR_MAX_PER_LANE; i++)
                if (i < cnt && !found && w[i] > 0.0f) {
                    const float cp = c;
                    c += w[i];
                    r = t[i + 1];                             // (no sample of the lane reaches tau: the end of its last positive bin)
                    if (c >= tau) {
                        const float f = fminf(fmaxf((tau - cp) / w[i], 0.0f), 1.0f);
                        r = t[i] + f * (t[i + 1] - t[i]);
                        found = true;
                    }
                }
        }
        rq[k] = __shfl(r, src, DURF_WAVE);
    }
    if (lane != 0) return;
    const bool has = W > 0.0f;
    const bool ok = acc[ray] >= A.min_acc && has && rq[0] <= A.max_range;
    const float r = ok ? rq[0] : 0.0f;
    if (range_q) range_q[ray] = r;
    if (range_mean) range_mean[ray] = has ? msum / W : 0.0f;
    if (valid) valid[ray] = ok ? 1 : 0;
    if (spread) spread[ray] = has ? rq[2] - rq[1] : 0.0f;
    if (xyz) {
        const float* o = origins + (size_t)ray * 3;
        const float* d = directions + (size_t)ray * 3;
        const float x = o[0] + r * d[0], y = o[1] + r * d[1], z = o[2] + r * d[2];
        float* p = xyz + (size_t)ray * 3;
        if (A.to_sensor) {
#pragma unroll
            for (int i = 0; i < 3; i++) p[i] = ((A.M[i * 4 + 0] * x + A.M[i * 4 + 1] * y) + A.M[i * 4 + 2] * z) + A.M[i * 4 + 3];
        } else {
            p[0] = x; p[1] = y; p[2] = z;
        }
    }
}

static int check_returns_args(int N, float q, float q_lo, float q_hi) {
    DURF_REQUIRE(N % 32 == 0 && N >= 32 && N <= 256, "num_samples a multiple of 32 in [32, 256]");
    DURF_REQUIRE(q > 0.0f && q < 1.0f, "0 < q < 1");
    DURF_REQUIRE(q_lo > 0.0f && q_hi < 1.0f && q_lo < q_hi, "0 < q_lo < q_hi < 1");
    return 0;
}

static int launch_lidar_returns(void* stream, int n, int N, const float* weights, const float* t_vals, const float* acc,
                                const float* origins, const float* directions, const LidarReturns& A, float* range_q,
                                float* range_mean, int32_t* valid, float* xyz, float* spread) {
    hipLaunchKernelGGL(k_lidar_returns, dim3(durf_cdiv(n, LIDAR_RET_WAVES)), dim3(LIDAR_RET_WAVES * DURF_WAVE), 0, (hipStream_t)stream,
                       n, N, weights, t_vals, acc, origins, directions, A, range_q, range_mean, valid, xyz, spread);
    DURF_CHECK_LAUNCH("k_lidar_returns");
    return 0;
}

// ---- the point cloud --------------------------------------------------------------------------------------------------------
#define LIDAR_CB DURF_LIDAR_COMPACT_BLOCK
#define LIDAR_CB_WAVES (LIDAR_CB / DURF_WAVE)

// pass 1: the valid rays of block b of LIDAR_CB rays -> sums[b]
__global__ void __launch_bounds__(LIDAR_CB)
k_lidar_count(int n, const int32_t* __restrict__ valid, int32_t* __restrict__ sums) {
    __shared__ int s_wave[LIDAR_CB_WAVES];
    const int t = threadIdx.x, i = blockIdx.x * LIDAR_CB + t;
    const unsigned long long m = __ballot(i < n && valid[i] != 0);
    if ((t & (DURF_WAVE - 1)) == 0) s_wave[t / DURF_WAVE] = __popcll(m);
    __syncthreads();
    if (t == 0) {
        int c = 0;
#pragma unroll
        for (int v = 0; v < LIDAR_CB_WAVES; v++) c += s_wave[v];
        sums[blockIdx.x] = c;
    }
}

// pass 2: k_scan_block_sums<int32_t, 1> (scan.h); the total goes to sums[nb] and count[0]

// pass 3: ray i, the m-th valid one, writes row m
__global__ void __launch_bounds__(LIDAR_CB)
k_lidar_scatter(int n, const int32_t* __restrict__ valid, const float* __restrict__ xyz, const float* __restrict__ range,
                const float* __restrict__ rgb, const int32_t* __restrict__ dyn, const int32_t* __restrict__ offs,
                float* __restrict__ points, int32_t* __restrict__ source) {
    __shared__ int s_wave[LIDAR_CB_WAVES];
    const int t = threadIdx.x, lane = t & (DURF_WAVE - 1), wave = t / DURF_WAVE, i = blockIdx.x * LIDAR_CB + t;
    const bool v = i < n && valid[i] != 0;
    const unsigned long long m = __ballot(v);
    if (lane == 0) s_wave[wave] = __popcll(m);
    __syncthreads();
    if (!v) return;
    int at = offs[blockIdx.x] + __popcll(m & ((1ull << lane) - 1ull));
#pragma unroll
    for (int u = 0; u < LIDAR_CB_WAVES; u++)
        if (u < wave) at += s_wave[u];
    // at < offs[nb] <= n: a row of the caller's [n,8] buffer
    const float* p = xyz + (size_t)i * 3;
    f32x4 a = {p[0], p[1], p[2], range[i]}, b = {0.f, 0.f, 0.f, 0.f};
    if (rgb) { b[0] = rgb[(size_t)i * 3]; b[1] = rgb[(size_t)i * 3 + 1]; b[2] = rgb[(size_t)i * 3 + 2]; }
    if (dyn) b[3] = (float)dyn[i];
    f32x4* row = (f32x4*)(points + (size_t)at * DURF_LIDAR_POINT_FLOATS);
    row[0] = a;
    row[1] = b;
    source[at] = i;
}

// ---- F sweeps in one call ---------------------------------------------------------------------------------------------------
namespace {
struct LidarWs {
    void* fwd;                           // durf_forward_masked's own workspace for one chunk
    size_t fwd_bytes;
    float* rays[6];
    float *rgb[DURF_FORWARD_MAX_LEVELS], *depth[DURF_FORWARD_MAX_LEVELS], *acc[DURF_FORWARD_MAX_LEVELS];
    float *weights[DURF_FORWARD_MAX_LEVELS], *t_vals[DURF_FORWARD_MAX_LEVELS], *t_mids[DURF_FORWARD_MAX_LEVELS];
    float* t_dists[DURF_FORWARD_MAX_LEVELS];
    int32_t* dyn;
    float* zo;
    size_t total;
};

LidarWs carve_lidar(void* base, int chunk, int N, int K, int L) {
    durf::Carver c{(char*)base, 0};
    LidarWs w{};
    const size_t B = chunk > 0 ? chunk : 0, n = N > 0 ? N : 0;
    w.fwd_bytes = durf_forward_workspace_bytes(chunk, N, K);
    w.fwd = c.take(w.fwd_bytes);
    for (int i = 0; i < 6; i++) w.rays[i] = (float*)c.take(B * (i < 3 ? 3 : 1) * 4);
    for (int l = 0; l < L && l < DURF_FORWARD_MAX_LEVELS; l++) {
        w.rgb[l] = (float*)c.take(B * 3 * 4);
        w.depth[l] = (float*)c.take(B * 4);
        w.acc[l] = (float*)c.take(B * 4);
        w.weights[l] = (float*)c.take(B * n * 4);
        w.t_vals[l] = (float*)c.take(B * (n + 1) * 4);
        w.t_mids[l] = (float*)c.take(B * n * 4);
        w.t_dists[l] = (float*)c.take(B * n * 4);
    }
    w.dyn = (int32_t*)c.take(B * 4);
    w.zo = (float*)c.take(B * 4);
    w.total = c.total();
    return w;
}
}  // namespace

extern "C" {

int durf_lidar_rays(void* stream, const float* sensor_host, const float* inclinations, const float* sweeps_host, int first, int count,
                    float near, float far, float* origins, float* directions, float* viewdirs, float* radii, float* near_out,
                    float* far_out) {
    LidarSweep S;
    int rc = lidar_sweep_args(sensor_host, sweeps_host, near, far, &S);
    if (rc != 0) return rc;
    DURF_REQUIRE(first >= 0 && count >= 0 && (long)first + count <= (long)S.H * S.W, "rays [first, first + count) inside the sweep");
    if (count == 0) return 0;
    DURF_REQUIRE(sweeps_host && inclinations, "the sweep row and the inclination table");
    DURF_REQUIRE(origins && directions && viewdirs && radii && near_out && far_out, "the six ray fields");
    float* const rays[6] = {origins, directions, viewdirs, radii, near_out, far_out};
    return launch_lidar_rays(stream, S, inclinations, first, count, rays);
}

int durf_lidar_returns(void* stream, int n, int N, const float* weights, const float* t_vals, const float* acc, const float* origins,
                       const float* directions, const float* to_sensor_host, float q, float q_lo, float q_hi, float min_acc,
                       float max_range, float* range_q, float* range_mean, int32_t* valid, float* xyz, float* spread) {
    DURF_REQUIRE(n >= 0, "n >= 0");
    int rc = check_returns_args(N, q, q_lo, q_hi);
    if (rc != 0) return rc;
    if (n == 0) return 0;
    DURF_REQUIRE(range_q || range_mean || valid || xyz || spread, "at least one output");
    DURF_REQUIRE(weights && t_vals && acc, "weights, t_vals and acc");
    DURF_REQUIRE(!xyz || (origins && directions), "xyz needs origins and directions");
    LidarReturns A{{q, q_lo, q_hi}, min_acc, max_range, to_sensor_host != nullptr, {}};
    for (int i = 0; i < 12 && to_sensor_host; i++) A.M[i] = to_sensor_host[i];
    return launch_lidar_returns(stream, n, N, weights, t_vals, acc, origins, directions, A, range_q, range_mean, valid, xyz, spread);
}

int durf_lidar_compact(void* stream, int n, const int32_t* valid, const float* xyz, const float* range, const float* rgb,
                       const int32_t* dyn_mask, float* points, int32_t* source, int32_t* count, int32_t* scratch) {
    DURF_REQUIRE(n >= 0 && n < (1 << 27), "0 <= n < 2^27");
    DURF_REQUIRE(count != nullptr && scratch != nullptr, "count and scratch");
    DURF_REQUIRE(n == 0 || (valid && xyz && range && points && source), "valid, xyz, range, points and source");
    DURF_REQUIRE(((size_t)points & 15) == 0, "points is 16-byte aligned");
    const int nb = (int)durf_cdiv(n, LIDAR_CB);
    if (nb > 0) {
        hipLaunchKernelGGL(k_lidar_count, dim3(nb), dim3(LIDAR_CB), 0, (hipStream_t)stream, n, valid, scratch);
        DURF_CHECK_LAUNCH("k_lidar_count");
    }
    hipLaunchKernelGGL((k_scan_block_sums<int32_t, 1>), dim3(1), dim3(SCAN_THREADS), 0, (hipStream_t)stream, nb, scratch, count);
    DURF_CHECK_LAUNCH("k_scan_block_sums<int32_t, 1>");
    if (nb > 0) {
        hipLaunchKernelGGL(k_lidar_scatter, dim3(nb), dim3(LIDAR_CB), 0, (hipStream_t)stream, n, valid, xyz, range, rgb, dyn_mask,
                           scratch, points, source);
        DURF_CHECK_LAUNCH("k_lidar_scatter");
    }
    return 0;
}

size_t durf_render_lidar_workspace_bytes(int chunk, int N, int K, int num_levels) {
    return carve_lidar(nullptr, chunk, N, K, num_levels).total;
}

int durf_render_lidar(void* stream, const durf_forward_args* a, const int32_t* box_enable, int F, const float* sensor_host,
                      const float* inclinations, const float* sweeps_host, const float* poses, float near, float far, int chunk,
                      float q, float q_lo, float q_hi, float min_acc, float* range, float* range_mean, float* distance, float* acc,
                      float* rgb, float* spread, int32_t* dynamic, int32_t* valid, float* xyz, void* workspace,
                      size_t workspace_bytes) {
    DURF_REQUIRE(a != nullptr, "arguments");
    DURF_REQUIRE(F > 0, "F > 0 sweeps");
    LidarSweep S;
    int rc = lidar_sweep_args(sensor_host, nullptr, near, far, &S);
    if (rc != 0) return rc;
    if ((rc = check_returns_args(a->N, q, q_lo, q_hi)) != 0) return rc;
    const int N = a->N, K = a->K, L = a->num_levels;
    DURF_REQUIRE(K >= 0 && K <= DURF_MAX_OBJ, "0 <= K <= DURF_MAX_OBJ");
    DURF_REQUIRE(L >= 1 && L <= DURF_FORWARD_MAX_LEVELS, "1 <= num_levels <= DURF_FORWARD_MAX_LEVELS");
    DURF_REQUIRE(a->t_rand == nullptr && a->u_rand == nullptr && !a->draw_noise && a->density_noise == 0.0f,
                 "render_lidar is test mode: randomized = False");
    DURF_REQUIRE(chunk > 0, "chunk > 0");
    const bool returns = range || range_mean || spread || valid || xyz;
    DURF_REQUIRE(returns || distance || acc || rgb || dynamic, "at least one output");
    DURF_REQUIRE(sweeps_host && inclinations && (K == 0 || poses), "the sweep rows, the inclination table and the box poses");
    DURF_REQUIRE(workspace != nullptr && ((size_t)workspace & 255) == 0, "workspace aligned to 256 bytes");
    const LidarWs w = carve_lidar(workspace, chunk, N, K, L);
    rc = durf::check_workspace("durf_render_lidar", workspace_bytes, w.total, "durf_render_lidar_workspace_bytes(%d, %d, %d, %d)", chunk,
                               N, K, L);
    if (rc != 0) return rc;
    const LidarReturns A{{q, q_lo, q_hi}, min_acc, sensor_host[5], 0, {}};
    const size_t n = (size_t)S.H * S.W;
    for (int f = 0; f < F; f++) {
        if ((rc = lidar_sweep_args(sensor_host, sweeps_host + (size_t)f * DURF_LIDAR_SWEEP_FLOATS, near, far, &S)) != 0) return rc;
        for (size_t i = 0; i < n; i += (size_t)chunk) {
            const int B = (int)(n - i < (size_t)chunk ? n - i : (size_t)chunk);
            if ((rc = launch_lidar_rays(stream, S, inclinations, (int)i, B, w.rays)) != 0) return rc;
            const size_t at = (size_t)f * n + i;          // (an output that is not asked for stays in the workspace, per chunk)
            durf_forward_args c = *a;
            c.B = B;
            c.origins = w.rays[0]; c.directions = w.rays[1]; c.viewdirs = w.rays[2]; c.radii = w.rays[3]; c.near = w.rays[4]; c.far = w.rays[5];
            c.pose = K > 0 ? poses + (size_t)f * K * 6 : nullptr;
            for (int l = 0; l < L; l++) {
                const bool last = l == L - 1;
                c.rgb[l] = last && rgb ? rgb + at * 3 : w.rgb[l];
                c.depth[l] = last && distance ? distance + at : w.depth[l];
                c.acc[l] = last && acc ? acc + at : w.acc[l];
                c.weights[l] = w.weights[l]; c.t_vals[l] = w.t_vals[l]; c.t_mids[l] = w.t_mids[l]; c.t_dists[l] = w.t_dists[l];
            }
            c.dyn_mask = dynamic ? dynamic + at : w.dyn;
            c.zo = w.zo;
            if ((rc = durf_forward_masked(stream, &c, box_enable, w.fwd, w.fwd_bytes)) != 0) return rc;
            if (returns) {
                rc = launch_lidar_returns(stream, B, N, w.weights[L - 1], w.t_vals[L - 1], c.acc[L - 1], w.rays[0], w.rays[1], A,
                                          range ? range + at : nullptr, range_mean ? range_mean + at : nullptr,
                                          valid ? valid + at : nullptr, xyz ? xyz + at * 3 : nullptr, spread ? spread + at : nullptr);
                if (rc != 0) return rc;
            }
        }
    }
    return 0;
}

}  // extern "C"
