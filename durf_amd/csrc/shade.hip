// A shaded picture of a triangle mesh (include/durf_shade.h; libdurf_shade.so): flat normals at the primary hits, a sun shadow and
// ambient occlusion from any-hit rays through the tree durf_cast_build leaves, and the colour of every sample.  The third
// consumer of cast_tree.h's walk, and the first that runs it in a loop per thread: cast_query.h brings the ray and its two
// rules, this file the rays themselves.  It reads the cast workspace and writes its outputs, nothing else: no atomics, nothing
// synchronises or copies to the host, no workgroup waits for another.
#include <cmath>
#include "cast_query.h"
#include "../../include/durf_shade.h"

static_assert(DURF_SHADE_MAX_DIRS >= 1, "at least one direction");

// the surface rule of a sample: point and normal, zero where the sample is not valid; toward [3] is read when `facing`
__device__ __forceinline__ void shade_surface_rule(int t, float u, float v, int V, int T, const float* __restrict__ vertices,
                                                   const int32_t* __restrict__ triangles, bool facing, const float* toward, float* point,
                                                   float* normal) {
#pragma unroll
    for (int a = 0; a < 3; a++) point[a] = normal[a] = 0.0f;
    float P[9];
    if (!tri_fetch(t, V, T, vertices, triangles, P)) return;
    float e1[3], e2[3], N[3];
    vec3_sub(P + 3, P, e1);
    vec3_sub(P + 6, P, e2);
#pragma unroll
    for (int a = 0; a < 3; a++) point[a] = (P[a] + u * e1[a]) + v * e2[a];
    vec3_cross(e1, e2, N);
    const float len2 = vec3_dot(N, N);
    if (!(len2 > 0.0f) || !cam_finite(len2)) return;                         // FLAT
    const float inv = 1.0f / sqrtf(len2);
    float n[3] = {N[0] * inv, N[1] * inv, N[2] * inv};
    const bool flip = facing && vec3_dot(n, toward) > 0.0f;
#pragma unroll
    for (int a = 0; a < 3; a++) normal[a] = flip ? -n[a] : n[a];
}

// ---- surface ------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(CB)
k_shade_surface(int n, int V, int T, const float* __restrict__ vertices, const int32_t* __restrict__ triangles, const int32_t* __restrict__ tri,
                const float* __restrict__ bary, const float* __restrict__ toward, float* __restrict__ point, float* __restrict__ normal) {
    const unsigned i = blockIdx.x * (unsigned)CB + threadIdx.x;              // n < 2^31
    if (i >= (unsigned)n) return;
    const int t = tri[i];
    float u = 0.0f, v = 0.0f, d[3] = {0.0f, 0.0f, 0.0f}, p[3], nr[3];
    if (t >= 0 && t < T) {                                                   // (bary is not read for a sample that is not valid)
        u = bary[(size_t)i * 3 + 1];
        v = bary[(size_t)i * 3 + 2];
    }
    if (toward) {
#pragma unroll
        for (int a = 0; a < 3; a++) d[a] = toward[(size_t)i * 3 + a];
    }
    shade_surface_rule(t, u, v, V, T, vertices, triangles, toward != nullptr, d, p, nr);
#pragma unroll
    for (int a = 0; a < 3; a++) {
        point[(size_t)i * 3 + a] = p[a];
        normal[(size_t)i * 3 + a] = nr[a];
    }
}

// ---- the primary rays of a camera: k_cast_cameras' body, then the surface rule ------------------------------------------------------
// The camera entry deals its pixels to the waves in tiles of 8 x 8, not in pieces of a row: slot = ((f tiles + tile) 64 + lane),
// lane = 8 ly + lx.  A wave of the occlusion launch is then compact in space and its lanes walk the same nodes (measured:
// DESIGN.md 17).  A slot outside the frame (a partial tile) is no sample.  The order affects speed only: outputs are by pixel.
struct ShadeTiles {
    int h, w, tx;                      // w == 0: no tiles, slot i is sample i
    unsigned long long per_frame;      // slots of one frame: tiles x 64 (a frame of one long row has 8 slots per pixel)
    unsigned hw;
};

// the pixel of a slot in [0, F h w), or -1
__device__ __forceinline__ long long shade_slot_pixel(const ShadeTiles& G, unsigned long long slot) {
    if (G.w == 0) return (long long)slot;
    const unsigned long long f = slot / G.per_frame;
    const unsigned long long r = slot - f * G.per_frame;
    const unsigned tile = (unsigned)(r / 64), lane = (unsigned)(r % 64);
    const int y = (int)(tile / G.tx) * 8 + (int)(lane / 8), x = (int)(tile % G.tx) * 8 + (int)(lane % 8);
    if (y >= G.h || x >= G.w) return -1;
    return (long long)(f * G.hw + (unsigned)y * (unsigned)G.w + (unsigned)x);
}

__global__ void __launch_bounds__(CB)
k_shade_primary(const CastTree R, const ShadeTiles G, unsigned long long slots, const float* __restrict__ cams, float tmin, float tmax, int cull,
                int V, const float* __restrict__ vertices, const int32_t* __restrict__ triangles, const float* __restrict__ records,
                const float* __restrict__ nodes, int32_t* __restrict__ tri, float* __restrict__ depth, float* __restrict__ bary,
                float* __restrict__ point_slots, float* __restrict__ normal_slots, float* __restrict__ normal) {
    __shared__ int s_stack[CSTACK * CB];
    __shared__ int s_off[CSTACK];
    cast_offsets_to_lds(R, s_off);
    const unsigned long long slot = (unsigned long long)blockIdx.x * CB + threadIdx.x;
    if (slot >= slots) return;                                               // (no barrier below)
    const long long i = shade_slot_pixel(G, slot);                           // F h w < 2^31
    float pt[3] = {0.0f, 0.0f, 0.0f}, nm[3] = {0.0f, 0.0f, 0.0f};
    if (i >= 0) {
        const int f = (int)((unsigned)i / G.hw), p = (int)((unsigned)i - (unsigned)f * G.hw);
        const float* cam = cams + (size_t)f * DURF_CAM_FLOATS;
        CastRay r;
        r.tmin = tmin;
        r.tmax = tmax;
        bool usable = (int)cam[DURF_CAM_H] == G.h && (int)cam[DURF_CAM_W] == G.w;
        if (usable) {
            float view[3], radius, nr, fr;
            pinhole_ray(cam, p, tmin, tmax, 0, r.o, r.d, view, &radius, &nr, &fr);
            usable = cast_ray_setup(r);
        }
        CastHit hit{-1, 0.0f, 0.0f, 0.0f, 0.0f};
        if (usable) hit = cast_walk<false>(R, records, nodes, r, cull, s_stack + threadIdx.x, s_off);
        cast_write(hit, usable, (size_t)i, tri, depth, bary);
        shade_surface_rule(usable ? hit.tri : -2, hit.u, hit.v, V, R.T, vertices, triangles, true, r.d, pt, nm);
#pragma unroll
        for (int a = 0; a < 3; a++) normal[(size_t)i * 3 + a] = nm[a];
    }
#pragma unroll
    for (int a = 0; a < 3; a++) {
        point_slots[(size_t)slot * 3 + a] = pt[a];                           // (a slot outside the frame: not live)
        normal_slots[(size_t)slot * 3 + a] = nm[a];
    }
}

// ---- occlusion ----------------------------------------------------------------------------------------------------------------------
struct ShadeDir { float v[3]; };      // the one direction of a call without `dirs` (the sun of durf_shade_cameras), by value

// One thread per sample (per slot of the camera entry's tiles); the loop over the directions is inside the thread, so neighbouring lanes (neighbouring pixels) walk the
// same direction at the same time and read the same nodes.  dirs is the same address in every lane: scalar loads.
__global__ void __launch_bounds__(CB)
k_shade_occlusion(const CastTree R, const ShadeTiles G, unsigned long long n, const float* __restrict__ points, const float* __restrict__ normals,
                  int S, const float* __restrict__ dirs, const ShadeDir one, float bias, float reach, int cull, const float* __restrict__ records,
                  const float* __restrict__ nodes, int32_t* __restrict__ used, int32_t* __restrict__ blocked) {
    __shared__ int s_stack[CSTACK * CB];
    __shared__ int s_off[CSTACK];
    cast_offsets_to_lds(R, s_off);
    const unsigned long long i = (unsigned long long)blockIdx.x * CB + threadIdx.x;      // the slot: points and normals are read there
    if (i >= n) return;                                                      // (no barrier below)
    const long long out = shade_slot_pixel(G, i);                            // the sample: the counts are written there
    if (out < 0) return;
    float p[3], nr[3];
    bool live = true, all_zero = true;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        p[a] = points[(size_t)i * 3 + a];
        nr[a] = normals[(size_t)i * 3 + a];
        live = live && cam_finite(p[a]) && cam_finite(nr[a]);
        all_zero = all_zero && nr[a] == 0.0f;
    }
    live = live && !all_zero;
    int n_used = 0, n_blocked = 0;
    if (live) {
        CastRay r;
#pragma unroll
        for (int a = 0; a < 3; a++) r.o[a] = p[a] + bias * nr[a];
        r.tmin = 0.0f;
        r.tmax = reach;
        for (int s = 0; s < S; s++) {                                        // (S is read before the loop: at most DURF_SHADE_MAX_DIRS)
            const float* __restrict__ ds = dirs + (size_t)s * 3;             // (not read when dirs is null)
            const float d[3] = {dirs ? ds[0] : one.v[0], dirs ? ds[1] : one.v[1], dirs ? ds[2] : one.v[2]};
            if (!(vec3_dot(nr, d) > 0.0f)) continue;
            n_used++;
#pragma unroll
            for (int a = 0; a < 3; a++) r.d[a] = d[a];
            if (!cast_ray_setup(r)) continue;                                // used, not blocked
            const CastHit hit = cast_walk<true>(R, records, nodes, r, cull, s_stack + threadIdx.x, s_off);
            n_blocked += hit.tri >= 0 ? 1 : 0;
        }
    }
    used[out] = n_used;
    blocked[out] = n_blocked;
}

// ---- compose ------------------------------------------------------------------------------------------------------------------------
struct ShadeLook { float light[3], background[3], ambient; };

// the albedo of durf_shade_cameras: tri_interp on a per-vertex colour, as durf_raster_interp does it (attr null: none)
struct ShadeGather {
    const float* attr;                 // [V,3]
    const int32_t* triangles;
    const float* bary;                 // [n,3]
    int V, T;
};

__global__ void __launch_bounds__(CB)
k_shade_compose(int n, const int32_t* __restrict__ tri, const float* __restrict__ normals, const int32_t* __restrict__ used,
                const int32_t* __restrict__ blocked, const int32_t* __restrict__ sun_blocked, const float* __restrict__ albedo,
                const ShadeGather G, const ShadeLook L, float* __restrict__ out_f, uint8_t* __restrict__ out_u8) {
    const unsigned i = blockIdx.x * (unsigned)CB + threadIdx.x;              // n < 2^31
    if (i >= (unsigned)n) return;
    const int t = tri[i];
    float c[3] = {L.background[0], L.background[1], L.background[2]};
    if (t >= 0) {
        const int nu = used[i], nb = blocked[i];
        const float ao = nu > 0 ? (float)(nu - nb) / (float)nu : 1.0f;
        const float nr[3] = {normals[(size_t)i * 3], normals[(size_t)i * 3 + 1], normals[(size_t)i * 3 + 2]};
        const float lam = fmaxf(vec3_dot(nr, L.light), 0.0f);
        const float sun = (sun_blocked && sun_blocked[i] > 0) ? 0.0f : 1.0f;
        const float shade = L.ambient * ao + (1.0f - L.ambient) * (lam * sun);
        c[0] = c[1] = c[2] = shade;
        if (albedo) {
#pragma unroll
            for (int k = 0; k < 3; k++) c[k] = albedo[(size_t)i * 3 + k] * shade;
        } else if (G.attr) {
            int v[3] = {-1, -1, -1};
            const bool hit = tri_indices(t, G.V, G.T, G.triangles, v);
            float q[3] = {0.0f, 0.0f, 0.0f};
            if (hit) {
#pragma unroll
                for (int k = 0; k < 3; k++) q[k] = G.bary[(size_t)i * 3 + k];
            }
#pragma unroll
            for (int k = 0; k < 3; k++) {
                c[k] = (hit ? tri_interp(q, v, G.attr, 3, k) : 0.0f) * shade;
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 3; k++) {
        if (out_f) out_f[(size_t)i * 3 + k] = c[k];
        if (out_u8) out_u8[(size_t)i * 3 + k] = (uint8_t)rgb8(c[k]);
    }
}

// ---- launchers ----------------------------------------------------------------------------------------------------------------------
namespace {

// S, bias, reach, cull, T and the cast workspace, in this order
int check_shade_rays(const char* who, int S, const float* dirs, float bias, float reach, int cull, int T, const void* workspace,
                     size_t workspace_bytes, CastTree* R, CastWs* ws) {
    if (!(S >= 1 && S <= DURF_SHADE_MAX_DIRS)) { durf_set_error("%s: requirement failed: S in 1 .. %d, S = %d", who, DURF_SHADE_MAX_DIRS, S); return -1; }
    if (!dirs) { durf_set_error("%s: requirement failed: dirs for S = %d", who, S); return -1; }
    if (!(bias >= 0.0f)) { durf_set_error("%s: requirement failed: bias >= 0, bias = %g", who, (double)bias); return -1; }
    if (!(reach > 0.0f)) { durf_set_error("%s: requirement failed: reach is +inf or > 0, reach = %g", who, (double)reach); return -1; }
    if (!(cull >= 0 && cull <= 2)) { durf_set_error("%s: requirement failed: cull in 0 .. 2, cull = %d", who, cull); return -1; }
    if (check_cast_t(who, T) != 0) return -1;
    *R = cast_tree(T);
    return check_cast_ws(who, workspace, workspace_bytes, *R, ws);
}

int check_shade_look(const char* who, const float* light, float ambient, const float* background, ShadeLook* L) {
    if (!(ambient >= 0.0f && ambient <= 1.0f)) { durf_set_error("%s: requirement failed: ambient in [0, 1], ambient = %g", who, (double)ambient); return -1; }
    if (!(light && background)) { durf_set_error("%s: requirement failed: light and background (host floats)", who); return -1; }
    for (int k = 0; k < 3; k++) {
        if (!(std::isfinite(light[k]) && std::isfinite(background[k]))) {
            durf_set_error("%s: requirement failed: light and background are finite", who);
            return -1;
        }
        L->light[k] = light[k];
        L->background[k] = background[k];
    }
    L->ambient = ambient;
    return 0;
}

void launch_occlusion(hipStream_t s, const CastTree& R, const CastWs& ws, const ShadeTiles& G, size_t n, const float* points, const float* normals,
                      int S, const float* dirs, const ShadeDir& one, float bias, float reach, int cull, int32_t* used, int32_t* blocked) {
    hipLaunchKernelGGL(k_shade_occlusion, dim3(durf_cdiv(n, CB)), dim3(CB), 0, s, R, G, (unsigned long long)n, points, normals, S, dirs, one, bias,
                       reach, cull, ws.records, ws.nodes, used, blocked);
}

ShadeTiles shade_tiles(int h, int w) {
    ShadeTiles G{};
    G.h = h, G.w = w, G.tx = (w + 7) / 8;
    G.per_frame = (unsigned long long)G.tx * (unsigned long long)((h + 7) / 8) * 64ull;      // at most 64 h w
    G.hw = (unsigned)h * (unsigned)w;
    return G;
}

// what durf_shade_cameras keeps between its launches: per pixel bary, normal and the sun's counts, per slot of the tiles point and normal
struct ShadeWs {
    float *bary, *normal, *point_slots, *normal_slots;
    int32_t *sun_used, *sun_blocked;
    size_t total;
};

ShadeWs carve_shade(void* base, size_t pixels, size_t slots) {
    durf::Carver c{(char*)base, 0};
    ShadeWs w{};
    w.bary = (float*)c.take(pixels * 12);
    w.normal = (float*)c.take(pixels * 12);
    w.point_slots = (float*)c.take(slots * 12);
    w.normal_slots = (float*)c.take(slots * 12);
    w.sun_used = (int32_t*)c.take(pixels * 4);
    w.sun_blocked = (int32_t*)c.take(pixels * 4);
    w.total = c.total() > 256 ? c.total() : 256;
    return w;
}

bool shade_frames_ok(int F, int h, int w) { return F >= 0 && h >= 1 && w >= 1 && (double)F * h * w < 2147483648.0; }

size_t shade_slots(int F, int h, int w) { return (size_t)F * shade_tiles(h, w).per_frame; }      // at most 64 F h w < 2^37

}  // namespace

extern "C" {

int durf_shade_surface(void* stream, int n, int V, int T, const float* vertices, const int32_t* triangles, const int32_t* tri,
                       const float* bary, const float* toward, float* point, float* normal) {
    if (!(n >= 0)) { durf_set_error("%s: requirement failed: n >= 0, n = %d", __func__, n); return -1; }
    if (check_cast_mesh(__func__, V, T, vertices, triangles) != 0) return -1;
    if (!((tri && bary) || n == 0)) { durf_set_error("%s: requirement failed: tri and bary for n = %d", __func__, n); return -1; }
    if (!((point && normal) || n == 0)) { durf_set_error("%s: requirement failed: point and normal for n = %d", __func__, n); return -1; }
    if (n == 0) return 0;
    hipLaunchKernelGGL(k_shade_surface, dim3(durf_cdiv((size_t)n, CB)), dim3(CB), 0, (hipStream_t)stream, n, V, T, vertices, triangles, tri, bary,
                       toward, point, normal);
    DURF_CHECK_LAUNCH("k_shade_surface");
    return 0;
}

int durf_shade_occlusion(void* stream, int n, const float* points, const float* normals, int S, const float* dirs, float bias, float reach,
                         int cull, int T, const void* workspace, size_t workspace_bytes, int32_t* used, int32_t* blocked) {
    if (!(n >= 0)) { durf_set_error("%s: requirement failed: n >= 0, n = %d", __func__, n); return -1; }
    CastTree R;
    CastWs ws;
    if (check_shade_rays(__func__, S, dirs, bias, reach, cull, T, workspace, workspace_bytes, &R, &ws) != 0) return -1;
    if (!((points && normals) || n == 0)) { durf_set_error("%s: requirement failed: points and normals for n = %d", __func__, n); return -1; }
    if (!((used && blocked) || n == 0)) { durf_set_error("%s: requirement failed: used and blocked for n = %d", __func__, n); return -1; }
    if (n == 0) return 0;
    launch_occlusion((hipStream_t)stream, R, ws, ShadeTiles{}, (size_t)n, points, normals, S, dirs, ShadeDir{}, bias, reach, cull, used, blocked);
    DURF_CHECK_LAUNCH("k_shade_occlusion");
    return 0;
}

int durf_shade_compose(void* stream, int n, const int32_t* tri, const float* normals, const int32_t* used, const int32_t* blocked,
                       const int32_t* sun_blocked, const float* albedo, const float* light, float ambient, const float* background,
                       float* out_f, uint8_t* out_u8) {
    if (!(n >= 0)) { durf_set_error("%s: requirement failed: n >= 0, n = %d", __func__, n); return -1; }
    ShadeLook L;
    if (check_shade_look(__func__, light, ambient, background, &L) != 0) return -1;
    if (!((tri && normals && used && blocked) || n == 0)) { durf_set_error("%s: requirement failed: tri, normals, used and blocked for n = %d", __func__, n); return -1; }
    if (!(out_f || out_u8 || n == 0)) { durf_set_error("%s: requirement failed: out_f or out_u8 for n = %d", __func__, n); return -1; }
    if (n == 0) return 0;
    hipLaunchKernelGGL(k_shade_compose, dim3(durf_cdiv((size_t)n, CB)), dim3(CB), 0, (hipStream_t)stream, n, tri, normals, used, blocked,
                       sun_blocked, albedo, ShadeGather{}, L, out_f, out_u8);
    DURF_CHECK_LAUNCH("k_shade_compose");
    return 0;
}

size_t durf_shade_workspace_bytes(int F, int h, int w) {
    if (!shade_frames_ok(F, h, w)) return 0;
    return carve_shade(nullptr, (size_t)F * h * w, shade_slots(F, h, w)).total;
}

int durf_shade_cameras(void* stream, int F, int h, int w, const float* cams_dev, float tmin, float tmax, int cull, int V, int T,
                       const float* vertices, const int32_t* triangles, const void* cast_ws, size_t cast_ws_bytes, int S, const float* dirs,
                       float bias, float reach, const float* light, int sun, float ambient, const float* albedo_vertex,
                       const float* background, void* workspace, size_t workspace_bytes, int32_t* tri, float* depth, float* normal,
                       int32_t* ao_used, int32_t* ao_blocked, float* out_f, uint8_t* out_u8) {
    if (!(F >= 0 && h >= 1 && w >= 1)) {
        durf_set_error("%s: requirement failed: F >= 0, h >= 1, w >= 1, F = %d, h = %d, w = %d", __func__, F, h, w);
        return -1;
    }
    if (!shade_frames_ok(F, h, w)) {
        durf_set_error("%s: requirement failed: F h w < 2^31 pixels, F = %d, h = %d, w = %d", __func__, F, h, w);
        return -1;
    }
    if (check_cast_mesh(__func__, V, T, vertices, triangles) != 0) return -1;
    if (!(tmin >= 0.0f)) { durf_set_error("%s: requirement failed: tmin >= 0, tmin = %g", __func__, (double)tmin); return -1; }
    if (tmax != tmax) { durf_set_error("%s: requirement failed: tmax is a number, tmax = %g", __func__, (double)tmax); return -1; }
    if (!(sun == 0 || sun == 1)) { durf_set_error("%s: requirement failed: sun in 0 .. 1, sun = %d", __func__, sun); return -1; }
    CastTree R;
    CastWs cw;
    if (check_shade_rays(__func__, S, dirs, bias, reach, cull, T, cast_ws, cast_ws_bytes, &R, &cw) != 0) return -1;
    ShadeLook L;
    if (check_shade_look(__func__, light, ambient, background, &L) != 0) return -1;
    if (!((cams_dev && tri && depth && ao_used && ao_blocked) || F == 0)) {
        durf_set_error("%s: requirement failed: cams_dev, tri, depth, ao_used and ao_blocked for F = %d", __func__, F);
        return -1;
    }
    if (!(out_f || out_u8 || F == 0)) { durf_set_error("%s: requirement failed: out_f or out_u8 for F = %d", __func__, F); return -1; }
    if (durf::check_workspace_aligned(__func__, workspace) != 0) return -1;
    const size_t n = (size_t)F * h * w, slots = shade_slots(F, h, w);
    const ShadeWs ws = carve_shade(workspace, n, slots);
    if (durf::check_workspace(__func__, workspace_bytes, ws.total, "durf_shade_workspace_bytes(%d, %d, %d)", F, h, w) != 0) return -1;
    if (F == 0) return 0;
    const hipStream_t s = (hipStream_t)stream;
    const ShadeTiles G = shade_tiles(h, w);
    float* nrm = normal ? normal : ws.normal;
    hipLaunchKernelGGL(k_shade_primary, dim3(durf_cdiv(slots, CB)), dim3(CB), 0, s, R, G, (unsigned long long)slots, cams_dev, tmin, tmax, cull, V,
                       vertices, triangles, cw.records, cw.nodes, tri, depth, ws.bary, ws.point_slots, ws.normal_slots, nrm);
    DURF_CHECK_LAUNCH("k_shade_primary");
    launch_occlusion(s, R, cw, G, slots, ws.point_slots, ws.normal_slots, S, dirs, ShadeDir{}, bias, reach, cull, ao_used, ao_blocked);
    DURF_CHECK_LAUNCH("k_shade_occlusion");
    if (sun) {
        launch_occlusion(s, R, cw, G, slots, ws.point_slots, ws.normal_slots, 1, nullptr, ShadeDir{{L.light[0], L.light[1], L.light[2]}}, bias,
                         __builtin_inff(), cull, ws.sun_used, ws.sun_blocked);
        DURF_CHECK_LAUNCH("k_shade_occlusion (sun)");
    }
    hipLaunchKernelGGL(k_shade_compose, dim3(durf_cdiv(n, CB)), dim3(CB), 0, s, (int)n, tri, nrm, ao_used, ao_blocked,
                       sun ? ws.sun_blocked : nullptr, nullptr, ShadeGather{albedo_vertex, triangles, ws.bary, V, T}, L, out_f, out_u8);
    DURF_CHECK_LAUNCH("k_shade_compose");
    return 0;
}

}  // extern "C"
