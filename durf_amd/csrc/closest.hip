// The closest point of a triangle mesh to arbitrary points (include/durf_closest.h; libdurf_closest.so): the second query of the
// implicit box tree that durf_cast_build leaves (cast_tree.h holds the tree, its workspace and the walk; csrc/cast.hip writes it)
// -- nearest by distance to a point instead of nearest along a ray.  The header defines the result as a minimum over all
// triangles and proves that no tree can change it; the kernels follow it.  This file reads the workspace and writes its outputs,
// nothing else: no atomics, nothing synchronises or copies to the host, no workgroup waits for another.
#include <cmath>
#include "cast_tree.h"
#include "triangles.h"
#include "lattice.h"
#include "../../include/durf_closest.h"

static_assert(DURF_CLOSEST_BLOCK == CB && DURF_CLOSEST_STACK == CSTACK, "the walk's workgroup and its one stack entry per level");
static_assert(DURF_CLOSEST_BRICK * DURF_CLOSEST_BRICK * DURF_CLOSEST_BRICK == 64 && CB % 64 == 0, "a brick per wave");

// the box bound: +inf for the empty box by the formula itself
__device__ __forceinline__ float closest_bound(const float* P, const CastBox& B) {
    float e[3];
#pragma unroll
    for (int a = 0; a < 3; a++) e[a] = fmaxf(fmaxf(B.lo[a] - P[a], P[a] - B.hi[a]), 0.0f);
    return vec3_dot(e, e);
}

struct ClosestBest {
    int tri;
    float d2, w, u, v, c[3];
};

// one candidate of the triangle rule: taken only if strictly nearer
__device__ __forceinline__ void closest_candidate(const float* P, const float* A, const float* e1, const float* e2, float w, float u, float v,
                                                  ClosestBest& best) {
    float c[3], q[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        c[k] = (A[k] + u * e1[k]) + v * e2[k];
        q[k] = P[k] - c[k];
    }
    const float d2 = vec3_dot(q, q);
    if (d2 < best.d2) best = ClosestBest{best.tri, d2, w, u, v, {c[0], c[1], c[2]}};
}

__device__ __forceinline__ float closest_clamped(float num, float den) { return den > 0.0f ? fminf(fmaxf(num / den, 0.0f), 1.0f) : 0.0f; }

// the triangle rule and the clamp on a valid triangle's vertices V [9]: d2_i with its weights and point
__device__ __forceinline__ ClosestBest closest_triangle(const float* P, const float* V) {
    const float *A = V, *B = V + 3, *C = V + 6;
    float e1[3], e2[3], s[3], f[3], r[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        e1[k] = B[k] - A[k];
        e2[k] = C[k] - A[k];
        s[k] = P[k] - A[k];
        f[k] = C[k] - B[k];
        r[k] = P[k] - B[k];
    }
    const float a = vec3_dot(e1, e1), b = vec3_dot(e1, e2), c = vec3_dot(e2, e2), d = vec3_dot(e1, s), e = vec3_dot(e2, s);
    const float l = vec3_dot(f, f), g = vec3_dot(f, r);
    ClosestBest best{-1, __builtin_inff(), 1.0f, 0.0f, 0.0f, {A[0], A[1], A[2]}};
    const float det = a * c - b * b;
    if (det > 0.0f) {
        const float u = (c * d - b * e) / det, v = (a * e - b * d) / det, w = (1.0f - u) - v;
        if (u >= 0.0f && v >= 0.0f && w >= 0.0f) closest_candidate(P, A, e1, e2, w, u, v, best);
    }
    float x = closest_clamped(d, a);
    closest_candidate(P, A, e1, e2, 1.0f - x, x, 0.0f, best);
    x = closest_clamped(e, c);
    closest_candidate(P, A, e1, e2, 1.0f - x, 0.0f, x, best);
    x = closest_clamped(g, l);
    closest_candidate(P, A, e1, e2, 0.0f, 1.0f - x, x, best);
    best.d2 = fmaxf(best.d2, closest_bound(P, cast_tri_box(A, B, C))) + 0.0f;
    return best;
}

// the query of a point: the nearest triangle within cap2 by (d2, id).  A node is skipped for lb > cap2 or lb > best.d2, strictly.
struct ClosestQuery {
    const float* P;
    float cap2;
    ClosestBest best;
    __device__ __forceinline__ bool enter(const CastBox& B, float& lb) {
        lb = closest_bound(P, B);
        return !(lb > cap2) && !(lb > best.d2);
    }
    __device__ __forceinline__ bool leaf(const float* V, int id) {
        ClosestBest t = closest_triangle(P, V);
        if (t.d2 <= cap2 && (t.d2 < best.d2 || (t.d2 == best.d2 && id < best.tri) || best.tri < 0)) {
            best = t;
            best.tri = id;
        }
        return false;
    }
};

// the query of one thread, from the point to its outputs at index i (tri, bary, point: nullable)
__device__ __forceinline__ void closest_query(const CastTree& R, const float* __restrict__ records, const float* __restrict__ nodes,
                                              const float* P, float max_dist, int* stack, const int* s_off, size_t i,
                                              int32_t* __restrict__ tri, float* __restrict__ dist, float* __restrict__ bary,
                                              float* __restrict__ point) {
    const bool usable = cam_finite(P[0]) && cam_finite(P[1]) && cam_finite(P[2]);
    ClosestQuery q{P, max_dist * max_dist, ClosestBest{-1, __builtin_inff(), 0.0f, 0.0f, 0.0f, {0.0f, 0.0f, 0.0f}}};
    if (usable) cast_tree_walk(R, records, nodes, q, stack, s_off);
    const ClosestBest& hit = q.best;
    const float nan = __builtin_nanf("");
    const bool found = usable && hit.tri >= 0;
    if (tri) tri[i] = !usable ? -2 : found ? hit.tri : -1;
    dist[i] = !usable ? nan : found ? sqrtf(hit.d2) : max_dist;
    if (bary) {
        bary[i * 3] = !usable ? nan : found ? hit.w : 0.0f;
        bary[i * 3 + 1] = !usable ? nan : found ? hit.u : 0.0f;
        bary[i * 3 + 2] = !usable ? nan : found ? hit.v : 0.0f;
    }
    if (point) {
#pragma unroll
        for (int k = 0; k < 3; k++) point[i * 3 + k] = !usable ? nan : found ? hit.c[k] : 0.0f;
    }
}

__global__ void __launch_bounds__(CB)
k_closest_points(const CastTree R, int n, const float* __restrict__ points, float max_dist, const float* __restrict__ records,
                 const float* __restrict__ nodes, int32_t* __restrict__ tri, float* __restrict__ dist, float* __restrict__ bary,
                 float* __restrict__ point) {
    __shared__ int s_stack[CSTACK * CB];
    __shared__ int s_off[CSTACK];
    cast_offsets_to_lds(R, s_off);
    const int i = blockIdx.x * CB + threadIdx.x;
    if (i >= n) return;                                                      // (no barrier below)
    const float P[3] = {points[(size_t)i * 3], points[(size_t)i * 3 + 1], points[(size_t)i * 3 + 2]};
    closest_query(R, records, nodes, P, max_dist, s_stack + threadIdx.x, s_off, (size_t)i, tri, dist, bary, point);
}

struct ClosestBricks { int bv, bw; long long bricks; };        // bricks along v and w, and all of them

// a wave per brick of 4 x 4 x 4 lattice points: lane = (di 4 + dj) 4 + dk
__global__ void __launch_bounds__(CB)
k_closest_grid(const CastTree R, const LatticeDims D, const LatticeFrame F, const ClosestBricks G, float max_dist, const float* __restrict__ records, const float* __restrict__ nodes,
               float* __restrict__ dist, int32_t* __restrict__ tri) {
    __shared__ int s_stack[CSTACK * CB];
    __shared__ int s_off[CSTACK];
    cast_offsets_to_lds(R, s_off);
    const long long brick = (long long)blockIdx.x * (CB / 64) + threadIdx.x / 64;
    if (brick >= G.bricks) return;                                           // (no barrier below)
    const int lane = threadIdx.x % 64;
    const long long bu = brick / ((long long)G.bv * G.bw);
    const int rest = (int)(brick - bu * ((long long)G.bv * G.bw));
    const int i = (int)bu * DURF_CLOSEST_BRICK + lane / 16, j = (rest / G.bw) * DURF_CLOSEST_BRICK + lane / 4 % 4, k = (rest % G.bw) * DURF_CLOSEST_BRICK + lane % 4;
    if (i >= D.nu || j >= D.nv || k >= D.nw) return;
    float P[3];
    lattice_point(F, (float)i, (float)j, (float)k, P);
    const size_t g = (size_t)lattice_index(D, i, j, k);                      // nu nv nw < 2^31
    closest_query(R, records, nodes, P, max_dist, s_stack + threadIdx.x, s_off, g, tri, dist, nullptr, nullptr);
}

// ---- launchers ----------------------------------------------------------------------------------------------------------------------
namespace {

// T, max_dist and the workspace, in this order
int closest_check(const char* who, float max_dist, int T, const void* workspace, size_t workspace_bytes, CastTree* R, CastWs* ws) {
    if (check_cast_t(who, T) != 0) return -1;
    if (!(max_dist == __builtin_inff() || (max_dist >= 1e-18f && max_dist <= 1e18f))) {
        durf_set_error("%s: requirement failed: max_dist is +inf or in [1e-18, 1e18], max_dist = %g", who, (double)max_dist);
        return -1;
    }
    *R = cast_tree(T);
    return check_cast_ws(who, workspace, workspace_bytes, *R, ws);
}

}  // namespace

extern "C" {

int durf_closest_points(void* stream, int n, const float* points, float max_dist, int T, const void* workspace, size_t workspace_bytes,
                        int32_t* tri, float* dist, float* bary, float* point) {
    if (!(n >= 0)) { durf_set_error("%s: requirement failed: n >= 0, n = %d", __func__, n); return -1; }
    CastTree R;
    CastWs ws;
    if (closest_check(__func__, max_dist, T, workspace, workspace_bytes, &R, &ws) != 0) return -1;
    if (!(points || n == 0)) { durf_set_error("%s: requirement failed: points for n = %d", __func__, n); return -1; }
    if (!((tri && dist) || n == 0)) { durf_set_error("%s: requirement failed: tri and dist for n = %d", __func__, n); return -1; }
    if (n == 0) return 0;
    hipLaunchKernelGGL(k_closest_points, dim3(durf_cdiv((size_t)n, CB)), dim3(CB), 0, (hipStream_t)stream, R, n, points, max_dist, ws.records,
                       ws.nodes, tri, dist, bary, point);
    DURF_CHECK_LAUNCH("k_closest_points");
    return 0;
}

int durf_closest_grid(void* stream, int nu, int nv, int nw, const float* origin, const float* du, const float* dv, const float* dw,
                      float max_dist, int T, const void* workspace, size_t workspace_bytes, float* dist, int32_t* tri) {
    if (!(nu >= 1 && nv >= 1 && nw >= 1)) {
        durf_set_error("%s: requirement failed: nu, nv, nw >= 1, nu = %d, nv = %d, nw = %d", __func__, nu, nv, nw);
        return -1;
    }
    if (!((double)nu * nv * nw < 2147483648.0)) {
        durf_set_error("%s: requirement failed: nu nv nw < 2^31 points, nu = %d, nv = %d, nw = %d", __func__, nu, nv, nw);
        return -1;
    }
    if (!(origin && du && dv && dw)) { durf_set_error("%s: requirement failed: origin, du, dv and dw (host floats)", __func__); return -1; }
    const LatticeFrame F = lattice_frame(origin, du, dv, dw);
    bool finite = true;
    for (int c = 0; c < 3; c++) finite = finite && std::isfinite(F.o[c]) && std::isfinite(F.du[c]) && std::isfinite(F.dv[c]) && std::isfinite(F.dw[c]);
    if (!finite) { durf_set_error("%s: requirement failed: origin, du, dv and dw are finite", __func__); return -1; }
    CastTree R;
    CastWs ws;
    if (closest_check(__func__, max_dist, T, workspace, workspace_bytes, &R, &ws) != 0) return -1;
    if (!dist) { durf_set_error("%s: requirement failed: dist for %d x %d x %d points", __func__, nu, nv, nw); return -1; }
    const LatticeDims D{nu, nv, nw, nu * nv * nw};
    ClosestBricks G{};
    G.bv = (int)durf_cdiv((size_t)nv, DURF_CLOSEST_BRICK), G.bw = (int)durf_cdiv((size_t)nw, DURF_CLOSEST_BRICK);
    G.bricks = (long long)durf_cdiv((size_t)nu, DURF_CLOSEST_BRICK) * G.bv * G.bw;       // at most 16 nu nv nw / 64 < 2^29
    hipLaunchKernelGGL(k_closest_grid, dim3(durf_cdiv((size_t)G.bricks, CB / 64)), dim3(CB), 0, (hipStream_t)stream, R, D, F, G, max_dist, ws.records,
                       ws.nodes, dist, tri);
    DURF_CHECK_LAUNCH("k_closest_grid");
    return 0;
}

}  // extern "C"
