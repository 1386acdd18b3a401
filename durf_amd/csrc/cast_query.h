// The ray query of the implicit box tree (include/durf_cast.h), defined once for everything that sends rays through it (cast.hip:
// the nearest hit and any hit; shade.hip: the secondary rays of a shaded picture): the ray, the header's box rule and triangle
// rule, the two queries of cast_tree.h's one walk, and the outputs of a hit.  Internal.
#pragma once
#include "cast_tree.h"
#include "camera.h"

// a valid triangle's vertices; false for an id outside 0 .. T-1, an index outside 0 .. V-1 or a coordinate that is not finite
__device__ __forceinline__ bool cast_fetch(int id, int V, int T, const float* __restrict__ vertices, const int32_t* __restrict__ triangles,
                                           float* P /* [9] */) {
    if (id < 0 || id >= T) return false;
    bool ok = true;
    int v[3];
#pragma unroll
    for (int c = 0; c < 3; c++) {
        v[c] = triangles[(size_t)id * 3 + c];
        ok = ok && v[c] >= 0 && v[c] < V;
    }
    if (!ok) return false;
#pragma unroll
    for (int c = 0; c < 3; c++)
#pragma unroll
        for (int a = 0; a < 3; a++) {
            P[3 * c + a] = vertices[(size_t)v[c] * 3 + a];
            ok = ok && cam_finite(P[3 * c + a]);
        }
    return ok;
}

struct CastRay {
    float o[3], d[3], inv[3];
    bool zero[3];
    float tmin, tmax;
};

// false for an unusable ray
__device__ __forceinline__ bool cast_ray_setup(CastRay& r) {
    bool ok = r.tmin >= 0.0f && r.tmax == r.tmax;
    bool all_zero = true;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        ok = ok && cam_finite(r.o[a]) && cam_finite(r.d[a]);
        all_zero = all_zero && r.d[a] == 0.0f;
        r.inv[a] = 1.0f / r.d[a];
        r.zero[a] = r.d[a] == 0.0f || !cam_finite(r.inv[a]);
    }
    return ok && !all_zero;
}

// the box rule; bn and bf are written whenever rule 1 lets the box through
__device__ __forceinline__ bool cast_box_rule(const CastRay& r, const CastBox& B, float& bn, float& bf) {
    bn = -__builtin_inff();
    bf = __builtin_inff();
    bool pass = true;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        if (B.lo[a] > B.hi[a]) return false;
        if (r.zero[a]) {
            pass = pass && B.lo[a] <= r.o[a] && r.o[a] <= B.hi[a];
        } else {
            const float x1 = (B.lo[a] - r.o[a]) * r.inv[a], x2 = (B.hi[a] - r.o[a]) * r.inv[a];
            bn = fmaxf(bn, fminf(x1, x2));
            bf = fminf(bf, fmaxf(x1, x2));
        }
    }
    return pass && bn <= bf && bf >= r.tmin && bn <= r.tmax;
}

// the triangle rule on a valid triangle's vertices: true when it counts, with t and (u, v, w)
__device__ __forceinline__ bool cast_triangle(const CastRay& r, int cull, const float* P, float& t, float& u, float& v, float& w) {
    float bn, bf;
    if (!cast_box_rule(r, cast_tri_box(P, P + 3, P + 6), bn, bf)) return false;
    const float* d = r.d;
    const float e1[3] = {P[3] - P[0], P[4] - P[1], P[5] - P[2]}, e2[3] = {P[6] - P[0], P[7] - P[1], P[8] - P[2]};
    const float p[3] = {d[1] * e2[2] - d[2] * e2[1], d[2] * e2[0] - d[0] * e2[2], d[0] * e2[1] - d[1] * e2[0]};
    const float det = (e1[0] * p[0] + e1[1] * p[1]) + e1[2] * p[2];
    if (!(det != 0.0f)) return false;                                        // (a NaN det is refused by inv below)
    const float inv = 1.0f / det;
    if (!cam_finite(inv)) return false;
    if ((cull == 1 && det < 0.0f) || (cull == 2 && det > 0.0f)) return false;
    const float s[3] = {r.o[0] - P[0], r.o[1] - P[1], r.o[2] - P[2]};
    u = ((s[0] * p[0] + s[1] * p[1]) + s[2] * p[2]) * inv;
    const float q[3] = {s[1] * e1[2] - s[2] * e1[1], s[2] * e1[0] - s[0] * e1[2], s[0] * e1[1] - s[1] * e1[0]};
    v = ((d[0] * q[0] + d[1] * q[1]) + d[2] * q[2]) * inv;
    w = (1.0f - u) - v;
    if (!(u >= 0.0f && v >= 0.0f && w >= 0.0f)) return false;
    const float t0 = ((e2[0] * q[0] + e2[1] * q[1]) + e2[2] * q[2]) * inv;
    if (t0 != t0) return false;
    t = fminf(fmaxf(t0, bn), bf) + 0.0f;
    return r.tmin <= t && t <= r.tmax;
}

struct CastHit {
    int tri;
    float t, u, v, w;
};

// the two queries of a ray: the nearest counting triangle by (t, id), or whether any counts (ANY: no prune by t, done at the first)
template <bool ANY>
struct CastQuery {
    const CastRay& r;
    int cull;
    CastHit best;
    __device__ __forceinline__ bool enter(const CastBox& B, float& bn) {
        float bf;
        return cast_box_rule(r, B, bn, bf) && (ANY || !(bn > best.t));
    }
    __device__ __forceinline__ bool leaf(const float* P, int id) {
        float t, u, v, w;
        if (cast_triangle(r, cull, P, t, u, v, w) && (t < best.t || (t == best.t && id < best.tri) || best.tri < 0)) best = CastHit{id, t, u, v, w};
        return ANY && best.tri >= 0;
    }
};

template <bool ANY>
__device__ __forceinline__ CastHit cast_walk(const CastTree& R, const float* __restrict__ records, const float* __restrict__ nodes,
                                             const CastRay& r, int cull, int* stack, const int* s_off) {
    CastQuery<ANY> q{r, cull, CastHit{-1, __builtin_inff(), 0.0f, 0.0f, 0.0f}};
    cast_tree_walk(R, records, nodes, q, stack, s_off);
    return q.best;
}

// tri, t and bary of a ray as the header writes them: -1 / 0 where nothing counts, -2 / NaN for an unusable ray
__device__ __forceinline__ void cast_write(const CastHit& hit, bool usable, size_t i, int32_t* __restrict__ tri, float* __restrict__ t,
                                           float* __restrict__ bary) {
    const float nan = __builtin_nanf("");
    const bool found = usable && hit.tri >= 0;
    tri[i] = !usable ? -2 : found ? hit.tri : -1;
    t[i] = !usable ? nan : found ? hit.t : 0.0f;
    if (bary) {
        bary[i * 3] = !usable ? nan : found ? hit.w : 0.0f;
        bary[i * 3 + 1] = !usable ? nan : found ? hit.u : 0.0f;
        bary[i * 3 + 2] = !usable ? nan : found ? hit.v : 0.0f;
    }
}
