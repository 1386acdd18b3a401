// The ray query of the implicit box tree (include/durf_cast.h), defined once for everything that sends rays through it (cast.hip:
// the nearest hit and any hit; shade.hip: the secondary rays of a shaded picture): the ray, the header's box rule and triangle
// rule, the two queries of cast_tree.h's one walk, the outputs of a hit, and the launchers' refusal of a mesh under the tree's
// limit.  The mesh itself -- the readable triangle and its fetch -- is triangles.h's.  Internal.
#pragma once
#include "cast_tree.h"
#include "triangles.h"

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
    float e1[3], e2[3], p[3], s[3], q[3];
    vec3_sub(P + 3, P, e1);
    vec3_sub(P + 6, P, e2);
    vec3_cross(d, e2, p);
    const float det = vec3_dot(e1, p);
    if (!(det != 0.0f)) return false;                                        // (a NaN det is refused by inv below)
    const float inv = 1.0f / det;
    if (!cam_finite(inv)) return false;
    if ((cull == 1 && det < 0.0f) || (cull == 2 && det > 0.0f)) return false;
    vec3_sub(r.o, P, s);
    u = vec3_dot(s, p) * inv;
    vec3_cross(s, e1, q);
    v = vec3_dot(d, q) * inv;
    w = (1.0f - u) - v;
    if (!(u >= 0.0f && v >= 0.0f && w >= 0.0f)) return false;
    const float t0 = vec3_dot(e2, q) * inv;
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

// the mesh of an entry that also takes the tree: triangles.h's refusals around the tree's own limit on T
inline int check_cast_mesh(const char* who, int V, int T, const float* vertices, const int32_t* triangles) {
    return check_mesh(who, V, T, check_cast_t(who, T), vertices, triangles);
}
