// The implicit box tree of include/durf_cast.h, defined once for everything that builds or walks it (cast.hip, closest.hip): its
// shape, its workspace, its boxes and records, and the one walk.  Nothing here knows what is asked of the tree: a query brings
// its box rule and its triangle rule (cast_tree_walk).  Internal.
#pragma once
#include "workspace.h"
#include "../../include/durf_cast.h"

#define CB DURF_CAST_BLOCK
#define CLEAF DURF_CAST_LEAF
#define CREC DURF_CAST_RECORD_FLOATS
#define CNODE DURF_CAST_NODE_FLOATS
#define CSTACK DURF_CAST_STACK
static_assert(CB == 256 && CLEAF == 4 && CREC == 10 && CNODE == 8 && CSTACK == 32 && DURF_CAST_TOP == CB, "the layouts the header states");

// the tree of T triangles: n(k) nodes on level k (0: the leaves), stored from node off[k]; the root is level K
struct CastTree {
    int T, K, n0;
    int off[CSTACK];
    int nodes;                         // off[K] + 1, 0 for T == 0
    __host__ __device__ int n(int k) const { return (int)(((long long)n0 + ((1ll << k) - 1)) >> k); }      // ceil halved k times
};

// n_0 = ceil(T / L) leaves, n_{k+1} = ceil(n_k / 2) until a level has one node, level 0 first
static inline CastTree cast_tree(int T) {
    CastTree R{};
    R.T = T;
    if (T == 0) return R;
    int n = (int)durf_cdiv((size_t)T, CLEAF), off = 0, k = 0;
    R.n0 = n;
    for (;; k++) {                                                           // n_0 <= 2^28: at most 29 levels
        R.off[k] = off;
        off += n;
        if (n == 1) break;
        n = (n + 1) / 2;
    }
    R.K = k;
    R.nodes = off;
    return R;
}

// the workspace: the records, then the nodes, each on a 256-byte boundary; 256 bytes for T == 0.  A reader takes them as const.
struct CastWs {
    float *records, *nodes;
    size_t total;
};

static inline CastWs cast_carve(void* base, const CastTree& R) {
    durf::Carver c{(char*)base, 0};
    CastWs w{};
    const size_t slots = R.T == 0 ? 0 : (size_t)R.n0 * CLEAF;
    w.records = (float*)c.take(slots * CREC * 4);
    w.nodes = (float*)c.take((size_t)R.nodes * CNODE * 4);
    w.total = c.total() > 256 ? c.total() : 256;
    return w;
}

static inline bool cast_t_ok(int T) { return T >= 0 && T < DURF_CAST_MAX_TRIANGLES; }

static inline int check_cast_t(const char* who, int T) {
    if (!cast_t_ok(T)) {
        durf_set_error("%s: requirement failed: 0 <= T < %d, T = %d", who, DURF_CAST_MAX_TRIANGLES, T);
        return -1;
    }
    return 0;
}

static inline int check_cast_ws(const char* who, const void* workspace, size_t workspace_bytes, const CastTree& R, CastWs* ws) {
    if (workspace == nullptr || ((size_t)workspace & 255) != 0) {
        durf_set_error("%s: requirement failed: workspace aligned to 256 bytes", who);
        return -1;
    }
    *ws = cast_carve((void*)workspace, R);
    return durf::check_workspace(who, workspace_bytes, ws->total, "durf_cast_workspace_bytes(%d)", R.T);
}

// the level offsets in LDS, where a thread indexes them by its own level (a by-value argument indexed so would go to scratch)
__device__ __forceinline__ void cast_offsets_to_lds(const CastTree& R, int* s_off) {
    if (threadIdx.x < CSTACK) s_off[threadIdx.x] = R.off[threadIdx.x];
    __syncthreads();
}

struct CastBox { float lo[3], hi[3]; };

__device__ __forceinline__ CastBox cast_empty_box() {
    const float inf = __builtin_inff();
    return CastBox{{inf, inf, inf}, {-inf, -inf, -inf}};
}

__device__ __forceinline__ CastBox cast_load_box(const float* nodes, int i) {
    const float4 a = *(const float4*)(nodes + (size_t)i * CNODE), b = *(const float4*)(nodes + (size_t)i * CNODE + 4);
    return CastBox{{a.x, a.y, a.z}, {b.x, b.y, b.z}};
}

__device__ __forceinline__ void cast_store_box(float* nodes, int i, const CastBox& B) {
    *(float4*)(nodes + (size_t)i * CNODE) = make_float4(B.lo[0], B.lo[1], B.lo[2], 0.0f);
    *(float4*)(nodes + (size_t)i * CNODE + 4) = make_float4(B.hi[0], B.hi[1], B.hi[2], 0.0f);
}

__device__ __forceinline__ void cast_union(CastBox& B, const CastBox& C) {
#pragma unroll
    for (int a = 0; a < 3; a++) {
        B.lo[a] = fminf(B.lo[a], C.lo[a]);
        B.hi[a] = fmaxf(B.hi[a], C.hi[a]);
    }
}

// the box of a triangle: min and max per axis, one ulp outward
__device__ __forceinline__ CastBox cast_tri_box(const float* A, const float* B, const float* C) {
    CastBox X;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        X.lo[a] = nextafterf(fminf(fminf(A[a], B[a]), C[a]), -__builtin_inff());
        X.hi[a] = nextafterf(fmaxf(fmaxf(A[a], B[a]), C[a]), __builtin_inff());
    }
    return X;
}

// record j of a leaf: nine coordinates and the id's bits
__device__ __forceinline__ void cast_load_record(const float* rec, int j, float* P /* [10] */) {
#pragma unroll
    for (int c = 0; c < CREC; c += 2) {
        const float2 x = *(const float2*)(rec + j * CREC + c);
        P[c] = x.x;
        P[c + 1] = x.y;
    }
}

// The walk.  Nodes are numbered as a heap: the root is 1, the children of h are 2 h and 2 h + 1, so a node of depth D =
// floor(log2 h) is node h - 2^D of level K - D.  `stack` is this thread's column of the workgroup's LDS array, CB ints apart.
// The query q keeps its own best and supplies the two rules the headers' proofs rest on:
//   bool q.enter(const CastBox&, float& key)   the monotone box rule together with the prune against q's best of that moment;
//                                              of two children that pass, the one with the smaller key is walked first
//   bool q.leaf(const float* P, int id)        the triangle rule on a valid record and the tie-break (value, id); true ends
//                                              the walk once the leaf is done (an any-hit query)
// The root is entered like any node: with nothing found yet a query's best is +inf, which prunes no key that is a number, so
// enter() decides there by the box rule alone.
template <class Q>
__device__ __forceinline__ void cast_tree_walk(const CastTree& R, const float* __restrict__ records, const float* __restrict__ nodes, Q& q,
                                               int* stack, const int* s_off) {
    if (R.nodes == 0) return;
    int sp = 0, cur = 0;
    float key;
    if (q.enter(cast_load_box(nodes, s_off[R.K]), key)) cur = 1;
    const long long max_steps = 4ll * R.nodes + 4;                           // every node is entered at most once, popped at most once
    for (long long step = 0; step < max_steps && cur != 0; step++) {
        const int depth = 31 - __clz(cur), k = R.K - depth;
        if (k == 0) {
            const int l = cur - (1 << depth);
            const float* rec = records + (size_t)l * (CLEAF * CREC);
            bool done = false;
#pragma unroll
            for (int j = 0; j < CLEAF; j++) {
                float P[10];
                cast_load_record(rec, j, P);
                const int id = __float_as_int(P[9]);
                if (id >= 0) done = q.leaf(P, id);
            }
            if (done) return;
            cur = 0;
        } else {
            const int c0 = 2 * cur, j0 = c0 - (2 << depth), nb = R.n(k - 1), base = s_off[k - 1];
            float k0 = 0.0f, k1 = 0.0f;
            bool p0 = false, p1 = false;
            if (j0 < nb) p0 = q.enter(cast_load_box(nodes, base + j0), k0);
            if (j0 + 1 < nb) p1 = q.enter(cast_load_box(nodes, base + j0 + 1), k1);
            if (p0 && p1) {
                const bool swap = k1 < k0;
                if (sp < CSTACK) stack[(sp++) * CB] = swap ? c0 : c0 + 1;    // (one entry per level: sp <= K < CSTACK)
                cur = swap ? c0 + 1 : c0;
            } else {
                cur = p0 ? c0 : p1 ? c0 + 1 : 0;
            }
        }
        while (cur == 0 && sp > 0) {                                         // (bounded by sp)
            const int h = stack[(--sp) * CB];
            const int dh = 31 - __clz(h), kh = R.K - dh;
            if (q.enter(cast_load_box(nodes, s_off[kh] + (h - (1 << dh))), key)) cur = h;
        }
    }
}
