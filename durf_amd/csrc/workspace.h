// How the one-call entry points (forward.hip, train.hip) lay their intermediates out in the caller-owned workspace: the one
// carver, the ray-head buffers both files carve first, and the refusal of a workspace that is too small.  Internal.
#pragma once
#include <cstdarg>
#include <cstdio>
#include "durf_common.h"

namespace durf {

// sub-buffers of the workspace, or just their total with base == null
struct Carver {
    char* base;
    size_t off;
    bool large_on_2mb = false;         // every buffer on 256 bytes, or those >= 1 MB on 2 MB boundaries (train.hip says why)
    void* take(size_t bytes) {
        const size_t al = large_on_2mb && bytes >= ((size_t)1 << 20) ? ((size_t)2 << 20) : (size_t)256;
        off = (off + al - 1) & ~(al - 1);
        void* p = base ? base + off : nullptr;
        off += bytes;
        return p;
    }
    size_t total() const { return (off + 255) & ~(size_t)255; }
};

// what the prologue and the compaction launch write for B rays and K boxes: the head of FwdWs and of TrainWs
struct RayHeadWs {
    float *o_s, *d_s;
    int32_t *hit, *idx_obj, *count_obj, *slot_obj, *idx_cls, *count_cls, *slot_cls;
    void* view;
};

inline void carve_ray_head(Carver& c, RayHeadWs& w, int B, int K) {
    const size_t Kc = K > 0 ? K : 1;
    w.o_s = (float*)c.take((size_t)B * 3 * 4);
    w.d_s = (float*)c.take((size_t)B * 3 * 4);
    w.hit = (int32_t*)c.take((size_t)B * Kc * 4);
    w.view = c.take((size_t)B * 32 * 2);
    w.idx_obj = (int32_t*)c.take(Kc * B * 4);
    w.count_obj = (int32_t*)c.take(Kc * 4);
    w.slot_obj = (int32_t*)c.take((size_t)B * Kc * 4);
    w.idx_cls = (int32_t*)c.take((size_t)2 * B * 4);
    w.count_cls = (int32_t*)c.take(8 * 4);
    w.slot_cls = (int32_t*)c.take((size_t)2 * B * 4);
}

// a workspace the caller sized for another shape is refused, not overrun; sizer: "durf_x_workspace_bytes(%d, ...)" + its arguments
inline int check_workspace(const char* who, size_t have, size_t need, const char* sizer, ...) {
    if (have >= need) return 0;
    char call[160];
    va_list ap;
    va_start(ap, sizer);
    vsnprintf(call, sizeof call, sizer, ap);
    va_end(ap);
    durf_set_error("%s: workspace of %zu bytes, %s = %zu", who, have, call, need);
    return -1;
}

// every workspace starts on 256 bytes, as the carver's sub-buffers do
inline int check_workspace_aligned(const char* who, const void* p) {
    if (p != nullptr && ((size_t)p & 255) == 0) return 0;
    durf_set_error("%s: requirement failed: workspace aligned to 256 bytes", who);
    return -1;
}

}  // namespace durf
