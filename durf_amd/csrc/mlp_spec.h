// Static description of the two MLPs of the ray pipeline (obbpose_model.py:293-418) as the
// fused kernels see them: 11 "stages", each a dense layer (or a fused pair) evaluated as
//      D[out_feature, sample] = W^T[out_feature, k] * X[k, sample]
// with v_mfma_f32_32x32x16_bf16, A = weights (LDS), B = activations (registers).
//
// Orientation trick: with samples on the MFMA N axis, the C/D layout (lane = sample,
// regs = 16 of 32 output features) IS the B-operand layout of the next layer up to a fixed
// permutation of the k index, which is folded into the packed weights.  Activations never
// leave registers between layers; only weights stream through LDS.
//
//   accumulator reg r of lane (n, hi) holds out-feature 32*mo + (r&3) + 8*(r>>2) + 4*hi
//   -> B fragment of k-step ks = 2*mo + (r>>3), slot e = r&7:
//      feature(ks, hi, e) = 16*ks + (e&3) + 8*(e>>2) + 4*hi              ("C-perm")
//   inputs that come from memory (encoding, view dirs) use the natural order
//      feature(ks, hi, e) = 16*ks + 8*hi + e                              ("natural")
#pragma once
#include <type_traits>
#include "durf_common.h"

template <int W_>
struct MlpSpec {
    static constexpr int W = W_;
    static constexpr int WT = W / 32;     // output M-tiles of a trunk layer
    static constexpr int KW = W / 16;     // k-steps spanning W features
    static constexpr int KE = DURF_ENC_DIM / 16;    // 4
    static constexpr int KV = DURF_VIEW_DIM / 16;   // 2
    static constexpr int WC = 128;        // net_width_condition
    static constexpr int KC = WC / 16;    // 8
    static constexpr int CT = WC / 32;    // 4
    static constexpr int NSTAGE = 11;
    // stage -> (#output M-tiles, #k-steps)
    //  0: enc -> W relu | 1-4,6,7: W -> W relu | 5: [W,enc] -> W relu
    //  8: W -> [bottleneck W (linear) ; density 1] | 9: [bottleneck, view] -> 128 relu | 10: 128 -> rgb 3
    __host__ __device__ static constexpr int n_mt(int s) { return s <= 7 ? WT : (s == 8 ? WT + 1 : (s == 9 ? CT : 1)); }
    __host__ __device__ static constexpr int n_ks(int s) {
        return s == 0 ? KE : (s == 5 ? KW + KE : (s == 9 ? KW + KV : (s == 10 ? KC : KW)));
    }
    // number of leading k-steps whose B fragments come from the previous stage (C-perm order)
    __host__ __device__ static constexpr int n_ks_perm(int s) { return s == 0 ? 0 : (s == 10 ? KC : KW); }
    // one weight tile = one output M-tile: n_ks chunks of 1 KB (64 lanes x 8 bf16) + 1 bias chunk
    __host__ __device__ static constexpr int tile_chunks(int s) { return n_ks(s) + 1; }
    __host__ __device__ static constexpr int stage_chunk_base(int s) {
        int c = 0;
        for (int i = 0; i < s; i++) c += n_mt(i) * tile_chunks(i);
        return c;
    }
    static constexpr int TOTAL_CHUNKS = stage_chunk_base(NSTAGE);
    static constexpr int MAX_TILE_CHUNKS = KW + KE + 1;
    // activation stash (training): regions 0..7 trunk outputs, 8 bottleneck, 9 view-layer out
    static constexpr int NSTASH = 10;
    __host__ __device__ static constexpr int stash_ks(int j) { return j == 9 ? KC : KW; }
    __host__ __device__ static constexpr int stash_ks_before(int j) { return j * KW; }
    static constexpr int STASH_KS_TOTAL = 9 * KW + KC;   // KB per 32-row tile
};

// flax Dense_l shapes (fan_in, fan_out) for an MLP of width W and input dim `in_dim`
__host__ __device__ inline void durf_layer_shape(int W, int in_dim, int l, int* fin, int* fout) {
    int fi, fo;
    if (l == 0) { fi = in_dim; fo = W; }
    else if (l <= 4) { fi = W; fo = W; }
    else if (l == 5) { fi = W + in_dim; fo = W; }
    else if (l <= 7) { fi = W; fo = W; }
    else if (l == 8) { fi = W; fo = 1; }
    else if (l == 9) { fi = W; fo = W; }
    else if (l == 10) { fi = W + 27; fo = 128; }
    else { fi = 128; fo = 3; }
    *fin = fi; *fout = fo;
}
__host__ __device__ inline size_t durf_layer_offset(int W, int in_dim, int layer, int want_bias) {
    size_t off = 0;
    for (int l = 0; l < layer; l++) {
        int fi, fo;
        durf_layer_shape(W, in_dim, l, &fi, &fo);
        off += (size_t)fi * fo + fo;
    }
    if (want_bias) {
        int fi, fo;
        durf_layer_shape(W, in_dim, layer, &fi, &fo);
        off += (size_t)fi * fo;
    }
    return off;
}

// Forward stage s, output M-tile mo, row i  ->  (flax layer, output column) or layer = -1
template <int W>
__host__ __device__ inline void durf_fwd_out_col(int s, int mo, int i, int* layer, int* col) {
    using S = MlpSpec<W>;
    int L = -1, c = 0;
    if (s <= 7) { L = s; c = 32 * mo + i; }
    else if (s == 8) { if (mo < S::WT) { L = 9; c = 32 * mo + i; } else if (i < 1) { L = 8; c = i; } }
    else if (s == 9) { L = 10; c = 32 * mo + i; }
    else { if (i < 3) { L = 11; c = i; } }
    *layer = L; *col = c;
}
// Forward stage s, k-step ks, lane half hi, slot e -> input row of the flax kernel, or -1 (pad)
template <int W>
__host__ __device__ inline int durf_fwd_in_row(int s, int ks, int hi, int e, int in_dim) {
    using S = MlpSpec<W>;
    const int np = S::n_ks_perm(s);
    if (ks < np) return 16 * ks + (e & 3) + 8 * (e >> 2) + 4 * hi;
    const int f = 16 * (ks - np) + 8 * hi + e;
    if (s == 0) return f < in_dim ? f : -1;
    if (s == 5) return f < in_dim ? W + f : -1;
    if (s == 9) return f < 27 ? W + f : -1;
    return -1;
}

// ---------------------------------------------------------------------------
// Weight fragments LDS -> registers: a REGISTER RING of 2-4 ds_read_b128 in flight, issued from inline asm with
// counted s_waitcnt lgkmcnt(n).  Left to itself hipcc (at the 256-register cap of these kernels) sinks every fragment
// read to just before the MFMA that consumes it -- "ds_read_b128 v[40:43]; s_waitcnt lgkmcnt(0); v_mfma", 1184 times per
// 256-sample block -- so each MFMA waited for a full LDS round trip.  LDS reads return in order, so fragment i is valid
// once at most min(ring - 1, reads after it) younger reads are outstanding; reads hipcc issues by itself in between
// (bias rows, masks) and scalar loads only make that wait conservative (at least one more LDS read has completed than
// the count requires, and the oldest completes first).
// Two output tiles at once (read i: tile i & 1, k-step i >> 1): their MFMAs alternate, so consecutive MFMAs never share
// an accumulator and each B fragment is used twice back to back.  `hook(ks)` runs after the second MFMA of k-step ks.
// ---------------------------------------------------------------------------
// ring depth, measured on MI355X (same-box A/B, 4096 rays x 128 samples; tools/time_fwd.py): forward 2 (690 -> 669 us
// with the training stores, 2-4 alike; 6-8 slower), backward 4 (605 -> 597 us at 2, 582 at 4)
#ifndef FWD_LDS_RING
#define FWD_LDS_RING 2
#endif
#ifndef BWD_LDS_RING
#define BWD_LDS_RING 4
#endif
typedef int v4i_ __attribute__((ext_vector_type(4)));
template <int I, int N, class F>
__device__ __forceinline__ void static_for(F&& f) {
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        static_for<I + 1, N>(f);
    }
}
template <int OFF>
__device__ __forceinline__ v4i_ lds_read16(unsigned addr) {
    v4i_ r;
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(r) : "v"(addr), "n"(OFF));
    return r;
}
template <int N>
__device__ __forceinline__ void lds_wait(v4i_& frag) {     // frag is valid once at most N younger LDS reads are outstanding
    asm volatile("s_waitcnt lgkmcnt(%1)" : "+v"(frag) : "n"(N));
}
__device__ __forceinline__ unsigned lds_addr_of(const char* p) {
    return (unsigned)(size_t)(const __attribute__((address_space(3))) char*)p;
}
template <int NA, int NB, int RING, class H>
__device__ __forceinline__ void mma_pair_ring(const char* slot0, const char* slot1, int lane, const bf16x8* inA,
                                              const bf16x8* inB, f32x16& acc0, f32x16& acc1, H&& hook) {
    constexpr int T = NA + NB, NR = 2 * T;
    constexpr int D = RING < NR ? RING : NR;
    const unsigned l0 = lds_addr_of(slot0) + lane * 16, l1 = lds_addr_of(slot1) + lane * 16;
    v4i_ ring[D];
    static_for<0, D>([&](auto i_) {
        constexpr int i = decltype(i_)::value;
        ring[i] = lds_read16<(i >> 1) * 1024>((i & 1) ? l1 : l0);
    });
    static_for<0, NR>([&](auto i_) {
        constexpr int i = decltype(i_)::value, ks = i >> 1;
        constexpr int later = (NR - 1 - i) < (D - 1) ? (NR - 1 - i) : (D - 1);
        lds_wait<later>(ring[i % D]);
        const bf16x8 a = __builtin_bit_cast(bf16x8, ring[i % D]);
        const bf16x8 b = ks < NA ? inA[ks < NA ? ks : 0] : inB[ks < NA ? 0 : ks - NA];
        if constexpr (i & 1) acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc1, 0, 0, 0);
        else acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc0, 0, 0, 0);
        if constexpr (i + D < NR) ring[i % D] = lds_read16<((i + D) >> 1) * 1024>(((i + D) & 1) ? l1 : l0);
        if constexpr (i & 1) hook(std::integral_constant<int, ks>{});
    });
}

// ---------------------------------------------------------------------------
// Weight stream L2 -> LDS of the fused kernels (k_mlp_fwd, k_mlp_bwd): two slots, one tile group each.
// 16 bytes per lane, global -> LDS (lane-linear destination), as a BUFFER load: descriptor in
// SGPRs, one constant per-lane VGPR offset (lane*16), the chunk offset in an SGPR.  The
// global_load_lds form needs a 64-bit per-lane VGPR address for every tile group; hipcc
// precomputes those, they spill, and a scratch reload next to an in-flight LDS-DMA makes it
// drain the whole weight prefetch (s_waitcnt vmcnt(0)).
// ---------------------------------------------------------------------------
struct WPipe {
    i32x4 rsrc;          // the packed weight stream (the backward's: transposed)
    unsigned gnext;      // byte offset of the next tile group to prefetch (the backward's persistent loop wraps it to 0)
    unsigned lds0;       // LDS byte address of the two slots
    char* lds;
    int slot_bytes;
    int par;             // slot that holds the tile about to be consumed
    int wave, lane;
    int nw;              // waves of the workgroup (8; 4 for launches that would leave half the chip idle: launch_mlp_fwd / launch_mlp_bwd)
    int since;           // vector-memory ops (stores) this wave issued after its last weight DMA (lower bound)
    __device__ __forceinline__ void skip(int chunks) { gnext += chunks * 1024u; }      // stages a variant does not run
    __device__ __forceinline__ void issue(int slot, int chunks) {
        const unsigned dst = lds0 + (unsigned)(slot * slot_bytes);
        for (int c = wave; c < chunks; c += nw)
            lds_dma16_cached(rsrc, gnext + c * 1024u, lane * 16u, dst + c * 1024u);
        gnext += chunks * 1024u;
        since = 0;
    }
    // Make the prefetched tile group visible, start the prefetch of the following one
    // (next_chunks KB, 0 = none) into the other slot, and return the slot to consume.
    // The wait covers this wave's part of the DMA but leaves the stores issued after it in
    // flight; the barrier then publishes every wave's part and frees the other slot.
    __device__ __forceinline__ const char* begin(int next_chunks) {
        wait_vmcnt_le(since);
        __builtin_amdgcn_s_barrier();
        issue(par ^ 1, next_chunks);
        const char* cur = lds + par * slot_bytes;
        par ^= 1;
        return cur;
    }
};

// Tiles are buffered in GROUPS: one barrier + one prefetch burst per group of up to
// SLOT/CH output tiles (4 for a WxW layer), so the 8 waves run unsynchronised for ~64 MFMAs
// each and the next group's weights have a whole group of compute time to arrive.
__host__ __device__ constexpr int group_tiles(int nmt, int ch, int slot) {
    int g = nmt < slot / ch ? nmt : slot / ch;
    return (g > 1) ? (g & ~1) : g;          // even, so tiles can be processed in pairs
}

// ---------------------------------------------------------------------------
// The object phase of a mixed workgroup (k_mlp_fwd<.., MIX>, k_mlp_bwd<.., MIX>), inlined behind the background loop: the
// workgroup turns into TWO groups of four waves that take items of the K object MLPs -- (object, tile pair), times the levels
// in the backward (LEVELS; level-major) -- off an atomic ticket counter until none is left.
//   KERNEL  the function-pointer type of the very instantiation that runs the phase; its last parameter is the phase's
//           argument struct ARGS (fields nobj and ticket; lv.n with LEVELS), read at the offset the kernel's own parameter
//           list gives it (kernarg_last, durf_common.h)
//   pairs_of(ow, k)  tile pairs of object k;  item(ow, kp, level, lds, lane, role, live, k, pair)  one item on four waves
//           and ITEM_LDS bytes at `lds` (kp: the arguments in the kernarg segment itself -- the backward reads its level
//           operands straight from there: a dynamically indexed copy would live in scratch).  The forward's item is
//           ms_fwd_pair ITSELF: behind a wrapper, lambda or function, hipcc schedules the background loop differently.
// Two things keep the phase from costing the background loop -- which sits at the 256-register cap -- anything: (i) nothing of
// it lives in a vector register across the loop (the lane number is re-derived, everything else is wave-uniform), (ii) its ~70
// dwords of arguments are fetched from the kernarg segment HERE, behind an opaque pointer, instead of at kernel entry (as
// ordinary arguments hipcc keeps them in scalar registers across the loop: 85 more SGPR spills, two more vector registers
// reserved for them).  What remains is one more vector register of SGPR spill lanes than the plain kernel has: 28 B of scratch
// instead of 12, six reloads per 256-sample block.  (As a real CALL -- own register allocation, the loop untouched -- the
// phase needs a 360-byte frame for the callee-saved registers, and a launch with that much scratch per lane took ~23 us
// longer whatever it did: profiles/r06_mix.txt.)
// The ticket: a zeroed int the launch leaves zeroed.  Every request adds 2 (one item per group); a workgroup asks for its next
// pair of items while the current one runs and stops at the first ticket past the end, so the launch makes
// ceil(items / 2) + nwg requests and the workgroup that draws the last of them -- every other one has made its last -- resets
// the counter.
// ---------------------------------------------------------------------------
template <class KERNEL, class ARGS, int ITEM_LDS, bool LEVELS, class PairsOf, class Item>
__device__ __forceinline__ void mix_object_items(char* smem, int wave, int nwg, PairsOf&& pairs_of, Item&& item) {
    static_assert(std::is_same<typename kernarg_last<KERNEL>::type, ARGS>::value, "the object arguments are the kernel's LAST parameter");
    typedef const __attribute__((address_space(4))) char* kptr_t;
    kptr_t ka = (kptr_t)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(ka));          // (opaque: the loads below stay below the background loop)
    const __attribute__((address_space(4))) ARGS* const kp = (const __attribute__((address_space(4))) ARGS*)(ka + kernarg_last<KERNEL>::offset);
    const unsigned smem_lds = lds_addr_of(smem);
    ARGS ow;
    load_kernarg(ow, (kptr_t)kp);          // (scalar loads: a constant-address-space source)
    const int lane = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
    // (the ticket requests are wave 1's: wave 0 starts every item with the ray loads of the encoding / the head gradients, and
    // a returning atomic ahead of them in its queue would be waited for with them)
    const bool first = wave == MIX_TICKET_WAVE && lane == 0;
    // (waves w and w + 4 share a SIMD: the second group's roles are rotated by two, so that the two groups' role-0 waves --
    // which carry an item's serial head: the encoding / the head gradients, the density and rgb heads -- run on different SIMDs)
    const int half = wave >> 2, w4 = (wave + MIX_ROLE_ROT * half) & 3;
    char* const lds = smem + half * ITEM_LDS;
    volatile __attribute__((address_space(3))) int* const tk =
        (volatile __attribute__((address_space(3))) int*)(size_t)(__builtin_amdgcn_readfirstlane(smem_lds) + 2u * ITEM_LDS);
    // (the objects' pair counts once per workgroup, in LDS: re-read from memory for every item they were a chain of K
    // dependent loads in front of it)
    volatile __attribute__((address_space(3))) int* const npl = tk + 4;
    if (wave == 0 && lane < ow.nobj) npl[lane] = (int)pairs_of(ow, lane);
    ms_barrier();
    size_t total = 0;
    for (int k = 0; k < ow.nobj; k++) total += (size_t)npl[k];
    total = (size_t)__builtin_amdgcn_readfirstlane((unsigned)total);
    size_t items = total;
    if constexpr (LEVELS) items = total * (size_t)ow.lv.n;
    const int last = 2 * (int)((items + 1) / 2 + nwg - 1);            // the value the LAST request of the launch returns
    int t = 0;
    // (a GLOBAL atomic: a flat one counts on lgkmcnt, and the first barrier of the item would wait for the request under way)
    DURF_G(int)* const ticket = (DURF_G(int)*)ow.ticket;
    if (first) { t = __hip_atomic_fetch_add(ticket, 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); *tk = t; }
    ms_barrier();
    t = __builtin_amdgcn_readfirstlane(*tk);
    while ((size_t)t < items) {
        int tn = 0;
        if (first) tn = __hip_atomic_fetch_add(ticket, 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // the next request is under way while this item runs
        const size_t it = (size_t)t + (size_t)half;
        const bool live = it < items;
        int level = 0;
        if constexpr (LEVELS) level = __builtin_amdgcn_readfirstlane(live ? (int)(it / total) : 0);
        size_t k = 0, pair = live ? it - (size_t)level * total : 0;
        for (; live && k + 1 < (size_t)ow.nobj; k++) {
            const size_t np = (size_t)npl[k];
            if (pair < np) break;
            pair -= np;
        }
        k = (size_t)__builtin_amdgcn_readfirstlane((unsigned)(live ? k : 0));
        item(ow, kp, level, lds, lane, w4, live, k, pair);
        if (first) *tk = tn;
        ms_barrier();
        t = __builtin_amdgcn_readfirstlane(*tk);
    }
    if (first && t == last) __hip_atomic_store(ticket, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Host side of a mixed launch: the LDS of a background block (two weight slots), which the two object groups must fit, set
// once per kernel, and the grid -- one workgroup per CU: the background blocks' (capacity: the counts live on the device),
// then room for `obj_items` object items, two per workgroup.
constexpr int MIX_LDS_BYTES = 2 * 4 * (MlpSpec<256>::KW + 1) * 1024;
template <auto KERNEL>
static inline void dynamic_lds_once(int bytes) {      // once per kernel (the attribute sticks to the function)
    static bool attr_set = false;
    if (!attr_set) {
        (void)hipFuncSetAttribute((const void*)KERNEL, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
        attr_set = true;
    }
}
template <auto KERNEL, int ITEM_LDS>
static inline unsigned mix_launch_grid(size_t rows, size_t obj_items) {
    static_assert(2 * ITEM_LDS + 96 <= MIX_LDS_BYTES, "two object groups fit the background block's LDS");
    dynamic_lds_once<KERNEL>(MIX_LDS_BYTES);
    const unsigned n = durf_cdiv(rows, 256) + durf_cdiv(obj_items, 2);
    return n < 256u ? n : 256u;
}

// Block shape of the persistent launches (k_mlp_fwd / k_mlp_bwd): a launch that fills at most half the chip with 256-sample
// blocks (8 waves) runs as 128-sample blocks (4 waves) -- twice the workgroups, each with half the dependent work, one per CU
// as before (cfg1: 128 -> 256 workgroups).  The background MLP only (W = 256, K = 1), and not the backward that also returns
// d(enc) (`pose`).  grid_x: persistent, at most one workgroup per CU and object.
struct MlpBlockShape { bool half; unsigned per, grid_x, block; };
static inline MlpBlockShape mlp_block_shape(int width, int K, size_t rows, bool pose) {
    const bool half = width == 256 && K == 1 && !pose && durf_cdiv(rows, 256) <= 128;
    const unsigned per = half ? 128u : 256u, nblk = durf_cdiv(rows, per);
    return {half, per, nblk < 256u ? nblk : 256u, half ? 256u : 512u};
}
// Grid of the M-split kernels (workgroups of 256 threads) over `items` 64-sample pairs -- capacity; the counts live on the
// device and decide (see the kernels) -- : one workgroup per CU at most, one round
static inline unsigned ms_grid(size_t items) { return (unsigned)(items < 256 ? items : 256); }
