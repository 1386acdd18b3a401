// The three-pass prefix sum of the feature libraries (lidar.hip, mesh.hip, geom.hip), for int and double: per-block sums, ONE
// workgroup's exclusive scan of the block sums (k_scan_block_sums), per-element offsets.  Passes 1 and 3 differ in what they
// compute and write and stay with their library; they share the device pieces below.  A block is a workgroup of WAVES waves.
// Every sum is taken in one stated order, so the double instantiation is deterministic (include/durf_geom.h); for int any
// order is exact.  Included by the feature libraries only.  Internal.
#pragma once
#include "durf_common.h"

#define SCAN_THREADS 1024               // k_scan_block_sums' one workgroup: a round scans this many block sums
#define SCAN_WAVES (SCAN_THREADS / DURF_WAVE)

// inclusive prefix sum across the 64 lanes of a wave (float: wave_incl_scan of durf_common.h)
template <typename T>
__device__ __forceinline__ T wave_incl_scan(T v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const T t = __shfl_up(v, o, 64);
        if (lane >= o) v += t;
    }
    return v;
}

// passes 1 and 3, before the barrier: v's inclusive scan over the wave; the wave's last lane leaves the wave's sum in s_wave
template <typename T>
__device__ __forceinline__ T scan_wave_to_lds(T v, T* s_wave) {
    const int lane = threadIdx.x & (DURF_WAVE - 1);
    const T inc = wave_incl_scan(v, lane);
    if (lane == DURF_WAVE - 1) s_wave[threadIdx.x / DURF_WAVE] = inc;
    return inc;
}

// pass 1, after the barrier: the block's sum, the waves' sums added in wave order (thread 0 writes it to sums[blockIdx.x])
template <int WAVES, typename T>
__device__ __forceinline__ T scan_block_sum(const T* s_wave) {
    T a = 0;
#pragma unroll
    for (int v = 0; v < WAVES; v++) a += s_wave[v];
    return a;
}

// pass 3, after the barrier: the sum of everything before this thread's wave -- the block's offset, then the earlier waves'
// sums added in wave order.  The caller adds its inclusive scan value (or that minus its own element, for exclusive offsets).
template <int WAVES, typename T>
__device__ __forceinline__ T scan_before_wave(T block_offset, const T* s_wave) {
    const int wave = threadIdx.x / DURF_WAVE;
    T before = block_offset;
#pragma unroll
    for (int u = 0; u < WAVES; u++)
        if (u < wave) before += s_wave[u];
    return before;
}

// pass 2: ONE workgroup turns R rows of block sums -- row r is sums[r (nb + 1) .. r (nb + 1) + nb) -- into their exclusive
// scans in place; row r's total goes to its slot nb and to totals[r].  Internal linkage: every library that includes this
// launches its own copy, whatever else is loaded into the process.
namespace {
template <typename T, int R>
__global__ void __launch_bounds__(SCAN_THREADS)
k_scan_block_sums(int nb, T* __restrict__ sums, T* __restrict__ totals) {
    __shared__ T s_wave[R][SCAN_WAVES];
    const int t = threadIdx.x, lane = t & (DURF_WAVE - 1), wave = t / DURF_WAVE;
    T carry[R] = {};
    for (int base = 0; base < nb; base += SCAN_THREADS) {                   // (uniform over the workgroup)
        const int i = base + t;
        T x[R], ix[R];
#pragma unroll
        for (int r = 0; r < R; r++) {
            x[r] = i < nb ? sums[(size_t)r * (nb + 1) + i] : T(0);
            ix[r] = wave_incl_scan(x[r], lane);
            if (lane == DURF_WAVE - 1) s_wave[r][wave] = ix[r];
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < R; r++) {
            T before = 0, all = 0;
#pragma unroll
            for (int v = 0; v < SCAN_WAVES; v++) {
                const T a = s_wave[r][v];
                if (v < wave) before += a;
                all += a;
            }
            if (i < nb) sums[(size_t)r * (nb + 1) + i] = (carry[r] + before) + (ix[r] - x[r]);
            carry[r] += all;
        }
        __syncthreads();                                                    // s_wave is rewritten by the next round
    }
    if (t == 0) {
#pragma unroll
        for (int r = 0; r < R; r++) {
            sums[(size_t)r * (nb + 1) + nb] = carry[r];
            totals[r] = carry[r];
        }
    }
}
}  // namespace
