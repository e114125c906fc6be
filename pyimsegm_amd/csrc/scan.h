// scan.h -- prefix sums inside a wave and inside a workgroup (int and uint32_t).  The scan of a whole array by one workgroup is
// launch_exclusive_scan (scan.hip, declared in slic.h).
#pragma once
#include "common.h"

namespace imsegm {

// inclusive prefix sum over the 64 lanes of a wave: six __shfl_up steps
template <typename T> __device__ __forceinline__ T wave_inclusive_scan(T v)
{
    const int lane = threadIdx.x & 63;
    T incl = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const T t = __shfl_up(incl, off, 64);
        if (lane >= off) incl += t;
    }
    return incl;
}

// exclusive prefix sum over a workgroup of NW waves; *total = the sum of all of them (in every thread).  Two barriers: every thread
// of the workgroup has to call it, and a caller may call it again at once.
template <int NW, typename T> __device__ __forceinline__ T block_exclusive_scan(T v, T *total)
{
    __shared__ T wsum[NW];
    int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    T incl = wave_inclusive_scan(v);
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    T base = 0, all = 0;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
        base += w < wave ? wsum[w] : 0;
        all += wsum[w];
    }
    *total = all;
    __syncthreads();
    return base + incl - v;
}

// One step of a stable compaction by a workgroup of 256 (k_compact_gather, k_annot_hist_gather): the output index of this lane's
// element -- *base plus the number of lanes below it in the workgroup whose flag is set; meaningful where the lane's own flag is
// set -- and *base moved on by the number of set flags.  Two barriers: every thread of the workgroup has to call it, and a caller
// may call it again at once.
__device__ __forceinline__ uint32_t block_stable_slot(bool flag, uint32_t *base)
{
    __shared__ uint32_t s_wave[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long votes = __ballot(flag);
    if (lane == 0) s_wave[wave] = (uint32_t)__popcll(votes);
    __syncthreads();
    uint32_t before = *base;
    for (int w = 0; w < wave; ++w) before += s_wave[w];
    *base += s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
    __syncthreads();
    return before + (uint32_t)__popcll(votes & ((1ull << lane) - 1ull));
}

}  // namespace imsegm
