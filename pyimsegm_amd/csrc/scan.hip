// scan.hip -- exclusive prefix sums of a short array in place by ONE workgroup, the total to an address of the caller's: the
// per-workgroup counts of the connectivity pass and of measure.label, the row counts of the edge extraction, the chunk counts of the
// point compaction (a few thousand entries each; 2^18 for the voxels of BASELINE configs[4]).
#include "scan.h"
#include "slic.h"

namespace imsegm {

template <typename T> __global__ void __launch_bounds__(1024) k_exclusive_scan(T *v, int n, T *total_out)
{
    // (four consecutive entries per lane and turn: a turn costs a trip to memory and its barriers whatever it carries)
    constexpr int PER = 4;
    __shared__ T carry;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (int base = 0; base < n; base += 1024 * PER) {
        const int i = base + threadIdx.x * PER;
        T e[PER], t = 0;
#pragma unroll
        for (int j = 0; j < PER; ++j) {
            e[j] = i + j < n ? v[i + j] : 0;
            t += e[j];
        }
        T total;
        T excl = carry + block_exclusive_scan<16>(t, &total);
#pragma unroll
        for (int j = 0; j < PER; ++j) {
            if (i + j < n) v[i + j] = excl;
            excl += e[j];
        }
        __syncthreads();
        if (threadIdx.x == 0) carry += total;
        __syncthreads();
    }
    if (threadIdx.x == 0) *total_out = carry;
}

void launch_exclusive_scan(int32_t *v, int n, int32_t *total_out, hipStream_t st)
{
    hipLaunchKernelGGL(k_exclusive_scan<int32_t>, 1, 1024, 0, st, v, n, total_out);
}

void launch_exclusive_scan(uint32_t *v, int n, uint32_t *total_out, hipStream_t st)
{
    hipLaunchKernelGGL(k_exclusive_scan<uint32_t>, 1, 1024, 0, st, v, n, total_out);
}

}  // namespace imsegm
