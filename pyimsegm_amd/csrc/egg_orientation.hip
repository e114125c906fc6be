// egg_orientation.hip -- the kernels behind imsegm_orient_stack / imsegm_stack_median_u8 (experiments_ovary_detect/
// run_egg_swap_orientation.py of the reference): the template of a stage as twice the per-pixel median of its stack of cut-outs, the
// nine integer sums that decide both swap tests, and the turn of the flagged cut-outs.  DESIGN.md section 4 "Egg orientation";
// pyimsegm_amd/egg_orientation.py stack_median2_host / orientation_sums_host are the definitions.  Integers only.
//
// Median: one lane per pixel, adjacent lanes on adjacent pixels of a plane, four waves of a workgroup share the N planes of the same
// 64 pixels.  The selection is a radix selection over the 8-bit values in two passes of 16 bins, high nibble then low nibble.  A
// lane's 16 counters are 16 bits wide and sit pairwise in eight LDS words, word j of lane l at [j][l]: a lane touches bank l only
// and only its own words, so the counting needs neither atomics nor barriers, and a count of at most 65 535 never carries into
// its neighbour.  Both order statistics s[(N - 1) / 2] and s[N / 2] come from the one selection: they lie in the same high bin, or
// the first is the largest value of its bin and the second the smallest of the next occupied one, which pass 2 tracks in a register.
#include <algorithm>

#include "egg_orientation.h"

namespace imsegm {

namespace {

constexpr int EO_MED_WAVES = 4, EO_SUM_THREADS = 1024, EO_SUM_WAVES = EO_SUM_THREADS / 64;

__global__ void __launch_bounds__(256) k_eo_extract(const uint8_t *__restrict__ stack, size_t hw, int C, int channel,
                                                    uint8_t *__restrict__ planes)
{
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= hw) return;
    const size_t at = (size_t)blockIdx.y * hw + p;
    planes[at] = stack[at * (size_t)C + (size_t)channel];
}

__device__ __forceinline__ uint32_t eo_count(const uint32_t (&hist)[EO_MED_WAVES][8][64], int bin, int lane)
{
    uint32_t c = 0;
#pragma unroll
    for (int wv = 0; wv < EO_MED_WAVES; ++wv) c += (hist[wv][bin >> 1][lane] >> ((bin & 1) * 16)) & 0xffffu;
    return c;
}

__global__ void __launch_bounds__(64 * EO_MED_WAVES) k_eo_median(const uint8_t *__restrict__ planes, int N, size_t hw,
                                                                uint16_t *__restrict__ template2)
{
    __shared__ uint32_t s_hist[EO_MED_WAVES][8][64];
    __shared__ int s_bin1[64], s_bin2[64], s_base[64], s_least[EO_MED_WAVES][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t p = (size_t)blockIdx.x * 64 + lane;
    const bool live = p < hw;
    const int k1 = (N - 1) / 2, k2 = N / 2;
    // pass 1: the high nibbles
#pragma unroll
    for (int j = 0; j < 8; ++j) s_hist[wave][j][lane] = 0;
    if (live) {
#pragma unroll 8
        for (int i = wave; i < N; i += EO_MED_WAVES) {
            const int bin = planes[(size_t)i * hw + p] >> 4;
            s_hist[wave][bin >> 1][lane] += 1u << ((bin & 1) * 16);
        }
    }
    __syncthreads();
    if (wave == 0) {
        int cum = 0, bin1 = -1, bin2 = -1, base = 0;
        for (int bin = 0; bin < 16; ++bin) {
            const int c = (int)eo_count(s_hist, bin, lane);
            if (bin1 < 0 && k1 < cum + c) {
                bin1 = bin;
                base = cum;
            }
            if (bin2 < 0 && k2 < cum + c) bin2 = bin;
            cum += c;
        }
        s_bin1[lane] = bin1;
        s_bin2[lane] = bin2;
        s_base[lane] = base;
    }
    __syncthreads();
    // pass 2: the low nibbles of the values in bin1; the smallest value of bin2
    const int bin1 = s_bin1[lane], bin2 = s_bin2[lane];
    int least = 255;
#pragma unroll
    for (int j = 0; j < 8; ++j) s_hist[wave][j][lane] = 0;
    if (live) {
#pragma unroll 8
        for (int i = wave; i < N; i += EO_MED_WAVES) {
            const int v = planes[(size_t)i * hw + p];
            const int high = v >> 4, low = v & 15;
            if (high == bin1) s_hist[wave][low >> 1][lane] += 1u << ((low & 1) * 16);
            if (high == bin2) least = min(least, v);
        }
    }
    s_least[wave][lane] = least;
    __syncthreads();
    if (wave == 0 && live) {
        const int r1 = k1 - s_base[lane], r2 = k2 - s_base[lane];
        int cum = 0, low1 = -1, low2 = -1;
        for (int bin = 0; bin < 16; ++bin) {
            const int c = (int)eo_count(s_hist, bin, lane);
            if (low1 < 0 && r1 < cum + c) low1 = bin;
            if (low2 < 0 && r2 < cum + c) low2 = bin;
            cum += c;
        }
        int second = bin1 * 16 + low2;
        if (bin2 != bin1) {
            second = s_least[0][lane];
#pragma unroll
            for (int wv = 1; wv < EO_MED_WAVES; ++wv) second = min(second, s_least[wv][lane]);
        }
        template2[p] = (uint16_t)(bin1 * 16 + low1 + second);
    }
}

__device__ __forceinline__ int wave_min_int(int v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = min(v, __shfl_xor(v, off, 64));
    return v;
}
__device__ __forceinline__ int wave_max_int(int v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = max(v, __shfl_xor(v, off, 64));
    return v;
}

__global__ void __launch_bounds__(256) k_eo_template_range(const uint16_t *__restrict__ template2, size_t hw, uint32_t *__restrict__ range)
{
    int lo = 0xffff, hi = 0;
    for (size_t p = (size_t)blockIdx.x * 256 + threadIdx.x; p < hw; p += (size_t)gridDim.x * 256) {
        const int t = template2[p];
        lo = min(lo, t);
        hi = max(hi, t);
    }
    lo = wave_min_int(lo);
    hi = wave_max_int(hi);
    if ((threadIdx.x & 63) == 0) {
        atomicMin(&range[0], (uint32_t)lo);
        atomicMax(&range[1], (uint32_t)hi);
    }
}

// the sum of v over the workgroup, in every thread (s_red: EO_SUM_WAVES words)
__device__ __forceinline__ long long eo_block_sum(long long v, long long *s_red)
{
    v = wave_sum_i64(v);
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
    __syncthreads();
    long long total = 0;
#pragma unroll
    for (int wv = 0; wv < EO_SUM_WAVES; ++wv) total += s_red[wv];
    __syncthreads();
    return total;
}

// One workgroup per image; three sweeps, the second and third out of the cache: the minimum comes before cnt and S, and both come
// before g.  The mirror of pixel p = r w + c is (h - 1 - r) w + (w - 1 - c) = h w - 1 - p.
__global__ void __launch_bounds__(EO_SUM_THREADS) k_eo_sums(const uint8_t *__restrict__ planes, uint32_t hw, uint32_t w,
                                                           const uint16_t *__restrict__ template2, const uint32_t *__restrict__ range,
                                                           int mode, long long *__restrict__ sums, uint8_t *__restrict__ flags)
{
    __shared__ long long s_red[EO_SUM_WAVES];
    __shared__ int s_lo[EO_SUM_WAVES], s_hi[EO_SUM_WAVES];
    const uint8_t *a = planes + (size_t)blockIdx.x * hw;
    const uint32_t tid = threadIdx.x;
    long long A = 0, P = 0, Pf = 0;
    int lo = 255, hi = 0;
    for (uint32_t p = tid; p < hw; p += EO_SUM_THREADS) {
        const int v = a[p], f = a[hw - 1u - p], t = template2[p];
        A += v;
        P += v * t;
        Pf += f * t;
        lo = min(lo, v);
        hi = max(hi, v);
    }
    A = eo_block_sum(A, s_red);
    P = eo_block_sum(P, s_red);
    Pf = eo_block_sum(Pf, s_red);
    lo = wave_min_int(lo);
    hi = wave_max_int(hi);
    if ((tid & 63) == 0) {
        s_lo[tid >> 6] = lo;
        s_hi[tid >> 6] = hi;
    }
    __syncthreads();
#pragma unroll
    for (int wv = 0; wv < EO_SUM_WAVES; ++wv) {
        lo = min(lo, s_lo[wv]);
        hi = max(hi, s_hi[wv]);
    }
    long long cnt = 0, S = 0;
    for (uint32_t p = tid; p < hw; p += EO_SUM_THREADS) {
        const int v = a[p];
        if (v > lo) {
            cnt += 1;
            S += v;
        }
    }
    cnt = eo_block_sum(cnt, s_red);
    S = eo_block_sum(S, s_red);
    // g = [a cnt > S]; the left third and the right third of the columns (a third of 0 columns: nothing, and everything)
    const uint32_t part = w / 3u;
    long long L = 0, R = 0;
    for (uint32_t p = tid; p < hw; p += EO_SUM_THREADS) {
        const long long v = a[p];
        if (v * cnt > S) {
            const uint32_t col = p % w;
            L += col < part;
            R += part == 0u || col >= w - part;
        }
    }
    L = eo_block_sum(L, s_red);
    R = eo_block_sum(R, s_red);
    if (tid == 0) {
        long long *out = sums + (size_t)blockIdx.x * EO_SUM_WORDS;
        out[EO_A] = A;
        out[EO_MIN] = lo;
        out[EO_MAX] = hi;
        out[EO_P] = P;
        out[EO_PF] = Pf;
        out[EO_CNT] = cnt;
        out[EO_S] = S;
        out[EO_L] = L;
        out[EO_R] = R;
        flags[blockIdx.x] = mode == EO_MODE_CC ? (lo != hi && range[0] != range[1] && P < Pf) : (L > R);
    }
}

// one lane per pixel pair (q, hw - 1 - q), q < hw / 2: the middle pixel of an odd count stays where it is
__global__ void __launch_bounds__(256) k_eo_turn(uint8_t *__restrict__ stack, size_t hw, int C, const uint8_t *__restrict__ flags)
{
    if (!flags[blockIdx.y]) return;
    const size_t q = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= hw / 2) return;
    uint8_t *img = stack + (size_t)blockIdx.y * hw * (size_t)C;
    uint8_t *front = img + q * (size_t)C, *back = img + (hw - 1 - q) * (size_t)C;
    for (int c = 0; c < C; ++c) {
        const uint8_t x = front[c];
        front[c] = back[c];
        back[c] = x;
    }
}

}  // namespace

int launch_eo_extract(const uint8_t *stack, int N, size_t hw, int C, int channel, uint8_t *planes, hipStream_t st)
{
    hipLaunchKernelGGL(k_eo_extract, dim3(cdiv((long)hw, 256), N), 256, 0, st, stack, hw, C, channel, planes);
    HIP_TRY(hipGetLastError());
    return 0;
}

int launch_eo_median(const uint8_t *planes, int N, size_t hw, uint16_t *template2, hipStream_t st)
{
    hipLaunchKernelGGL(k_eo_median, cdiv((long)hw, 64), 64 * EO_MED_WAVES, 0, st, planes, N, hw, template2);
    HIP_TRY(hipGetLastError());
    return 0;
}

int launch_eo_template_range(const uint16_t *template2, size_t hw, uint32_t *range, hipStream_t st)
{
    HIP_TRY(hipMemsetAsync(range, 0xff, 4, st));
    HIP_TRY(hipMemsetAsync(range + 1, 0, 4, st));
    hipLaunchKernelGGL(k_eo_template_range, std::min(cdiv((long)hw, 256), 1024), 256, 0, st, template2, hw, range);
    HIP_TRY(hipGetLastError());
    return 0;
}

int launch_eo_sums(const uint8_t *planes, int N, int h, int w, const uint16_t *template2, const uint32_t *range, int mode, long long *sums,
                   uint8_t *flags, hipStream_t st)
{
    hipLaunchKernelGGL(k_eo_sums, N, EO_SUM_THREADS, 0, st, planes, (uint32_t)((size_t)h * w), (uint32_t)w, template2, range, mode, sums,
                       flags);
    HIP_TRY(hipGetLastError());
    return 0;
}

int launch_eo_turn(uint8_t *stack, int N, size_t hw, int C, const uint8_t *flags, hipStream_t st)
{
    if (hw < 2) return 0;
    hipLaunchKernelGGL(k_eo_turn, dim3(cdiv((long)(hw / 2), 256), N), 256, 0, st, stack, hw, C, flags);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // namespace imsegm
