// annotation.hip -- annotation colours: the device side of imsegm/annotation.py -- convert_img_colors_to_labels_reverted (:113-125),
// convert_img_labels_to_colors (:146-160), PIL's getcolors behind unique_image_colors / image_frequent_colors (:61-67, :184-188),
// image_color_2_labels / quantize_image_nearest_color (:245-248, :271-275) and image_inpaint_pixels under
// quantize_image_nearest_pixel (:279-321).
//
// Everything is integer arithmetic:
//   match     4 interleaved uint8 pixels = 12 bytes per lane and turn, against a table of packed colours in LDS
//   paint     4 int32 labels = 16 bytes per lane and turn, 12 bytes out
//   hist      one uint32 bin per 24-bit colour; ONE atomic per run of equal colours among the lanes of a wave; bins in use are
//             compacted in key order with the chunk counts going through launch_exclusive_scan (scan.hip)
//   nearest   exact nearest-feature transform, the sibling of the distance transform of boundary.hip: it carries WHICH pixel is
//             nearest.  columns: src(y, x) = row of the nearest valid pixel of column x (the upper one at equal distance); rows: the
//             outward search of k_edt_rows over (d2, flat index) packed into one uint64, so that one min keeps the smaller squared
//             distance and, at equal distance, the smaller row-major index.
#include "annotation.h"
#include "scan.h"
#include "slic.h"

namespace imsegm {

struct Px4 {                                           // 4 interleaved pixels as they lie in memory (little endian)
    uint32_t a, b, c;                                  // r0 g0 b0 r1 | g1 b1 r2 g2 | b2 r3 g3 b3
};

__device__ __forceinline__ void px4_keys(const Px4 &v, uint32_t (&key)[4])
{
    key[0] = __builtin_bswap32(v.a) >> 8;
    key[1] = ((v.a >> 24) << 16) | ((v.b & 0xffu) << 8) | ((v.b >> 8) & 0xffu);
    key[2] = (((v.b >> 16) & 0xffu) << 16) | ((v.b >> 24) << 8) | (v.c & 0xffu);
    key[3] = __builtin_bswap32(v.c) & 0xffffffu;
}
// the three bytes of a packed colour in memory order (r in the lowest byte)
__device__ __forceinline__ uint32_t key_bytes(uint32_t key) { return __builtin_bswap32(key << 8); }
__device__ __forceinline__ Px4 px4_pack(const uint32_t (&key)[4])
{
    const uint32_t p0 = key_bytes(key[0]), p1 = key_bytes(key[1]), p2 = key_bytes(key[2]), p3 = key_bytes(key[3]);
    Px4 v;
    v.a = p0 | (p1 << 24);
    v.b = (p1 >> 8) | (p2 << 16);
    v.c = (p2 >> 16) | (p3 << 8);
    return v;
}
__device__ __forceinline__ uint32_t px_key(const uint8_t *p) { return ((uint32_t)p[0] << 16) | ((uint32_t)p[1] << 8) | (uint32_t)p[2]; }
__device__ __forceinline__ void px_store(uint8_t *p, uint32_t key)
{
    p[0] = (uint8_t)(key >> 16);
    p[1] = (uint8_t)(key >> 8);
    p[2] = (uint8_t)key;
}
// |r - r'| + |g - g'| + |b - b'| of two packed colours (the fourth byte of both is 0)
__device__ __forceinline__ uint32_t key_l1(uint32_t a, uint32_t b) { return __builtin_amdgcn_sad_u8(a, b, 0u); }

// ---------------------------------------------------------------------------------------------------
// match: NP pixels at once against the table (one LDS read per entry serves all of them).  MODE 0: the label of the LAST entry that
// equals the pixel, -1 for none.  MODE 1, 2: the index of the FIRST entry at the smallest L1 distance.
// ---------------------------------------------------------------------------------------------------
template <int MODE, int NP>
__device__ __forceinline__ void match_pixels(const uint32_t (&key)[NP], const uint32_t *s_key, const int32_t *s_lab, int K, int (&res)[NP])
{
    uint32_t best[NP];
#pragma unroll
    for (int j = 0; j < NP; ++j) {
        res[j] = MODE == 0 ? -1 : 0;
        best[j] = 0xffffffffu;
    }
    for (int k = 0; k < K; ++k) {
        const uint32_t ck = s_key[k];
        if (MODE == 0) {
            const int lab = s_lab[k];
#pragma unroll
            for (int j = 0; j < NP; ++j) res[j] = key[j] == ck ? lab : res[j];
        } else {
#pragma unroll
            for (int j = 0; j < NP; ++j) {
                const uint32_t d = key_l1(key[j], ck);
                if (d < best[j]) {
                    best[j] = d;
                    res[j] = k;
                }
            }
        }
    }
}

template <int MODE>
__global__ void __launch_bounds__(256)
k_annot_match(const uint8_t *__restrict__ image, size_t n, const uint32_t *__restrict__ keys, const int32_t *__restrict__ labels, int K,
              void *__restrict__ out, unsigned long long *__restrict__ unmatched)
{
    __shared__ uint32_t s_key[ANNOT_MAX_COLORS];
    __shared__ int32_t s_lab[ANNOT_MAX_COLORS];
    __shared__ int s_unmatched;
    for (int k = threadIdx.x; k < K; k += 256) {
        s_key[k] = keys[k];
        s_lab[k] = MODE == 0 ? labels[k] : k;
    }
    if (threadIdx.x == 0) s_unmatched = 0;
    __syncthreads();
    const size_t n4 = n / 4;                           // whole groups of 4 pixels; the n % 4 pixels behind them one by one
    int32_t *out_lab = reinterpret_cast<int32_t *>(out);
    uint8_t *out_rgb = reinterpret_cast<uint8_t *>(out);
    int missed = 0;
    for (size_t g = (size_t)blockIdx.x * 256 + threadIdx.x; g < n4; g += (size_t)gridDim.x * 256) {
        const Px4 v = *reinterpret_cast<const Px4 *>(image + 12 * g);
        uint32_t key[4];
        int res[4];
        px4_keys(v, key);
        match_pixels<MODE, 4>(key, s_key, s_lab, K, res);
        if (MODE == 2) {
            uint32_t chosen[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) chosen[j] = s_key[res[j]];
            *reinterpret_cast<Px4 *>(out_rgb + 12 * g) = px4_pack(chosen);
        } else {
            *reinterpret_cast<int4 *>(out_lab + 4 * g) = make_int4(res[0], res[1], res[2], res[3]);
            if (MODE == 0) missed += (res[0] < 0) + (res[1] < 0) + (res[2] < 0) + (res[3] < 0);
        }
    }
    if (blockIdx.x == 0 && threadIdx.x < (int)(n - 4 * n4)) {
        const size_t i = 4 * n4 + threadIdx.x;
        uint32_t key[1] = { px_key(image + 3 * i) };
        int res[1];
        match_pixels<MODE, 1>(key, s_key, s_lab, K, res);
        if (MODE == 2) {
            px_store(out_rgb + 3 * i, s_key[res[0]]);
        } else {
            out_lab[i] = res[0];
            if (MODE == 0) missed += res[0] < 0;
        }
    }
    if (MODE == 0 && unmatched) {
        // (labels are >= 0, the entry point refuses others: a negative result is a pixel no entry equals)
        missed = wave_sum_i32(missed);
        if ((threadIdx.x & 63) == 0 && missed) atomicAdd(&s_unmatched, missed);
        __syncthreads();
        if (threadIdx.x == 0 && s_unmatched) atomicAdd(unmatched, (unsigned long long)s_unmatched);
    }
}

// ---------------------------------------------------------------------------------------------------
// paint: label -> colour through the table [min_label, min_label + n_table) in LDS
// ---------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
k_annot_paint(const int32_t *__restrict__ labels, size_t n, int min_label, int n_table, const uint32_t *__restrict__ keys,
              const uint8_t *__restrict__ present, uint8_t *__restrict__ image_out, int *__restrict__ missing)
{
    __shared__ uint32_t s_key[ANNOT_MAX_COLORS];
    __shared__ uint8_t s_present[ANNOT_MAX_COLORS];
    for (int k = threadIdx.x; k < n_table; k += 256) {
        s_key[k] = keys[k];
        s_present[k] = present[k];
    }
    __syncthreads();
    const size_t n4 = n / 4;
    bool bad = false;
    auto colour = [&](int lab) -> uint32_t {
        const long long at = (long long)lab - (long long)min_label;
        const bool in_table = at >= 0 && at < (long long)n_table;
        const bool ok = in_table && s_present[in_table ? (int)at : 0] != 0;
        bad |= !ok;
        return ok ? s_key[(int)at] : 0u;
    };
    for (size_t g = (size_t)blockIdx.x * 256 + threadIdx.x; g < n4; g += (size_t)gridDim.x * 256) {
        const int4 lab = *reinterpret_cast<const int4 *>(labels + 4 * g);
        const uint32_t chosen[4] = { colour(lab.x), colour(lab.y), colour(lab.z), colour(lab.w) };
        *reinterpret_cast<Px4 *>(image_out + 12 * g) = px4_pack(chosen);
    }
    if (blockIdx.x == 0 && threadIdx.x < (int)(n - 4 * n4)) {
        const size_t i = 4 * n4 + threadIdx.x;
        px_store(image_out + 3 * i, colour(labels[i]));
    }
    // one integer atomic per wave that met such a label: the word only ever goes from 0 to 1
    if (__ballot(bad) != 0 && (threadIdx.x & 63) == 0) atomicOr(missing, 1);
}

// ---------------------------------------------------------------------------------------------------
// histogram: the lanes of a wave hold consecutive items; a lane whose key differs from its left neighbour's opens a run and adds
// the run's length times `weight` with one atomic
// ---------------------------------------------------------------------------------------------------
__device__ __forceinline__ void hist_add_runs(uint32_t key, bool valid, uint32_t weight, uint32_t *__restrict__ bins)
{
    const int lane = threadIdx.x & 63;
    const uint32_t left = (uint32_t)__shfl_up((int)key, 1, 64);
    const unsigned long long valids = __ballot(valid);
    const bool left_valid = lane > 0 && ((valids >> (lane - 1)) & 1ull);
    const bool head = valid && (!left_valid || left != key);
    const unsigned long long stops = __ballot(head) | ~valids;      // where a run ends: the next head or the first invalid lane
    if (head) {
        const unsigned long long after = lane == 63 ? 0ull : stops & ~((2ull << lane) - 1ull);
        const int end = after ? __ffsll((long long)after) - 1 : 64;
        atomicAdd(&bins[key], (uint32_t)(end - lane) * weight);
    }
}

__global__ void __launch_bounds__(256)
k_annot_hist(const uint8_t *__restrict__ image, size_t n, uint32_t *__restrict__ bins)
{
    const size_t n4 = n / 4;
    const int lane = threadIdx.x & 63;
    // (the loop condition is the same in every lane of a wave: the ballots inside see whole waves)
    for (size_t g0 = (size_t)blockIdx.x * 256 + (threadIdx.x & ~63); g0 < n4; g0 += (size_t)gridDim.x * 256) {
        const size_t g = g0 + lane;
        const bool valid = g < n4;
        uint32_t key[4] = { 0u, 0u, 0u, 0u };
        if (valid) px4_keys(*reinterpret_cast<const Px4 *>(image + 12 * g), key);
        const bool mixed = valid && !(key[0] == key[1] && key[1] == key[2] && key[2] == key[3]);
        if (__ballot(mixed) == 0) {                    // every lane's four pixels share a colour: the painted areas of an annotation
            hist_add_runs(key[0], valid, 4u, bins);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) hist_add_runs(key[j], valid, 1u, bins);
        }
    }
    if (blockIdx.x == 0 && threadIdx.x < (int)(n - 4 * n4)) atomicAdd(&bins[px_key(image + 3 * (4 * n4 + threadIdx.x))], 1u);
}

// bins in use per chunk of ANNOT_HIST_CHUNK bins, then (after the scan of the counts) their keys and counts in key order
__global__ void __launch_bounds__(256)
k_annot_hist_count(const uint32_t *__restrict__ bins, uint32_t *__restrict__ chunk_counts)
{
    __shared__ int s_wave[4];
    const size_t start = (size_t)blockIdx.x * ANNOT_HIST_CHUNK;
    int c = 0;
#pragma unroll
    for (int it = 0; it < ANNOT_HIST_CHUNK / 256; ++it) c += bins[start + (size_t)it * 256 + threadIdx.x] != 0u;
    c = wave_sum_i32(c);
    if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) chunk_counts[blockIdx.x] = (uint32_t)(s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3]);
}

__global__ void __launch_bounds__(256)
k_annot_hist_gather(const uint32_t *__restrict__ bins, const uint32_t *__restrict__ offsets, uint32_t *__restrict__ keys_out,
                    uint32_t *__restrict__ counts_out)
{
    const size_t start = (size_t)blockIdx.x * ANNOT_HIST_CHUNK;
    uint32_t base = offsets[blockIdx.x];
    if (offsets[blockIdx.x + 1] == base) return;       // (uniform over the workgroup: no bin of this chunk is in use)
    for (int it = 0; it < ANNOT_HIST_CHUNK / 256; ++it) {
        const size_t i = start + (size_t)it * 256 + threadIdx.x;
        const uint32_t count = bins[i];
        const uint32_t at = block_stable_slot(count != 0u, &base);
        if (count != 0u) {
            keys_out[at] = (uint32_t)i;
            counts_out[at] = count;
        }
    }
}

// ---------------------------------------------------------------------------------------------------
// nearest valid pixel, column pass: threads along x, down and up again.  src(y, x) = the row of the nearest pixel of column x whose
// label is not -1, the upper one when the nearest above and below are equally far, -1 when the column has none.
// ---------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64)
k_nv_columns(const int32_t *__restrict__ labels, int H, int W, int32_t *__restrict__ src, int *__restrict__ any_valid)
{
    const int x = blockIdx.x * 64 + threadIdx.x;
    int above = -1;
    if (x < W) {
        const int32_t *lx = labels + x;
        int32_t *sx = src + x;
#pragma unroll 8
        for (int y = 0; y < H; ++y) {
            above = lx[(size_t)y * W] != -1 ? y : above;
            sx[(size_t)y * W] = above;
        }
        int below = -1;
#pragma unroll 8
        for (int y = H - 1; y >= 0; --y) {
            const int up = sx[(size_t)y * W];
            below = up == y ? y : below;               // (the down sweep left y itself exactly at the valid pixels)
            if (below >= 0 && (up < 0 || below - y < y - up)) sx[(size_t)y * W] = below;
        }
    }
    if (__ballot(above >= 0) != 0 && threadIdx.x == 0) atomicOr(any_valid, 1);
}

// ---------------------------------------------------------------------------------------------------
// row pass: k_edt_rows of boundary.hip with the source row of every column in the LDS windows instead of its distance.  A candidate is
// (k^2 + (y - src)^2) << 32 | (src W + x'): the minimum of that word is the smallest squared distance and, among equals, the smallest
// row-major index.  A lane stops at the first k with k^2 ABOVE its best distance -- a pixel of this very row at k^2 == best may still
// have the smaller index.
// ---------------------------------------------------------------------------------------------------
constexpr int NV_B = 256, NV_T = 256;
constexpr unsigned long long NV_NONE = ~0ull;

__global__ void __launch_bounds__(NV_B)
k_nv_rows(const int32_t *__restrict__ labels, const int32_t *__restrict__ src, int H, int W, int32_t *__restrict__ out)
{
    __shared__ int32_t s_left[NV_T + NV_B], s_right[NV_T + NV_B];
    const int t = threadIdx.x, x0 = blockIdx.x * NV_B, x = x0 + t, y = blockIdx.y;
    const int32_t *row = src + (size_t)y * W;
    const bool inside = x < W;
    unsigned long long best = NV_NONE;
    bool done = !inside;
    auto candidate = [&](int s, int xs, uint32_t k2) {
        const uint32_t g = (uint32_t)(s > y ? s - y : y - s);
        const unsigned long long c = ((unsigned long long)(k2 + g * g) << 32) | (unsigned long long)((uint32_t)s * (uint32_t)W + (uint32_t)xs);
        best = c < best ? c : best;
    };
    if (inside) {
        const int s = row[x];
        if (s >= 0) candidate(s, x, 0u);
    }
    for (int r = 0;; ++r) {
        const int base = r * NV_T;                     // this round: k = base + 1 .. base + T
        const int left0 = x0 - base - NV_T, right0 = x0 + base;        // first pixel of either window
        const bool windows_in_row = left0 + NV_T + NV_B - 1 > 0 || right0 + 1 < W;
        if (!windows_in_row || !__syncthreads_or(!done)) break;
        for (int i = t; i < NV_T + NV_B; i += NV_B) {
            const int xl = left0 + i, xr = right0 + i;
            s_left[i] = (xl >= 0 && xl < W) ? row[xl] : -1;
            s_right[i] = (xr >= 0 && xr < W) ? row[xr] : -1;
        }
        __syncthreads();
        if (!done) {
            for (int kk = 1; kk <= NV_T; ++kk) {
                const int k = base + kk;
                const uint32_t k2 = (uint32_t)k * (uint32_t)k;
                if (k2 > (uint32_t)(best >> 32) || (k > x && x + k >= W)) {
                    done = true;
                    break;
                }
                const int sl = s_left[t + NV_T - kk], sr = s_right[t + kk];           // src(x - k), src(x + k)
                if (sl >= 0) candidate(sl, x - k, k2);
                if (sr >= 0) candidate(sr, x + k, k2);
            }
        }
        __syncthreads();                               // the next round overwrites the windows
    }
    if (inside) out[(size_t)y * W + x] = best != NV_NONE ? labels[(uint32_t)best] : -1;
}

// ---------------------------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------------------------
static int stream_grid(size_t items)
{
    // memory-bound passes: at most 2048 workgroups of 256 lanes, the rest by the grid stride
    const size_t blocks = (items + 255) / 256;
    return (int)(blocks < 1 ? 1 : (blocks > 2048 ? 2048 : blocks));
}

int launch_annot_match(const uint8_t *image, size_t n_pixels, const uint32_t *keys, const int32_t *labels, int n_colors, int mode,
                       void *out, unsigned long long *unmatched, hipStream_t st)
{
    if (n_colors < 1 || n_colors > ANNOT_MAX_COLORS) {
        set_error("annotation: a colour table holds 1 to " + std::to_string(ANNOT_MAX_COLORS) + " colours");
        return -1;
    }
    const int grid = stream_grid(n_pixels / 4);
    if (mode == 0)
        hipLaunchKernelGGL(k_annot_match<0>, grid, 256, 0, st, image, n_pixels, keys, labels, n_colors, out, unmatched);
    else if (mode == 1)
        hipLaunchKernelGGL(k_annot_match<1>, grid, 256, 0, st, image, n_pixels, keys, labels, n_colors, out, unmatched);
    else if (mode == 2)
        hipLaunchKernelGGL(k_annot_match<2>, grid, 256, 0, st, image, n_pixels, keys, labels, n_colors, out, unmatched);
    else {
        set_error("annotation: mode is 0 (exact), 1 (nearest colour, index) or 2 (nearest colour, colour)");
        return -1;
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

int launch_annot_paint(const int32_t *labels, size_t n_pixels, int min_label, int n_table, const uint32_t *keys, const uint8_t *present,
                       uint8_t *image_out, int *missing, hipStream_t st)
{
    if (n_table < 1 || n_table > ANNOT_MAX_COLORS) {
        set_error("annotation: a colour table holds 1 to " + std::to_string(ANNOT_MAX_COLORS) + " colours");
        return -1;
    }
    hipLaunchKernelGGL(k_annot_paint, stream_grid(n_pixels / 4), 256, 0, st, labels, n_pixels, min_label, n_table, keys, present, image_out,
                       missing);
    HIP_TRY(hipGetLastError());
    return 0;
}

int launch_annot_hist(const uint8_t *image, size_t n_pixels, uint32_t *bins, hipStream_t st)
{
    hipLaunchKernelGGL(k_annot_hist, stream_grid(n_pixels / 4), 256, 0, st, image, n_pixels, bins);
    HIP_TRY(hipGetLastError());
    return 0;
}

int launch_annot_hist_count(const uint32_t *bins, uint32_t *chunk_counts, hipStream_t st)
{
    hipLaunchKernelGGL(k_annot_hist_count, ANNOT_HIST_CHUNKS, 256, 0, st, bins, chunk_counts);
    launch_exclusive_scan(chunk_counts, ANNOT_HIST_CHUNKS, chunk_counts + ANNOT_HIST_CHUNKS, st);
    HIP_TRY(hipGetLastError());
    return 0;
}

int launch_annot_hist_gather(const uint32_t *bins, const uint32_t *chunk_counts, uint32_t *keys_out, uint32_t *counts_out, hipStream_t st)
{
    hipLaunchKernelGGL(k_annot_hist_gather, ANNOT_HIST_CHUNKS, 256, 0, st, bins, chunk_counts, keys_out, counts_out);
    HIP_TRY(hipGetLastError());
    return 0;
}

int launch_annot_nearest_valid(const int32_t *labels, int H, int W, int32_t *src, int32_t *out, int *any_valid, hipStream_t st)
{
    hipLaunchKernelGGL(k_nv_columns, cdiv(W, 64), 64, 0, st, labels, H, W, src, any_valid);
    hipLaunchKernelGGL(k_nv_rows, dim3(cdiv(W, NV_B), H), NV_B, 0, st, labels, src, H, W, out);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // namespace imsegm
