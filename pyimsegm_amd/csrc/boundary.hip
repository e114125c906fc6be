// boundary.hip -- boundary masks of label maps, the exact Euclidean distance transform of a mask's complement and the stable
// compaction of boundary points: the device side of imsegm/labeling.py contour_binary_map (:34-79), compute_distance_map
// (:146-169) and compute_boundary_distances (:684-716).
//
// Everything is integer arithmetic up to ONE fp64 square root per value:
//   mask      uint8 per pixel, three modes (thick / contour of a label / contour with the image border)
//   columns   g(y, x) = |y - y'| to the nearest set pixel (y', x) of the column, or NONE       (one thread per column, two sweeps)
//   rows      d2(y, x) = min over x' of (x - x')^2 + g(y, x')^2                               (uint32, outward search in LDS tiles)
//   value     sqrt((double)d2)
// Volumes run the two passes per slice (launch_edt_slices) and add the depth pass of boundary3d.hip.
// A uint32 converts to fp64 exactly and the fp64 sqrt of hipcc is the correctly rounded IEEE operation unless a fast-math flag
// relaxes it: pyimsegm_amd/build.py compiles every file of the library with ONE list of flags (build.FLAGS) that holds no
// -ffast-math, -Ofast, -fapprox-func or -funsafe-math-optimizations and adds -ffp-contract=off; there are no per-file flags, so
// none can reach this file (tests/test_boundary_reference_host.py checks the list).  The result therefore equals numpy's sqrt of
// the brute-force integer minimum, and scipy's distance_transform_edt (the same square root of the same integer), bit for bit.
//
// Squared distances are uint32: the caller refuses maps with H^2 + W^2 > 2^32 - 1 (launch_edt_* return an error, nothing wraps).
#include "scan.h"
#include "slic.h"

namespace imsegm {

constexpr uint32_t EDT_NONE = 0xffffffffu;      // "no set pixel in this column" / "no distance yet": above every real value

// ---------------------------------------------------------------------------------------------------
// mask: mode 0 = skimage.segmentation.find_boundaries(mode='thick') (a 4-neighbour INSIDE the image carries another label),
// 1 = labeling.py:59-66 (interior pixels that carry `label` and have a 4-neighbour that does not), 2 = the same plus every pixel
// of the image border that carries `label` (:67-77).  `any_set` (one int, zeroed by the launcher) is raised when a pixel is set.
// ---------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
k_boundary_mask(const int32_t *__restrict__ labels, int H, int W, int mode, int label, uint8_t *__restrict__ mask,
                int *__restrict__ any_set)
{
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    bool set = false;
    if (x < W && y < H) {
        const size_t i = (size_t)y * W + x;
        const int c = labels[i];
        const bool up = y > 0, down = y + 1 < H, left = x > 0, right = x + 1 < W;
        const int lu = up ? labels[i - W] : c, ld = down ? labels[i + W] : c, ll = left ? labels[i - 1] : c, lr = right ? labels[i + 1] : c;
        if (mode == 0) {
            set = lu != c || ld != c || ll != c || lr != c;
        } else {
            const bool interior = up && down && left && right;
            if (c == label) set = interior ? (lu != label || ld != label || ll != label || lr != label) : mode == 2;
        }
        mask[i] = set ? 1 : 0;
    }
    // one integer atomic per wave that has a set pixel: the word only ever goes from 0 to 1
    if (__ballot(set) != 0 && (threadIdx.x & 63) == 0) atomicOr(any_set, 1);
}

// ---------------------------------------------------------------------------------------------------
// column pass: threads along x (a wave reads and writes 64 neighbouring columns of one row), down and up again.
// A volume is a stack of slices (slice = blockIdx.y, `slice_set` = one flag per slice from k_boundary_mask3d): a slice without a
// set voxel is left alone, the row pass does not read its g.  An image is one slice and passes no flags.
// ---------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64)
k_edt_columns(const uint8_t *__restrict__ mask, int H, int W, const int *__restrict__ slice_set, uint32_t *__restrict__ g)
{
    const int x = blockIdx.x * 64 + threadIdx.x;
    if (x >= W || (slice_set && slice_set[blockIdx.y] == 0)) return;
    const size_t slice = (size_t)blockIdx.y * (size_t)H * (size_t)W;
    const uint8_t *m = mask + slice + x;
    uint32_t *gx = g + slice + x;
    uint32_t d = EDT_NONE;
#pragma unroll 8
    for (int y = 0; y < H; ++y) {
        d = m[(size_t)y * W] ? 0u : (d == EDT_NONE ? EDT_NONE : d + 1u);
        gx[(size_t)y * W] = d;
    }
    d = EDT_NONE;
#pragma unroll 8
    for (int y = H - 1; y >= 0; --y) {
        d = m[(size_t)y * W] ? 0u : (d == EDT_NONE ? EDT_NONE : d + 1u);
        if (d < gx[(size_t)y * W]) gx[(size_t)y * W] = d;
    }
}

// ---------------------------------------------------------------------------------------------------
// row pass: a workgroup owns EDT_B neighbouring pixels of one row.  Round r looks at the offsets k = r T + 1 .. (r + 1) T to the
// left and to the right; the g values those need -- T + B - 1 on either side -- are staged in LDS (pixels outside the row as NONE).
// A lane stops at the first k with k^2 >= its best value (no farther column can do better: g^2 >= 0), the workgroup when every
// lane has stopped or both windows have left the row.  Exact for any mask; the worst case (a single set pixel) is W / 2 steps
// per pixel, the usual one (superpixel boundaries) a few dozen.  No mask at all (any_set == 0): scipy's distance_transform_edt
// then answers as if ONE zero sat at row -1, column 0 (seen with scipy 1.7 to 1.15: its feature transform starts from index -1 /
// 0 and nothing overwrites it), i.e. d2 = (y + 1)^2 + x^2 -- restated here, the test compares against scipy at run time.
// In a volume (slice = blockIdx.z, `slice_set` given) a slice without a set voxel costs no search: its d2 is NONE, which the depth
// pass of boundary3d.hip never adds to; the answer for a volume without any set voxel is given there.
// ---------------------------------------------------------------------------------------------------
constexpr int EDT_B = 256, EDT_T = 256;

__global__ void __launch_bounds__(EDT_B)
k_edt_rows(const uint32_t *__restrict__ g, int H, int W, const int *__restrict__ any_set, const int *__restrict__ slice_set,
           uint32_t *__restrict__ d2_out, double *__restrict__ dist_out)
{
    __shared__ uint32_t s_left[EDT_T + EDT_B], s_right[EDT_T + EDT_B];
    const int t = threadIdx.x, x0 = blockIdx.x * EDT_B, x = x0 + t, y = blockIdx.y;
    const size_t slice = (size_t)blockIdx.z * (size_t)H * (size_t)W;
    const uint32_t *row = g + slice + (size_t)y * W;
    const bool inside = x < W;
    uint32_t best = EDT_NONE;
    bool done = !inside;
    if (slice_set) {                                   // (uniform over the slice)
        if (slice_set[blockIdx.z] == 0) {
            done = true;
        } else if (inside) {
            const uint32_t g0 = row[x];
            if (g0 != EDT_NONE) best = g0 * g0;
        }
    } else if (*any_set == 0) {                        // (uniform over the grid)
        best = (uint32_t)(y + 1) * (uint32_t)(y + 1) + (uint32_t)x * (uint32_t)x;
        done = true;
    } else if (inside) {
        const uint32_t g0 = row[x];
        if (g0 != EDT_NONE) best = g0 * g0;
    }
    for (int r = 0;; ++r) {
        const int base = r * EDT_T;                    // this round: k = base + 1 .. base + T
        const int left0 = x0 - base - EDT_T, right0 = x0 + base;       // first pixel of either window
        const bool windows_in_row = left0 + EDT_T + EDT_B - 1 > 0 || right0 + 1 < W;
        if (!windows_in_row || !__syncthreads_or(!done)) break;
        for (int i = t; i < EDT_T + EDT_B; i += EDT_B) {
            const int xl = left0 + i, xr = right0 + i;
            s_left[i] = (xl >= 0 && xl < W) ? row[xl] : EDT_NONE;
            s_right[i] = (xr >= 0 && xr < W) ? row[xr] : EDT_NONE;
        }
        __syncthreads();
        if (!done) {
            for (int kk = 1; kk <= EDT_T; ++kk) {
                const uint32_t k = (uint32_t)(base + kk), k2 = k * k;
                if (k2 >= best || ((int)k > x && x + (int)k >= W)) {
                    done = true;
                    break;
                }
                const uint32_t gl = s_left[t + EDT_T - kk], gr = s_right[t + kk];     // g(x - k), g(x + k)
                if (gl != EDT_NONE) best = min(best, k2 + gl * gl);
                if (gr != EDT_NONE) best = min(best, k2 + gr * gr);
            }
        }
        __syncthreads();                               // the next round overwrites the windows
    }
    if (inside) {
        const size_t i = slice + (size_t)y * W + x;
        if (d2_out) d2_out[i] = best;
        if (dist_out) dist_out[i] = sqrt((double)best);
    }
}

// ---------------------------------------------------------------------------------------------------
// stable compaction of the set pixels of a mask (row-major order is part of the result: a scan, no atomic append).
// A workgroup owns CP_CHUNK consecutive pixels: k_compact_count counts them, launch_exclusive_scan (scan.hip) turns the counts into
// exclusive offsets and leaves the total behind them, k_compact_gather writes (row, column) and sqrt(d2) of every set pixel to its
// place.
// ---------------------------------------------------------------------------------------------------
constexpr int CP_ITEMS = 8, CP_CHUNK = 256 * CP_ITEMS;

__global__ void __launch_bounds__(256)
k_compact_count(const uint8_t *__restrict__ mask, size_t n, uint32_t *__restrict__ counts)
{
    __shared__ int s_wave[4];
    const size_t start = (size_t)blockIdx.x * CP_CHUNK;
    int c = 0;
#pragma unroll
    for (int it = 0; it < CP_ITEMS; ++it) {
        const size_t i = start + (size_t)it * 256 + threadIdx.x;
        c += (i < n && mask[i]) ? 1 : 0;
    }
    c = wave_sum_i32(c);
    if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) counts[blockIdx.x] = (uint32_t)(s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3]);
}

__global__ void __launch_bounds__(256)
k_compact_gather(const uint8_t *__restrict__ mask, const uint32_t *__restrict__ d2, size_t n, int W, const uint32_t *__restrict__ offsets,
                 int32_t *__restrict__ points, double *__restrict__ dist)
{
    const size_t start = (size_t)blockIdx.x * CP_CHUNK;
    uint32_t base = offsets[blockIdx.x];
    for (int it = 0; it < CP_ITEMS; ++it) {
        const size_t i = start + (size_t)it * 256 + threadIdx.x;
        const bool set = i < n && mask[i];
        const uint32_t at = block_stable_slot(set, &base);
        if (set) {
            points[2 * (size_t)at] = (int32_t)(i / (size_t)W);
            points[2 * (size_t)at + 1] = (int32_t)(i % (size_t)W);
            dist[at] = sqrt((double)d2[i]);
        }
    }
}

// the same for a volume of slices of HW = H * W voxels: (slice, row, column) triples in raster order
__global__ void __launch_bounds__(256)
k_compact_gather3d(const uint8_t *__restrict__ mask, const uint32_t *__restrict__ d2, size_t n, size_t HW, int W,
                   const uint32_t *__restrict__ offsets, int32_t *__restrict__ points, double *__restrict__ dist)
{
    const size_t start = (size_t)blockIdx.x * CP_CHUNK;
    uint32_t base = offsets[blockIdx.x];
    for (int it = 0; it < CP_ITEMS; ++it) {
        const size_t i = start + (size_t)it * 256 + threadIdx.x;
        const bool set = i < n && mask[i];
        const uint32_t at = block_stable_slot(set, &base);
        if (set) {
            const size_t in_slice = i % HW;
            points[3 * (size_t)at] = (int32_t)(i / HW);
            points[3 * (size_t)at + 1] = (int32_t)(in_slice / (size_t)W);
            points[3 * (size_t)at + 2] = (int32_t)(in_slice % (size_t)W);
            dist[at] = sqrt((double)d2[i]);
        }
    }
}

// ---------------------------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------------------------
int edt_size_ok(int H, int W)
{
    if (H < 1 || W < 1) {
        set_error("boundary: height and width must be positive");
        return 0;
    }
    // uint32 squared distances: (H - 1)^2 + (W - 1)^2, and H^2 + (W - 1)^2 for a map without a set pixel, must stay below EDT_NONE
    const unsigned long long h = (unsigned long long)H, w = (unsigned long long)W;
    if (h * h + w * w > 0xffffffffull) {
        set_error("boundary: H^2 + W^2 exceeds 2^32 - 1, squared distances would not fit 32 bits");
        return 0;
    }
    return 1;
}

int launch_boundary_mask(const int32_t *labels, int H, int W, int mode, int label, uint8_t *mask, int *any_set, hipStream_t st)
{
    if (mode < 0 || mode > 2) {
        set_error("boundary: mode is 0 (thick), 1 (contour of a label) or 2 (contour with the image border)");
        return -1;
    }
    HIP_TRY(hipMemsetAsync(any_set, 0, sizeof(int), st));
    hipLaunchKernelGGL(k_boundary_mask, dim3(cdiv(W, 64), cdiv(H, 4)), 256, 0, st, labels, H, W, mode, label, mask, any_set);
    HIP_TRY(hipGetLastError());
    return 0;
}

int launch_edt(const uint8_t *mask, const int *any_set, int H, int W, uint32_t *g, uint32_t *d2_out, double *dist_out, hipStream_t st)
{
    if (!edt_size_ok(H, W)) return -1;
    if (H > 65535) {                                   // (gridDim.y of the row pass)
        set_error("boundary: more than 65535 rows");
        return -1;
    }
    hipLaunchKernelGGL(k_edt_columns, cdiv(W, 64), 64, 0, st, mask, H, W, (const int *)nullptr, g);
    hipLaunchKernelGGL(k_edt_rows, dim3(cdiv(W, EDT_B), H), EDT_B, 0, st, g, H, W, any_set, (const int *)nullptr, d2_out, dist_out);
    HIP_TRY(hipGetLastError());
    return 0;
}

int launch_edt_slices(const uint8_t *mask, const int *slice_set, int D, int H, int W, uint32_t *g, uint32_t *d2_out, hipStream_t st)
{
    hipLaunchKernelGGL(k_edt_columns, dim3(cdiv(W, 64), D), 64, 0, st, mask, H, W, slice_set, g);
    hipLaunchKernelGGL(k_edt_rows, dim3(cdiv(W, EDT_B), H, D), EDT_B, 0, st, g, H, W, (const int *)nullptr, slice_set, d2_out,
                       (double *)nullptr);
    HIP_TRY(hipGetLastError());
    return 0;
}

size_t compact_count_words(size_t n) { return (n + CP_CHUNK - 1) / CP_CHUNK + 1; }

int launch_compact_count(const uint8_t *mask, size_t n, uint32_t *counts, hipStream_t st)
{
    const int nb = (int)(compact_count_words(n) - 1);
    hipLaunchKernelGGL(k_compact_count, nb, 256, 0, st, mask, n, counts);
    launch_exclusive_scan(counts, nb, counts + nb, st);
    HIP_TRY(hipGetLastError());
    return 0;
}

int launch_compact_gather(const uint8_t *mask, const uint32_t *d2, size_t n, int W, const uint32_t *offsets, int32_t *points,
                          double *dist, hipStream_t st)
{
    const int nb = (int)(compact_count_words(n) - 1);
    hipLaunchKernelGGL(k_compact_gather, nb, 256, 0, st, mask, d2, n, W, offsets, points, dist);
    HIP_TRY(hipGetLastError());
    return 0;
}

int launch_compact_gather3d(const uint8_t *mask, const uint32_t *d2, size_t n, int H, int W, const uint32_t *offsets, int32_t *points,
                            double *dist, hipStream_t st)
{
    const int nb = (int)(compact_count_words(n) - 1);
    hipLaunchKernelGGL(k_compact_gather3d, nb, 256, 0, st, mask, d2, n, (size_t)H * (size_t)W, W, offsets, points, dist);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // namespace imsegm
