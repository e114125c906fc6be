// ellipse_place.hip -- fitted ellipses into a label map with the reference's overlap test (imsegm/ellipse_fitting.py
// add_overlap_ellipse :282-349, whose mask is scikit-image's draw.ellipse), and the label histogram under every ellipse
// (ellipse_place.h; C ABI in api_ellipse.hip).
//
// Arithmetic: the inside test of a pixel is one fp64 expression on integers and the sin / cos the host passes in, operation by
// operation as numpy evaluates it (the library is built with -ffp-contract=off, and the expression says so once more); everything
// else is integer counting, and the overlap ratio is one IEEE fp64 division.  Integer atomics only: same call, same bytes.
//
// The fold is sequential by definition -- whether ellipse e is painted depends on what e - 1 left -- and every step is small (a
// box of some 10^4 pixels, a table of ELLIPSE_PLACE_LABELS labels), so ONE workgroup walks the boxes in one launch: the running
// label counts and the histogram under the current ellipse stay in LDS, a workgroup barrier orders the paint of one ellipse before
// the reads of the next, and no flag crosses a launch or a compute unit.
#include "ellipse_place.h"

namespace imsegm {

namespace {

constexpr int T = ELLIPSE_PLACE_LABELS;
constexpr int PLACE_THREADS = 1024, PLACE_ROWS = PLACE_THREADS / 64;      // the fold: 64 columns x 16 rows per step
constexpr int OVER_THREADS = 256, OVER_ROWS = OVER_THREADS / 64;          // the overlaps: 64 columns x 4 rows per step,
constexpr int OVER_BAND = 32;                                             // one workgroup per band of 32 box rows

__global__ __launch_bounds__(256) void k_ellipse_label_counts(const int32_t *__restrict__ segm, size_t n_pixels,
                                                             int32_t *__restrict__ counts, int32_t *__restrict__ beyond)
{
    __shared__ int hist[T];
    for (int i = threadIdx.x; i < T; i += 256) hist[i] = 0;
    __syncthreads();
    bool over = false;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n_pixels; i += (size_t)gridDim.x * 256) {
        const int v = segm[i];
        if (v >= T)
            over = true;
        else if (v >= 1)
            atomicAdd(&hist[v], 1);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < T; i += 256)
        if (hist[i]) atomicAdd(&counts[i], hist[i]);
    if (over) atomicOr(beyond, 1);
}

__global__ __launch_bounds__(PLACE_THREADS) void k_ellipse_place(int32_t *__restrict__ segm, int width, int n,
                                                                 const int32_t *__restrict__ geom, const double *__restrict__ sincos,
                                                                 const int32_t *__restrict__ labels, double thr_overlap,
                                                                 const int32_t *__restrict__ counts, const int32_t *__restrict__ beyond,
                                                                 uint8_t *__restrict__ placed)
{
    __shared__ int hist[T];        // labels under the current ellipse
    __shared__ int count[T];       // pixels of every label in the map as it stands
    __shared__ int s_area, s_reject;
    const int tid = threadIdx.x, tx = tid & 63, ty = tid >> 6;
    if (*beyond) {                 // a value without a slot: the call reports it, the map stays as it came
        for (int e = tid; e < n; e += PLACE_THREADS) placed[e] = 0;
        return;
    }
    for (int i = tid; i < T; i += PLACE_THREADS) {
        hist[i] = 0;
        count[i] = counts[i];
    }
    if (tid == 0) s_area = 0, s_reject = 0;
    __syncthreads();
    for (int e = 0; e < n; ++e) {
        const Ellipse el = load_ellipse(geom, sincos, e);
        const int label = labels[e];
        int mine = 0;
        for (int row = el.r0 + ty; row <= el.r1; row += PLACE_ROWS)
            for (int col = el.c0 + tx; col <= el.c1; col += 64)
                if (inside_ellipse(el, row, col)) {
                    ++mine;
                    const int v = segm[(size_t)row * width + col];
                    if (v >= 1 && v < T) atomicAdd(&hist[v], 1);
                }
        mine = wave_sum_i32(mine);
        if (tx == 0 && mine) atomicAdd(&s_area, mine);
        __syncthreads();
        // the reference's loop over lb = 1 .. max(segm): only a label under the mask can reach a ratio above thr_overlap >= 0, and
        // such a label has pixels, so it is at most max(segm)
        const int area = s_area;
        if (area > 0)
            for (int lb = 1 + tid; lb < T; lb += PLACE_THREADS) {
                const int overlap = hist[lb];
                if (overlap > 0 && (double)overlap / (double)min(count[lb], area) > thr_overlap) s_reject = 1;
            }
        __syncthreads();
        const bool place = area > 0 && !s_reject;
        __syncthreads();
        if (place)
            for (int row = el.r0 + ty; row <= el.r1; row += PLACE_ROWS)
                for (int col = el.c0 + tx; col <= el.c1; col += 64)
                    if (inside_ellipse(el, row, col)) segm[(size_t)row * width + col] = label;
        for (int lb = tid; lb < T; lb += PLACE_THREADS) {
            if (place) count[lb] -= hist[lb];
            hist[lb] = 0;
        }
        if (tid == 0) {
            placed[e] = place ? 1 : 0;
            s_area = 0, s_reject = 0;
        }
        __syncthreads();           // (orders the paint before the next ellipse's reads, too)
        if (place && tid == 0 && label >= 1 && label < T) count[label] += area;
        __syncthreads();
    }
}

__global__ __launch_bounds__(OVER_THREADS) void k_ellipse_overlaps(const int32_t *__restrict__ segm, int width, int n,
                                                                  const int32_t *__restrict__ geom, const double *__restrict__ sincos,
                                                                  int nb_labels, long long *__restrict__ counts,
                                                                  long long *__restrict__ areas)
{
    __shared__ int hist[T];
    const int tid = threadIdx.x, tx = tid & 63, ty = tid >> 6;
    for (int e = blockIdx.y; e < n; e += gridDim.y) {
        const Ellipse el = load_ellipse(geom, sincos, e);
        const long long first = (long long)el.r0 + (long long)blockIdx.x * OVER_BAND;
        if (first > el.r1 || el.c1 < el.c0) continue;                 // (uniform over the workgroup)
        const int last = (int)min(first + OVER_BAND - 1, (long long)el.r1);
        for (int i = tid; i < nb_labels; i += OVER_THREADS) hist[i] = 0;
        __syncthreads();
        int mine = 0;
        for (int row = (int)first + ty; row <= last; row += OVER_ROWS)
            for (int col = el.c0 + tx; col <= el.c1; col += 64)
                if (inside_ellipse(el, row, col)) {
                    ++mine;
                    const int v = segm[(size_t)row * width + col];
                    if (v >= 0 && v < nb_labels) atomicAdd(&hist[v], 1);
                }
        mine = wave_sum_i32(mine);
        if (tx == 0 && mine) atomic_add_i64(&areas[e], mine);
        __syncthreads();
        for (int i = tid; i < nb_labels; i += OVER_THREADS)
            if (hist[i]) atomic_add_i64(&counts[(size_t)e * nb_labels + i], hist[i]);
        __syncthreads();
    }
}

}  // namespace

int launch_ellipse_label_counts(const int32_t *segm, size_t n_pixels, int32_t *counts, int32_t *beyond, hipStream_t st)
{
    const int blocks = (int)min((size_t)1024, (n_pixels + 256 * 16 - 1) / (256 * 16));
    hipLaunchKernelGGL(k_ellipse_label_counts, max(blocks, 1), 256, 0, st, segm, n_pixels, counts, beyond);
    HIP_TRY(hipGetLastError());
    return 0;
}

int launch_ellipse_place(int32_t *segm, int width, int n, const int32_t *geom, const double *sincos, const int32_t *labels,
                         double thr_overlap, const int32_t *counts, const int32_t *beyond, uint8_t *placed, hipStream_t st)
{
    hipLaunchKernelGGL(k_ellipse_place, 1, PLACE_THREADS, 0, st, segm, width, n, geom, sincos, labels, thr_overlap, counts, beyond,
                       placed);
    HIP_TRY(hipGetLastError());
    return 0;
}

int launch_ellipse_overlaps(const int32_t *segm, int width, int n, const int32_t *geom, const double *sincos, int nb_labels,
                            int max_box_rows, long long *counts, long long *areas, hipStream_t st)
{
    if (max_box_rows < 1) return 0;                                   // no ellipse has a pixel: the zeroed tables are the answer
    const dim3 grid((unsigned)cdiv(max_box_rows, OVER_BAND), (unsigned)min(n, 65535));
    hipLaunchKernelGGL(k_ellipse_overlaps, grid, OVER_THREADS, 0, st, segm, width, n, geom, sincos, nb_labels, counts, areas);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // namespace imsegm
