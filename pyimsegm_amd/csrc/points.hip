// points.hip -- the centre-candidate point descriptors of the reference for BATCHES of positions (one launch each):
//   compute_label_histograms_positions   the reference's imsegm/descriptors.py:1288-1369  (label maps and probability layers)
//   compute_ray_features_positions       descriptors.py:1805-1895 (the mask `segm in border_labels`, the walk of
//                                        features_cython.pyx:244-282 and scipy.ndimage.gaussian_filter1d along the angle)
// The reference loops over the positions in Python, with one Cython call per position and per disc.
#include "raywalk.h"
#include "slic.h"

namespace imsegm {

constexpr int RING_THREADS = 256;

// index of the first disc (squared radii r2[0] < r2[1] < ...) that holds a pixel at squared distance d2; D: none
__device__ __forceinline__ int first_disc(const int *r2, int D, int d2)
{
    int ring = 0;
    while (ring < D && d2 > r2[ring]) ++ring;
    return ring;
}

// the window of the largest disc around (py, px), clipped to the map as adjust_bounding_box_crop clips a (2r+1) x (2r+1) box around
// a position inside the map: rows [y0, y0 + h), columns [x0, x0 + w)
struct Clip { int y0, x0, h, w; };
__device__ __forceinline__ Clip clip_window(int py, int px, int rmax, int H, int W)
{
    Clip c;
    c.y0 = max(py - rmax, 0);
    c.x0 = max(px - rmax, 0);
    c.h = max(min(py + rmax + 1, H) - c.y0, 0);
    c.w = max(min(px + rmax + 1, W) - c.x0, 0);
    return c;
}

// Label histograms under D concentric discs (skimage.morphology.disk(r): dy^2 + dx^2 <= r^2) around every position; the window of
// the largest disc is read ONCE, each pixel counts for the first disc that holds it, the discs are the running sums of these rings.
// A class map has a handful of labels, so an atomic per pixel would put a whole wave on the same few counters: every lane counts
// in a column of its own, cnt[bin][lane] (plain LDS read-modify-write, lanes on distinct banks), and the columns are summed at the
// end.  bin = ring * (nb_labels + 1) + label; labels outside [0, nb_labels) go to the bin nb_labels: they count for the size of the
// disc and for no label.  hist[p][d][l], size[p][d]: integers, exact, independent of order.
__global__ void __launch_bounds__(RING_THREADS)
k_ring_hist2d(const int16_t *__restrict__ segm, int H, int W, const int32_t *__restrict__ positions, int P,
              const int32_t *__restrict__ radii2, int D, int rmax, int nb_labels, unsigned int *__restrict__ hist,
              unsigned int *__restrict__ size)
{
    extern __shared__ unsigned int cnt[];                   // [K][RING_THREADS]
    __shared__ unsigned int tot[RING_MAX_BINS];
    __shared__ int r2[RING_MAX_BINS];
    const int p = blockIdx.x, tid = threadIdx.x;
    if (p >= P) return;
    const int L1 = nb_labels + 1, K = D * L1;
    for (int k = 0; k < K; ++k) cnt[k * RING_THREADS + tid] = 0;
    if (tid < D) r2[tid] = radii2[tid];
    __syncthreads();
    const int py = positions[2 * p], px = positions[2 * p + 1];
    const Clip c = clip_window(py, px, rmax, H, W);
    const int n = c.h * c.w;
    for (int i = tid; i < n; i += RING_THREADS) {
        const int r = i / c.w, y = c.y0 + r, x = c.x0 + (i - r * c.w);
        const int dy = y - py, dx = x - px;
        const int ring = first_disc(r2, D, dy * dy + dx * dx);
        if (ring >= D) continue;
        const int l = segm[(size_t)y * W + x];
        const int bin = ring * L1 + ((l >= 0 && l < nb_labels) ? l : nb_labels);
        cnt[bin * RING_THREADS + tid] += 1;
    }
    __syncthreads();
    const int lane = tid & 63, wave = tid >> 6;
    for (int k = wave; k < K; k += RING_THREADS / 64) {
        unsigned int v = 0;
        for (int q = 0; q < RING_THREADS; q += 64) v += cnt[k * RING_THREADS + q + lane];
        for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
        if (lane == 0) tot[k] = v;
    }
    __syncthreads();
    if (tid < nb_labels) {
        unsigned int run = 0;
        for (int d = 0; d < D; ++d) {
            run += tot[d * L1 + tid];
            hist[((size_t)p * D + d) * nb_labels + tid] = run;
        }
    } else if (tid == nb_labels) {
        unsigned int run = 0;
        for (int d = 0; d < D; ++d) {
            for (int b = 0; b < L1; ++b) run += tot[d * L1 + b];
            size[(size_t)p * D + d] = run;
        }
    }
}

// The same discs over probability layers (compute_label_hist_proba, descriptors.py:1498-1528): sum[p][d][c] = sum of proba[y][x][c]
// under disc d, in float64 and in a FIXED order -- every lane adds its pixels in raster order into a column of its own per ring,
// the 256 columns are folded by halves, the rings are added from the inside out.  No float atomics: two runs give the same bits.
// One workgroup per (position, layer).
__global__ void __launch_bounds__(RING_THREADS)
k_ring_hist_proba2d(const double *__restrict__ proba, int H, int W, int C, const int32_t *__restrict__ positions, int P,
                    const int32_t *__restrict__ radii2, int D, int rmax, double *__restrict__ sum, unsigned int *__restrict__ size)
{
    extern __shared__ double acc[];                          // [D][RING_THREADS], then the pixel counts [D][RING_THREADS]
    __shared__ int r2[RING_PROBA_MAX_DISCS];
    unsigned int *cnt = reinterpret_cast<unsigned int *>(acc + (size_t)D * RING_THREADS);
    const int p = blockIdx.x, ch = blockIdx.y, tid = threadIdx.x;
    if (p >= P || ch >= C) return;
    for (int d = 0; d < D; ++d) {
        acc[d * RING_THREADS + tid] = 0.0;
        cnt[d * RING_THREADS + tid] = 0;
    }
    if (tid < D) r2[tid] = radii2[tid];
    __syncthreads();
    const int py = positions[2 * p], px = positions[2 * p + 1];
    const Clip c = clip_window(py, px, rmax, H, W);
    const int n = c.h * c.w;
    for (int i = tid; i < n; i += RING_THREADS) {
        const int r = i / c.w, y = c.y0 + r, x = c.x0 + (i - r * c.w);
        const int dy = y - py, dx = x - px;
        const int ring = first_disc(r2, D, dy * dy + dx * dx);
        if (ring >= D) continue;
        acc[ring * RING_THREADS + tid] += proba[((size_t)y * W + x) * C + ch];
        cnt[ring * RING_THREADS + tid] += 1;
    }
    __syncthreads();
    for (int s = RING_THREADS / 2; s > 0; s >>= 1) {
        if (tid < s)
            for (int d = 0; d < D; ++d) {
                acc[d * RING_THREADS + tid] += acc[d * RING_THREADS + tid + s];
                cnt[d * RING_THREADS + tid] += cnt[d * RING_THREADS + tid + s];
            }
        __syncthreads();
    }
    if (tid == 0) {
        double run = 0.0;
        unsigned int pixels = 0;
        for (int d = 0; d < D; ++d) {
            run += acc[d * RING_THREADS];
            pixels += cnt[d * RING_THREADS];
            sum[((size_t)p * D + d) * C + ch] = run;
            if (ch == 0) size[(size_t)p * D + d] = pixels;
        }
    }
}

// index of scipy.ndimage's boundary mode 'reflect' (d c b a | a b c d | d c b a) for a line of A values: periodic with 2 A
__device__ __forceinline__ int reflect_index(int i, int A)
{
    const int period = 2 * A;
    int m = i % period;
    if (m < 0) m += period;
    return m < A ? m : period - 1 - m;
}

// Ray features against the mask `segm in border` (descriptors.py:1869-1871), formed here from the label table: no binary image is
// built or uploaded.  The walk is ray_walk (raywalk.h).  One wave per position; its A distances stay in LDS for the optional
// smoothing along the angle, which is scipy.ndimage.gaussian_filter1d(ray, sigma) on the float32 row: taps[j] = the normalised
// weight at distance j (from the host), boundary 'reflect', float64 sums in scipy's symmetric order (ni_filters.c NI_Correlate1D: the centre tap, then the pairs from the
// farthest to the nearest, (x[i - j] + x[i + j]) * taps[j]), stored as float32.
__global__ void __launch_bounds__(64)
k_ray_features_labels2d(const int32_t *__restrict__ segm, int H, int W, const int32_t *__restrict__ border, int n_border,
                        const int32_t *__restrict__ positions, int P, const float *__restrict__ grad, int A, int edge,
                        const double *__restrict__ taps, int radius, float *__restrict__ out)
{
    extern __shared__ float ray[];                          // [A]
    const int p = blockIdx.x;
    if (p >= P) return;
    auto masked = [&](int y, int x) -> bool {
        const int32_t l = segm[(size_t)y * W + x];
        bool hit = false;
        for (int b = 0; b < n_border; ++b) hit |= l == border[b];
        return hit;
    };
    const int py = positions[2 * p], px = positions[2 * p + 1];
    const bool inside = py >= 0 && py < H && px >= 0 && px < W;
    const bool start = inside ? masked(py, px) : false;
    const int diag = ray_walk_limit(H, W);
    for (int a = threadIdx.x; a < A; a += blockDim.x) {
        const float res = ray_walk(py, px, inside, start, grad[2 * a], grad[2 * a + 1], H, W, diag, edge, masked);
        if (taps)
            ray[a] = res;
        else
            out[(size_t)p * A + a] = res;
    }
    if (!taps) return;
    __syncthreads();
    for (int a = threadIdx.x; a < A; a += blockDim.x) {
        double t = (double)ray[a] * taps[0];
        for (int j = radius; j >= 1; --j) t += ((double)ray[reflect_index(a - j, A)] + (double)ray[reflect_index(a + j, A)]) * taps[j];
        out[(size_t)p * A + a] = (float)t;
    }
}

int launch_ring_hist2d(const int16_t *segm, int H, int W, const int32_t *positions, int P, const int32_t *radii2, int D, int rmax,
                       int nb_labels, unsigned int *hist, unsigned int *size, hipStream_t st)
{
    const size_t lds = (size_t)D * (nb_labels + 1) * RING_THREADS * sizeof(unsigned int);
    if (P > 0)
        hipLaunchKernelGGL(k_ring_hist2d, P, RING_THREADS, lds, st, segm, H, W, positions, P, radii2, D, rmax, nb_labels, hist, size);
    HIP_TRY(hipGetLastError());
    return 0;
}

int launch_ring_hist_proba2d(const double *proba, int H, int W, int C, const int32_t *positions, int P, const int32_t *radii2, int D,
                             int rmax, double *sum, unsigned int *size, hipStream_t st)
{
    const size_t lds = (size_t)D * RING_THREADS * (sizeof(double) + sizeof(unsigned int));
    if (P > 0)
        hipLaunchKernelGGL(k_ring_hist_proba2d, dim3(P, C), RING_THREADS, lds, st, proba, H, W, C, positions, P, radii2, D, rmax, sum,
                           size);
    HIP_TRY(hipGetLastError());
    return 0;
}

int launch_ray_features_labels2d(const int32_t *segm, int H, int W, const int32_t *border, int n_border, const int32_t *positions,
                                 int P, const float *grad, int A, int edge, const double *taps, int radius, float *out, hipStream_t st)
{
    const size_t lds = taps ? (size_t)A * sizeof(float) : 0;
    if (P > 0)
        hipLaunchKernelGGL(k_ray_features_labels2d, P, 64, lds, st, segm, H, W, border, n_border, positions, P, grad, A, edge, taps,
                           radius, out);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // namespace imsegm
