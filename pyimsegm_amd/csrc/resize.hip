// resize.hip -- the anti-aliased resize of a batch of unequally sized uint8 crops to one size, and the bytes export_image makes of
// the result: skimage.transform.resize(img, output_shape) with the defaults of scikit-image 0.18.3 as
// experiments_ovary_detect/run_ellipse_cut_scale.py :69 calls it on every cut-out of a stage, restated by
// pyimsegm_amd/ellipse_cut_scale.py resize_image_host, which these kernels equal byte for byte.
//
//   blur      scipy.ndimage.gaussian_filter on the uint8 crop itself (resize blurs before it converts): two passes, down the rows
//             and along them, with a uint8 intermediate -- after each pass the fp64 sum is cast back to uint8 by truncation.  One
//             workgroup blurs a tile of RESIZE_TILE_H x RESIZE_TILE_W pixels of one crop, the tile and its halo along the axis in
//             LDS; the grid is the sum of the tiles of all crops, found through a prefix of per-crop tile counts.  The sum is in
//             scipy's order for a symmetric kernel (ni_filters.c NI_Correlate1D): the centre product first, then
//             (x[-j] + x[+j]) * w[j] from the outermost pair inwards.  The second pass folds the smallest and largest byte of every
//             crop into two words (integer atomics).
//   gather    the bilinear lookup of _warp_fast (order 1, mode 'reflect' = mirror without repeating the edge) with the exact factors
//             H / h, W / w, in the expression and rounding order of resize_image_host, clipped to the range of the blurred crop;
//             the largest value of every image through an integer atomic on its bit pattern (the values are not negative).
//   export    (uint8)(v / max * 255): one division and one multiplication in this order.
//
// Every operation is fp64 and the file is built with -ffp-contract=off like all others: nothing is fused.  No kernel evaluates a
// transcendental: the weights come from the host, as scipy makes them.  Integer atomics only: same call, same bytes.
#include "resize.h"

namespace imsegm {

namespace {

constexpr int THREADS = 256;
constexpr size_t WEIGHT_BYTES = (RESIZE_TAPS * sizeof(double) + 15) & ~(size_t)15;

// index beyond 0 .. n - 1 mirrored without repeating the edge (-1 -> 1, n -> n - 2), as often as it takes; n = 1 reads its pixel
__device__ __forceinline__ int mirror(int i, int n)
{
    if (n == 1) return 0;
    const int period = 2 * (n - 1);
    int m = (i < 0 ? -i : i) % period;
    return m > n - 1 ? period - m : m;
}

// the crop of a tile: the last k with tile_prefix[k] <= tile (crops without tiles do not occur: every crop has a pixel)
__device__ __forceinline__ int crop_of_tile(const int *tile_prefix, int n, int tile)
{
    int lo = 0, hi = n;                               // tile_prefix[lo] <= tile < tile_prefix[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (tile_prefix[mid] <= tile)
            lo = mid;
        else
            hi = mid;
    }
    return lo;
}

template <int AXIS>
__global__ void __launch_bounds__(THREADS)
k_resize_blur(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, const ResizeCrop *__restrict__ crops,
              const int *__restrict__ tile_prefix, int n, int C, const double *__restrict__ weights, unsigned *__restrict__ range)
{
    extern __shared__ __align__(16) unsigned char s_raw[];
    double *s_w = reinterpret_cast<double *>(s_raw);
    uint8_t *s_px = s_raw + WEIGHT_BYTES;
    const int k = crop_of_tile(tile_prefix, n, blockIdx.x);
    const ResizeCrop crop = crops[k];
    const int R = crop.radius[AXIS], H = crop.h, W = crop.w;
    const int tiles_w = cdiv(W, RESIZE_TILE_W), tile = blockIdx.x - tile_prefix[k];
    const int r0 = (tile / tiles_w) * RESIZE_TILE_H, p0 = (tile % tiles_w) * RESIZE_TILE_W;
    const int rows = RESIZE_TILE_H + (AXIS == 0 ? 2 * R : 0), pixels = RESIZE_TILE_W + (AXIS == 1 ? 2 * R : 0), cols = pixels * C;
    const uint8_t *in = src + crop.offset;
    for (int j = threadIdx.x; j <= R; j += THREADS) s_w[j] = weights[((size_t)k * 2 + AXIS) * RESIZE_TAPS + j];
    for (int idx = threadIdx.x; idx < rows * cols; idx += THREADS) {
        const int lr = idx / cols, lb = idx - lr * cols, lp = lb / C, ch = lb - lp * C;
        // along the axis: the mirror; across it: rows and pixels beyond the crop are loaded from its last ones and never used
        const int sr = AXIS == 0 ? mirror(r0 + lr - R, H) : min(r0 + lr, H - 1);
        const int sp = AXIS == 1 ? mirror(p0 + lp - R, W) : min(p0 + lp, W - 1);
        s_px[idx] = in[((size_t)sr * W + sp) * C + ch];
    }
    __syncthreads();
    const int stride = AXIS == 0 ? cols : C, tile_cols = RESIZE_TILE_W * C;
    unsigned lo = 0xffu, hi = 0u;
    bool wrote = false;
    for (int e = threadIdx.x; e < RESIZE_TILE_H * tile_cols; e += THREADS) {
        const int lr = e / tile_cols, lb = e - lr * tile_cols, lp = lb / C;
        if (r0 + lr >= H || p0 + lp >= W) continue;
        const uint8_t *centre = s_px + (AXIS == 0 ? (lr + R) * cols + lb : lr * cols + lb + R * C);
        double tmp = (double)centre[0] * s_w[0];
        for (int j = R; j >= 1; --j) tmp += ((double)centre[-j * stride] + (double)centre[j * stride]) * s_w[j];
        const uint8_t byte = (uint8_t)tmp;
        dst[crop.offset + ((size_t)(r0 + lr) * W + p0) * C + lb] = byte;
        lo = min(lo, (unsigned)byte), hi = max(hi, (unsigned)byte), wrote = true;
    }
    if (range && __ballot(wrote) != 0) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            lo = min(lo, (unsigned)__shfl_xor((int)lo, off, 64));
            hi = max(hi, (unsigned)__shfl_xor((int)hi, off, 64));
        }
        if ((threadIdx.x & 63) == 0) {
            atomicMin(range + 2 * k, lo);
            atomicMax(range + 2 * k + 1, hi);
        }
    }
}

// (low neighbour, high neighbour, weight of the high one) of output index `o` of `out_n` on an axis of `in_n` pixels
__device__ __forceinline__ void lookup_axis(int in_n, int out_n, int o, bool single, int &low, int &high, double &d)
{
    const double x = single ? (double)in_n / 2.0 - 0.5 : ((double)in_n / (double)out_n) * ((double)o + 0.5) - 0.5;
    const double lo = floor(x), hi = ceil(x);
    d = x - lo;
    low = mirror((int)lo, in_n), high = mirror((int)hi, in_n);
}

__global__ void __launch_bounds__(THREADS)
k_resize_gather(const uint8_t *__restrict__ blurred, const ResizeCrop *__restrict__ crops, int C, int h, int w,
                const unsigned *__restrict__ range, double *__restrict__ out, unsigned long long *__restrict__ max_bits)
{
    const int k = blockIdx.y, o = blockIdx.x * THREADS + threadIdx.x;
    const ResizeCrop crop = crops[k];
    unsigned long long top_bits = 0ull;
    if (o < h * w) {
        const int y = o / w, x = o - y * w;
        const bool single = h == 1 && w == 1;
        int ra, rb, ca, cb;
        double dr, dc;
        lookup_axis(crop.h, h, y, single, ra, rb, dr);
        lookup_axis(crop.w, w, x, single, ca, cb, dc);
        const uint8_t *in = blurred + crop.offset;
        const double scale = 1. / 255, low = (double)range[2 * k] * scale, high = (double)range[2 * k + 1] * scale;
        const size_t at_aa = ((size_t)ra * crop.w + ca) * C, at_ab = ((size_t)ra * crop.w + cb) * C;
        const size_t at_ba = ((size_t)rb * crop.w + ca) * C, at_bb = ((size_t)rb * crop.w + cb) * C;
        double *o_px = out + (((size_t)k * h + y) * w + x) * C;
        for (int ch = 0; ch < C; ++ch) {
            const double p00 = (double)in[at_aa + ch] * scale, p01 = (double)in[at_ab + ch] * scale;
            const double p10 = (double)in[at_ba + ch] * scale, p11 = (double)in[at_bb + ch] * scale;
            double v = (1 - dr) * ((1 - dc) * p00 + dc * p01) + dr * ((1 - dc) * p10 + dc * p11);
            v = fmin(fmax(v, low), high);
            o_px[ch] = v;
            top_bits = max(top_bits, (unsigned long long)__double_as_longlong(v));
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) top_bits = max(top_bits, (unsigned long long)__shfl_xor((long long)top_bits, off, 64));
    if ((threadIdx.x & 63) == 0 && top_bits) atomicMax(max_bits + k, top_bits);
}

__global__ void __launch_bounds__(THREADS)
k_resize_export(const double *__restrict__ out, size_t per_image, const unsigned long long *__restrict__ max_bits,
                uint8_t *__restrict__ out_u8)
{
    const int k = blockIdx.y;
    const size_t i = (size_t)blockIdx.x * THREADS + threadIdx.x;
    if (i >= per_image) return;
    const double top = __longlong_as_double((long long)max_bits[k]);
    double v = out[(size_t)k * per_image + i];
    if (top > 0) v = v / top * 255;
    out_u8[(size_t)k * per_image + i] = (uint8_t)v;
}

}  // namespace

int launch_resize_blur(const uint8_t *src, uint8_t *dst, const ResizeCrop *crops, const int *tile_prefix, int total_tiles, int n, int C,
                       const double *weights, int axis, int max_radius, unsigned *range, hipStream_t st)
{
    if (n < 1 || total_tiles < 1 || C < 1 || C > 4 || max_radius < 0 || max_radius > RESIZE_MAX_RADIUS || (axis != 0 && axis != 1)) {
        set_error("resize: internal error, a blur launch outside its caps");
        return -1;
    }
    const size_t rows = RESIZE_TILE_H + (axis == 0 ? 2 * max_radius : 0), pixels = RESIZE_TILE_W + (axis == 1 ? 2 * max_radius : 0);
    const size_t lds = WEIGHT_BYTES + rows * pixels * C;
    if (axis == 0)
        hipLaunchKernelGGL(k_resize_blur<0>, total_tiles, THREADS, lds, st, src, dst, crops, tile_prefix, n, C, weights, range);
    else
        hipLaunchKernelGGL(k_resize_blur<1>, total_tiles, THREADS, lds, st, src, dst, crops, tile_prefix, n, C, weights, range);
    HIP_TRY(hipGetLastError());
    return 0;
}

int launch_resize_gather(const uint8_t *blurred, const ResizeCrop *crops, int n, int C, int h, int w, const unsigned *range, double *out,
                         unsigned long long *max_bits, hipStream_t st)
{
    if (n < 1 || n > 65535 || h < 1 || w < 1 || (size_t)h * (size_t)w > ((size_t)1 << 30)) {
        set_error("resize: internal error, a gather launch outside its grid");
        return -1;
    }
    hipLaunchKernelGGL(k_resize_gather, dim3(cdiv((long)h * w, THREADS), n), THREADS, 0, st, blurred, crops, C, h, w, range, out, max_bits);
    HIP_TRY(hipGetLastError());
    return 0;
}

int launch_resize_export(const double *out, int n, size_t per_image, const unsigned long long *max_bits, uint8_t *out_u8, hipStream_t st)
{
    if (n < 1 || n > 65535 || per_image < 1 || per_image > ((size_t)1 << 32)) {
        set_error("resize: internal error, an export launch outside its grid");
        return -1;
    }
    hipLaunchKernelGGL(k_resize_export, dim3(cdiv((long)per_image, THREADS), n), THREADS, 0, st, out, per_image, max_bits, out_u8);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // namespace imsegm
