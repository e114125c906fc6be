// cut_objects.hip -- cutting every labelled object of an image out, centred and turned level: the device side of
// imsegm/utilities/data_io.py cut_object (:1060-1128) for all labels of one map at once.
//
//   moments   one pass over the label map.  The lanes of a wave hold 64 consecutive pixels of a row; a lane whose label differs from
//             its left neighbour's opens a run, looks the label up in the ascending list in LDS (binary search) and adds the run's
//             exact sums -- count, sum r, sum c, sum r^2, sum c^2, sum r c in closed form, int64 -- and its ends to the label's words:
//             one set of atomics per run, as the colour counts of annotation.hip.
//   boxes     the turned mask of every object inside its window of the canvas; the bounding box is reduced per wave, then one
//             atomic min / max per wave and bound.
//   write     every crop pixel through the two composed index maps; C bytes per pixel, lanes along crop rows.
//
// The mask of an object is a functor: LabelMask (segm == label, imsegm_cut_objects) or EllipseMask (the pixels of one ellipse inside
// its clipped box by the inside test of ellipse_place.h, imsegm_ellipse_cut_scale -- no mask is rasterised or uploaded, and ellipses
// may overlap one another).  The moments of the ellipse masks are summed pixel by pixel inside the boxes, per wave, with the same
// integer atomics.
//
// Both index maps are scipy's order-0 lookups in mode 'constant' (ndimage.shift, ndimage.rotate -> affine_transform): a coordinate
// below 0 or above n - 1 is outside the source, otherwise the index is floor(x + 0.5).  The rotation coordinate is
// ((0 + i m0) + j m1) + offset, three fp64 operations in scipy's order; the file is built with -ffp-contract=off like all others, so
// none of them is fused.  No kernel evaluates a transcendental: cosine and sine arrive in the matrix.
#include "cut_objects.h"
#include "ellipse_place.h"

namespace imsegm {

__device__ __forceinline__ int cut_find_label(const int32_t *s_lab, int n, int32_t v)
{
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (s_lab[mid] < v)
            lo = mid + 1;
        else
            hi = mid;
    }
    return (lo < n && s_lab[lo] == v) ? lo : -1;
}

__device__ __forceinline__ void cut_add(unsigned long long *p, long long v) { atomicAdd(p, (unsigned long long)v); }

// ---------------------------------------------------------------------------------------------------
// moments: a workgroup owns 256 consecutive pixels of one row, a wave 64 of them
// ---------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
k_cut_moments(const int32_t *__restrict__ segm, int H, int W, int chunks, const int32_t *__restrict__ labels, int n,
              unsigned long long *__restrict__ moments, int *__restrict__ box_min, int *__restrict__ box_max)
{
    __shared__ int32_t s_lab[CUT_MAX_LABELS];
    for (int k = threadIdx.x; k < n; k += 256) s_lab[k] = labels[k];
    __syncthreads();
    const int y = blockIdx.x / chunks, x = (blockIdx.x % chunks) * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const bool valid = x < W;                         // (the valid lanes of a wave are its first ones)
    const int32_t v = valid ? segm[(size_t)y * W + x] : 0;
    const int32_t left = __shfl_up(v, 1, 64);
    const bool head = valid && (lane == 0 || left != v);
    const unsigned long long stops = __ballot(head) | ~__ballot(valid);      // where a run ends: the next head or the first invalid lane
    if (!head) return;
    const int k = cut_find_label(s_lab, n, v);
    if (k < 0) return;
    const unsigned long long after = lane == 63 ? 0ull : stops & ~((2ull << lane) - 1ull);
    const int end = after ? __ffsll((long long)after) - 1 : 64;
    const long long L = end - lane, r = y, c0 = x;
    const long long sc = L * c0 + L * (L - 1) / 2;
    const long long scc = L * c0 * c0 + c0 * L * (L - 1) + (L - 1) * L * (2 * L - 1) / 6;
    unsigned long long *m = moments + (size_t)k * CUT_MOMENT_WORDS;
    cut_add(m + 0, L);
    cut_add(m + 1, r * L);
    cut_add(m + 2, sc);
    cut_add(m + 3, r * r * L);
    cut_add(m + 4, scc);
    cut_add(m + 5, r * sc);
    atomicMin(box_min + 2 * k, y);
    atomicMax(box_max + 2 * k, y);
    atomicMin(box_min + 2 * k + 1, x);
    atomicMax(box_max + 2 * k + 1, x + (int)L - 1);
}

// ---------------------------------------------------------------------------------------------------
// the two kinds of masks
// ---------------------------------------------------------------------------------------------------
struct LabelMask {
    const int32_t *segm, *labels;
    int W;
    typedef int32_t Object;
    __device__ __forceinline__ Object object(int k) const { return labels[k]; }
    __device__ __forceinline__ bool holds(const Object &label, int sr, int sc) const { return segm[(size_t)sr * W + sc] == label; }
};
struct EllipseMask {
    const int32_t *geom;
    const double *sincos;
    typedef Ellipse Object;
    __device__ __forceinline__ Object object(int k) const { return load_ellipse(geom, sincos, k); }
    __device__ __forceinline__ bool holds(const Object &el, int sr, int sc) const
    {
        return sr >= el.r0 && sr <= el.r1 && sc >= el.c0 && sc <= el.c1 && inside_ellipse(el, sr, sc);
    }
};

__device__ __forceinline__ int wave_min_i32(int v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = min(v, __shfl_xor(v, off, 64));
    return v;
}
__device__ __forceinline__ int wave_max_i32(int v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = max(v, __shfl_xor(v, off, 64));
    return v;
}

// ---------------------------------------------------------------------------------------------------
// moments of ellipse masks: a workgroup owns a band of CUT_ELL_BAND rows of one clipped box, 64 columns x 4 rows per step
// ---------------------------------------------------------------------------------------------------
constexpr int CUT_ELL_BAND = 32;

__global__ void __launch_bounds__(256)
k_cut_ellipse_moments(const int32_t *__restrict__ geom, const double *__restrict__ sincos, unsigned long long *__restrict__ moments,
                      int *__restrict__ box_min, int *__restrict__ box_max)
{
    const int k = blockIdx.y, tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const Ellipse el = load_ellipse(geom, sincos, k);
    const long long first = (long long)el.r0 + (long long)blockIdx.x * CUT_ELL_BAND;
    if (first > el.r1 || el.c1 < el.c0) return;       // (uniform over the workgroup)
    const int last = (int)min(first + CUT_ELL_BAND - 1, (long long)el.r1);
    long long cnt = 0, s_r = 0, s_c = 0, s_rr = 0, s_cc = 0, s_rc = 0;
    int lo_r = 0x7fffffff, hi_r = -1, lo_c = 0x7fffffff, hi_c = -1;
    for (int row = (int)first + ty; row <= last; row += 4)
        for (int col = el.c0 + tx; col <= el.c1; col += 64)
            if (inside_ellipse(el, row, col)) {
                const long long r = row, c = col;
                ++cnt, s_r += r, s_c += c, s_rr += r * r, s_cc += c * c, s_rc += r * c;
                lo_r = min(lo_r, row), hi_r = max(hi_r, row), lo_c = min(lo_c, col), hi_c = max(hi_c, col);
            }
    if (__ballot(cnt > 0) == 0) return;               // (uniform over the wave)
    cnt = wave_sum_i64(cnt), s_r = wave_sum_i64(s_r), s_c = wave_sum_i64(s_c);
    s_rr = wave_sum_i64(s_rr), s_cc = wave_sum_i64(s_cc), s_rc = wave_sum_i64(s_rc);
    lo_r = wave_min_i32(lo_r), hi_r = wave_max_i32(hi_r), lo_c = wave_min_i32(lo_c), hi_c = wave_max_i32(hi_c);
    if (tx == 0) {
        unsigned long long *m = moments + (size_t)k * CUT_MOMENT_WORDS;
        cut_add(m + 0, cnt);
        cut_add(m + 1, s_r);
        cut_add(m + 2, s_c);
        cut_add(m + 3, s_rr);
        cut_add(m + 4, s_cc);
        cut_add(m + 5, s_rc);
        atomicMin(box_min + 2 * k, lo_r);
        atomicMax(box_max + 2 * k, hi_r);
        atomicMin(box_min + 2 * k + 1, lo_c);
        atomicMax(box_max + 2 * k + 1, hi_c);
    }
}

// ---------------------------------------------------------------------------------------------------
// canvas pixel (i, j) of an object -> its source pixel; CUT_INSIDE, or outside the source at one of the two steps
// ---------------------------------------------------------------------------------------------------
enum { CUT_INSIDE = 0, CUT_OUTSIDE_TURN = 1, CUT_OUTSIDE_SHIFT = 2 };

__device__ __forceinline__ int cut_source_step(const CutGeom &g, int H, int W, int i, int j, int &sr, int &sc)
{
    const double di = (double)i, dj = (double)j, top_r = (double)(H - 1), top_c = (double)(W - 1);
    const double cr = ((0.0 + di * g.m00) + dj * g.m01) + g.off_r;
    const double cc = ((0.0 + di * g.m10) + dj * g.m11) + g.off_c;
    if (!(cr >= 0.0 && cr <= top_r && cc >= 0.0 && cc <= top_c)) return CUT_OUTSIDE_TURN;    // outside the shifted frame (and NaN)
    const double xr = floor(cr + 0.5) + g.s_r, xc = floor(cc + 0.5) + g.s_c;
    if (!(xr >= 0.0 && xr <= top_r && xc >= 0.0 && xc <= top_c)) return CUT_OUTSIDE_SHIFT;   // shifted in from outside the source
    sr = (int)floor(xr + 0.5);                        // in [0, H - 1]: xr <= H - 1
    sc = (int)floor(xc + 0.5);
    return CUT_INSIDE;
}

__device__ __forceinline__ bool cut_source(const CutGeom &g, int H, int W, int i, int j, int &sr, int &sc)
{
    return cut_source_step(g, H, W, i, j, sr, sc) == CUT_INSIDE;
}

constexpr int CUT_TILE_W = 64, CUT_TILE_H = 16;       // a workgroup of 64 x 4 lanes walks 4 rows down

template <typename Mask>
__global__ void __launch_bounds__(256)
k_cut_canvas_boxes(const Mask mask, int H, int W, const CutGeom *__restrict__ geom, const CutFrame *__restrict__ frames,
                   int *__restrict__ box_min, int *__restrict__ box_max)
{
    const int k = blockIdx.z;
    const CutFrame f = frames[k];
    const int j = f.c0 + blockIdx.x * CUT_TILE_W + (threadIdx.x & 63);
    const int i0 = f.r0 + blockIdx.y * CUT_TILE_H + (threadIdx.x >> 6);
    if (f.c0 + (int)blockIdx.x * CUT_TILE_W >= f.c1 || f.r0 + (int)blockIdx.y * CUT_TILE_H >= f.r1) return;   // (uniform over the workgroup)
    const CutGeom g = geom[k];
    const typename Mask::Object object = mask.object(k);
    int lo_i = 0x7fffffff, hi_i = -1, lo_j = 0x7fffffff, hi_j = -1;
    if (j < f.c1) {
#pragma unroll
        for (int step = 0; step < CUT_TILE_H / 4; ++step) {
            const int i = i0 + 4 * step;
            int sr, sc;
            if (i < f.r1 && cut_source(g, H, W, i, j, sr, sc) && mask.holds(object, sr, sc)) {
                lo_i = min(lo_i, i);
                hi_i = max(hi_i, i);
                lo_j = j;
                hi_j = j;
            }
        }
    }
    if (__ballot(hi_i >= 0) == 0) return;             // (uniform over the wave)
    lo_i = wave_min_i32(lo_i);
    hi_i = wave_max_i32(hi_i);
    lo_j = wave_min_i32(lo_j);
    hi_j = wave_max_i32(hi_j);
    if ((threadIdx.x & 63) == 0) {
        atomicMin(box_min + 2 * k, lo_i);
        atomicMax(box_max + 2 * k, hi_i);
        atomicMin(box_min + 2 * k + 1, lo_j);
        atomicMax(box_max + 2 * k + 1, hi_j);
    }
}

// turn_outside_holds: a canvas pixel from outside the turned frame counts as a pixel of the mask -- what the reference makes of an
// int64 mask, whose ndimage.rotate(cval=nan) stores INT64_MIN there (imsegm_ellipse_cut_scale; 0 for boolean masks)
template <int C, typename Mask>
__global__ void __launch_bounds__(256)
k_cut_write(const uint8_t *__restrict__ image, const Mask mask, int H, int W, const CutGeom *__restrict__ geom,
            const CutCrop *__restrict__ crops, int use_mask, int turn_outside_holds, uint32_t bg, uint8_t *__restrict__ out)
{
    const int k = blockIdx.z;
    const CutCrop crop = crops[k];
    const int x = blockIdx.x * CUT_TILE_W + (threadIdx.x & 63);
    const int y0 = blockIdx.y * CUT_TILE_H + (threadIdx.x >> 6);
    if ((int)blockIdx.x * CUT_TILE_W >= crop.w || (int)blockIdx.y * CUT_TILE_H >= crop.h || x >= crop.w) return;
    const CutGeom g = geom[k];
    const typename Mask::Object object = mask.object(k);
#pragma unroll
    for (int step = 0; step < CUT_TILE_H / 4; ++step) {
        const int y = y0 + 4 * step;
        if (y >= crop.h) break;
        int sr, sc;
        const int where = cut_source_step(g, H, W, crop.r0 + y, crop.c0 + x, sr, sc);
        const bool inside = where == CUT_INSIDE;
        const size_t src = inside ? (size_t)sr * W + sc : 0;
        const bool keep = !use_mask || (inside && mask.holds(object, sr, sc)) || (turn_outside_holds && where == CUT_OUTSIDE_TURN);
        uint8_t *o = out + crop.offset + ((size_t)y * crop.w + x) * C;
#pragma unroll
        for (int ch = 0; ch < C; ++ch) {
            const uint8_t value = inside ? image[src * C + ch] : (uint8_t)0;     // 0: what both scipy steps leave outside in a uint8 image
            o[ch] = keep ? value : (uint8_t)(bg >> (8 * ch));
        }
    }
}

// ---------------------------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------------------------
int launch_cut_moments(const int32_t *segm, int H, int W, const int32_t *labels, int n, unsigned long long *moments, int *box_min,
                       int *box_max, hipStream_t st)
{
    if (n < 1 || n > CUT_MAX_LABELS) {
        set_error("cut_objects: 1 to " + std::to_string(CUT_MAX_LABELS) + " labels");
        return -1;
    }
    const int chunks = cdiv(W, 256);
    if ((size_t)chunks * (size_t)H > 0x7fffffffull) {
        set_error("cut_objects: the map is too large for one launch");
        return -1;
    }
    hipLaunchKernelGGL(k_cut_moments, chunks * H, 256, 0, st, segm, H, W, chunks, labels, n, moments, box_min, box_max);
    HIP_TRY(hipGetLastError());
    return 0;
}

static int cut_grid_ok(int n, int max_h, int max_w)
{
    if (n < 1 || n > CUT_MAX_LABELS || max_h < 1 || max_w < 1 || cdiv(max_h, CUT_TILE_H) > 65535) {
        set_error("cut_objects: internal error, a launch outside its grid");
        return 0;
    }
    return 1;
}

int launch_cut_canvas_boxes(const int32_t *segm, int H, int W, const int32_t *labels, const CutGeom *geom, const CutFrame *frames, int n,
                            int max_h, int max_w, int *box_min, int *box_max, hipStream_t st)
{
    if (!cut_grid_ok(n, max_h, max_w)) return -1;
    const LabelMask mask = { segm, labels, W };
    hipLaunchKernelGGL(k_cut_canvas_boxes<LabelMask>, dim3(cdiv(max_w, CUT_TILE_W), cdiv(max_h, CUT_TILE_H), n), 256, 0, st, mask, H, W, geom,
                       frames, box_min, box_max);
    HIP_TRY(hipGetLastError());
    return 0;
}

int launch_cut_ellipse_moments(const int32_t *ell_geom, const double *sincos, int n, int max_box_rows, unsigned long long *moments,
                               int *box_min, int *box_max, hipStream_t st)
{
    if (n < 1 || n > CUT_MAX_LABELS) {
        set_error("ellipse_cut_scale: 1 to " + std::to_string(CUT_MAX_LABELS) + " ellipses");
        return -1;
    }
    if (max_box_rows < 1) return 0;                   // no ellipse has a pixel: the prepared words are the answer
    hipLaunchKernelGGL(k_cut_ellipse_moments, dim3(cdiv(max_box_rows, CUT_ELL_BAND), n), 256, 0, st, ell_geom, sincos, moments, box_min,
                       box_max);
    HIP_TRY(hipGetLastError());
    return 0;
}

int launch_cut_canvas_boxes_ellipses(const int32_t *ell_geom, const double *sincos, int H, int W, const CutGeom *geom, const CutFrame *frames,
                                     int n, int max_h, int max_w, int *box_min, int *box_max, hipStream_t st)
{
    if (!cut_grid_ok(n, max_h, max_w)) return -1;
    const EllipseMask mask = { ell_geom, sincos };
    hipLaunchKernelGGL(k_cut_canvas_boxes<EllipseMask>, dim3(cdiv(max_w, CUT_TILE_W), cdiv(max_h, CUT_TILE_H), n), 256, 0, st, mask, H, W,
                       geom, frames, box_min, box_max);
    HIP_TRY(hipGetLastError());
    return 0;
}

template <typename Mask>
static int cut_write(const uint8_t *image, const Mask &mask, int H, int W, int C, const CutGeom *geom, const CutCrop *crops, int n, int max_h,
                     int max_w, int use_mask, int turn_outside_holds, uint32_t bg, uint8_t *out, hipStream_t st)
{
    if (!cut_grid_ok(n, max_h, max_w)) return -1;
    const dim3 grid(cdiv(max_w, CUT_TILE_W), cdiv(max_h, CUT_TILE_H), n);
#define CUT_WRITE(CH) \
    hipLaunchKernelGGL((k_cut_write<CH, Mask>), grid, 256, 0, st, image, mask, H, W, geom, crops, use_mask, turn_outside_holds, bg, out)
    if (C == 1)
        CUT_WRITE(1);
    else if (C == 2)
        CUT_WRITE(2);
    else if (C == 3)
        CUT_WRITE(3);
    else if (C == 4)
        CUT_WRITE(4);
    else {
        set_error("cut_objects: 1 to 4 channels");
        return -1;
    }
#undef CUT_WRITE
    HIP_TRY(hipGetLastError());
    return 0;
}

int launch_cut_write(const uint8_t *image, const int32_t *segm, int H, int W, int C, const int32_t *labels, const CutGeom *geom,
                     const CutCrop *crops, int n, int max_h, int max_w, int use_mask, uint32_t bg, uint8_t *out, hipStream_t st)
{
    const LabelMask mask = { segm, labels, W };
    return cut_write(image, mask, H, W, C, geom, crops, n, max_h, max_w, use_mask, 0, bg, out, st);
}

int launch_cut_write_ellipses(const uint8_t *image, const int32_t *ell_geom, const double *sincos, int H, int W, int C, const CutGeom *geom,
                              const CutCrop *crops, int n, int max_h, int max_w, uint32_t bg, uint8_t *out, hipStream_t st)
{
    const EllipseMask mask = { ell_geom, sincos };
    return cut_write(image, mask, H, W, C, geom, crops, n, max_h, max_w, 1, 1, bg, out, st);
}

}  // namespace imsegm
