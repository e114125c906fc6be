// colorspace.hip -- the uploaded RGB image in another colour space (hsv, luv, lab, hed, xyz), as utilities/data_io.py states the
// conversions (the skimage.color functions the reference reaches through imsegm/utilities/data_io.py:28-58), written as a float64
// interleaved H x W x 3 image -- the layout of an uploaded float64 image, so the statistic kernels read it unchanged.
//
// One elementwise kernel, templated on the type of the upload and the colour space.  A lane takes FOUR consecutive pixels: 12
// bytes of a uint8 image are three dwords, of a float32 image three 16-byte loads, of a float64 image six; the 96 bytes it
// writes are six 16-byte stores.  The pixels that do not fill a group of four (at most three) go one by one.  Traffic for a
// uint8 image: 3 B read + 24 B written per pixel.
//
// uint8 input: the transcendental of a VALUE (the sRGB linearisation of xyz / lab / luv, the log ratio of hed) comes from a
// 256-entry table every workgroup builds in LDS with the same device functions the float path evaluates per pixel (as
// slic_pre.hip does).  hsv needs no transcendental at all: with -ffp-contract=off it is numpy's result bit for bit.
#include "slic.h"

#include <algorithm>
#include <cfloat>
#include <cmath>

namespace imsegm {
namespace {

// u0, v0 of data_io.rgb2luv -- 4 * xn / (xn + 15 yn + 3 zn) and 9 * yn / (...) of the D65 white point, as numpy evaluates the
// Python expression (tests/test_colorspace_reference_host.py compares these literals with that expression)
constexpr double LUV_U0 = 0.19783982482140777;
constexpr double LUV_V0 = 0.4683363029324097;
constexpr int PX = 4;            // pixels per lane

// np.nan_to_num
__device__ __forceinline__ double finite_or_limit(double v)
{
    if (v != v) return 0.0;
    if (v > DBL_MAX) return DBL_MAX;
    if (v < -DBL_MAX) return -DBL_MAX;
    return v;
}

// data_io.rgb2xyz: one channel value to linear light
__device__ __forceinline__ double srgb_linear(double v) { return (v > 0.04045) ? det_pow24((v + 0.055) / 1.055) : v / 12.92; }

// data_io.rgb2hed: log(max(v, 1e-6)) / log(1e-6); a NaN stays one as under np.maximum
__device__ __forceinline__ double hed_ratio(double v, double log_floor) { return log(v < 1e-6 ? 1e-6 : v) / log_floor; }

__device__ __forceinline__ void hsv_px(double r, double g, double b, double &h, double &s, double &v)
{
    v = fmax(fmax(r, g), b);
    const double delta = v - fmin(fmin(r, g), b);
    s = delta / v;
    // the later assignment wins where several channels hold the maximum: blue over green over red
    double hue = (b == v) ? 4.0 + (r - g) / delta : (g == v) ? 2.0 + (b - r) / delta : (g - b) / delta;
    hue = hue / 6.0;
    // numpy's floored modulo by 1: fmod, then + 1 for a negative remainder (a tiny one rounds to 1.0) and +0 for a zero one
    double m = hue - trunc(hue);
    if (m != 0.0) {
        if (m < 0.0) m += 1.0;
    } else {
        m = 0.0;
    }
    if (delta == 0.0) {
        s = 0.0;
        m = 0.0;
    }
    h = m;
}

// rows of the matrix summed left to right (as rgb2lab_px does)
__device__ __forceinline__ void linear_to_xyz(double l0, double l1, double l2, double &X, double &Y, double &Z)
{
    X = l0 * 0.412453 + l1 * 0.357580 + l2 * 0.180423;
    Y = l0 * 0.212671 + l1 * 0.715160 + l2 * 0.072169;
    Z = l0 * 0.019334 + l1 * 0.119193 + l2 * 0.950227;
}

// the second half of rgb2lab_px (common.h), for values that come out of the table already linear
__device__ __forceinline__ void xyz_to_lab(double X, double Y, double Z, double &L, double &A, double &B)
{
    double f[3] = { X / 0.95047, Y / 1.0, Z / 1.08883 };
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double t = f[c];
        f[c] = (t > 0.008856) ? det_cbrt(t) : 7.787 * t + 16.0 / 116.0;
    }
    L = (116.0 * f[1]) - 16.0;
    A = 500.0 * (f[0] - f[1]);
    B = 200.0 * (f[1] - f[2]);
}

__device__ __forceinline__ void xyz_to_luv(double X, double Y, double Z, double &L, double &U, double &V)
{
    const double y = Y / 1.0;
    L = (y > 0.008856) ? 116.0 * det_cbrt(y) - 16.0 : 903.3 * y;
    const double denom = X + 15.0 * Y + 3.0 * Z + DBL_EPSILON;
    U = 13.0 * L * (4.0 * X / denom - LUV_U0);
    V = 13.0 * L * (9.0 * Y / denom - LUV_V0);
}

// one pixel; PRE: a0 .. a2 have been through the transcendental of their value already (table of a uint8 image)
template <int SPACE, bool PRE>
__device__ __forceinline__ void convert_px(double a0, double a1, double a2, const ColorMatrix &mat, double log_floor, double *out)
{
    double o0, o1, o2;
    if constexpr (SPACE == CS_HSV) {
        hsv_px(a0, a1, a2, o0, o1, o2);
    } else if constexpr (SPACE == CS_HED) {
        const double t0 = PRE ? a0 : hed_ratio(a0, log_floor), t1 = PRE ? a1 : hed_ratio(a1, log_floor),
                     t2 = PRE ? a2 : hed_ratio(a2, log_floor);
        o0 = t0 * mat.m[0] + t1 * mat.m[3] + t2 * mat.m[6];
        o1 = t0 * mat.m[1] + t1 * mat.m[4] + t2 * mat.m[7];
        o2 = t0 * mat.m[2] + t1 * mat.m[5] + t2 * mat.m[8];
    } else if constexpr (SPACE == CS_LAB && !PRE) {
        rgb2lab_px(a0, a1, a2, o0, o1, o2);
    } else {
        const double l0 = PRE ? a0 : srgb_linear(a0), l1 = PRE ? a1 : srgb_linear(a1), l2 = PRE ? a2 : srgb_linear(a2);
        double X, Y, Z;
        linear_to_xyz(l0, l1, l2, X, Y, Z);
        if constexpr (SPACE == CS_XYZ) {
            o0 = X;
            o1 = Y;
            o2 = Z;
        } else if constexpr (SPACE == CS_LAB) {
            xyz_to_lab(X, Y, Z, o0, o1, o2);
        } else {
            xyz_to_luv(X, Y, Z, o0, o1, o2);
        }
    }
    out[0] = finite_or_limit(o0);
    out[1] = finite_or_limit(o1);
    out[2] = finite_or_limit(o2);
}

// the twelve values of four consecutive pixels, by whole dwords / 16-byte loads
__device__ __forceinline__ void load_group(const uint8_t *p, int (&v)[3 * PX])
{
    const uint32_t *w = reinterpret_cast<const uint32_t *>(p);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const uint32_t word = w[k];
#pragma unroll
        for (int j = 0; j < 4; ++j) v[4 * k + j] = (int)((word >> (8 * j)) & 0xffu);
    }
}
__device__ __forceinline__ void load_group(const float *p, double (&v)[3 * PX])
{
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float4 q = reinterpret_cast<const float4 *>(p)[k];
        v[4 * k + 0] = (double)q.x;
        v[4 * k + 1] = (double)q.y;
        v[4 * k + 2] = (double)q.z;
        v[4 * k + 3] = (double)q.w;
    }
}
__device__ __forceinline__ void load_group(const double *p, double (&v)[3 * PX])
{
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const double2 q = reinterpret_cast<const double2 *>(p)[k];
        v[2 * k + 0] = q.x;
        v[2 * k + 1] = q.y;
    }
}

template <typename T, int SPACE>
__global__ void __launch_bounds__(256)
k_convert_color(const T *__restrict__ src, size_t n, ColorMatrix mat, double log_floor, double *__restrict__ dst)
{
    constexpr bool U8 = std::is_same<T, uint8_t>::value;
    constexpr bool TABLE = U8 && SPACE != CS_HSV;
    __shared__ double lut[TABLE ? 256 : 1];
    if constexpr (TABLE) {
        const double x = (double)threadIdx.x / 255.0;
        lut[threadIdx.x] = SPACE == CS_HED ? hed_ratio(x, log_floor) : srgb_linear(x);
        __syncthreads();
    }
    const size_t groups = n / PX, items = groups + (n - groups * PX);
    for (size_t t = (size_t)blockIdx.x * 256 + threadIdx.x; t < items; t += (size_t)gridDim.x * 256) {
        if (t < groups) {
            double in[3 * PX], out[3 * PX];
            if constexpr (U8) {
                int raw[3 * PX];
                load_group(src + t * (3 * PX), raw);
#pragma unroll
                for (int i = 0; i < 3 * PX; ++i) in[i] = TABLE ? lut[raw[i]] : (double)raw[i] / 255.0;
            } else {
                load_group(src + t * (3 * PX), in);
            }
#pragma unroll
            for (int p = 0; p < PX; ++p) convert_px<SPACE, TABLE>(in[3 * p], in[3 * p + 1], in[3 * p + 2], mat, log_floor, out + 3 * p);
            double2 *o = reinterpret_cast<double2 *>(dst + t * (3 * PX));
#pragma unroll
            for (int k = 0; k < 6; ++k) o[k] = make_double2(out[2 * k], out[2 * k + 1]);
        } else {                      // the last n % 4 pixels
            const size_t p = groups * PX + (t - groups);
            double in[3], out[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                if constexpr (U8) in[c] = TABLE ? lut[src[3 * p + c]] : (double)src[3 * p + c] / 255.0;
                else in[c] = (double)src[3 * p + c];
            }
            convert_px<SPACE, TABLE>(in[0], in[1], in[2], mat, log_floor, out);
#pragma unroll
            for (int c = 0; c < 3; ++c) dst[3 * p + c] = out[c];
        }
    }
}

template <typename T>
int launch_typed(const T *src, size_t n, int space, const ColorMatrix &mat, double *dst, hipStream_t st)
{
    const size_t items = n / PX + n % PX;
    const int grid = (int)std::min<size_t>(std::max<size_t>(cdiv((long)items, 256), 1), 4096);
    const double log_floor = std::log(1e-6);
    switch (space) {
    case CS_HSV: hipLaunchKernelGGL((k_convert_color<T, CS_HSV>), grid, 256, 0, st, src, n, mat, log_floor, dst); break;
    case CS_LUV: hipLaunchKernelGGL((k_convert_color<T, CS_LUV>), grid, 256, 0, st, src, n, mat, log_floor, dst); break;
    case CS_LAB: hipLaunchKernelGGL((k_convert_color<T, CS_LAB>), grid, 256, 0, st, src, n, mat, log_floor, dst); break;
    case CS_HED: hipLaunchKernelGGL((k_convert_color<T, CS_HED>), grid, 256, 0, st, src, n, mat, log_floor, dst); break;
    case CS_XYZ: hipLaunchKernelGGL((k_convert_color<T, CS_XYZ>), grid, 256, 0, st, src, n, mat, log_floor, dst); break;
    default: set_error("convert_color: unknown colour space"); return -1;
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // namespace

int launch_convert_color(const void *src, int dtype, size_t n, int space, const ColorMatrix &matrix, double *dst, hipStream_t st)
{
    if (dtype == DT_U8) return launch_typed(static_cast<const uint8_t *>(src), n, space, matrix, dst, st);
    if (dtype == DT_F32) return launch_typed(static_cast<const float *>(src), n, space, matrix, dst, st);
    if (dtype == DT_F64) return launch_typed(static_cast<const double *>(src), n, space, matrix, dst, st);
    set_error("convert_color: unsupported dtype");
    return -1;
}

}  // namespace imsegm
