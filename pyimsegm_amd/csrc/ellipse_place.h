// ellipse_place.h -- launchers of csrc/ellipse_place.hip (rasterising fitted ellipses into a label map with the reference's overlap
// test, and the label histogram under every ellipse; the C ABI is in api_ellipse.hip)
#pragma once
#include "common.h"

namespace imsegm {

// Labels 0 .. ELLIPSE_PLACE_LABELS - 1 own a slot of the label tables (IMSEGM_ELLIPSE_PLACE_LABELS of include/imsegm_hip.h).  The fold
// keeps two int32 tables of that length in LDS -- the running pixel count of every label and the histogram under the current
// ellipse: 2 x 16 KiB of the 64 KiB a workgroup may take.
constexpr int ELLIPSE_PLACE_LABELS = 4096;
// what a centre coordinate or a radius may be in absolute value: row - centre stays inside int32 for every row of a map
constexpr int ELLIPSE_PLACE_MAX_COORD = 1 << 30;

// One ellipse is 8 int32 of `geom` -- centre row, centre column, row radius, column radius, first row, first column, last row, last
// column of its bounding box clipped to the map (inclusive; last < first: no pixel) -- and 2 doubles of `sincos`: sin and cos of
// its angle.  Both come from the host, so that no kernel evaluates a transcendental or a ceil.
constexpr int ELLIPSE_GEOM_INTS = 8;

// scikit-image 0.18.3's inside test of draw.ellipse for the offsets (a, b) of a pixel from the centre:
// ((a cos + b sin) / r_rad)^2 + ((a sin - b cos) / c_rad)^2 < 1, every product, sum and quotient rounded on its own, the comparison
// strict (ellipse_place.hip on integer offsets; center_annotation.hip on the offsets of draw.disk: equal radii, sin 0, cos 1)
__device__ __forceinline__ bool ellipse_inside_offsets(double a, double b, double sn, double cs, double r_rad, double c_rad)
{
#pragma clang fp contract(off)
    const double u = (a * cs + b * sn) / r_rad;
    const double v = (a * sn - b * cs) / c_rad;
    return u * u + v * v < 1.0;
}

// one ellipse as the kernels hold it (ellipse_place.hip; the ellipse masks of cut_objects.hip)
struct Ellipse {
    int r, c, r_rad, c_rad, r0, c0, r1, c1;
    double sn, cs;
};

__device__ __forceinline__ Ellipse load_ellipse(const int32_t *geom, const double *sincos, int e)
{
    const int32_t *g = geom + (size_t)e * ELLIPSE_GEOM_INTS;
    Ellipse el;
    el.r = g[0], el.c = g[1], el.r_rad = g[2], el.c_rad = g[3], el.r0 = g[4], el.c0 = g[5], el.r1 = g[6], el.c1 = g[7];
    el.sn = sincos[2 * (size_t)e], el.cs = sincos[2 * (size_t)e + 1];
    return el;
}

// the inside test above for the integer offsets of a pixel of the clipped box from the integer centre
__device__ __forceinline__ bool inside_ellipse(const Ellipse &el, int row, int col)
{
    return ellipse_inside_offsets((double)(row - el.r), (double)(col - el.c), el.sn, el.cs, (double)el.r_rad, (double)el.c_rad);
}

// Host side (api_ellipse.hip): the arguments every call that walks ellipse boxes shares -- a map (or image) `segm` of H x W below 2^31
// pixels, n >= 0 ellipses with radii >= 1, centres and radii within ELLIPSE_PLACE_MAX_COORD and boxes clipped to the map; -1 with a
// message otherwise.  *max_box_rows: the tallest clipped box (0: no ellipse has a pixel).
int check_ellipses(const char *who, const void *segm, int H, int W, int n, const int32_t *geom, const double *sincos, int *max_box_rows);

// counts[v] += number of pixels with value v for 1 <= v < ELLIPSE_PLACE_LABELS (counts zeroed by the caller); *beyond = 1 when a
// value >= ELLIPSE_PLACE_LABELS is met
int launch_ellipse_label_counts(const int32_t *segm, size_t n_pixels, int32_t *counts, int32_t *beyond, hipStream_t st);
// the fold over the n ellipses in order; does nothing (placed = 0) when *beyond is set
int launch_ellipse_place(int32_t *segm, int width, int n, const int32_t *geom, const double *sincos, const int32_t *labels,
                         double thr_overlap, const int32_t *counts, const int32_t *beyond, uint8_t *placed, hipStream_t st);
// counts[e][l] (zeroed by the caller) = pixels of value l under ellipse e for 0 <= l < nb_labels <= ELLIPSE_PLACE_LABELS,
// areas[e] (zeroed too) = pixels under ellipse e; max_box_rows: the tallest clipped box
int launch_ellipse_overlaps(const int32_t *segm, int width, int n, const int32_t *geom, const double *sincos, int nb_labels,
                            int max_box_rows, long long *counts, long long *areas, hipStream_t st);

}  // namespace imsegm
