// cut_objects.h -- launchers of csrc/cut_objects.hip (cutting all labelled objects of an image out, centred and turned level:
// imsegm/utilities/data_io.py cut_object :1060-1128 for every label of a map at once; the C ABI is in api_cut_objects.hip)
#pragma once
#include "common.h"

namespace imsegm {

// labels of one call (IMSEGM_CUT_OBJECTS_MAX_LABELS of include/imsegm_hip.h): the ascending list lives in LDS, one word per label
constexpr int CUT_MAX_LABELS = 1024;
// exact integer sums per label: count, sum r, sum c, sum r^2, sum c^2, sum r c
constexpr int CUT_MOMENT_WORDS = 6;

// the two composed index maps of one object (section "Cut objects" of DESIGN.md): canvas (i, j) -> shifted frame
// x = ((0 + i m0) + j m1) + off per axis -> source k + s per axis; a coordinate below 0 or above n - 1 is outside, else floor(x + 0.5)
struct CutGeom {
    double s_r, s_c, m00, m01, m10, m11, off_r, off_c;
};
// the turned frame of one object and the window of it outside which the turned mask is False (half open)
struct CutFrame {
    int canvas_h, canvas_w, r0, r1, c0, c1;
};
// the crop of one object on its canvas and where its h x w x C bytes start in the packed output
struct CutCrop {
    int r0, c0, h, w;
    long long offset;
};

// moments[k * 6 ..] += the sums of the pixels equal to labels[k] (zeroed by the caller); box_min[2 k ..] / box_max[2 k ..] = the smallest
// / largest row and column of them (set to INT_MAX-like / -1 by the caller: bytes 0x7f / 0xff).  labels: n ascending values.
int launch_cut_moments(const int32_t *segm, int H, int W, const int32_t *labels, int n, unsigned long long *moments, int *box_min,
                       int *box_max, hipStream_t st);
// box_min / box_max (prepared as above) of the turned mask of every object on its canvas, evaluated inside the windows only;
// max_h x max_w: the largest window
int launch_cut_canvas_boxes(const int32_t *segm, int H, int W, const int32_t *labels, const CutGeom *geom, const CutFrame *frames, int n,
                            int max_h, int max_w, int *box_min, int *box_max, hipStream_t st);
// out[crop.offset + (y w + x) C + ch] for every crop pixel: the image through both maps, 0 outside the source; with use_mask the
// bytes of bg (ch-th byte of the word) where the turned mask is False.  max_h x max_w: the largest crop
int launch_cut_write(const uint8_t *image, const int32_t *segm, int H, int W, int C, const int32_t *labels, const CutGeom *geom,
                     const CutCrop *crops, int n, int max_h, int max_w, int use_mask, uint32_t bg, uint8_t *out, hipStream_t st);

// The same three steps for the masks of n ellipses in the geom / sincos form of ellipse_place.h, each mask on its own -- the int64
// mask add_overlap_ellipse(zeros, ell, 1) of run_ellipse_cut_scale.py :63, which is never rasterised.  max_box_rows: the tallest
// clipped box.  The crops are written with use_mask, and a canvas pixel from outside the turned frame keeps its 0: the reference's
// ndimage.rotate(cval=nan) leaves INT64_MIN in an int64 mask there, which counts as a pixel of the mask.
int launch_cut_ellipse_moments(const int32_t *ell_geom, const double *sincos, int n, int max_box_rows, unsigned long long *moments,
                               int *box_min, int *box_max, hipStream_t st);
int launch_cut_canvas_boxes_ellipses(const int32_t *ell_geom, const double *sincos, int H, int W, const CutGeom *geom, const CutFrame *frames,
                                     int n, int max_h, int max_w, int *box_min, int *box_max, hipStream_t st);
int launch_cut_write_ellipses(const uint8_t *image, const int32_t *ell_geom, const double *sincos, int H, int W, int C, const CutGeom *geom,
                              const CutCrop *crops, int n, int max_h, int max_w, uint32_t bg, uint8_t *out, hipStream_t st);

}  // namespace imsegm
