// resize.h -- launchers of csrc/resize.hip (the anti-aliased resize of a batch of unequally sized uint8 crops to one size:
// skimage.transform.resize of scikit-image 0.18.3 as experiments_ovary_detect/run_ellipse_cut_scale.py :69 calls it, and the array half
// of export_image, imsegm/utilities/data_io.py :459-462; the C ABI is in api_resize.hip)
#pragma once
#include "common.h"

namespace imsegm {

// the largest blur radius (IMSEGM_RESIZE_MAX_RADIUS of include/imsegm_hip.h): a 16-row tile with a halo of 64 rows above and below,
// 64 pixels of 4 channels wide, takes 36 KiB of LDS
constexpr int RESIZE_MAX_RADIUS = 64;
constexpr int RESIZE_TAPS = RESIZE_MAX_RADIUS + 1;         // weights per crop and axis: distance 0 .. radius from the centre
constexpr int RESIZE_TILE_H = 16, RESIZE_TILE_W = 64;      // pixels of a crop one workgroup blurs

// one crop: where its h x w x C bytes start in the packed buffers, its size and the blur radius along the rows' and columns' axis
struct ResizeCrop {
    long long offset;
    int h, w, radius[2];
};

// one pass of scipy.ndimage.gaussian_filter on uint8 along `axis` (0: down the rows, 1: along a row) of every crop: dst byte =
// (uint8)tmp with tmp = x[0] w[0], then tmp += (x[-j] + x[+j]) w[j] for j = radius .. 1, all fp64, neighbours beyond the edge mirrored
// without repeating it.  weights: n x 2 x RESIZE_TAPS.  tile_prefix: n + 1 running sums of the tiles of the crops.  With `range`
// (n x 2 words, prepared as 0xffffffff / 0) the smallest and largest byte written per crop are folded in (integer atomics).
int launch_resize_blur(const uint8_t *src, uint8_t *dst, const ResizeCrop *crops, const int *tile_prefix, int total_tiles, int n, int C,
                       const double *weights, int axis, int max_radius, unsigned *range, hipStream_t st);
// out[((k h + y) w + x) C + ch]: the bilinear lookup in crop k (as float: byte * (1. / 255)) at r = (H / h)(y + 0.5) - 0.5,
// c = (W / w)(x + 0.5) - 0.5 (h = w = 1: the centre), clipped to the range of the crop; max_bits[k] (zeroed by the caller) = the bits
// of the largest value of image k -- the values are not negative, so their bit patterns order as they do
int launch_resize_gather(const uint8_t *blurred, const ResizeCrop *crops, int n, int C, int h, int w, const unsigned *range, double *out,
                         unsigned long long *max_bits, hipStream_t st);
// out_u8 = (uint8)(v / max * 255) where the maximum of the image is above 0, else (uint8)v
int launch_resize_export(const double *out, int n, size_t per_image, const unsigned long long *max_bits, uint8_t *out_u8, hipStream_t st);

}  // namespace imsegm
