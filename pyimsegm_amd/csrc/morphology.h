// morphology.h -- what api_morphology.hip launches from morphology.hip: hole filling, disc erosion / dilation of uint8 masks and the
// rays of all centres on the two smoothed masks of imsegm/ellipse_fitting.py split_segm_background_foreground (:400-443)
#pragma once
#include "common.h"

namespace imsegm {

// the largest disc radius the tiles of k_disc_morph hold with their halo (IMSEGM_MORPH_MAX_RADIUS of include/imsegm_hip.h)
constexpr int MORPH_MAX_RADIUS = 64;

// seg_bg[p] = 1 - binary_fill_holes(segm > 0)[p] and seg_fg[p] = (segm[p] == 1): ONE labelling of the 4-connected components of the
// pixels with segm <= 0 (union-find, smallest index = root), a flag per root that a border pixel raised, one write pass.
// parent: H * W words, touches: H * W bytes of scratch.  H <= 65535 and H * W < 2^31 (morph_size_ok)
int morph_size_ok(int H, int W);
int launch_fill_holes_split(const int32_t *segm, int H, int W, int32_t *parent, uint8_t *touches, uint8_t *seg_bg, uint8_t *seg_fg,
                            hipStream_t st);
// out = erosion (dilate == 0) or dilation (dilate == 1) of the mask `in` by the disc dy^2 + dx^2 <= r^2, pixels outside the image
// not counted (1 <= r <= MORPH_MAX_RADIUS; in != out)
int launch_disc_morph(const uint8_t *in, int H, int W, int r, int dilate, uint8_t *out, hipStream_t st);
// The same erosion / dilation for all objects of a label map at once (the levels of center_annotation.hip): a pixel belongs to the
// mask of its own label only -- bit `level` of the byte in[p] for the erosion, in[p] != 0 for the dilation --, its radius is
// radius[label * MORPH_LEVEL_SLOTS + level] (at most r, the halo of the launch, 0 <= r <= MORPH_MAX_RADIUS), labels outside
// 1 .. max_label are background.  The erosion writes 0 / 1 into every byte of out; the dilation writes level + 1 where it finds a
// survivor and leaves the other bytes as they are.
constexpr int MORPH_LEVEL_SLOTS = 8;
struct MorphLabels {
    const int32_t *labels = nullptr;
    const int32_t *radius = nullptr;
    int level = 0, max_label = 0;
    const int32_t *boxes = nullptr;                    // (launch_disc_morph_boxed only)
};
int launch_disc_morph_labelled(const uint8_t *in, int H, int W, int r, int dilate, uint8_t *out, const MorphLabels &ml, hipStream_t st);
// launch_disc_morph for n_boxes planes at once: plane b = 1 .. n_boxes has the height, width and pixel offset in `in` and `out` of
// row b of `boxes` (MORPH_BOX_WORDS words per row: first row, first column, height, width, offset; row 0 is not used; a height or
// width of 0: no plane).  H, W: no plane is larger.  One launch, plane = blockIdx.z + 1.
constexpr int MORPH_BOX_WORDS = 8;
int launch_disc_morph_boxed(const uint8_t *in, int H, int W, int r, int dilate, uint8_t *out, const int32_t *boxes, int n_boxes,
                            hipStream_t st);
// rays of P positions on seg_bg with edge 'up' into rays_bg and on seg_fg with edge 'down' into rays_fg (P x A float32 each, either
// may be null), one launch
int launch_boundary_rays(const uint8_t *seg_bg, const uint8_t *seg_fg, int H, int W, const int32_t *positions, int P, const float *grad,
                         int A, float *rays_bg, float *rays_fg, hipStream_t st);

}  // namespace imsegm
