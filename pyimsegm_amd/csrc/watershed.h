// watershed.h -- what api_watershed.hip launches from watershed.hip: the marker flood and the glue of the per-label clean-up of
// experiments_ovary_detect/run_ovary_egg-segmentation.py segment_watershed (:239-275 of the reference).  Hole filling, squared
// distances, component labels and disc erosion / dilation are the kernels of morphology.hip, boundary.hip and center_annotation.hip.
#pragma once
#include "common.h"

namespace imsegm {

// labels 1 .. WS_MAX_LABELS (IMSEGM_WATERSHED_MAX_LABELS of include/imsegm_hip.h).  A word of the flood's state map holds 0 outside
// the mask, WS_FREE for an unlabelled mask pixel, a label, or WS_CLAIM + label for a pixel claimed in the running round.
constexpr int WS_MAX_LABELS = 1024, WS_CLAIM = 1 << 20, WS_FREE = 0x7fffffff;
constexpr int WS_THREADS = 1024, WS_BLOCKS = 256;

// mask[p] = !background[p]; *any_background (one device int, zeroed here) raised when a pixel is background: the `any_set` of launch_edt
int launch_ws_mask(const uint8_t *background, size_t n, uint8_t *mask, int *any_background, hipStream_t st);
// keys[p] = -(int32) d2[p] in place (the caller has checked height^2 + width^2 < 2^31)
int launch_ws_negate(uint32_t *d2, size_t n, hipStream_t st);
// The flood of DESIGN.md section 4 "Watershed".  comp: the component number of every mask pixel (1 .. *n_comp, 0 outside; any
// partition into unions of 4-connected components), keys: int32 per pixel, seeds: n_seeds (pixel, label) pairs with distinct
// pixels and labels 1 .. WS_MAX_LABELS (a seed outside the mask is dropped).  state: n words, out: n words (may alias state),
// count, base, fill: n + 1 words each, arena: 2 n words, top: one word.
int launch_ws_flood(const int32_t *comp, const uint32_t *n_comp, const int32_t *keys, int H, int W, const int32_t *seed_pixels,
                    const int32_t *seed_labels, int n_seeds, int32_t *state, uint32_t *count, uint32_t *base, uint32_t *fill,
                    uint32_t *arena, uint32_t *top, int32_t *out, hipStream_t st);

// per label 1 .. max_label the bounding box (boxes[4 l .. 4 l + 3] = first row, first column, last row, last column; an absent label
// keeps first > last); *beyond (one device int, zeroed here) raised when a value above max_label is present
int launch_ws_boxes(const int32_t *segm, int H, int W, int max_label, int32_t *boxes, int *beyond, hipStream_t st);
// The clean-up works on one plane per label, all labels in one launch per stage (label = blockIdx.z + 1).  launch_ws_box_plan: the
// plane of label l is its box padded by `pad` and cut at the image; row l of `table` (MORPH_BOX_WORDS words, morphology.h) holds its
// first row, first column, height, width and its pixel offset in the plane buffers.  When the planes together exceed `capacity`
// pixels *overflow (one device int, zeroed here) is raised and every plane is empty.
int launch_ws_box_plan(const int32_t *boxes, int H, int W, int max_label, int pad, size_t capacity, int32_t *table, int *overflow,
                       hipStream_t st);
// planes[offset_l + y * bw + x] = segm[r0 + y][c0 + x] == l
int launch_ws_extract(const int32_t *segm, int H, int W, const int32_t *table, int max_label, uint8_t *planes, hipStream_t st);
// binary_fill_holes inside every plane, in place: the union-find of unionfind.h on the clear pixels of the plane (parent: one word
// per plane pixel), a flag per root that the plane's border reaches (touches: one byte per plane pixel)
int launch_ws_fill_holes(uint8_t *planes, int H, int W, const int32_t *table, int max_label, int32_t *parent, uint8_t *touches,
                         hipStream_t st);
// clean[r0 + y][c0 + x] = the largest label whose plane is set there (clean zeroed by the caller): ascending paint order
int launch_ws_paint(const uint8_t *planes, int H, int W, const int32_t *table, int max_label, int32_t *clean, hipStream_t st);
// wide[p] = plane[p] != 0 (int32: what launch_fill_holes_split reads)
int launch_ws_widen(const uint8_t *plane, size_t n, int32_t *wide, hipStream_t st);
// plane[p] = !background[p]
int launch_ws_invert(const uint8_t *background, size_t n, uint8_t *plane, hipStream_t st);

}  // namespace imsegm
