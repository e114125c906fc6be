// annotation.h -- launchers of csrc/annotation.hip (annotation colours <-> label maps, colour counts, the nearest-valid-pixel
// transform; the C ABI is in api_annotation.hip)
#pragma once
#include "common.h"

namespace imsegm {

// entries of a colour table (IMSEGM_ANNOT_MAX_COLORS of include/imsegm_hip.h): one packed word and one label per entry in LDS
constexpr int ANNOT_MAX_COLORS = 256;
// bins of the colour histogram: one uint32 per 24-bit colour (64 MiB of device scratch, zeroed per call)
constexpr size_t ANNOT_HIST_BINS = (size_t)1 << 24;
// bins a workgroup of the compaction owns; ANNOT_HIST_BINS / ANNOT_HIST_CHUNK chunk counts (+ 1 for the total) go through the scan
constexpr int ANNOT_HIST_CHUNK = 2048;
constexpr int ANNOT_HIST_CHUNKS = (int)(ANNOT_HIST_BINS / ANNOT_HIST_CHUNK);

// mode 0 / 1 / 2 = IMSEGM_ANNOT_MATCH_EXACT / _NEAREST / _NEAREST_COLOR; keys: n_colors packed colours r << 16 | g << 8 | b,
// labels: n_colors int32 (mode 0 only).  out: int32 per pixel (modes 0, 1) or uint8 x 3 per pixel (mode 2).  *unmatched (zeroed by
// the caller, may be null) += pixels without an entry in mode 0.
int launch_annot_match(const uint8_t *image, size_t n_pixels, const uint32_t *keys, const int32_t *labels, int n_colors, int mode,
                       void *out, unsigned long long *unmatched, hipStream_t st);
// image_out[i] = colour keys[labels[i] - min_label]; *missing (zeroed by the caller) is raised when a label lies outside
// [min_label, min_label + n_table) or its present byte is 0 (such a pixel is painted black)
int launch_annot_paint(const int32_t *labels, size_t n_pixels, int min_label, int n_table, const uint32_t *keys, const uint8_t *present,
                       uint8_t *image_out, int *missing, hipStream_t st);
// bins[key] += pixels of that colour (bins: ANNOT_HIST_BINS uint32, zeroed by the caller)
int launch_annot_hist(const uint8_t *image, size_t n_pixels, uint32_t *bins, hipStream_t st);
// chunk_counts: ANNOT_HIST_CHUNKS + 1 uint32; after the call the exclusive offsets of the chunks and, last, the number of bins in use
int launch_annot_hist_count(const uint32_t *bins, uint32_t *chunk_counts, hipStream_t st);
// the bins in use in ascending key order: keys_out / counts_out hold chunk_counts[ANNOT_HIST_CHUNKS] entries
int launch_annot_hist_gather(const uint32_t *bins, const uint32_t *chunk_counts, uint32_t *keys_out, uint32_t *counts_out, hipStream_t st);
// labels == -1: invalid.  src (H x W int32 scratch) receives the column pass; out[i] = labels[nearest valid pixel of i] (out must
// not be labels); *any_valid (zeroed by the caller) is raised when the map has a valid pixel -- without one `out` is meaningless.
// The caller has checked edt_size_ok(H, W) and H <= 65535.
int launch_annot_nearest_valid(const int32_t *labels, int H, int W, int32_t *src, int32_t *out, int *any_valid, hipStream_t st);

}  // namespace imsegm
