// center_annotation.h -- what api_center_annotation.hip launches from center_annotation.hip: the correction and labelling of a map
// of annotated eggs and the centre levels of all objects of a label map (experiments_ovary_centres/run_create_annotation.py of the
// reference: load_correct_segm :68-83, segm_set_center_levels :100-132, compute_eggs_center :52-65)
#pragma once
#include "common.h"
#include "morphology.h"

struct imsegm_ctx;

namespace imsegm {

// labels 1 .. CA_MAX_LABELS own a slot of the per-label tables, a level one of the MORPH_LEVEL_SLOTS bits of a code byte
// (IMSEGM_CENTER_ANNOT_MAX_LABELS / _MAX_LEVELS of include/imsegm_hip.h)
constexpr int CA_MAX_LABELS = 1024, CA_SLOTS = CA_MAX_LABELS + 1, CA_MAX_LEVELS = MORPH_LEVEL_SLOTS;

// the disc of one (label, level): scikit-image 0.18.3's draw.disk(centre, radius, shape) -- the bounding box clipped to the map
// (inclusive; last < first: no pixel), the centre as offsets from the clipped first row and column, the radius
struct CaDisc {
    double r_org, c_org, radius;
    int32_t r0, c0, r1, c1;
    int32_t pad[2];
};

// out[p] = img[p] > 0 (uint8 or int32 pixels)
int launch_ca_threshold(const void *img, int is_i32, size_t n, uint8_t *out, hipStream_t st);
// mask (0 / 1 bytes) -> kept: the 4-connected components with fewer than min_size pixels removed; labels: the 8-connected components
// of kept numbered from 1 in raster order of their first pixels, 0 elsewhere; *n_labels (device word): their number.
// parent, size: H * W words of scratch each; roots: H * W bytes; counts: compact_count_words(H * W) words.
int launch_ca_label(const uint8_t *mask, int H, int W, int min_size, int32_t *parent, int32_t *size, uint8_t *roots, uint32_t *counts,
                    uint8_t *kept, int32_t *labels, hipStream_t st);
// d2[p] = squared distance of p to the nearest pixel of another label, 0 for labels outside 1 .. max_label; a map of ONE value has
// no such pixel: *foreign (device word, zeroed here) stays 0 and d2 = (y + 1)^2 + x^2, what scipy's distance_transform_edt answers
// for a mask without a zero.  g: H * W words of scratch.  The caller has checked edt_size_ok(H, W) and H <= 65535.
int launch_ca_distances(const int32_t *labels, int H, int W, int max_label, uint32_t *g, int *foreign, uint32_t *d2, hipStream_t st);
// per label (tables of CA_SLOTS entries, zeroed by the caller): max2 = the largest d2 (skipped when d2 is null), sums = pixel count,
// row sum, column sum (3 words per label); one set of atomics per run of equal labels
int launch_ca_reduce(const int32_t *labels, const uint32_t *d2, int H, int W, int max_label, uint32_t *max2,
                     unsigned long long *sums, hipStream_t st);
// code[p]: bit i set when sqrt(d2) / sqrt(max2[label]) > levels[i] in fp64; counts[label * CA_MAX_LEVELS + i] (zeroed by the
// caller) = the number of such pixels
int launch_ca_code(const int32_t *labels, const uint32_t *d2, int H, int W, int max_label, const uint32_t *max2, const double *levels,
                   int n_levels, uint8_t *code, uint32_t *counts, hipStream_t st);
// bit i >= 1 of code[p] cleared outside discs[label * CA_MAX_LEVELS + i]; out[p] = bit 0 of code[p] (level 1 of the result)
int launch_ca_discs(const int32_t *labels, int H, int W, int max_label, const CaDisc *discs, int n_levels, uint8_t *code, uint8_t *out,
                    hipStream_t st);

// (api_center_annotation.hip, for imsegm_debug_center_distances) the front of imsegm_center_levels' chain -- the function that chain
// calls, up to its code pass -- on a host label map: d2 [H * W], max2 [max_label + 1] and count, row sum, column sum
// [3 (max_label + 1)] come to the host.  IMSEGM_E_OBJECT_CAPS for a map outside the size caps.
int ca_debug_distances(imsegm_ctx *ctx, const int32_t *labels, int H, int W, int max_label, uint32_t *d2_out, uint32_t *max2_out,
                       int64_t *sums_out);

}  // namespace imsegm
