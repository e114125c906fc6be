// object_shapes.h -- what api_object_shapes.hip hands to the kernels of object_shapes.hip: the objects of one annotated label map
// (imsegm/region_growing.py compute_object_shapes :289-331) with their moments, rounded centres of mass and raw 'down' rays.
#pragma once
#include "common.h"

namespace imsegm {

constexpr int OS_MAX_SPAN = 65536;        // IMSEGM_OBJECT_SHAPES_MAX_SPAN: entries of the presence table in the multi-label case

// the words of the header the chain keeps on the device (the host reads OS_MODE and OS_COUNT once, with the results)
enum { OS_MIN = 0, OS_MAX = 1, OS_MODE = 2, OS_COUNT = 3, OS_HDR_INTS = 16 };
// OS_MODE: at most two values with a 0 and a non-zero among them: scipy.ndimage.label | more than two values within the span | more
// than two values beyond it (nothing computed) | at most two values without a 0 or without a non-zero: no objects
enum { OS_RELABEL = 0, OS_VALUES = 1, OS_SPAN = 2, OS_NONE = 3 };

constexpr int OS_RANGE_BLOCKS = 1024;     // at most this many partial (min, max, between) triples

struct OsView {
    int H = 0, W = 0, A = 0, max_objects = 0;
    int table_len = 0;                    // max(H * W, OS_MAX_SPAN)
    const int32_t *segm = nullptr;        // H x W
    int32_t *parent = nullptr;            // H x W: the forest of the relabelled case
    int32_t *key = nullptr;               // H x W: root (relabelled) or value - min (multi-label) of an object pixel, -1 elsewhere
    int32_t *table = nullptr;             // table_len: presence of a key, then its rank among the present ones (-1: absent)
    int32_t *partial = nullptr;           // OS_RANGE_BLOCKS x 3
    int32_t *blocksum = nullptr;          // cdiv(table_len, 1024) + 1
    int32_t *hdr = nullptr;               // OS_HDR_INTS
    int32_t *obj_key = nullptr;           // max_objects
    const float *directions = nullptr;    // A x 2
    int32_t *labels = nullptr;            // max_objects
    long long *moments = nullptr;         // max_objects x 3: pixel count, row sum, column sum (zeroed by the launch)
    int32_t *centres = nullptr;           // max_objects x 2
    float *rays = nullptr;                // max_objects x A
};

int launch_object_shapes(const OsView &v, hipStream_t st);

}  // namespace imsegm
