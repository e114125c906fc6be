// forest.h -- launchers of csrc/forest.hip (predict_proba of a random forest, bit for bit; the C ABI is in api_forest.hip)
#pragma once
#include "../../include/imsegm_hip.h"
#include "common.h"

namespace imsegm {

constexpr int FOREST_ROWS = IMSEGM_FOREST_ROWS;
constexpr int FOREST_LDS_NODES = IMSEGM_FOREST_LDS_NODES;
static_assert(FOREST_ROWS % 64 == 0, "whole waves");
static_assert(FOREST_LDS_NODES * sizeof(imsegm_forest_node) <= 32768, "five workgroups of the walk share the 160 KB of a CU");

// rows of the transposed float32 table and of the leaf indices: the table's rows, padded to whole workgroups
inline size_t forest_row_stride(int n_rows) { return ((size_t)n_rows + FOREST_ROWS - 1) / FOREST_ROWS * FOREST_ROWS; }

// The device pointers of one call.  `table` is [n_rows][F] float64; z [F][stride] float32 and leaf [T][stride] int32 are scratch
// written before they are read; `flag` is one word the caller has cleared: bit 0 a non-finite value (or one that leaves float32),
// bit 1 a walk that found no leaf (a forest the host check would have refused).
struct ForestArgs {
    int n_rows, F, C, T;
    size_t stride;
    const double *table, *mean, *scale, *leaf_values;
    const imsegm_forest_node *nodes;
    const int32_t *tree_start;
    float *z;
    int32_t *leaf;
    double *proba;
    int32_t *flag;
};

// scale -> walk (one workgroup per tree and block of rows) -> ordered sum per (row, class); n_leaves bounds the rows a walk hands on
int launch_forest_proba(const ForestArgs &a, int n_leaves, hipStream_t st);

}  // namespace imsegm
