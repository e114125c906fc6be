// region_growing.h -- what api_region_growing.hip hands to the kernels of region_growing.hip: the resident state of one growth
// (imsegm/region_growing.py region_growing_shape_slic_greedy / _graphcut) as device pointers, and the launches.
#pragma once
#include "common.h"

namespace imsegm {

struct RgView {
    int K = 0, n_obj = 0, E = 0, H = 0, W = 0;
    const int32_t *slic = nullptr;        // H x W label map of the session
    int32_t *points = nullptr;            // K x 2: np.round(centres).astype(int)
    long long *sums = nullptr;            // K x 3: pixel count, row sum, column sum
    const int32_t *edges = nullptr;       // E x 2
    const int32_t *nb_off = nullptr;      // K + 1: CSR neighbour list of the edges ...
    const int32_t *nb = nullptr;          // ... 2 E
    double *lut_data = nullptr;           // K x (n_obj + 1)
    double *lut_shape = nullptr;          // K x (n_obj + 1)
    int32_t *labels = nullptr;            // K
    uint8_t *flags = nullptr;             // n_obj x K
    int32_t *slots = nullptr;             // n_obj x K + 1: exclusive scan of the flags, the total behind them
    int32_t *cand_obj = nullptr, *cand_sp = nullptr;   // n_obj x K
    double *cand_change = nullptr;        // n_obj x K
    double *crit = nullptr;               // 1
};

struct RgCoefs {
    double data, shape, pairwise;         // pairwise <= 0: no pairwise term at all (compute_rg_crit :1129)
    double pen_bg, pen_fg;                // -log(prob_label_trans[0 / 1]) with inf replaced by GC_REPLACE_INF
};

// per selected object of one imsegm_rg_shape_costs call
struct RgShapeJob {
    const int32_t *objects;               // n_sel: 0-based object
    const double *centres;                // n_sel x 2
    const double *shifts;                 // n_sel
    const int32_t *dims;                  // n_sel x 2: A, D
    const long long *offsets;             // n_sel: where the object's A x D table starts in `tables`
    const double *tables;
    double *proba;                        // n_sel x K or null
};

int launch_rg_points(const double *centres, int K, int32_t *points, hipStream_t st);
int launch_rg_shape_cost(const RgView &v, const RgShapeJob &job, int n_sel, hipStream_t st);
int launch_rg_object_rays(const RgView &v, const int32_t *positions, const float *directions, int A, float *out, hipStream_t st);
int launch_rg_candidates(const RgView &v, int allow_obj_swap, hipStream_t st);
int launch_rg_scores(const RgView &v, const RgCoefs &c, bool with_scores, hipStream_t st);
int launch_rg_crit(const RgView &v, const RgCoefs &c, hipStream_t st);

}  // namespace imsegm
