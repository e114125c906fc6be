// backhalf.h -- the fused back half of the colour pipeline behind a label map, set up ONCE for a single session (api_fused.hip)
// and for the images of a batch (batch.hip): the parameter block the host sends, the scratch of the terms and the cut, the chain
// class model -> unary / edge terms -> integer energies -> alpha-expansion -> label look-up table -> gathers, and what its
// status words mean.  The kernels take a ZBatch that defaults to "one image": the callers differ in the pointers they hand over.
#pragma once
#include "session.h"

namespace imsegm {

inline size_t al64(size_t v) { return (v + 63) & ~(size_t)63; }

// ---- argument checks shared by imsegm_cut_general_graph, the fused segment call and the batch (each sets the error text)
int check_pairwise(const double *pairwise, int C);
int decode_edge_type(int edge_type, int *edge_code, int *spatial_norm);

// ---- host -> device parameter block of one image (offsets; all members size_t: the struct is part of a memcmp key)
struct ParamBlock {
    size_t o_misc;      // K | E | status | gc status | energy (8) ... scalars[8] at +64: initialised by the same copy
    size_t o_pw, o_sm, o_cl, o_sc, o_pc, o_mp, o_ld, o_lw, o_pr, o_ct, o_ps, bytes;
};
// F: dimension of the mixture; proba_rows: K when probabilities (at o_pr) are uploaded instead of a mixture, else 0;
// n_inputs: columns the PCA in front of the mixture reads (scaler vectors of that length, components_.T at o_ct, shift | scale at
// o_ps), 0 without one
ParamBlock param_block(int C, int F, int proba_rows, int n_inputs = 0);

// ---- device scratch of the terms and the cut behind the parameter block (offsets from the block's base, 64-byte aligned)
struct TermsScratch {
    size_t d_proba, d_unary, d_unary_i, d_w, d_wi, d_edist, d_elen, d_gl, d_lut, d_fstd, d_work, d_red, end;
};
// F: columns of the feature table; proba_in_params: d_proba is P.o_pr; reduced_cols: columns of the projected rows (d_red), 0
// without a PCA
TermsScratch terms_scratch(const ParamBlock &P, int K, int C, int F, int Ecap, bool proba_in_params, int reduced_cols = 0);

// table width and mixture dimension a class model asks for
inline int gmm_inputs(const imsegm_gmm *g) { return g->n_inputs ? g->n_inputs : g->n_features; }
// limits of the model and of its PCA (sets the error text)
int check_gmm(const imsegm_gmm *gmm, int table_columns, int C);

// ---- the chain: launch_gc_terms -> launch_alpha_expansion / launch_unary_argmin -> launch_label_lut -> gathers
struct BackHalf {
    unsigned char *base;             // device: parameter block + scratch (of image 0 of a batch)
    ParamBlock par;
    TermsScratch scr;
    int smax, metric;                // param_fill: max |int(pairwise * 100)|, smooth_is_metric of those integers,
    double pmax;                     // max pairwise,
    const imsegm_gmm *gmm;           // the mixture, or null: probabilities uploaded in its place,
    bool have_lut;                   // a class look-up table was uploaded
    const double *features;          // [K][F] or null
    int32_t *K_dev, *E_dev;          // label / edge count on the device
    int32_t *edges, *arc_start, *arc_to, *arc_rev, *edge_arc;
    double *centres;
    const int32_t *labels;           // [n] label map
    size_t n;
    int32_t *segm_out;               // [n]
    double *soft_out;                // [n][C] or null (one image only)
    int K_cap, Ecap, C, F, ndim, edge_code, spatial_norm, use_graphcut;      // F: columns of the feature table
    int Fm = 0;                      // dimension of the mixture behind a PCA, 0: F
    double edge_cost;
    ZBatch zb;                       // zs != 0: a batch (the label counts differ: the cut reads K_dev)

    template <typename T> T *at(size_t off) const { return reinterpret_cast<T *>(base + off); }
    int32_t *misc() const { return at<int32_t>(par.o_misc); }
};
// into a zeroed host row of b.par.bytes: K, the pairwise matrix and its pygco integers, the class look-up table (or null), the
// mixture or (gmm null) `proba` [K][C]; b.smax .. b.have_lut are set
void param_fill(BackHalf &b, unsigned char *row, int K, const double *pairwise, const int32_t *classes_lut, const imsegm_gmm *gmm,
                const double *proba);
int backhalf_enqueue(imsegm_ctx *ctx, const BackHalf &b);

// the four words in front of a parameter block after the chain -> 0, -1 or -2 (more graph edges than the edge table holds: the
// caller may retry with a larger table) and the error text
int backhalf_status(const int32_t *misc, int use_graphcut);

}  // namespace imsegm
