// backhalf.hip -- the fused back half behind a label map: parameter block, scratch, launch chain, status words (backhalf.h)
#include "backhalf.h"

namespace imsegm {

int check_pairwise(const double *pairwise, int C)
{
    for (int a = 0; a < C; ++a)
        for (int b = 0; b < C; ++b)
            if (pairwise[a * C + b] != pairwise[b * C + a]) {
                set_error("Cost matrix not square or not symmetric");
                return -1;
            }
    return 0;
}

int decode_edge_type(int edge_type, int *edge_code, int *spatial_norm)
{
    *edge_code = edge_type & 0xff;
    *spatial_norm = (edge_type & IMSEGM_EDGE_SPATIAL_NORM) ? 1 : 0;
    if (*edge_code < 0 || *edge_code > 5) {
        set_error("segment: unknown edge type");
        return -1;
    }
    return 0;
}

int check_gmm(const imsegm_gmm *gmm, int table_columns, int C)
{
    if (gmm_inputs(gmm) != table_columns || gmm->n_classes != C) {
        set_error("class model does not match the resident features / number of classes");
        return -1;
    }
    if (gmm->n_features < 1 || gmm->n_features > 256 || gmm->n_inputs < 0 || gmm->n_inputs > 256 || C > 16) {
        set_error("device class model: at most 256 features and 16 classes");
        return -1;
    }
    if (gmm->n_inputs && (gmm->n_features > gmm->n_inputs || !gmm->pca_components_t || !gmm->pca_shift)) {
        set_error("class model with a PCA: 1 <= n_features <= n_inputs <= 256, components and shift are required");
        return -1;
    }
    return 0;
}

ParamBlock param_block(int C, int F, int proba_rows, int n_inputs)
{
    ParamBlock P;
    size_t o = 0;
    auto take = [&](size_t bytes) { size_t at = o; o += al64(bytes); return at; };
    P.o_misc = take(256);
    P.o_pw = take((size_t)C * C * 8);
    P.o_sm = take((size_t)C * C * 4);
    P.o_cl = take((size_t)C * 4);
    P.o_sc = take((size_t)2 * (n_inputs ? n_inputs : F) * 8);
    P.o_pc = take((size_t)C * F * F * 8);
    P.o_mp = take((size_t)C * F * 8);
    P.o_ld = take((size_t)C * 8);
    P.o_lw = take((size_t)C * 8);
    P.o_pr = take((size_t)proba_rows * C * 8);
    P.o_ct = take((size_t)n_inputs * F * 8);
    P.o_ps = take(n_inputs ? (size_t)2 * F * 8 : 0);
    P.bytes = o;
    return P;
}

void param_fill(BackHalf &b, unsigned char *row, int K, const double *pairwise, const int32_t *classes_lut, const imsegm_gmm *gmm,
                const double *proba)
{
    const ParamBlock &P = b.par;
    const int C = b.C, F = b.Fm ? b.Fm : b.F, Fs = b.F;       // (mixture dimension, scaler length)
    reinterpret_cast<int32_t *>(row + P.o_misc)[0] = K;          // E = 0 | status = 0 | gc status = 0 | energy = 0 behind it
    memcpy(row + P.o_pw, pairwise, (size_t)C * C * 8);
    int32_t *si = reinterpret_cast<int32_t *>(row + P.o_sm);
    b.smax = 0; b.pmax = -DBL_MAX; b.gmm = gmm; b.have_lut = classes_lut != nullptr;
    for (int i = 0; i < C * C; ++i) {
        si[i] = (int32_t)(pairwise[i] * 100);                    // pygco: smooth cost * 100, truncated
        b.smax = std::max(b.smax, std::abs(si[i]));
        b.pmax = std::max(b.pmax, pairwise[i]);
    }
    b.metric = smooth_is_metric(si, C);
    if (classes_lut) memcpy(row + P.o_cl, classes_lut, (size_t)C * 4);
    if (gmm) {
        if (gmm->scaler_mean) memcpy(row + P.o_sc, gmm->scaler_mean, (size_t)Fs * 8);
        if (gmm->scaler_scale) memcpy(row + P.o_sc + (size_t)Fs * 8, gmm->scaler_scale, (size_t)Fs * 8);
        if (gmm->n_inputs) {
            memcpy(row + P.o_ct, gmm->pca_components_t, (size_t)Fs * F * 8);
            memcpy(row + P.o_ps, gmm->pca_shift, (size_t)F * 8);
            if (gmm->pca_scale) memcpy(row + P.o_ps + (size_t)F * 8, gmm->pca_scale, (size_t)F * 8);
        }
        memcpy(row + P.o_pc, gmm->prec_chol, (size_t)C * F * F * 8);
        memcpy(row + P.o_mp, gmm->mu_proj, (size_t)C * F * 8);
        memcpy(row + P.o_ld, gmm->log_det, (size_t)C * 8);
        memcpy(row + P.o_lw, gmm->log_weights, (size_t)C * 8);
    } else if (proba) {                                          // (null: the caller copies them on the device)
        memcpy(row + P.o_pr, proba, (size_t)K * C * 8);
    }
}

TermsScratch terms_scratch(const ParamBlock &P, int K, int C, int F, int Ecap, bool proba_in_params, int reduced_cols)
{
    TermsScratch S;
    size_t d = P.bytes;
    auto take = [&](size_t bytes) { size_t at = d; d += al64(bytes); return at; };
    S.d_proba = proba_in_params ? P.o_pr : take((size_t)K * C * 8);
    S.d_unary = take((size_t)K * C * 8);
    S.d_unary_i = take((size_t)K * C * 4);
    S.d_w = take((size_t)Ecap * 8);
    S.d_wi = take((size_t)Ecap * 4);
    S.d_edist = take((size_t)Ecap * 8);
    S.d_elen = take((size_t)Ecap * 8);
    S.d_gl = take((size_t)K * 4);
    S.d_lut = take((size_t)K * 4);
    S.d_fstd = take((size_t)2 * std::max(F, 1) * 8);
    S.d_work = take(alpha_expansion_work_bytes(K, Ecap));
    S.d_red = take((size_t)K * reduced_cols * 8);
    S.end = d;
    return S;
}

int backhalf_enqueue(imsegm_ctx *ctx, const BackHalf &b)
{
    hipStream_t st = ctx->stream;
    const ParamBlock &P = b.par;
    const TermsScratch &S = b.scr;
    const imsegm_gmm *gmm = b.gmm;
    int32_t *status = b.misc() + 2;
    // ---- class probabilities, unary / edge terms, integer energies
    TermsArgs a;
    memset(&a, 0, sizeof(a));
    a.zs = b.zb.zs;
    a.Kp = b.K_dev; a.K_cap = b.K_cap; a.Ep = b.E_dev; a.edge_capacity = b.Ecap; a.F = b.Fm ? b.Fm : b.F; a.F_tab = b.F; a.C = b.C;
    a.features = b.features;
    a.gmm = gmm ? 1 : 0;
    if (gmm) {
        a.scaler_mean = gmm->scaler_mean ? b.at<double>(P.o_sc) : nullptr;
        a.scaler_scale = gmm->scaler_scale ? b.at<double>(P.o_sc) + b.F : nullptr;
        a.prec_chol = b.at<double>(P.o_pc);
        a.mu_proj = b.at<double>(P.o_mp);
        a.log_det = b.at<double>(P.o_ld);
        a.log_w = b.at<double>(P.o_lw);
        a.const_term = gmm->const_term;
        if (gmm->n_inputs) {
            a.pca_ct = b.at<double>(P.o_ct);
            a.pca_shift = b.at<double>(P.o_ps);
            a.pca_scale = gmm->pca_scale ? b.at<double>(P.o_ps) + a.F : nullptr;
            a.reduced = b.at<double>(S.d_red);
        }
    }
    a.proba = b.at<double>(S.d_proba);
    a.edge_type = b.edge_code; a.spatial_norm = b.spatial_norm; a.edge_cost = b.edge_cost;
    a.edges = b.edges; a.centres = b.centres; a.ndim = b.ndim;
    a.edge_dist = b.at<double>(S.d_edist); a.edge_len = b.at<double>(S.d_elen);
    a.unary = b.at<double>(S.d_unary); a.weights = b.at<double>(S.d_w);
    a.pairwise = b.at<double>(P.o_pw); a.pairwise_max = b.pmax;
    a.unary_i = b.at<int32_t>(S.d_unary_i); a.weights_i = b.at<int32_t>(S.d_wi);
    a.smooth_max = b.smax; a.status = status; a.scalars = b.at<double>(P.o_misc + 64); a.fstd = b.at<double>(S.d_fstd);
    const int spt = ctx->begin(PG_TERMS);
    if (launch_gc_terms(a, st, b.zb.nz)) return -1;
    ctx->end(spt);
    // ---- alpha-expansion: one workgroup per image of ONE launch (or the argmin of the unary cost for gc_regul <= 0)
    int32_t *glab = b.at<int32_t>(S.d_gl);
    const int spg = ctx->begin(PG_GC);
    if (b.use_graphcut) {
        GcProblem p;
        p.K = b.K_cap; p.C = b.C; p.E = b.Ecap; p.E_dev = b.E_dev;
        p.K_dev = b.zb.zs ? b.K_dev : nullptr;               // (one image: K_cap is its label count)
        p.edges = b.edges; p.w = a.weights_i; p.unary = a.unary_i; p.smooth = b.at<int32_t>(P.o_sm);
        p.metric = b.metric;
        if (launch_alpha_expansion(p, b.arc_start, b.arc_to, b.arc_rev, b.edge_arc, -1, glab, b.at<long long>(P.o_misc + 16), status + 1,
                                   b.base + S.d_work, st, b.zb))
            return -1;
    } else if (launch_unary_argmin(a.unary, b.K_dev, b.K_cap, b.C, glab, st, b.zb)) {
        return -1;
    }
    ctx->end(spg);
    // ---- gathers: classes_[graph_labels][slic] and proba[slic]
    int32_t *lut = b.at<int32_t>(S.d_lut);
    if (launch_label_lut(glab, b.K_dev, b.K_cap, b.have_lut ? b.at<int32_t>(P.o_cl) : nullptr, lut, st, b.zb)) return -1;
    const int spq = ctx->begin(PG_GATHER);
    if (launch_gather_labels(lut, b.labels, b.n, b.segm_out, st, b.zb)) return -1;
    if (b.soft_out && launch_gather_proba(a.proba, b.C, b.labels, b.n, b.soft_out, st)) return -1;
    ctx->end(spq);
    return 0;
}

int backhalf_status(const int32_t *misc, int use_graphcut)
{
    if (misc[2] & 2) {
        set_error("segment: more graph edges than the edge table holds");
        return -2;
    }
    if (use_graphcut && (misc[2] & 1)) {
        set_error("cut_general_graph: smoothness term is larger than GCO_MAX_ENERGYTERM");
        return -1;
    }
    if (use_graphcut && misc[3] != 0) {
        set_error("alpha_expansion: max-flow did not converge");
        return -1;
    }
    return 0;
}

}  // namespace imsegm
