// api_object_cut.hip -- C ABI of the cuts whose front runs on the device (object_cut.h): gco.cut_grid_graph on float costs, the
// pixel variant of imsegm/region_growing.py object_segmentation_graphcut_pixels, and the general cut with an explicit weight
// maximum.  The cut itself is launch_alpha_expansion as imsegm_cut_general_graph runs it.
#include "backhalf.h"
#include "object_cut.h"

#include <cfloat>
#include <climits>

namespace imsegm {

// device layout of one cut inside ctx->gc_buf: [work | unary | w | smooth | edges | arc_start | arc_to | arc_rev | edge_arc |
// labels | energy, status, the words of the conversion | what the entry point keeps in front of the conversion]
struct CutPlan {
    size_t work_bytes, o_u, o_w, o_s, o_e, o_as, o_at, o_ar, o_ea, o_lab, o_en, o_st, o_red, o_extra, bytes;
};

static CutPlan cut_plan(int K, int C, int E, size_t extra_bytes)
{
    const size_t En = (size_t)std::max(E, 1);
    CutPlan p;
    p.work_bytes = al64(alpha_expansion_work_bytes(K, E));
    p.o_u = 0;
    p.o_w = p.o_u + al64((size_t)K * C * 4);
    p.o_s = p.o_w + al64(En * 4);
    p.o_e = p.o_s + al64((size_t)C * C * 4);
    p.o_as = p.o_e + al64(En * 8);
    p.o_at = p.o_as + al64((size_t)(K + 1) * 4);
    p.o_ar = p.o_at + al64(En * 8);
    p.o_ea = p.o_ar + al64(En * 8);
    p.o_lab = p.o_ea + al64(En * 8);
    p.o_en = p.o_lab + al64((size_t)K * 4);
    p.o_st = p.o_en + 64;
    p.o_red = p.o_st + 64;
    p.o_extra = p.o_red + 64;
    p.bytes = p.o_extra + al64(extra_bytes);
    return p;
}

static int cut_sizes_ok(const char *who, long K, int C, long E)
{
    if (K < 1 || C < 1 || E < 0) {
        set_error(std::string(who) + ": bad sizes");
        return -1;
    }
    if (K > (1L << 29) || 2 * E > (long)INT_MAX) {
        set_error(std::string(who) + ": more sites than 32-bit arc indices hold");
        return -1;
    }
    return 0;
}

// (int32)(pairwise * 100) as pyGCO passes it on, its largest magnitude
static int smooth_integers(const double *pairwise, int C, int32_t *si)
{
    int smax = 0;
    for (int i = 0; i < C * C; ++i) {
        si[i] = (int32_t)(pairwise[i] * 100);
        smax = std::max(smax, std::abs(si[i]));
    }
    return smax;
}

// GCO refuses energy terms above GCO_MAX_ENERGYTERM = 10000000
static int energy_term_ok(const char *who, long long wmax, int smax)
{
    if (wmax * smax > 10000000LL) {
        set_error(std::string(who) + ": smoothness term is larger than GCO_MAX_ENERGYTERM");
        return -1;
    }
    return 0;
}

// the integer problem is complete on the device: cut it, bring labels and energy back
static int cut_run(imsegm_ctx *ctx, const CutPlan &pl, int K, int C, int E, const int32_t *si, int n_iter, int32_t *labels_out,
                   int64_t *energy_out)
{
    hipStream_t st = ctx->stream;
    unsigned char *dev = ctx->gc_buf.as<unsigned char>(), *io = dev + pl.work_bytes;
    int32_t *d_lab = (int32_t *)(io + pl.o_lab), *d_status = (int32_t *)(io + pl.o_st);
    long long *d_energy = (long long *)(io + pl.o_en);
    HIP_TRY(hipMemsetAsync(d_status, 0, 4, st));
    GcProblem p;
    p.K = K; p.C = C; p.E = E;
    p.edges = (int32_t *)(io + pl.o_e); p.w = (int32_t *)(io + pl.o_w); p.unary = (int32_t *)(io + pl.o_u); p.smooth = (int32_t *)(io + pl.o_s);
    p.metric = smooth_is_metric(si, C);
    int sp = ctx->begin(PG_GC);
    if (launch_alpha_expansion(p, (int32_t *)(io + pl.o_as), (int32_t *)(io + pl.o_at), (int32_t *)(io + pl.o_ar), (int32_t *)(io + pl.o_ea),
                               n_iter, d_lab, d_energy, d_status, dev, st))
        return -1;
    ctx->end(sp);
    long long energy = 0;
    int32_t status = 0;
    HIP_TRY(hipMemcpyAsync(labels_out, d_lab, (size_t)K * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(&energy, d_energy, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(&status, d_status, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    const int32_t misc[4] = { K, E, 0, status };
    if (backhalf_status(misc, 1)) return -1;
    if (energy_out) *energy_out = energy;
    return 0;
}

// the words of the conversion after launch_gc_convert: the refusal pyGCO's integers call for, before the cut is launched
static int conversion_ok(imsegm_ctx *ctx, const char *who, const unsigned long long *d_red, int smax, double *dwf_out)
{
    unsigned long long red[GC_RED_WORDS];
    HIP_TRY(hipMemcpyAsync(red, d_red, sizeof(red), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (dwf_out) memcpy(dwf_out, &red[GC_RED_DWF], 8);
    return energy_term_ok(who, std::llabs((long long)red[GC_RED_WMAX]), smax);
}

// arcs of a general edge list (a < b): every site's arcs in the order of the edges it is part of, reverse arcs, edge -> arcs
static void arcs_of_edges(const int32_t *edges, int E, int K, int32_t *arc_start, int32_t *arc_to, int32_t *arc_rev, int32_t *edge_arc)
{
    std::fill(arc_start, arc_start + K + 1, 0);
    for (int j = 0; j < 2 * E; ++j) arc_start[edges[j] + 1]++;
    for (int i = 0; i < K; ++i) arc_start[i + 1] += arc_start[i];
    std::vector<int32_t> next(arc_start, arc_start + K);
    for (int j = 0; j < E; ++j) {
        const int a = edges[2 * j], b = edges[2 * j + 1], ia = next[a]++, ib = next[b]++;
        arc_to[ia] = b;
        arc_to[ib] = a;
        arc_rev[ia] = ib;
        arc_rev[ib] = ia;
        edge_arc[2 * j] = ia;
        edge_arc[2 * j + 1] = ib;
    }
}

}  // namespace imsegm

extern "C" {

int imsegm_cut_grid_graph(imsegm_ctx *ctx, const double *unary, int H, int W, int C, const double *pairwise, const double *cost_v,
                          const double *cost_h, int n_iter, int32_t *labels_out, int64_t *energy_out)
{
    if (bind(ctx)) return -1;
    if (H < 1 || W < 1) {
        set_error("cut_grid_graph: bad sizes");
        return -1;
    }
    const long Kl = (long)H * W, El = grid_edges(H, W);
    if (cut_sizes_ok("cut_grid_graph", Kl, C, El)) return -1;
    const int K = (int)Kl, E = (int)El, Ev = (H - 1) * W;
    if (!unary || !pairwise || !labels_out || (Ev > 0 && !cost_v) || (E - Ev > 0 && !cost_h)) {
        set_error("cut_grid_graph: null argument");
        return -1;
    }
    if (check_pairwise(pairwise, C)) return -1;
    hipStream_t st = ctx->stream;
    // in front of the conversion: the float costs as gco takes them
    const size_t n_unary = (size_t)K * C, o_fu = 0, o_fw = al64(n_unary * 8), extra = o_fw + al64((size_t)std::max(E, 1) * 8);
    const CutPlan pl = cut_plan(K, C, E, extra);
    if (ctx->gc_buf.ensure(pl.work_bytes + pl.bytes + 256)) return -1;
    unsigned char *io = ctx->gc_buf.as<unsigned char>() + pl.work_bytes;
    std::vector<int32_t> si((size_t)C * C);
    const int smax = smooth_integers(pairwise, C, si.data());
    double mp = -DBL_MAX;
    for (int i = 0; i < C * C; ++i) mp = std::max(mp, pairwise[i]);
    double *d_fu = (double *)(io + pl.o_extra + o_fu), *d_fw = (double *)(io + pl.o_extra + o_fw);
    unsigned long long *d_red = (unsigned long long *)(io + pl.o_red);
    HIP_TRY(hipMemsetAsync(d_red, 0, 64, st));
    HIP_TRY(hipMemcpyAsync(io + pl.o_s, si.data(), si.size() * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_fu, unary, n_unary * 8, hipMemcpyHostToDevice, st));
    if (Ev > 0) HIP_TRY(hipMemcpyAsync(d_fw, cost_v, (size_t)Ev * 8, hipMemcpyHostToDevice, st));
    if (E - Ev > 0) HIP_TRY(hipMemcpyAsync(d_fw + Ev, cost_h, (size_t)(E - Ev) * 8, hipMemcpyHostToDevice, st));
    int sp = ctx->begin(PG_TERMS);
    if (launch_max_abs(d_fu, n_unary, d_red, GC_RED_MU, st)) return -1;
    if (launch_max_abs(d_fw, (size_t)E, d_red, GC_RED_MW, st)) return -1;
    if (launch_gc_convert(d_fu, n_unary, d_fw, E, E > 0, mp, d_red, (int32_t *)(io + pl.o_u), (int32_t *)(io + pl.o_w), st)) return -1;
    ctx->end(sp);
    sp = ctx->begin(PG_GRAPH);
    const GridArcs arcs = { (int32_t *)(io + pl.o_e), (int32_t *)(io + pl.o_as), (int32_t *)(io + pl.o_at), (int32_t *)(io + pl.o_ar),
                            (int32_t *)(io + pl.o_ea) };
    if (launch_grid_arcs(H, W, arcs, st)) return -1;
    ctx->end(sp);
    if (conversion_ok(ctx, "cut_general_graph", d_red, smax, nullptr)) return -1;
    return cut_run(ctx, pl, K, C, E, si.data(), n_iter, labels_out, energy_out);
}

int imsegm_object_cut_pixels(imsegm_ctx *ctx, const int32_t *segm, int H, int W, const int32_t *centres, int n_centres,
                             const double *a_bg, const double *a_fg, const double *s_bg, int n_labels, const double *b, int n_dist,
                             double coef_shape, double gc_regul, int seed_size, int n_iter, int32_t *labels_out, int64_t *energy_out,
                             int32_t *unary_int_out, double *dwf_out)
{
    if (bind(ctx)) return -1;
    if (H < 1 || W < 1 || n_centres < 1 || n_labels < 1 || n_dist < 1 || seed_size > 32767) {
        set_error("object_cut_pixels: bad sizes");
        return -1;
    }
    if (!segm || !centres || !a_bg || !a_fg || !s_bg || !b || !labels_out) {
        set_error("object_cut_pixels: null argument");
        return -1;
    }
    const int C = n_centres + 1;
    if (C > 64) {
        set_error("alpha_expansion: more than 64 labels are not supported by the single-workgroup kernel");
        return -1;
    }
    const long Kl = (long)H * W, El = grid_edges(H, W);
    if (cut_sizes_ok("object_cut_pixels", Kl, C, El)) return -1;
    const int K = (int)Kl, E = (int)El;
    const size_t table_bytes = object_unary_lds_bytes(n_labels, n_dist, n_centres);
    if (table_bytes > OBJECT_UNARY_LDS_MAX) {
        set_error("object_cut_pixels: the tables do not fit the LDS");
        return -1;
    }
    hipStream_t st = ctx->stream;
    // pairwise = (1 - eye) * gc_regul as the reference forms it
    std::vector<double> pairwise((size_t)C * C);
    for (int a = 0; a < C; ++a)
        for (int c = 0; c < C; ++c) pairwise[(size_t)a * C + c] = (a == c ? 0.0 : 1.0) * gc_regul;
    std::vector<int32_t> si((size_t)C * C);
    const int smax = smooth_integers(pairwise.data(), C, si.data());
    double mp = -DBL_MAX;
    for (int i = 0; i < C * C; ++i) mp = std::max(mp, pairwise[i]);
    // upload: [words of the conversion (64) | smooth | centres | a_bg | a_fg | s_bg | b] in one staged block, the class map on its own
    const size_t u_red = 0, u_s = 64, u_c = u_s + al64((size_t)C * C * 4), u_t = u_c + al64((size_t)n_centres * 16);
    const size_t up_bytes = u_t + al64(((size_t)3 * n_labels + n_dist) * 8);
    const size_t o_up = 0, o_segm = al64(up_bytes), extra = o_segm + al64((size_t)K * 4);
    const CutPlan pl = cut_plan(K, C, E, extra);
    if (ctx->gc_buf.ensure(pl.work_bytes + pl.bytes + 256)) return -1;
    unsigned char *io = ctx->gc_buf.as<unsigned char>() + pl.work_bytes, *d_up = io + pl.o_extra + o_up;
    unsigned char *host = static_cast<unsigned char *>(ctx->stage(up_bytes));
    if (!host) {
        set_error("cannot allocate pinned staging memory");
        return -1;
    }
    memset(host, 0, u_s);
    const double one = 1.0;
    if (E > 0) memcpy(host + u_red + 8 * GC_RED_MW, &one, 8);                 // every edge weighs 1
    memcpy(host + u_s, si.data(), si.size() * 4);
    memcpy(host + u_c, centres, (size_t)n_centres * 16);
    double *ht = (double *)(host + u_t);
    memcpy(ht, a_bg, (size_t)n_labels * 8);
    memcpy(ht + n_labels, a_fg, (size_t)n_labels * 8);
    memcpy(ht + 2 * (size_t)n_labels, s_bg, (size_t)n_labels * 8);
    memcpy(ht + 3 * (size_t)n_labels, b, (size_t)n_dist * 8);
    HIP_TRY(hipMemcpyAsync(d_up, host, up_bytes, hipMemcpyHostToDevice, st));
    ctx->mark_stage_in_flight();
    int32_t *d_segm = (int32_t *)(io + pl.o_extra + o_segm);
    HIP_TRY(hipMemcpyAsync(d_segm, segm, (size_t)K * 4, hipMemcpyHostToDevice, st));
    unsigned long long *d_red = (unsigned long long *)(io + pl.o_red);
    HIP_TRY(hipMemcpyAsync(d_red, d_up + u_red, 64, hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipMemcpyAsync(io + pl.o_s, d_up + u_s, (size_t)C * C * 4, hipMemcpyDeviceToDevice, st));
    const double *dt = (const double *)(d_up + u_t);
    ObjectUnary o;
    o.segm = d_segm; o.H = H; o.W = W; o.n_centres = n_centres; o.centres = (const int32_t *)(d_up + u_c);
    o.a_bg = dt; o.a_fg = dt + n_labels; o.s_bg = dt + 2 * (size_t)n_labels; o.n_labels = n_labels;
    o.b = dt + 3 * (size_t)n_labels; o.n_dist = n_dist;
    o.coef_shape = coef_shape; o.seed_size = seed_size;
    int32_t *d_ui = (int32_t *)(io + pl.o_u);
    int sp = ctx->begin(PG_TERMS);
    if (launch_object_unary_max(o, d_red, st)) return -1;
    if (launch_gc_convert(nullptr, 0, nullptr, E, E > 0, mp, d_red, nullptr, (int32_t *)(io + pl.o_w), st)) return -1;
    if (launch_object_unary_int(o, d_red, d_ui, st)) return -1;
    ctx->end(sp);
    sp = ctx->begin(PG_GRAPH);
    const GridArcs arcs = { (int32_t *)(io + pl.o_e), (int32_t *)(io + pl.o_as), (int32_t *)(io + pl.o_at), (int32_t *)(io + pl.o_ar),
                            (int32_t *)(io + pl.o_ea) };
    if (launch_grid_arcs(H, W, arcs, st)) return -1;
    ctx->end(sp);
    if (unary_int_out) HIP_TRY(hipMemcpyAsync(unary_int_out, d_ui, (size_t)K * C * 4, hipMemcpyDeviceToHost, st));
    if (conversion_ok(ctx, "cut_general_graph", d_red, smax, dwf_out)) return -1;
    return cut_run(ctx, pl, K, C, E, si.data(), n_iter, labels_out, energy_out);
}

// imsegm_cut_general_graph with pyGCO's scaling maximum of |edge_weights| given by the caller where it is larger than the one of
// the edges handed over (edges the caller has dropped because they join a site with itself still scale the energies: DESIGN.md).
// The float costs go up and are converted by the kernels of the grid entry; the arcs of a general edge list are built on the host.
int imsegm_cut_general_graph_scaled(imsegm_ctx *ctx, const int32_t *edges, int n_edges, const double *edge_weights,
                                    const double *unary_cost, int n_sites, int n_labels, const double *pairwise_cost,
                                    double weight_max, int n_iter, int32_t *labels_out, int64_t *energy_out)
{
    if (bind(ctx)) return -1;
    const int K = n_sites, C = n_labels, E = n_edges;
    if (cut_sizes_ok("cut_general_graph", K, C, E)) return -1;
    for (int j = 0; j < E; ++j) {
        int a = edges[2 * j], b = edges[2 * j + 1];
        if (a < 0 || b >= K || a >= b) {
            set_error("cut_general_graph: edges must satisfy 0 <= edges[:,0] < edges[:,1] < n_sites");
            return -1;
        }
    }
    if (check_pairwise(pairwise_cost, C)) return -1;
    hipStream_t st = ctx->stream;
    const size_t n_unary = (size_t)K * C, o_fu = 0, o_fw = al64(n_unary * 8), extra = o_fw + al64((size_t)std::max(E, 1) * 8);
    const CutPlan pl = cut_plan(K, C, E, extra);
    if (ctx->gc_buf.ensure(pl.work_bytes + pl.bytes + 256)) return -1;
    unsigned char *io = ctx->gc_buf.as<unsigned char>() + pl.work_bytes;
    // staged upload: [smooth | edges | arc_start | arc_to | arc_rev | edge_arc] at the offsets of the plan, and the words of the
    // conversion with the caller's maximum already in the place of max |w|
    const size_t up_bytes = pl.o_lab - pl.o_s;
    unsigned char *host = static_cast<unsigned char *>(ctx->stage(up_bytes + 64));
    if (!host) {
        set_error("cannot allocate pinned staging memory");
        return -1;
    }
    auto at = [&](size_t off) { return (int32_t *)(host + (off - pl.o_s)); };
    const int smax = smooth_integers(pairwise_cost, C, at(pl.o_s));
    const std::vector<int32_t> si(at(pl.o_s), at(pl.o_s) + (size_t)C * C);
    double mp = -DBL_MAX;
    for (int i = 0; i < C * C; ++i) mp = std::max(mp, pairwise_cost[i]);
    if (E > 0) memcpy(at(pl.o_e), edges, (size_t)E * 8);
    arcs_of_edges(edges, E, K, at(pl.o_as), at(pl.o_at), at(pl.o_ar), at(pl.o_ea));
    unsigned long long *hred = (unsigned long long *)(host + up_bytes);
    memset(hred, 0, 64);
    if (weight_max >= 0) memcpy(&hred[GC_RED_MW], &weight_max, 8);
    unsigned long long *d_red = (unsigned long long *)(io + pl.o_red);
    HIP_TRY(hipMemcpyAsync(io + pl.o_s, host, up_bytes, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_red, hred, 64, hipMemcpyHostToDevice, st));
    ctx->mark_stage_in_flight();
    double *d_fu = (double *)(io + pl.o_extra + o_fu), *d_fw = (double *)(io + pl.o_extra + o_fw);
    HIP_TRY(hipMemcpyAsync(d_fu, unary_cost, n_unary * 8, hipMemcpyHostToDevice, st));
    if (E > 0) HIP_TRY(hipMemcpyAsync(d_fw, edge_weights, (size_t)E * 8, hipMemcpyHostToDevice, st));
    int sp = ctx->begin(PG_TERMS);
    if (launch_max_abs(d_fu, n_unary, d_red, GC_RED_MU, st)) return -1;
    if (launch_max_abs(d_fw, (size_t)E, d_red, GC_RED_MW, st)) return -1;
    // (pyGCO saw the dropped edges too: their weights scale even where no edge is left)
    if (launch_gc_convert(d_fu, n_unary, d_fw, E, E > 0 || weight_max >= 0, mp, d_red, (int32_t *)(io + pl.o_u), (int32_t *)(io + pl.o_w), st))
        return -1;
    ctx->end(sp);
    // the refusal concerns the edges GCO gets: the largest of THEIR integer weights
    double mw_kept = 0;
    for (int i = 0; i < E; ++i) mw_kept = std::max(mw_kept, fabs(edge_weights[i]));
    double dwf = 0;
    if (conversion_ok(ctx, "cut_general_graph", d_red, 0, &dwf)) return -1;
    if (energy_term_ok("cut_general_graph", std::llabs((long long)(int32_t)((mw_kept / dwf) * 1000)), smax)) return -1;
    return cut_run(ctx, pl, K, C, E, si.data(), n_iter, labels_out, energy_out);
}

// the arcs k_grid_arcs builds for a height x width grid, for the test that holds them against the host loop
int imsegm_debug_grid_arcs(imsegm_ctx *ctx, int height, int width, int32_t *edges_out, int32_t *arc_start_out, int32_t *arc_to_out,
                           int32_t *arc_rev_out, int32_t *edge_arc_out)
{
    if (bind(ctx)) return -1;
    if (height < 1 || width < 1 || cut_sizes_ok("debug_grid_arcs", (long)height * width, 1, grid_edges(height, width))) {
        set_error("debug_grid_arcs: bad sizes");
        return -1;
    }
    const int K = height * width, E = (int)grid_edges(height, width);
    const CutPlan pl = cut_plan(K, 1, E, 0);
    if (ctx->gc_buf.ensure(pl.work_bytes + pl.bytes + 256)) return -1;
    unsigned char *io = ctx->gc_buf.as<unsigned char>() + pl.work_bytes;
    hipStream_t st = ctx->stream;
    const GridArcs arcs = { (int32_t *)(io + pl.o_e), (int32_t *)(io + pl.o_as), (int32_t *)(io + pl.o_at), (int32_t *)(io + pl.o_ar),
                            (int32_t *)(io + pl.o_ea) };
    if (launch_grid_arcs(height, width, arcs, st)) return -1;
    HIP_TRY(hipMemcpyAsync(arc_start_out, arcs.arc_start, (size_t)(K + 1) * 4, hipMemcpyDeviceToHost, st));
    if (E > 0) {
        HIP_TRY(hipMemcpyAsync(edges_out, arcs.edges, (size_t)E * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(arc_to_out, arcs.arc_to, (size_t)E * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(arc_rev_out, arcs.arc_rev, (size_t)E * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(edge_arc_out, arcs.edge_arc, (size_t)E * 8, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

}  // extern "C"
