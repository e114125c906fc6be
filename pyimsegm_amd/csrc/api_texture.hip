// api_texture.hip -- C ABI of the Leung-Malik texture stage (high-pass, batteries, response statistics)
// (one of the files api.hip was split into in round 6: the C ABI of include/imsegm_hip.h by stage; the helpers they share are
// declared in session.h)
#include "session.h"

extern "C" {

int imsegm_image2d_lm_prepare(imsegm_image2d *im, const double *taps, int radius, const double *channel_mix)
{
    if (!im || bind(im->ctx)) return -1;
    if (im->dtype < 0) {
        set_error("no image uploaded");
        return -1;
    }
    if (radius < 0 || !taps || (!channel_mix && !im->is_volume)) {
        set_error("lm_prepare: bad arguments");
        return -1;
    }
    hipStream_t st = im->ctx->stream;
    // colour image: three channel planes of H x W; gray volume: its D slices, filtered independently (descriptors.py:981-994)
    const size_t np = im->is_volume ? im->n : 3 * im->n;
    if (im->tex_planes.ensure(np * 8) || im->labA.ensure(np * 8) || im->labB.ensure(np * 8)) return -1;
    if (im->tex_small.ensure(((size_t)radius + 1 + 9) * 8 + 1024 * 8 + 4096 + ((size_t)2 * radius + 64) * 8)) return -1;
    double *d_taps = im->tex_small.as<double>();
    double *d_mix = d_taps + radius + 1;
    double *d_full = d_taps + radius + 1 + 9 + 1024 + 512;        // behind the partial sums of the batteries
    HIP_TRY(hipMemcpyAsync(d_taps, taps, ((size_t)radius + 1) * 8, hipMemcpyHostToDevice, st));
    if (channel_mix) HIP_TRY(hipMemcpyAsync(d_mix, channel_mix, 9 * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (im->is_volume) {
        if (launch_texture_prepare_volume(im->img.p, im->dtype, im->D, im->H, im->W, d_taps, radius, im->tex_planes.as<double>(),
                                          im->labA.as<double>(), im->labB.as<double>(), st, d_full))
            return -1;
    } else if (launch_texture_prepare(im->img.p, im->dtype, im->H, im->W, d_taps, radius, d_mix, im->tex_planes.as<double>(),
                                      im->labA.as<double>(), im->labB.as<double>(), st, d_full)) {
        return -1;
    }
    im->tex_ready = true;
    return 0;
}

int imsegm_image2d_lm_battery(imsegm_image2d *im, const double *weights, int n_kernels, int radius, double clip,
                              double *sum_squares_out)
{
    if (!im || bind(im->ctx)) return -1;
    if (!im->tex_ready) {
        set_error("lm_battery: call imsegm_image2d_lm_prepare first");
        return -1;
    }
    hipStream_t st = im->ctx->stream;
    const size_t n = im->is_volume ? (im->n + 2) / 3 : im->n;          // the buffers below hold 3 * n values
    const int P = im->is_volume ? im->D : 3;
    const size_t S = 2 * (size_t)radius + 1;
    const size_t wbytes = S * S * n_kernels * 8;
    const size_t wpad = S * (S + 16) * n_kernels;                    // the row-padded copy the battery kernel reads (texture.hip)
    if (im->tex_resp.ensure(3 * n * 8 + wbytes + wpad * 8 + 1024 * 8 + 64)) return -1;
    double *resp = im->tex_resp.as<double>();
    double *d_w = resp + 3 * n;
    double *partial = d_w + S * S * n_kernels + wpad;
    double *d_sum = partial + 1024;
    HIP_TRY(hipMemcpyAsync(d_w, weights, wbytes, hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));
    int spx = im->ctx->begin(PG_TEX);
    if (launch_filter_battery(im->tex_planes.as<double>(), im->H, im->W, d_w, n_kernels, radius, clip, resp, partial, d_sum, st, P))
        return -1;
    im->ctx->end(spx);
    HIP_TRY(hipMemcpyAsync(sum_squares_out, d_sum, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

int imsegm_image2d_lm_features(imsegm_image2d *im, const double *weights, const int *n_kernels, int n_batteries, int radius, double clip,
                               int feature_mask, double *features_out)
{
    return imsegm_image2d_lm_features_sep(im, weights, n_kernels, nullptr, nullptr, nullptr, nullptr, n_batteries, radius, clip,
                                          feature_mask, features_out);
}

int imsegm_image2d_lm_features_sep(imsegm_image2d *im, const double *weights, const int *n_kernels, const int *dense_parity,
                                   const double *sep_taps, const int *sep_groups, const int *sep_rank, int n_batteries, int radius,
                                   double clip, int feature_mask, double *features_out)
{
    if (!im || bind(im->ctx)) return -1;
    if (wrong_kind(im, false)) return -1;
    if (!im->tex_ready || !im->have_labels) {
        set_error("lm_features: call imsegm_image2d_lm_prepare first, with a label map installed");
        return -1;
    }
    if (!n_kernels || n_batteries < 1 || feature_mask < 1 || feature_mask > 7 ||
        (sep_taps && (!sep_groups || !sep_rank))) {
        set_error("lm_features: bad arguments");
        return -1;
    }
    imsegm_ctx *ctx = im->ctx;
    hipStream_t st = ctx->stream;
    const size_t n = im->n;
    const int K = im->n_labels;
    const size_t S = 2 * (size_t)radius + 1;
    // per battery: the dense weights as the caller lays them out, room for the row-padded copy launch_filter_battery makes of them,
    // then the taps of its separable kernels (groups x rank components of 2 S doubles)
    std::vector<size_t> off((size_t)n_batteries + 1, 0), sep_off((size_t)n_batteries, 0);
    size_t dense_total = 0;
    for (int b = 0; b < n_batteries; ++b) {
        const int nk = n_kernels[b], ng = sep_taps ? sep_groups[b] : 0, rk = sep_taps ? sep_rank[b] : 0;
        if ((nk != 0 && nk != 1 && nk != 2 && nk != 4 && nk != 6 && nk != 8) || ng < 0 || ng > 2 || (ng > 0 && (rk < 1 || rk > 4)) ||
            (nk == 0 && ng == 0)) {
            set_error("filter battery: 0, 1, 2, 4, 6 or 8 dense kernels and up to 2 separable ones of rank 1..4 per battery");
            return -1;
        }
        sep_off[b] = off[b] + S * S * nk + S * (S + 16) * nk;
        off[b + 1] = sep_off[b] + (size_t)ng * rk * 2 * S;
        dense_total += S * S * nk;
    }
    if (dense_total > 0 && !weights) {
        set_error("lm_features: dense kernels without weights");
        return -1;
    }
    const size_t wtotal = off[n_batteries];
    // responses of up to ROUND consecutive batteries side by side: the separable kernels of a round share ONE launch (one load of
    // the input tile for all of them -- the five batteries of one sigma of the bank)
    const int ROUND = std::min(n_batteries, (int)SEP_MAX_JOBS);
    // (scratch of the sums of squares: 1024 partial sums of launch_response_sumsq, or one per workgroup and battery of the round when
    // the separable kernels -- the last writers of a response -- form them on the way)
    const size_t n_partial = std::max<size_t>(1024, sep_taps ? sep_sumsq_scratch(im->H, im->W, 3, radius, ROUND) : 0);
    if (im->tex_resp.ensure((3 * n * ROUND + wtotal + n_partial + (size_t)n_batteries + 8) * 8 + 64)) return -1;
    double *resp = im->tex_resp.as<double>();
    double *d_w = resp + 3 * n * ROUND;
    double *partial = d_w + wtotal;
    double *d_ssq = partial + n_partial;
    double *host = static_cast<double *>(ctx->stage(wtotal * 8));
    if (!host) {
        set_error("cannot allocate pinned staging memory");
        return -1;
    }
    {
        const double *src = weights, *ssrc = sep_taps;
        for (int b = 0; b < n_batteries; ++b) {
            const size_t cnt = S * S * n_kernels[b];
            if (cnt) memcpy(host + off[b], src, cnt * 8);
            src += cnt;
            const size_t scnt = sep_taps ? (size_t)sep_groups[b] * sep_rank[b] * 2 * S : 0;
            if (scnt) memcpy(host + sep_off[b], ssrc, scnt * 8);
            ssrc += scnt;
        }
    }
    HIP_TRY(hipMemcpyAsync(d_w, host, wtotal * 8, hipMemcpyHostToDevice, st));
    ctx->mark_stage_in_flight();
    // statistics scratch (as stats_run) and the K x F table
    const int Fb = color_feature_columns(feature_mask), F = Fb * n_batteries;
    int table_F = F, col0 = 0;
    if (take_placement(im, F, features_out != nullptr, &table_F, &col0)) return -1;
    if (im->feat.ensure(stats_scratch_bytes(K)) || im->featK.ensure((size_t)K * table_F * 8 + 64)) return -1;
    const StatsScratch ss = stats_scratch_at(im->feat.p, K);
    for (int b0 = 0; b0 < n_batteries; b0 += ROUND) {
        const int cnt = std::min(ROUND, n_batteries - b0);
        int spx = ctx->begin(PG_TEX);
        SepJobs jobs;
        memset(&jobs, 0, sizeof(jobs));
        double *ssq_of_job[SEP_MAX_JOBS] = { nullptr };
        bool has_sep[SEP_MAX_JOBS] = { false };
        for (int j = 0; j < cnt; ++j) {
            const int b = b0 + j;
            double *rj = resp + (size_t)j * 3 * n;
            if (launch_battery_dense(im->tex_planes.as<double>(), im->H, im->W, d_w + off[b], n_kernels[b], radius, clip, rj, st, 3,
                                     dense_parity ? dense_parity[b] : 0))
                return -1;
            has_sep[j] = sep_taps && sep_groups[b] > 0;
            if (has_sep[j]) {
                ssq_of_job[jobs.n] = d_ssq + b;
                SepJob &q = jobs.job[jobs.n++];
                q.resp = rj; q.taps = d_w + sep_off[b]; q.groups = sep_groups[b]; q.rank = sep_rank[b]; q.merge = n_kernels[b] > 0 ? 1 : 0;
            }
        }
        const bool fused_ssq = jobs.n > 0 && sep_sumsq_scratch(im->H, im->W, 3, radius, jobs.n) > 0;
        if (launch_battery_sep(im->tex_planes.as<double>(), im->H, im->W, radius, clip, jobs, st, 3, fused_ssq ? partial : nullptr,
                               fused_ssq ? ssq_of_job : nullptr))
            return -1;
        for (int j = 0; j < cnt; ++j)
            if (!(fused_ssq && has_sep[j]) && launch_response_sumsq(resp + (size_t)j * 3 * n, 3 * n, partial, d_ssq + b0 + j, st)) return -1;
        ctx->end(spx);
        // |r| <= norm  =>  |r * mul / div| <= mul = log(1 + norm) / 0.03: the bound the fixed-point scales follow, without the norm
        // coming to the host (prescale 2: the kernels derive mul, div and the scales from *ssq; the 32768 > mul below is unused)
        int sps = ctx->begin(PG_STATS);
        for (int j = 0; j < cnt; ++j) {
            const int b = b0 + j;
            if (launch_color_stats(resp + (size_t)j * 3 * n, IMSEGM_F64, im->labels.as<int32_t>(), im->H, im->W, K, 32768.0,
                                   (feature_mask & 2) != 0, ss.acc, ss.mean, ss.energy, ss.var, ss.mean32, st, 1, 2, 1.0, 1.0, -1, d_ssq + b))
                return -1;
            if (launch_features_assemble(ss.mean, ss.energy, ss.var, K, feature_mask, im->featK.as<double>(), st, table_F, col0 + b * Fb))
                return -1;
        }
        ctx->end(sps);
    }
    // called for the resident table (no host copy asked for): imsegm_image2d_segment reads it by feat_F; with a host copy the
    // table counts as consumed, as before
    im->feat_mask = features_out ? 0 : 8;
    im->forest_ready = false;
    im->feat_F = table_F;
    if (features_out) {
        HIP_TRY(hipMemcpyAsync(features_out, im->featK.p, (size_t)K * F * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    return 0;
}

int imsegm_image2d_response_stats(imsegm_image2d *im, double mul, double div, double *mean_out, double *energy_out,
                                  double *var_out)
{
    if (!im || bind(im->ctx)) return -1;
    if (!im->tex_ready || !im->have_labels || im->tex_resp.cap < (im->is_volume ? im->n : 3 * im->n) * 8) {
        set_error("response_stats needs a filter response and a label map");
        return -1;
    }
    if (!(div != 0.0)) {
        set_error("response_stats: zero norm");
        return -1;
    }
    const double maxabs = fabs(mul);           // |r| <= norm = div  =>  |r * mul / div| <= |mul|
    if (!im->is_volume) return stats_run(im, im->tex_resp.p, IMSEGM_F64, maxabs, 1, 1, mul, div, mean_out, energy_out, var_out);
    // volume: the response is one plane of (D * H) x W read as all three channels (plane stride 0); K values each
    const int K = im->n_labels;
    std::vector<double> m((size_t)K * 3), e((size_t)K * 3), v((size_t)K * 3);
    const int keepH = im->H;
    im->H = im->D * keepH;
    int rc = stats_run(im, im->tex_resp.p, IMSEGM_F64, maxabs, 1, 1, mul, div, mean_out ? m.data() : nullptr,
                       energy_out ? e.data() : nullptr, var_out ? v.data() : nullptr, 0);
    im->H = keepH;
    if (rc) return rc;
    for (int k = 0; k < K; ++k) {
        if (mean_out) mean_out[k] = m[(size_t)k * 3];
        if (energy_out) energy_out[k] = e[(size_t)k * 3];
        if (var_out) var_out[k] = v[(size_t)k * 3];
    }
    return 0;
}

// the response of the last lm_battery for the statistics below: [3][H][W] planes (a volume: its D slices, one plane of D * H * W);
// the median and the gradient borrow tex_aux only -- tex_planes and tex_resp stay, the next lm_battery needs no lm_prepare
static int response_for_stats(imsegm_image2d *im, double mul, double div, const double *out, const char *what)
{
    if (!im->tex_ready || !im->have_labels || im->tex_resp.cap < (im->is_volume ? im->n : 3 * im->n) * 8 || !out) {
        set_error(std::string(what) + " needs a filter response, a label map and an output");
        return -1;
    }
    if (!(div > 0.0) || !(mul >= 0.0)) {          // (r * mul) / div is monotone in r: the median ranks the raw response
        set_error(std::string(what) + ": needs mul >= 0 and a positive norm div");
        return -1;
    }
    return 0;
}

int imsegm_image2d_response_median(imsegm_image2d *im, double mul, double div, double *median_out)
{
    if (!im || bind(im->ctx)) return -1;
    if (response_for_stats(im, mul, div, median_out, "response_median")) return -1;
    hipStream_t st = im->ctx->stream;
    const int K = im->n_labels, C = im->is_volume ? 1 : 3;
    const size_t n = im->n, sb = median_scratch_bytes(n, K), ob = (size_t)K * C * 8, o_pad = (ob + 255) & ~(size_t)255;
    if (im->tex_aux.ensure(o_pad + sb)) return -1;
    double *d_out = im->tex_aux.as<double>();
    int sps = im->ctx->begin(PG_STATS);
    if (launch_segment_median(im->tex_resp.p, IMSEGM_F64, C, 1, n, n, im->labels.as<int32_t>(), K, MedianNorm{ 1, mul, div },
                              im->tex_aux.as<unsigned char>() + o_pad, sb, d_out, st))
        return -1;
    im->ctx->end(sps);
    HIP_TRY(hipMemcpyAsync(median_out, d_out, ob, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

int imsegm_image2d_response_mean_gradient(imsegm_image2d *im, double mul, double div, double *mean_out)
{
    if (!im || bind(im->ctx)) return -1;
    if (response_for_stats(im, mul, div, mean_out, "response_mean_gradient")) return -1;
    if (im->H < 2 || im->W < 2) {
        set_error("Shape of array too small to calculate a numerical gradient, at least (edge_order + 1) elements are required.");
        return -1;
    }
    hipStream_t st = im->ctx->stream;
    const int K = im->n_labels;
    const size_t nv = im->is_volume ? im->n : 3 * im->n;
    if (im->tex_aux.ensure(nv * 8 + 64)) return -1;
    int sps = im->ctx->begin(PG_STATS);
    // every plane (channel / slice) on its own, never across them
    if (launch_gradient_image(im->tex_resp.p, im->tex_aux.p, IMSEGM_F64, im->is_volume ? im->D : 3, im->H, im->W, 1, st,
                              MedianNorm{ 1, mul, div }))
        return -1;
    im->ctx->end(sps);
    // |v| <= mul (|r| <= norm = div)  =>  |gradient along y + along x| <= 2 mul; 4 mul leaves room for the rounding
    const double maxabs = 4.0 * mul;
    std::vector<double> m((size_t)K * 3);
    int rc;
    if (im->is_volume) {
        const int keepH = im->H;
        im->H = im->D * keepH;
        rc = stats_run(im, im->tex_aux.p, IMSEGM_F64, maxabs, 1, 0, 1.0, 1.0, m.data(), nullptr, nullptr, 0);
        im->H = keepH;
        if (!rc)
            for (int k = 0; k < K; ++k) mean_out[k] = m[(size_t)k * 3];
    } else {
        rc = stats_run(im, im->tex_aux.p, IMSEGM_F64, maxabs, 1, 0, 1.0, 1.0, m.data(), nullptr, nullptr);
        if (!rc) memcpy(mean_out, m.data(), (size_t)K * 3 * 8);
    }
    return rc;
}

int imsegm_image2d_get_response(imsegm_image2d *im, double *planes_out)
{
    if (!im || bind(im->ctx)) return -1;
    const size_t nv = im->is_volume ? im->n : 3 * im->n;
    if (im->tex_resp.cap < nv * 8) {
        set_error("no filter response");
        return -1;
    }
    HIP_TRY(hipMemcpyAsync(planes_out, im->tex_resp.p, nv * 8, hipMemcpyDeviceToHost, im->ctx->stream));
    HIP_TRY(hipStreamSynchronize(im->ctx->stream));
    return 0;
}


}  // extern "C"
