// api_ellipse.hip -- C ABI of the RANSAC scoring of ellipse trials (imsegm/ellipse_fitting.py ransac_segm): a stateless call on a
// context and host arrays.  Arguments are checked before the device is touched -- every index the kernels form comes from the
// offsets checked here; the kernels are in ellipse.hip.  Behind it the last step of the ellipse methods, add_overlap_ellipse: fitted
// ellipses into a label map, and the label histogram under every ellipse (kernels in ellipse_place.hip); every box the kernels walk
// is checked against the map here.
#include "ellipse.h"
#include "ellipse_place.h"
#include "session.h"

#include <cmath>
#include <vector>

static_assert(ELLIPSE_PLACE_LABELS == IMSEGM_ELLIPSE_PLACE_LABELS, "LDS budget of ellipse_place.hip");

namespace imsegm {

// the arguments the calls that walk ellipse boxes share (ellipse_place.h)
int check_ellipses(const char *who, const void *segm, int H, int W, int n, const int32_t *geom, const double *sincos, int *max_box_rows)
{
    const std::string name(who);
    if (H < 1 || W < 1 || H > ELLIPSE_PLACE_MAX_COORD || W > ELLIPSE_PLACE_MAX_COORD || (long long)H * W >= (1ll << 31)) {
        set_error(name + ": height and width must be positive and the map smaller than 2^31 pixels");
        return -1;
    }
    if (!segm || n < 0 || (n > 0 && (!geom || !sincos))) {
        set_error(name + ": null array or a negative number of ellipses");
        return -1;
    }
    *max_box_rows = 0;
    for (int e = 0; e < n; ++e) {
        const int32_t *g = geom + (size_t)e * ELLIPSE_GEOM_INTS;
        if (g[2] < 1 || g[3] < 1 || g[2] > ELLIPSE_PLACE_MAX_COORD || g[3] > ELLIPSE_PLACE_MAX_COORD ||
            g[0] < -ELLIPSE_PLACE_MAX_COORD || g[0] > ELLIPSE_PLACE_MAX_COORD || g[1] < -ELLIPSE_PLACE_MAX_COORD ||
            g[1] > ELLIPSE_PLACE_MAX_COORD) {
            set_error(name + ": ellipse " + std::to_string(e) + " has a radius below 1 or a centre or radius beyond 2^30");
            return -1;
        }
        if (g[6] < g[4] || g[7] < g[5]) continue;                     // no pixel: the kernels' loops do not run
        if (g[4] < 0 || g[5] < 0 || g[6] >= H || g[7] >= W) {
            set_error(name + ": the box of ellipse " + std::to_string(e) + " is not clipped to the map");
            return -1;
        }
        if (g[6] - g[4] + 1 > *max_box_rows) *max_box_rows = g[6] - g[4] + 1;
    }
    return 0;
}

}  // namespace imsegm

extern "C" {

int imsegm_ellipse_ransac(imsegm_ctx *ctx, int n_eggs, const int32_t *point_offsets, const double *points, int n_trials,
                          const double *params, const uint8_t *success, const int32_t *trial_egg, const double *points_all,
                          const double *point_value, int n_all, double residual_threshold, int32_t *best_out, int32_t *kept_out,
                          uint8_t *mask_out, double *criterion_out, double *residuals_out)
{
    if (!point_offsets || !points || !params || !success || !trial_egg || !points_all || !point_value || !best_out || !kept_out ||
        !mask_out || !criterion_out) {
        set_error("ellipse_ransac: null array");
        return -1;
    }
    if (n_eggs < 1 || n_trials < 1 || n_all < 1) {
        set_error("ellipse_ransac: at least one egg, one trial and one centre are required");
        return -1;
    }
    if (point_offsets[0] != 0) {
        set_error("ellipse_ransac: the point offsets start at 0");
        return -1;
    }
    int max_points = 0;
    for (int e = 0; e < n_eggs; ++e) {
        const long long count = (long long)point_offsets[e + 1] - point_offsets[e];
        if (count < 0) {
            set_error("ellipse_ransac: the point offsets are not monotone");
            return -1;
        }
        if (count < 5) {
            set_error("ellipse_ransac: egg " + std::to_string(e) + " has fewer than 5 points");
            return -1;
        }
        if (count > (1 << 22)) {
            set_error("ellipse_ransac: more than 2^22 points of one egg");
            return -1;
        }
        if (count > max_points) max_points = (int)count;
    }
    const size_t n_points = (size_t)point_offsets[n_eggs];
    std::vector<int32_t> trial_off((size_t)n_eggs + 1, 0);
    std::vector<long long> pair_off((size_t)n_trials + 1, 0);
    for (int t = 0; t < n_trials; ++t) {
        const int e = trial_egg[t];
        if (e < 0 || e >= n_eggs || (t > 0 && e < trial_egg[t - 1])) {
            set_error("ellipse_ransac: the egg of every trial must lie in [0, n_eggs) and not decrease");
            return -1;
        }
        trial_off[(size_t)e + 1] += 1;
        pair_off[(size_t)t + 1] = pair_off[t] + (point_offsets[e + 1] - point_offsets[e]);
    }
    for (int e = 0; e < n_eggs; ++e) trial_off[(size_t)e + 1] += trial_off[e];
    const size_t n_pairs = (size_t)pair_off[n_trials];
    if (n_pairs > ((size_t)1 << 31)) {
        set_error("ellipse_ransac: more than 2^31 (trial, point) pairs");
        return -1;
    }
    if (bind(ctx)) return -1;
    hipStream_t st = ctx->stream;

    size_t at = 0;
    auto take = [&at](size_t bytes) {
        const size_t here = at;
        at += (bytes + 255) & ~(size_t)255;
        return here;
    };
    const size_t o_poff = take(((size_t)n_eggs + 1) * 4), o_toff = take(((size_t)n_eggs + 1) * 4);
    const size_t o_pair = take(((size_t)n_trials + 1) * 8), o_tegg = take((size_t)n_trials * 4), o_ok = take((size_t)n_trials);
    const size_t o_params = take((size_t)n_trials * 40), o_points = take(n_points * 16);
    const size_t o_all = take((size_t)n_all * 16), o_value = take((size_t)n_all * 8);
    const size_t o_crit = take((size_t)n_trials * 8), o_res = take(n_pairs * 8), o_inl = take(n_pairs);
    const size_t o_best = take((size_t)n_eggs * 4), o_kept = take((size_t)n_eggs * 4), o_mask = take(n_points);
    if (ctx->gc_buf.ensure(at)) return -1;
    unsigned char *dev = ctx->gc_buf.as<unsigned char>();
    HIP_TRY(hipMemcpyAsync(dev + o_poff, point_offsets, ((size_t)n_eggs + 1) * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(dev + o_toff, trial_off.data(), ((size_t)n_eggs + 1) * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(dev + o_pair, pair_off.data(), ((size_t)n_trials + 1) * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(dev + o_tegg, trial_egg, (size_t)n_trials * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(dev + o_ok, success, (size_t)n_trials, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(dev + o_params, params, (size_t)n_trials * 40, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(dev + o_points, points, n_points * 16, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(dev + o_all, points_all, (size_t)n_all * 16, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(dev + o_value, point_value, (size_t)n_all * 8, hipMemcpyHostToDevice, st));

    EllipseJob job;
    job.n_eggs = n_eggs;
    job.n_trials = n_trials;
    job.n_all = n_all;
    job.max_points = max_points;
    job.point_off = reinterpret_cast<const int32_t *>(dev + o_poff);
    job.trial_off = reinterpret_cast<const int32_t *>(dev + o_toff);
    job.trial_egg = reinterpret_cast<const int32_t *>(dev + o_tegg);
    job.pair_off = reinterpret_cast<const long long *>(dev + o_pair);
    job.points = reinterpret_cast<const double *>(dev + o_points);
    job.params = reinterpret_cast<const double *>(dev + o_params);
    job.ok = dev + o_ok;
    job.points_all = reinterpret_cast<const double *>(dev + o_all);
    job.value = reinterpret_cast<const double *>(dev + o_value);
    job.threshold = residual_threshold;
    job.criterion = reinterpret_cast<double *>(dev + o_crit);
    job.residuals = reinterpret_cast<double *>(dev + o_res);
    job.inliers = dev + o_inl;
    job.best = reinterpret_cast<int32_t *>(dev + o_best);
    job.kept = reinterpret_cast<int32_t *>(dev + o_kept);
    job.mask = dev + o_mask;
    if (launch_ellipse_criterion(job, st)) return -1;
    if (launch_ellipse_residuals(job, st)) return -1;
    if (launch_ellipse_select(job, st)) return -1;
    HIP_TRY(hipMemcpyAsync(best_out, job.best, (size_t)n_eggs * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(kept_out, job.kept, (size_t)n_eggs * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(mask_out, job.mask, n_points, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(criterion_out, job.criterion, (size_t)n_trials * 8, hipMemcpyDeviceToHost, st));
    if (residuals_out) HIP_TRY(hipMemcpyAsync(residuals_out, job.residuals, n_pairs * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

int imsegm_ellipse_place(imsegm_ctx *ctx, int32_t *segm, int height, int width, int n, const int32_t *geom, const double *sincos,
                         const int32_t *labels, double thr_overlap, uint8_t *placed)
{
    int max_box_rows = 0;
    if (check_ellipses("ellipse_place", segm, height, width, n, geom, sincos, &max_box_rows)) return -1;
    if (n > 0 && (!labels || !placed)) {
        set_error("ellipse_place: null array");
        return -1;
    }
    if (!(thr_overlap >= 0.0)) {
        set_error("ellipse_place: thr_overlap must not be negative or NaN");
        return -1;
    }
    for (int e = 0; e < n; ++e)
        if (labels[e] >= IMSEGM_ELLIPSE_PLACE_LABELS) {
            set_error("ellipse_place: label " + std::to_string(labels[e]) + " has no slot in the label table");
            return -1;
        }
    if (n == 0) return 0;
    if (bind(ctx)) return -1;
    hipStream_t st = ctx->stream;
    const size_t pixels = (size_t)height * width;
    size_t at = 0;
    auto take = [&at](size_t bytes) {
        const size_t here = at;
        at += (bytes + 255) & ~(size_t)255;
        return here;
    };
    const size_t o_segm = take(pixels * 4), o_counts = take((size_t)IMSEGM_ELLIPSE_PLACE_LABELS * 4 + 4);
    const size_t o_geom = take((size_t)n * ELLIPSE_GEOM_INTS * 4), o_sincos = take((size_t)n * 16), o_labels = take((size_t)n * 4);
    const size_t o_placed = take((size_t)n);
    if (ctx->gc_buf.ensure(at)) return -1;
    unsigned char *dev = ctx->gc_buf.as<unsigned char>();
    int32_t *d_segm = reinterpret_cast<int32_t *>(dev + o_segm), *d_counts = reinterpret_cast<int32_t *>(dev + o_counts);
    int32_t *d_beyond = d_counts + IMSEGM_ELLIPSE_PLACE_LABELS;
    HIP_TRY(hipMemcpyAsync(d_segm, segm, pixels * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(dev + o_geom, geom, (size_t)n * ELLIPSE_GEOM_INTS * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(dev + o_sincos, sincos, (size_t)n * 16, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(dev + o_labels, labels, (size_t)n * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(d_counts, 0, (size_t)IMSEGM_ELLIPSE_PLACE_LABELS * 4 + 4, st));
    if (launch_ellipse_label_counts(d_segm, pixels, d_counts, d_beyond, st)) return -1;
    if (launch_ellipse_place(d_segm, width, n, reinterpret_cast<const int32_t *>(dev + o_geom),
                             reinterpret_cast<const double *>(dev + o_sincos), reinterpret_cast<const int32_t *>(dev + o_labels),
                             thr_overlap, d_counts, d_beyond, dev + o_placed, st))
        return -1;
    int32_t beyond = 0;
    HIP_TRY(hipMemcpyAsync(&beyond, d_beyond, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(placed, dev + o_placed, (size_t)n, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (beyond) {
        set_error("ellipse_place: the map holds a value that has no slot in the label table (IMSEGM_ELLIPSE_PLACE_LABELS)");
        return -1;
    }
    // only the rows an ellipse was painted into come back
    int first = height, last = -1;
    for (int e = 0; e < n; ++e) {
        const int32_t *g = geom + (size_t)e * ELLIPSE_GEOM_INTS;
        if (!placed[e]) continue;
        if (g[4] < first) first = g[4];
        if (g[6] > last) last = g[6];
    }
    if (last >= first) {
        const size_t from = (size_t)first * width;
        HIP_TRY(hipMemcpyAsync(segm + from, d_segm + from, (size_t)(last - first + 1) * width * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    return 0;
}

int imsegm_ellipse_overlaps(imsegm_ctx *ctx, const int32_t *segm, int height, int width, int n, const int32_t *geom,
                            const double *sincos, int nb_labels, int64_t *counts, int64_t *areas)
{
    int max_box_rows = 0;
    if (check_ellipses("ellipse_overlaps", segm, height, width, n, geom, sincos, &max_box_rows)) return -1;
    if (nb_labels < 1 || nb_labels > IMSEGM_ELLIPSE_PLACE_LABELS) {
        set_error("ellipse_overlaps: between 1 and IMSEGM_ELLIPSE_PLACE_LABELS labels");
        return -1;
    }
    if (n > 0 && (!counts || !areas)) {
        set_error("ellipse_overlaps: null array");
        return -1;
    }
    if (n == 0) return 0;
    if (bind(ctx)) return -1;
    hipStream_t st = ctx->stream;
    const size_t pixels = (size_t)height * width, table = (size_t)n * nb_labels;
    size_t at = 0;
    auto take = [&at](size_t bytes) {
        const size_t here = at;
        at += (bytes + 255) & ~(size_t)255;
        return here;
    };
    const size_t o_segm = take(pixels * 4), o_geom = take((size_t)n * ELLIPSE_GEOM_INTS * 4), o_sincos = take((size_t)n * 16);
    const size_t o_counts = take(table * 8), o_areas = take((size_t)n * 8);
    if (ctx->gc_buf.ensure(at)) return -1;
    unsigned char *dev = ctx->gc_buf.as<unsigned char>();
    HIP_TRY(hipMemcpyAsync(dev + o_segm, segm, pixels * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(dev + o_geom, geom, (size_t)n * ELLIPSE_GEOM_INTS * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(dev + o_sincos, sincos, (size_t)n * 16, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(dev + o_counts, 0, at - o_counts, st));             // the counts and, behind them, the areas
    if (launch_ellipse_overlaps(reinterpret_cast<const int32_t *>(dev + o_segm), width, n, reinterpret_cast<const int32_t *>(dev + o_geom),
                                reinterpret_cast<const double *>(dev + o_sincos), nb_labels, max_box_rows,
                                reinterpret_cast<long long *>(dev + o_counts), reinterpret_cast<long long *>(dev + o_areas), st))
        return -1;
    HIP_TRY(hipMemcpyAsync(counts, dev + o_counts, table * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(areas, dev + o_areas, (size_t)n * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

}  // extern "C"
