// api_ellipse.hip -- C ABI of the RANSAC scoring of ellipse trials (imsegm/ellipse_fitting.py ransac_segm): a stateless call on a
// context and host arrays.  Arguments are checked before the device is touched -- every index the kernels form comes from the
// offsets checked here; the kernels are in ellipse.hip.
#include "ellipse.h"
#include "session.h"

#include <vector>

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

}  // extern "C"
