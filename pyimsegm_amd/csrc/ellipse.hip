// ellipse.hip -- scoring of the RANSAC trials of imsegm/ellipse_fitting.py ransac_segm (:228-254) for all trials of all egg
// candidates of an image at once: the region criterion of EllipseModelSegm.criterion (:121-139), the point-to-ellipse distances of
// skimage's EllipseModel.residuals, and the update rule that picks the winning trial.  All fp64, sums in a fixed order, no
// floating-point atomics: the same call gives the same bytes.  The numpy statement of the same three definitions is
// pyimsegm_amd/ellipse_fitting.py (on='host').
#include "ellipse.h"

#include <math.h>

namespace imsegm {

constexpr int EC_THREADS = 256;                      // k_ellipse_criterion: four waves per trial
constexpr int ER_ITERATIONS = 128;                   // cap of the closest-point iteration (bisection alone needs 53 halvings)

// One workgroup per trial: sum of value[n] over the centres n inside the trial's ellipse.  Thread i adds centres i, i + 256, ... in
// that order (an outside centre adds 0.0), the 64 partial sums of a wave meet in a butterfly, the four waves in one expression:
// the tree depends on n_all alone, so two trials that enclose the same centres get the same bytes.
__global__ __launch_bounds__(EC_THREADS) void k_ellipse_criterion(const double *__restrict__ params, const uint8_t *__restrict__ ok,
                                                                  const double2 *__restrict__ points_all,
                                                                  const double *__restrict__ value, int n_all,
                                                                  double *__restrict__ criterion)
{
    __shared__ double part[EC_THREADS / 64];
    const int t = blockIdx.x;
    if (!ok[t]) {                                    // (uniform over the workgroup)
        if (threadIdx.x == 0) criterion[t] = __longlong_as_double(0x7ff8000000000000ll);
        return;
    }
    const double r_org = params[5 * t], c_org = params[5 * t + 1], r_rad = params[5 * t + 2], c_rad = params[5 * t + 3];
    const double phi = params[5 * t + 4];
    const double sin_phi = sin(phi), cos_phi = cos(phi);
    double acc = 0.0;
    for (int n = threadIdx.x; n < n_all; n += EC_THREADS) {
        const double2 pos = points_all[n];
        const double r = pos.x - r_org, c = pos.y - c_org;
        // the reference's expression, operation by operation (the library is built with -ffp-contract=off); a zero or NaN radius
        // gives inf / NaN and a comparison that is false, as in numpy
        const double q1 = (r * cos_phi + c * sin_phi) / r_rad, q2 = (r * sin_phi - c * cos_phi) / c_rad;
        const double dist_1 = q1 * q1, dist_2 = q2 * q2;
        acc += (dist_1 + dist_2 <= 1.0) ? value[n] : 0.0;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) criterion[t] = (part[0] + part[1]) + (part[2] + part[3]);
}

// Distance of (x, y) to the closest point of the ellipse (xc, yc, a, b, theta) in the basin of the reference's starting parameter
// t0 = atan2(y - yc, x - xc) - theta.  In the ellipse's own frame t0 is the polar angle of the point, so it lies in the point's
// quadrant; there d/dt of the squared distance,
//     g(t) = a u sin t - b v cos t + (b^2 - a^2) sin t cos t        (u, v: the point in the ellipse's frame),
// is <= 0 at the quadrant's start, >= 0 at its end and has one sign change, at the closest point of the whole ellipse.  Folded into
// the first quadrant (|u|, |v|, |a|, |b|) that is a root bracketed by [0, pi/2]: Newton steps from the folded t0, replaced by a
// bisection whenever the step leaves the bracket, the slope is not positive or the step does not halve the one before.  The loop
// is capped; NaN parameters make every comparison false and end it at once with a NaN distance.
__device__ __forceinline__ double ellipse_distance(double x, double y, double xc, double yc, double a, double b, double theta)
{
    const double ctheta = cos(theta), stheta = sin(theta);
    const double dx = x - xc, dy = y - yc;
    const double u = fabs(dx * ctheta + dy * stheta), v = fabs(dy * ctheta - dx * stheta);
    a = fabs(a);
    b = fabs(b);
    const double A = a * u, B = b * v, C = b * b - a * a;
    double lo = 0.0, hi = 1.5707963267948966, t = atan2(v, u), before = hi;
    for (int it = 0; it < ER_ITERATIONS; ++it) {
        const double s = sin(t), c = cos(t);
        const double g = A * s - B * c + C * s * c;
        const double dg = A * c + B * s + C * (c * c - s * s);
        // a stationary point with a negative slope is the maximum at one end of the quadrant (a point on an axis): walk off it
        const double sign = (g == 0.0 && dg < 0.0) ? (t < 0.7853981633974483 ? -1.0 : 1.0) : g;
        if (sign < 0.0)
            lo = t;
        else if (sign > 0.0)
            hi = t;
        else
            break;                                   // the root itself, a flat g (circle centre) or NaN
        const double step = g / dg;
        double next = t - step;
        if (dg > 0.0 && next >= lo && next <= hi && fabs(step + step) <= fabs(before)) {
            before = step;
        } else {
            next = 0.5 * (lo + hi);
            before = hi - lo;
        }
        if (next == t) break;                        // converged (or the bracket has closed)
        t = next;
    }
    const double ex = u - a * cos(t), ey = v - b * sin(t);
    return sqrt(ex * ex + ey * ey);
}

// One lane per (trial, point) pair of the trial's own egg: blockIdx.x is the trial, blockIdx.y the 64-point chunk of its egg.
__global__ __launch_bounds__(64) void k_ellipse_residuals(const double *__restrict__ params, const uint8_t *__restrict__ ok,
                                                          const int32_t *__restrict__ trial_egg, const int32_t *__restrict__ point_off,
                                                          const long long *__restrict__ pair_off, const double2 *__restrict__ points,
                                                          double threshold, double *__restrict__ residuals,
                                                          uint8_t *__restrict__ inliers)
{
    const int t = blockIdx.x;
    const int egg = trial_egg[t];
    const int first = point_off[egg], count = point_off[egg + 1] - first;
    const int p = blockIdx.y * 64 + threadIdx.x;
    if (p >= count) return;
    const long long at = pair_off[t] + p;
    if (!ok[t]) {
        residuals[at] = __longlong_as_double(0x7ff8000000000000ll);
        inliers[at] = 0;
        return;
    }
    const double2 pos = points[first + p];
    const double d = ellipse_distance(pos.x, pos.y, params[5 * t], params[5 * t + 1], params[5 * t + 2], params[5 * t + 3],
                                      params[5 * t + 4]);
    residuals[at] = d;
    inliers[at] = fabs(d) < threshold;               // NaN: false, as in numpy
}

// One wave per egg walks the egg's trials in order with the reference's update rule (:247-254): a failed trial is skipped; a
// criterion below the best so far replaces the model; only then a larger inlier count replaces the kept mask.
__global__ __launch_bounds__(64) void k_ellipse_select(const int32_t *__restrict__ trial_off, const int32_t *__restrict__ point_off,
                                                       const long long *__restrict__ pair_off, const uint8_t *__restrict__ ok,
                                                       const double *__restrict__ criterion, const uint8_t *__restrict__ inliers,
                                                       int32_t *__restrict__ best_out, int32_t *__restrict__ kept_out,
                                                       uint8_t *__restrict__ mask_out)
{
    const int egg = blockIdx.x, lane = threadIdx.x;
    const int t0 = trial_off[egg], t1 = trial_off[egg + 1];
    const int first = point_off[egg], count = point_off[egg + 1] - first;
    double best_fit = __longlong_as_double(0x7ff0000000000000ll);
    int best = -1, kept = -1, best_count = 0;
    for (int t = t0; t < t1; ++t) {                  // (every condition below is uniform over the wave)
        if (!ok[t]) continue;
        const double fit = criterion[t];
        if (!(fit < best_fit)) continue;
        best = t - t0;
        best_fit = fit;
        const uint8_t *row = inliers + pair_off[t];
        int n = 0;
        for (int p = lane; p < count; p += 64) n += row[p];
        n = wave_sum_i32(n);
        if (n > best_count) {
            kept = t - t0;
            best_count = n;
        }
    }
    const uint8_t *row = inliers + pair_off[kept >= 0 ? t0 + kept : 0];
    for (int p = lane; p < count; p += 64) mask_out[first + p] = kept >= 0 ? row[p] : 0;
    if (lane == 0) {
        best_out[egg] = best;
        kept_out[egg] = kept;
    }
}

int launch_ellipse_criterion(const EllipseJob &job, hipStream_t st)
{
    hipLaunchKernelGGL(k_ellipse_criterion, job.n_trials, EC_THREADS, 0, st, job.params, job.ok,
                       reinterpret_cast<const double2 *>(job.points_all), job.value, job.n_all, job.criterion);
    HIP_TRY(hipGetLastError());
    return 0;
}

int launch_ellipse_residuals(const EllipseJob &job, hipStream_t st)
{
    hipLaunchKernelGGL(k_ellipse_residuals, dim3(job.n_trials, cdiv(job.max_points, 64)), 64, 0, st, job.params, job.ok, job.trial_egg,
                       job.point_off, job.pair_off, reinterpret_cast<const double2 *>(job.points), job.threshold, job.residuals,
                       job.inliers);
    HIP_TRY(hipGetLastError());
    return 0;
}

int launch_ellipse_select(const EllipseJob &job, hipStream_t st)
{
    hipLaunchKernelGGL(k_ellipse_select, job.n_eggs, 64, 0, st, job.trial_off, job.point_off, job.pair_off, job.ok, job.criterion,
                       job.inliers, job.best, job.kept, job.mask);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // namespace imsegm
