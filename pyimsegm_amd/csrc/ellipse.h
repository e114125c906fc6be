// ellipse.h -- launchers of csrc/ellipse.hip (RANSAC scoring of ellipse trials; the C ABI is in api_ellipse.hip)
#pragma once
#include "common.h"

namespace imsegm {

// Trials are numbered over all eggs, an egg's trials next to each other: egg e owns trials [trial_off[e], trial_off[e + 1]) and
// points [point_off[e], point_off[e + 1]).  The (trial, point) pairs of trial t start at pair_off[t]; a trial has one pair per point
// of its own egg.
struct EllipseJob {
    int n_eggs, n_trials, n_all, max_points;       // max_points: the longest point list of an egg
    const int32_t *point_off, *trial_off, *trial_egg;
    const long long *pair_off;
    const double *points;                          // [P_total][2]
    const double *params;                          // [n_trials][5]: xc, yc, a, b, theta
    const uint8_t *ok;                             // [n_trials]: the estimate of the trial succeeded
    const double *points_all, *value;              // [n_all][2], [n_all]
    double threshold;
    double *criterion;                             // [n_trials] (NaN for a failed trial)
    double *residuals;                             // [pairs] (NaN for a failed trial)
    uint8_t *inliers;                              // [pairs]
    int32_t *best, *kept;                          // [n_eggs]: index among the egg's own trials, or -1
    uint8_t *mask;                                 // [P_total]
};

int launch_ellipse_criterion(const EllipseJob &job, hipStream_t st);
int launch_ellipse_residuals(const EllipseJob &job, hipStream_t st);
int launch_ellipse_select(const EllipseJob &job, hipStream_t st);

}  // namespace imsegm
