#!/usr/bin/env python
"""Golden vectors of the reference's `imsegm/ellipse_fitting.py` -- `EllipseModelSegm.estimate`, `.criterion`, `.residuals` per
RANSAC trial and the answer of the UNCHANGED `ransac_segm` -- from a run of the reference module under the build container's conda
Python 3.9 with the real scikit-image 0.18.3 and its scipy (build container: /opt/conda/bin/python3.9
tests/golden/make_golden_ellipse.py, through `_reference_env.ReferenceEnv` like the other generators).

Inputs are the seeded cases of tests/ellipse_cases.py; only numbers are stored, plus the seed and the CRC32 of the inputs.  Per
case: the sampled indices of every trial (the `np.random.choice` calls `ransac_segm` makes under the stored seed), the reference's
params and success flag, its criterion, its |residuals| per (trial, point), and the final (params, inliers) of `ransac_segm`.

Per (trial, point) pair the generator also finds, in long double, the minimum of the distance in the basin of scikit-image's
starting parameter t0 = arctan2(y - yc, x - xc) - theta (a dense grid over the circle, downhill from t0, then eight zooms) and the
minimum over the whole circle, and asserts that the two agree: the basin of t0 holds the closest point of the whole ellipse.  A
pair whose `leastsq` residual is more than MARK above or below that minimum is MARKED (leastsq stopped outside the basin
minimum -- a point near the centre of a long ellipse) and left out of residual comparisons.

Conditions asserted per case, so that a test cannot hide a failure (the generator re-seeds until they hold; they concern the
reference alone):

* no reference residual lies within 1e-3 of the residual threshold;
* any two criterion values that decide an update (`fit < best_fit` taken or refused) are exactly equal or differ by more than
  1e-9 relative;
* no centre lies within 1e-6 of the inside test's boundary value 1, for any successful trial;
* at most 2 % of the pairs are marked;
* the winning trial and the kept mask do not change when the marked pairs' residuals are replaced by the basin minimum, and they
  are what `ransac_segm` returned.

`<case>_residual_tol` = 10 x max |leastsq residual - basin minimum| over the unmarked pairs (floor 1e-9)."""
import os
import sys

import numpy as np

from _reference_env import HERE, ROOT, ReferenceEnv

sys.path.insert(0, os.path.join(ROOT, 'tests'))
GRID = 1 << 14
MARK = 1e-4
LD = np.longdouble


def distance_ld(t, point, params):
    xc, yc, a, b, theta = (LD(v) for v in params)
    xt = xc + a * np.cos(theta) * np.cos(t) - b * np.sin(theta) * np.sin(t)
    yt = yc + a * np.sin(theta) * np.cos(t) + b * np.cos(theta) * np.sin(t)
    return np.sqrt((LD(point[0]) - xt) ** 2 + (LD(point[1]) - yt) ** 2)


def zoom(t_mid, width, point, params):
    for _ in range(8):
        t = t_mid + np.linspace(-width, width, 65, dtype=LD)
        t_mid, width = t[np.argmin(distance_ld(t, point, params))], width / 16
    return distance_ld(t_mid, point, params)


def basin_and_global_minimum(point, params):
    grid = np.arange(GRID, dtype=LD) * (2 * LD(np.pi) / GRID)
    dist = distance_ld(grid, point, params)
    t0 = np.arctan2(point[1] - params[1], point[0] - params[0]) - params[4]
    start = int(np.round(float(t0) / (2 * np.pi) * GRID)) % GRID
    rolled = np.roll(dist, -start)                                # rolled[0] is the grid point at t0
    if rolled[1] < rolled[0]:
        steps = int(np.argmax(np.diff(np.concatenate([rolled, rolled[:1]])) >= 0))
    elif rolled[-1] < rolled[0]:
        steps = -int(np.argmax(np.diff(np.concatenate([rolled[:1], rolled[::-1]])) >= 0))   # leftwards: rolled[0], [-1], [-2], ...
    else:
        steps = 0
    cell = 2 * LD(np.pi) / GRID
    basin = zoom(grid[(start + steps) % GRID], cell, point, params)
    whole = zoom(grid[int(np.argmin(dist))], cell, point, params)
    return basin, whole


def run_case(ref, C, name, seed):
    """the arrays of one case, or the name of the condition that failed"""
    inputs = C.golden_inputs(name, seed)
    points, points_all = inputs['points'], inputs['points_all']
    args = (points_all, inputs['weights'], inputs['labels'], C.TABLE_PROB)
    nb_samples = int(C.MIN_SAMPLES * len(points))
    np.random.seed(seed)
    samples = np.array([np.random.choice(len(points), nb_samples, replace=False) for _ in range(C.MAX_TRIALS)])
    params, success = np.zeros((C.MAX_TRIALS, 5)), np.zeros(C.MAX_TRIALS, dtype=bool)
    criterion, residuals = np.full(C.MAX_TRIALS, np.nan), np.full((C.MAX_TRIALS, len(points)), np.nan)
    basin = np.full((C.MAX_TRIALS, len(points)), np.nan)
    for t in range(C.MAX_TRIALS):
        model = ref.EllipseModelSegm()
        success[t] = bool(model.estimate(points[samples[t]]))
        if not success[t]:
            continue
        params[t] = model.params
        criterion[t] = model.criterion(*args)
        residuals[t] = np.abs(model.residuals(points))
        if np.abs(C.inside(points_all.astype(np.float64), params[t])[1] - 1).min() <= 1e-6:
            return 'a centre on the boundary of the inside test'
        for p in range(len(points)):
            both = basin_and_global_minimum(points[p], params[t])
            assert abs(both[0] - both[1]) <= 1e-12 * max(1, both[1]), ('basin minimum is not the closest point', name, seed, t, p, both)
            basin[t, p] = float(both[0])
    if not success.any():
        return 'no successful trial'
    if np.nanmin(np.abs(residuals - C.RESIDUAL_THRESHOLD)) <= 1e-3:
        return 'a residual at the threshold'
    best_fit = np.inf
    for t in np.nonzero(success)[0]:
        if np.isfinite(best_fit) and criterion[t] != best_fit and abs(criterion[t] - best_fit) <= 1e-9 * max(abs(criterion[t]), abs(best_fit)):
            return 'a near tie of the criterion'
        best_fit = min(best_fit, criterion[t])
    marked = success[:, None] & ~(np.abs(residuals - basin) <= MARK)
    if marked.sum() > C.MARKED_CAP * success.sum() * len(points):
        return 'more than 2 % marked pairs'
    with np.errstate(invalid='ignore'):
        decided = C.update_rule(success, criterion, residuals < C.RESIDUAL_THRESHOLD)
        repaired = np.where(marked, basin, residuals)
        if decided != C.update_rule(success, criterion, repaired < C.RESIDUAL_THRESHOLD):
            return 'the answer depends on a marked pair'
        if decided[1] >= 0 and not np.array_equal(residuals[decided[1]] < C.RESIDUAL_THRESHOLD, repaired[decided[1]] < C.RESIDUAL_THRESHOLD):
            return 'the kept mask depends on a marked pair'
    np.random.seed(seed)
    model, inliers = ref.ransac_segm(points, ref.EllipseModelSegm, *args, C.MIN_SAMPLES, C.RESIDUAL_THRESHOLD, max_trials=C.MAX_TRIALS)
    assert decided[0] >= 0 and decided[1] >= 0 and np.array_equal(inliers, residuals[decided[1]] < C.RESIDUAL_THRESHOLD), decided
    compared = success[:, None] & ~marked
    spread = float(np.abs(residuals - basin)[compared].max())
    print(name, 'seed', seed, 'trials ok', int(success.sum()), 'marked', int(marked.sum()), 'spread', spread, 'best/kept', decided,
          'final', np.round(model.params, 3))
    return {'seed': seed, 'crc': C.input_crc(inputs), 'samples': samples, 'params': params, 'success': success, 'criterion': criterion,
            'residuals': residuals, 'basin': basin, 'marked': marked, 'residual_tol': max(10 * spread, 1e-9), 'best': decided[0],
            'kept': decided[1], 'final_params': np.array(model.params), 'final_inliers': np.asarray(inliers)}


def doctest_data(ref, C, out):
    """inputs of the reference's doctests that its drawing and scikit-image helpers produce (ellipse_fitting.py:51-59, :196-208)"""
    from imsegm.utilities.drawing import ellipse_perimeter
    rr, cc = ellipse_perimeter(20, 30, 12, 16, np.deg2rad(30))
    out['doctest_perimeter'] = np.array([rr, cc]).T
    seg = ref.add_overlap_ellipse(np.zeros((120, 150), dtype=int), (60, 75, 40, 65, np.deg2rad(30)), 1)
    slic, points_all, labels = ref.get_slic_points_labels(seg, slic_size=10, slic_regul=0.3)
    out['doctest_points'] = np.array(ref.prepare_boundary_points_ray_dist(seg, [(40, 90)], 2, sel_bg=1, sel_fg=0)[0])
    out['doctest_points_all'], out['doctest_labels'], out['doctest_weights'] = points_all, labels, np.bincount(slic.ravel())
    # points on the line x = 0: a zero column in the scatter matrix of the linear part, a singular matrix in every LAPACK
    out['collinear_success'] = np.array([bool(ref.EllipseModelSegm().estimate(C.COLLINEAR[i:i + 6])) for i in range(6)])


def main():
    with ReferenceEnv() as env:
        if not hasattr(np, 'int'):
            np.int = int
        import imsegm.ellipse_fitting as ref
        import ellipse_cases as C
        out = {'versions': env.versions}
        for name in C.GOLDEN_CASES:
            for seed in range(100):
                case = run_case(ref, C, name, seed)
                if isinstance(case, dict):
                    break
                print(name, 'seed', seed, 'rejected:', case)
            else:
                raise SystemExit('no seed of %s meets the conditions' % name)
            out.update({'%s_%s' % (name, key): np.asarray(value) for key, value in case.items()})
        doctest_data(ref, C, out)
    target = os.path.join(HERE, 'ellipse.npz')
    np.savez_compressed(target, **out)
    print(target, os.path.getsize(target), 'bytes')


if __name__ == '__main__':
    main()
