"""Seeded inputs the tests of ``pyimsegm_amd.ellipse_fitting`` share with tests/golden/make_golden_ellipse.py, and the tolerances
of the comparisons with tests/golden/ellipse.npz.

A golden case is one egg candidate: a class map (the Voronoi classes 0-2 of ``synthetic.voronoi_image`` with a known ellipse of
class 3 painted in), superpixel-like centres on a jittered grid with the class under each of them, region sizes as weights, and
boundary points: perimeter points of the known ellipse with Gaussian noise, plus outliers -- a few of them near the centre.  The
fixture stores the seed the generator settled on (it re-seeds until the conditions of its docstring hold) and the CRC32 of the
inputs.

Tolerances ("Ellipse RANSAC"):

* residuals: the fixture's ``<case>_residual_tol`` = 10 x the largest |leastsq residual - basin minimum| over the compared pairs of
  the case (floor 1e-9 absolute): the spread of where scipy's ``leastsq`` stops, which is not restated;
* criterion: 1e-12 relative to the sum of |value| over the centres inside (fp64, a few thousand terms, another order);
* estimate: ``ESTIMATE_RTOL`` -- the fit is ill-conditioned without centring of the data, so two LAPACK builds do not agree to the
  last digits.  Measured against the fixture with this repository's numpy (OpenBLAS): largest relative difference 6.4e-12 (case
  ``long``; ``round`` 4.2e-12); asserted: 100 x that, or 1e-6, whichever is larger.
"""
import zlib

import numpy as np

GOLDEN_CASES = ('round', 'long')
#: name: (true ellipse r, c, r_rad, c_rad, phi), boundary points on the perimeter, outliers, noise of the perimeter points
SHAPES = {'round': ((62., 80., 34., 46., 0.5), 44, 10, 0.6), 'long': ((64., 78., 14., 58., -0.3), 56, 12, 0.5)}
HEIGHT, WIDTH, STEP = 128, 160, 8
TABLE_PROB = [[0.01, 0.3, 0.2, 0.95], [0.99, 0.7, 0.8, 0.05]]
MIN_SAMPLES, RESIDUAL_THRESHOLD, MAX_TRIALS = 0.35, 3., 40
MEASURED_ESTIMATE_RDIFF = 6.4e-12
ESTIMATE_RTOL = max(100 * MEASURED_ESTIMATE_RDIFF, 1e-6)
CRITERION_RTOL = 1e-12
MARKED_CAP = 0.02
#: points on the line x = 0: a zero column in the scatter matrix of the linear part, which every LAPACK reports as singular (on
#: another line the pivots are zero only up to the rounding of the factorisation at hand) -- every estimate fails
COLLINEAR = np.stack([np.zeros(12), np.arange(12.)], axis=1)


def crc(*arrays):
    value = 0
    for arr in arrays:
        value = zlib.crc32(np.ascontiguousarray(arr).tobytes(), value)
    return value


def inside(points, params):
    """the inside test of the region criterion and the value it compares with 1"""
    r_org, c_org, r_rad, c_rad, phi = params
    r, c = points[:, 0] - r_org, points[:, 1] - c_org
    with np.errstate(all='ignore'):
        value = ((r * np.cos(phi) + c * np.sin(phi)) / r_rad) ** 2 + ((r * np.sin(phi) - c * np.cos(phi)) / c_rad) ** 2
    return value <= 1, value


def perimeter(params, angles):
    """points (r, c) of the ellipse at the parameter angles, in the convention of ``EllipseModel.predict_xy``"""
    xc, yc, a, b, theta = params
    return np.stack([xc + a * np.cos(theta) * np.cos(angles) - b * np.sin(theta) * np.sin(angles),
                     yc + a * np.sin(theta) * np.cos(angles) + b * np.cos(theta) * np.sin(angles)], axis=1)


def golden_inputs(name, seed):
    """the inputs of one golden case under one seed: dict of points [P, 2], points_all [N, 2] (int), labels [N], weights [N]"""
    from pyimsegm_amd.utilities.synthetic import voronoi_image
    true, nb_perimeter, nb_outliers, noise = SHAPES[name]
    rng = np.random.default_rng(seed)
    classes = voronoi_image(HEIGHT, WIDTH, nb_seeds=10, seed=seed, return_classes=True)[1]
    rows, cols = np.mgrid[:HEIGHT, :WIDTH]
    egg = inside(np.stack([rows.ravel(), cols.ravel()], axis=1).astype(np.float64), true)[0].reshape(HEIGHT, WIDTH)
    classes = np.where(egg, 3, classes)
    grid = np.stack(np.meshgrid(np.arange(STEP // 2, HEIGHT, STEP), np.arange(STEP // 2, WIDTH, STEP), indexing='ij'), axis=-1)
    points_all = grid.reshape(-1, 2) + rng.integers(-2, 3, (grid.shape[0] * grid.shape[1], 2))
    labels = classes[points_all[:, 0], points_all[:, 1]]
    weights = rng.integers(40, 90, len(points_all))
    # the perimeter in the criterion's convention (r_rad along phi): the same curve as predict_xy's with these five numbers
    on_curve = perimeter(true, np.sort(rng.uniform(0, 2 * np.pi, nb_perimeter))) + rng.normal(0, noise, (nb_perimeter, 2))
    far = np.stack([rng.uniform(10, HEIGHT - 10, nb_outliers), rng.uniform(10, WIDTH - 10, nb_outliers)], axis=1)
    far[:3] = np.array(true[:2]) + rng.normal(0, 2.5, (3, 2))                  # near the centre: where leastsq may leave the basin
    points = np.round(np.concatenate([on_curve, far]), 3)
    return {'points': points[rng.permutation(len(points))], 'points_all': points_all, 'labels': labels, 'weights': weights}


def input_crc(inputs):
    return crc(inputs['points'], inputs['points_all'].astype(np.int64), inputs['labels'].astype(np.int64),
               inputs['weights'].astype(np.int64))


def update_rule(success, criterion, inliers):
    """the reference's update rule over the trials in order: (best trial, kept trial), -1 for none"""
    best, kept, best_fit, best_count = -1, -1, np.inf, 0
    for t in range(len(success)):
        if not success[t] or not criterion[t] < best_fit:
            continue
        best, best_fit = t, criterion[t]
        if inliers[t].sum() > best_count:
            kept, best_count = t, inliers[t].sum()
    return best, kept


# ---- shapes of the device tests ------------------------------------------------------------------------------------------------
def random_ellipses(rng, count, centre=(60., 70.), spread=15.):
    return np.stack([centre[0] + rng.normal(0, spread, count), centre[1] + rng.normal(0, spread, count), rng.uniform(5, 45, count),
                     rng.uniform(5, 45, count), rng.uniform(-np.pi, np.pi, count)], axis=1)


def device_job(seed, trials_per_egg, points_per_egg, n_all, failed=()):
    """a scoring job with ragged eggs: random ellipses as trials (no estimate involved), random points and centres with values
    of both signs; ``failed``: eggs whose trials all carry the failure flag"""
    rng = np.random.default_rng(seed)
    offsets = np.concatenate([[0], np.cumsum(points_per_egg)]).astype(np.int32)
    points = np.stack([rng.uniform(0, 120, offsets[-1]), rng.uniform(0, 140, offsets[-1])], axis=1)
    params = random_ellipses(rng, int(np.sum(trials_per_egg)))
    trial_egg = np.repeat(np.arange(len(trials_per_egg), dtype=np.int32), trials_per_egg)
    success = (rng.uniform(size=len(params)) > 0.1).astype(np.uint8)
    success[np.isin(trial_egg, list(failed))] = 0
    points_all = rng.integers(0, 140, (n_all, 2)).astype(np.float64)
    value = rng.integers(40, 90, n_all) * rng.choice([-4.5, 1.2, 2.9], n_all)
    return dict(point_offsets=offsets, points=points, params=params, success=success, trial_egg=trial_egg, points_all=points_all,
                point_value=value, residual_threshold=6.)
