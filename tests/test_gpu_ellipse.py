"""``imsegm_ellipse_ransac`` (csrc/ellipse.hip) against the numpy statement of the same definitions
(``pyimsegm_amd.ellipse_fitting.score_trials_host``) on the same inputs, and against tests/golden/ellipse.npz (the reference itself):
criteria, distances, the update rule, ties, degenerate trials, ragged eggs, repeatability, ``ransac_segm`` / ``ransac_segm_batch`` on
the device, and the rejected arguments.

Host against device, both fp64 and the same operations: the distances may differ by the last bits of sin / cos, far below the
1e-9 absolute the comparison allows (the floor of the fixture's tolerance); every job is checked to have no distance within 1e-6
of the threshold and no centre within 1e-9 of the inside test's boundary, so that masks and inside sets must be EQUAL."""
import itertools
import os

import numpy as np
import pytest

import ellipse_cases as C

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'ellipse.npz')
TRIALS, POINTS, CENTRES = (1, 63, 64, 65, 250), (5, 6, 64, 65), (1, 255, 256, 257, 2049)


@pytest.fixture(scope='module')
def hip():
    from pyimsegm_amd import _hip
    _hip.default_context()
    return _hip


@pytest.fixture(scope='module')
def ell(hip):
    from pyimsegm_amd import ellipse_fitting
    return ellipse_fitting


@pytest.fixture(scope='module')
def golden():
    return np.load(GOLDEN)


def run(hip, job):
    return hip.ellipse_ransac(job['point_offsets'], job['points'], job['params'], job['success'], job['trial_egg'], job['points_all'],
                              job['point_value'], job['residual_threshold'], with_residuals=True)


def compare(hip, ell, job, what):
    """device against host on one job; returns the device's results"""
    got = run(hip, job)
    want = ell.score_trials_host(job['point_offsets'], job['points'], job['params'], job['success'], job['trial_egg'], job['points_all'],
                                 job['point_value'], job['residual_threshold'], with_residuals=True)
    ok = job['success'].astype(bool)
    finite = np.isfinite(want[4])
    assert np.abs(np.abs(want[4][finite]) - job['residual_threshold']).min(initial=np.inf) > 1e-6, (what, 'a distance at the threshold: choose another seed')
    inside = ell.inside_ellipses(job['points_all'], job['params'])
    for t in np.nonzero(ok)[0]:
        value = C.inside(job['points_all'], job['params'][t])[1]
        assert not (np.abs(value - 1) <= 1e-9).any(), (what, 'a centre on the boundary: choose another seed')
        scale = np.abs(job['point_value'][inside[t]]).sum()
        assert abs(got[3][t] - want[3][t]) <= C.CRITERION_RTOL * scale, (what, t, got[3][t], want[3][t])
    assert np.isnan(got[3][~ok]).all() and np.array_equal(np.isnan(got[4]), np.isnan(want[4])), what
    assert np.abs(got[4] - want[4])[finite].max(initial=0.) <= 1e-9, (what, np.abs(got[4] - want[4])[finite].max())
    for i, name in enumerate(('best', 'kept', 'mask')):
        assert got[i].dtype == want[i].dtype and np.array_equal(got[i], want[i]), (what, name, got[i], want[i])
    return got


def test_one_egg_every_size(hip, ell):
    # the criterion's shape is (trials, centres), the distances' (trials, points): every pair of each, the third size fixed
    sizes = [(t, p, 257) for t, p in itertools.product(TRIALS, POINTS)] + [(t, 6, n) for t, n in itertools.product(TRIALS, CENTRES)]
    for seed, (trials, points, centres) in enumerate(sizes):
        compare(hip, ell, C.device_job(seed, [trials], [points], centres), (trials, points, centres))


def test_ragged_eggs(hip, ell):
    compare(hip, ell, C.device_job(500, [65, 7, 250], [5, 65, 64], 257), 'three eggs')
    got = compare(hip, ell, C.device_job(501, [64, 63, 1], [6, 64, 65], 2049, failed=(1, )), 'failed egg in the middle')
    assert got[0][1] == -1 and got[1][1] == -1 and not got[2][6:70].any() and got[0][0] >= 0 and got[0][2] >= 0
    got = compare(hip, ell, C.device_job(502, [5, 0, 9], [5, 5, 5], 255), 'an egg without trials')
    assert got[0][1] == -1 and got[1][1] == -1


def special_job():
    rng = np.random.default_rng(77)
    points_all = rng.integers(20, 100, (300, 2)).astype(np.float64)
    value = -rng.integers(40, 90, 300).astype(np.float64) * rng.choice([0.7, 1.2, 2.9], 300)          # all negative
    params = np.array([[60., 60., 30., 20., 0.4],
                       [60., 60., 90., 80., 0.4],        # encloses every centre ...
                       [60., 60., 90., 80., 0.4],        # ... and so does its bit-identical twin ...
                       [61., 59., 95., 85., 0.1],        # ... and this larger one: the same inside set, the same bytes
                       [60., 60., 0., 0., 0.3],          # radii as nan_to_num leaves them: nothing inside, distances to a point
                       [60., 60., 0., 25., 0.3],
                       [60., 60., np.nan, 25., 0.3]])
    on_curve = np.array([60. + 90. * np.cos(0.4), 60. + 90. * np.sin(0.4)])                           # t = 0 of trials 1 and 2
    points = np.concatenate([[on_curve, [60., 60.]], rng.uniform(0, 120, (7, 2))])
    return dict(point_offsets=np.array([0, len(points)], dtype=np.int32), points=points, params=params,
                success=np.ones(len(params), dtype=np.uint8), trial_egg=np.zeros(len(params), dtype=np.int32), points_all=points_all,
                point_value=value, residual_threshold=30.)


def test_ties_degenerate_trials_and_special_points(hip, ell):
    job = special_job()
    best, kept, mask, criterion, residuals = compare(hip, ell, job, 'special')
    assert best[0] == 1                                           # the first of the tie wins (strict <)
    assert criterion[1].tobytes() == criterion[2].tobytes() == criterion[3].tobytes()
    assert abs(criterion[1] - job['point_value'].sum()) <= C.CRITERION_RTOL * -job['point_value'].sum() and criterion[1] < criterion[0] < 0
    assert criterion[4] == 0. and criterion[5] == 0. and criterion[6] == 0.                          # inf / NaN: nothing is inside
    residuals = residuals.reshape(len(job['params']), -1)
    assert residuals[1, 0] <= 1e-12 and abs(residuals[1, 1] - 80.) <= 1e-12                          # on the ellipse; its centre
    assert np.allclose(residuals[4], np.hypot(*(job['points'] - 60.).T), rtol=1e-13, atol=0)
    assert np.isnan(residuals[6]).all() and np.isfinite(residuals[:6]).all()


def test_same_call_same_bytes(hip):
    job = C.device_job(900, [250, 65], [65, 64], 2049)
    first, second = run(hip, job), run(hip, job)
    for a, b in zip(first, second):
        assert a.tobytes() == b.tobytes()


@pytest.mark.parametrize('name', C.GOLDEN_CASES)
def test_against_the_reference(hip, golden, name):
    inputs = C.golden_inputs(name, int(golden[name + '_seed']))
    assert C.input_crc(inputs) == int(golden[name + '_crc'])
    from pyimsegm_amd import ellipse_fitting as ell
    params, success, points = golden[name + '_params'], golden[name + '_success'], inputs['points']
    value = ell.point_values(inputs['points_all'], inputs['weights'], inputs['labels'], C.TABLE_PROB)
    best, kept, mask, criterion, residuals = hip.ellipse_ransac([0, len(points)], points, params, success, np.zeros(len(params), dtype=np.int32),
                                                                inputs['points_all'], value, C.RESIDUAL_THRESHOLD, with_residuals=True)
    for t in np.nonzero(success)[0]:
        scale = np.abs(value[C.inside(inputs['points_all'].astype(np.float64), params[t])[0]]).sum()
        assert abs(criterion[t] - golden[name + '_criterion'][t]) <= C.CRITERION_RTOL * scale, (name, t)
    marked, tol = golden[name + '_marked'], float(golden[name + '_residual_tol'])
    assert marked.sum() <= C.MARKED_CAP * success.sum() * len(points)
    diff = np.abs(residuals.reshape(marked.shape) - golden[name + '_residuals'])[success[:, None] & ~marked].max()
    print(name, 'residuals: largest difference', diff, 'allowed', tol, 'marked pairs', int(marked.sum()))
    assert diff <= tol
    assert (best[0], kept[0]) == (int(golden[name + '_best']), int(golden[name + '_kept']))
    assert np.array_equal(mask.astype(bool), golden[name + '_final_inliers'])


def test_ransac_on_the_device(hip, ell, golden, monkeypatch):
    cases = [C.golden_inputs(name, int(golden[name + '_seed'])) for name in C.GOLDEN_CASES]
    shared = cases[0]
    args = (shared['points_all'], shared['weights'], shared['labels'], C.TABLE_PROB, C.MIN_SAMPLES, C.RESIDUAL_THRESHOLD, C.MAX_TRIALS)
    list_points = [cases[0]['points'], C.COLLINEAR, cases[1]['points'], cases[0]['points'][::-1]]
    np.random.seed(3)
    batch = ell.ransac_segm_batch(list_points, *args)             # no `on`: a device is present
    after = np.random.random()
    np.random.seed(3)
    single = [ell.ransac_segm(points, ell.EllipseModelSegm, *args, on='device') for points in list_points]
    assert after == np.random.random()
    np.random.seed(3)
    host = ell.ransac_segm_batch(list_points, *args, on='host')
    assert batch[1] == (None, None) and batch[0][0] is not None and batch[2][0] is not None
    for one, other, third in zip(batch, single, host):
        for model, inliers in (other, third):
            assert (one[0] is None) == (model is None) and (one[0] is None or one[0].params == model.params)
            assert (one[1] is None) == (inliers is None) and (one[1] is None or np.array_equal(one[1], inliers))
    # the golden case under its own seed: the reference's answer
    name, inputs = C.GOLDEN_CASES[0], cases[0]
    np.random.seed(int(golden[name + '_seed']))
    model, inliers = ell.ransac_segm(inputs['points'], ell.EllipseModelSegm, *args)
    want = golden[name + '_final_params']
    assert np.array_equal(inliers, golden[name + '_final_inliers'])
    assert np.max(np.abs(np.array(model.params) - want) / np.abs(want)) <= C.ESTIMATE_RTOL
    monkeypatch.setenv('IMSEGM_RANSAC_ON', 'host')
    assert ell._place(None) == 'host' and ell._place('device') == 'device'
    monkeypatch.delenv('IMSEGM_RANSAC_ON')
    assert ell._place(None) == 'device'


def test_bad_arguments_leave_the_context_usable(hip, ell):
    good = C.device_job(7, [9, 4], [6, 11], 40)
    bad = [dict(good, params=good['params'][:0], success=good['success'][:0], trial_egg=good['trial_egg'][:0]),       # no trial
           dict(good, point_offsets=np.array([0, 4, 17], dtype=np.int32)),                                            # an egg of 4 points
           dict(good, points_all=good['points_all'][:0], point_value=good['point_value'][:0]),                        # no centre
           dict(good, point_offsets=np.array([0, 12, 6, 17], dtype=np.int32)),                                        # not monotone
           dict(good, trial_egg=np.where(np.arange(13) == 5, 2, good['trial_egg']).astype(np.int32)),                 # an egg that is not there
           dict(good, trial_egg=good['trial_egg'][::-1].copy())]                                                      # decreasing
    for job in bad:
        with pytest.raises(hip.HipError):
            run(hip, job)
        compare(hip, ell, good, 'after a rejected call')
