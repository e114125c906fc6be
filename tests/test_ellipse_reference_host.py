"""``pyimsegm_amd.ellipse_fitting`` on the host against tests/golden/ellipse.npz (the reference's ``imsegm/ellipse_fitting.py`` itself
under scikit-image 0.18.3; generator, conditions and tolerances: tests/golden/make_golden_ellipse.py, tests/ellipse_cases.py): the
direct fit, the region criterion, the basin-constrained point-to-ellipse distances and ``ransac_segm(on='host')`` end to end, the
reference's doctest vectors, its errors, and the import without scikit-image.  No GPU."""
import doctest
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

import ellipse_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'ellipse.npz')


@pytest.fixture(scope='module')
def golden():
    return np.load(GOLDEN)


@pytest.fixture(scope='module')
def ell():
    from pyimsegm_amd import ellipse_fitting
    return ellipse_fitting


@pytest.fixture(scope='module')
def cases(golden):
    """the regenerated inputs of the golden cases (CRC checked), computed once"""
    found = {}
    for name in C.GOLDEN_CASES:
        found[name] = C.golden_inputs(name, int(golden[name + '_seed']))
        assert C.input_crc(found[name]) == int(golden[name + '_crc']), 'the seeded inputs of %s drifted' % name
    return found


def test_doctest_vectors(ell, golden):
    examples = importlib.import_module('tests.doctests.ellipse_fitting').EXAMPLES
    parser, runner = doctest.DocTestParser(), doctest.DocTestRunner(verbose=False)
    for name, text in examples.items():
        runner.run(parser.get_doctest(text, dict(ell.__dict__, golden=golden), 'ellipse_fitting.' + name, ell.__name__, 0))
    result = runner.summarize(verbose=False)
    assert result.failed == 0 and result.attempted >= 20


@pytest.mark.parametrize('name', C.GOLDEN_CASES)
def test_estimate(ell, golden, cases, name):
    points, samples = cases[name]['points'], golden[name + '_samples']
    params, success = ell.estimate_stack(points[samples])
    assert np.array_equal(success, golden[name + '_success'])
    want = golden[name + '_params']
    rdiff = np.max(np.abs(params - want)[success] / np.abs(want)[success])
    print(name, 'estimate: largest relative difference', rdiff)
    assert rdiff <= C.ESTIMATE_RTOL
    for t in (0, len(samples) - 1):                            # one sample set alone is the stack of one: the same bytes
        model = ell.EllipseModelSegm()
        assert model.estimate(points[samples[t]]) == bool(success[t])
        assert not success[t] or model.params == params[t].tolist()


@pytest.mark.parametrize('name', C.GOLDEN_CASES)
def test_criterion(ell, golden, cases, name):
    inputs, params = cases[name], golden[name + '_params']
    value = ell.point_values(inputs['points_all'], inputs['weights'], inputs['labels'], C.TABLE_PROB)
    score = ell.score_trials_host([0, len(inputs['points'])], inputs['points'], params, golden[name + '_success'],
                                  np.zeros(len(params), dtype=np.int32), inputs['points_all'], value, C.RESIDUAL_THRESHOLD)
    for t in np.nonzero(golden[name + '_success'])[0]:
        model = ell.EllipseModelSegm()
        model.params = params[t].tolist()
        scale = np.abs(value[C.inside(inputs['points_all'].astype(np.float64), params[t])[0]]).sum()
        for got in (model.criterion(inputs['points_all'], inputs['weights'], inputs['labels'], C.TABLE_PROB), score[3][t]):
            assert abs(got - golden[name + '_criterion'][t]) <= C.CRITERION_RTOL * scale, (name, t)


@pytest.mark.parametrize('name', C.GOLDEN_CASES)
def test_residuals(ell, golden, cases, name):
    points, params, success = cases[name]['points'], golden[name + '_params'], golden[name + '_success']
    marked, tol = golden[name + '_marked'], float(golden[name + '_residual_tol'])
    assert marked.sum() <= C.MARKED_CAP * success.sum() * len(points)
    got = ell.ellipse_distances(points[None, :, :], params[:, None, :])
    compared = success[:, None] & ~marked
    diff = np.abs(got - golden[name + '_residuals'])[compared].max()
    print(name, 'residuals: largest difference', diff, 'allowed', tol, 'marked pairs', int(marked.sum()))
    assert diff <= tol
    model = ell.EllipseModelSegm()
    model.params = params[np.nonzero(success)[0][0]].tolist()
    assert np.array_equal(model.residuals(points), got[np.nonzero(success)[0][0]])


@pytest.mark.parametrize('name', C.GOLDEN_CASES)
def test_ransac_on_host_end_to_end(ell, golden, cases, name):
    inputs, seed = cases[name], int(golden[name + '_seed'])
    np.random.seed(seed)
    details = {}
    model, inliers = ell.ransac_segm_batch([inputs['points']], inputs['points_all'], inputs['weights'], inputs['labels'], C.TABLE_PROB,
                                           C.MIN_SAMPLES, C.RESIDUAL_THRESHOLD, C.MAX_TRIALS, on='host', _details=details)[0]
    assert np.array_equal(details['samples'][0], golden[name + '_samples'])
    assert (details['best'][0], details['kept'][0]) == (int(golden[name + '_best']), int(golden[name + '_kept']))
    assert inliers.dtype == bool and np.array_equal(inliers, golden[name + '_final_inliers'])
    want = golden[name + '_final_params']
    assert np.max(np.abs(np.array(model.params) - want) / np.abs(want)) <= C.ESTIMATE_RTOL
    np.random.seed(seed)
    again, same = ell.ransac_segm(inputs['points'], ell.EllipseModelSegm, inputs['points_all'], inputs['weights'], inputs['labels'],
                                  C.TABLE_PROB, C.MIN_SAMPLES, C.RESIDUAL_THRESHOLD, C.MAX_TRIALS, on='host')
    assert again.params == model.params and np.array_equal(same, inliers)


def test_other_model_class_runs_the_plain_loop(ell, golden, cases):
    """a model class of the caller's is fitted trial by trial on the host, on the same random stream"""
    inputs, seed = cases['round'], int(golden['round_seed'])

    class Mine(ell.EllipseModelSegm):
        pass

    args = (inputs['points_all'], inputs['weights'], inputs['labels'], C.TABLE_PROB, C.MIN_SAMPLES, C.RESIDUAL_THRESHOLD, C.MAX_TRIALS)
    np.random.seed(seed)
    model, inliers = ell.ransac_segm(inputs['points'], Mine, *args)
    after = np.random.random()
    np.random.seed(seed)
    want, want_inliers = ell.ransac_segm(inputs['points'], ell.EllipseModelSegm, *args, on='host')
    assert after == np.random.random()
    assert isinstance(model, Mine) and model.params == want.params and np.array_equal(inliers, want_inliers)


def test_errors(ell, golden):
    model = ell.EllipseModelSegm()
    model.params = [4, 7, 3, 6, 0.2]
    points = np.array([[1, 2], [3, 4], [5, 6]])
    with pytest.raises(ValueError, match='different sizes'):
        model.criterion(points, np.ones(2), np.zeros(3, dtype=int))
    with pytest.raises(ValueError, match='table shape'):
        model.criterion(points, np.ones(3), np.zeros(3, dtype=int), np.ones((3, 2)) / 2)
    with pytest.raises(ValueError, match='exceed the table'):
        model.criterion(points, np.ones(3), np.array([0, 2, 1]), [[0.1, 0.9], [0.9, 0.1]])
    args = (golden['doctest_points_all'], golden['doctest_weights'], golden['doctest_labels'], [0.01, 0.75, 0.95, 0.9])
    for klass in (ell.EllipseModelSegm, dict):
        with pytest.raises(ValueError, match='ration'):
            ell.ransac_segm(C.COLLINEAR, klass, *args, 1.5, on='host')
        with pytest.raises(ValueError, match='nb-samples'):
            ell.ransac_segm(C.COLLINEAR, klass, *args, 13, on='host')
        with pytest.raises(ValueError, match='max_trials'):
            ell.ransac_segm(C.COLLINEAR, klass, *args, 6, max_trials=-1, on='host')
    with pytest.raises(ValueError, match="'host' or 'device'"):
        ell.ransac_segm(C.COLLINEAR, ell.EllipseModelSegm, *args, 6, on='gpu')


def test_no_successful_trial(ell, golden):
    assert not golden['collinear_success'].any()                  # the reference fails on these points as well
    assert not ell.estimate_stack(np.stack([C.COLLINEAR[i:i + 6] for i in range(6)]))[1].any()
    args = (golden['doctest_points_all'], golden['doctest_weights'], golden['doctest_labels'], [0.01, 0.75, 0.95, 0.9])
    assert ell.ransac_segm(C.COLLINEAR, ell.EllipseModelSegm, *args, 6, 3, max_trials=15, on='host') == (None, None)
    assert ell.ransac_segm(C.COLLINEAR, ell.EllipseModelSegm, *args, 6, 3, max_trials=0, on='host') == (None, None)


def test_degenerate_parameters_end(ell):
    """zero radii (what nan_to_num leaves of a failed square root) and NaN: finite loops, distances as numpy compares them"""
    points = np.array([[3., 4.], [0., 0.], [10., 0.], [0., 7.]])
    flat = ell.ellipse_distances(points, np.array([0., 0., 0., 5., 0.]))          # the segment x = 0, |y| <= 5
    assert np.allclose(flat, [3., 0., 10., 2.], atol=1e-12)
    dot = ell.ellipse_distances(points, np.array([0., 0., 0., 0., 0.3]))
    assert np.allclose(dot, [5., 0., 10., 7.], atol=1e-12)
    assert np.isnan(ell.ellipse_distances(points, np.array([0., 0., np.nan, 5., 0.]))).all()
    inside = ell.inside_ellipses(points, np.array([[0., 0., 0., 5., 0.], [0., 0., np.nan, 5., 0.]]))
    assert not inside.any()
    on_curve = ell.ellipse_distances(np.array([[20., 0.], [0., 0.], [0., 5.]]), np.array([0., 0., 20., 5., 0.]))
    assert np.allclose(on_curve, [0., 5., 0.], atol=1e-12)              # on the ellipse, at its centre, on the minor axis


def test_imports_without_scikit_image():
    code = ("import sys; sys.modules['skimage'] = None; sys.path.insert(0, %r); import pyimsegm_amd.ellipse_fitting as e; "
            "import numpy as np; m = e.EllipseModelSegm(); "
            "assert m.estimate(m.predict_xy(np.linspace(0, 6, 9), (5, 6, 3, 2, 0.3))); assert 'skimage.measure' not in sys.modules" % ROOT)
    assert subprocess.run([sys.executable, '-c', code], cwd=ROOT).returncode == 0
