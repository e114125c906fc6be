"""The class models with a PCA or a Bayesian mixture (tests/reduced_model_cases.py) on the CPU: that the 80-bit reference sees every
step the device has to take -- a row of ``components_.T``, the centring term, the whitening scale, the Bayesian constants, an input
column of the last 64-column block --, that scikit-learn's own fp64 deviation from it is the recorded one (the device tolerance is
16 x that figure), and that ``_hip.DeviceGmm`` accepts these models and carries scikit-learn's own intermediate values.  No GPU."""
import numpy as np
import pytest

import reduced_model_cases as R

pytestmark = pytest.mark.skipif(not R.LONGDOUBLE_OK, reason=R.LONGDOUBLE_REASON)

ALL_CASES = R.CASES + [R.WIDE_CASE] + R.BAYES_CASES
PCA_CASES = [case for case in ALL_CASES if R.model_steps(R.build(case)[0])[1] is not None and case[3] < 1000]


def moved(model, table, ref):
    return float(np.abs(R.reference_proba(model, table) - ref).max())


def test_longdouble_digamma_agrees_with_scipy():
    from scipy.special import digamma
    x = np.concatenate([np.linspace(0.01, 30, 500), [0.5, 1., 33.7, 100., 1e4]])
    want = digamma(x)
    keep = np.abs(want) > 1e-2                  # (relative: away from the root at 1.4616)
    assert np.max(np.abs(R.digamma_ld(x).astype(np.float64) - want)[keep] / np.abs(want[keep])) <= 1e-15
    assert abs(float(R.digamma_ld(1.0)[0]) + 0.5772156649015329) <= 1e-16


@pytest.mark.parametrize('case', ALL_CASES, ids=R.case_id)
def test_most_rows_are_undecided(case):
    _, _, ref = R.case_data(case)
    assert np.allclose(ref.sum(axis=1).astype(np.float64), 1., atol=1e-15)
    assert R.undecided_share(ref) >= 0.7


@pytest.mark.parametrize('case', ALL_CASES, ids=R.case_id)
def test_fp64_sensitivity_is_the_recorded_one(case):
    model, table, ref = R.case_data(case)
    got = float(np.abs(model.predict_proba(table) - ref).max())
    recorded = R.PROBA_DEVIATION[R.case_id(case)]
    print('%s: scikit-learn against longdouble %.3e (recorded %.3e)' % (R.case_id(case), got, recorded))
    assert 0.5 * recorded <= got <= 2 * recorded


@pytest.mark.parametrize('case', PCA_CASES, ids=R.case_id)
def test_every_step_of_the_projection_moves_the_reference(case):
    model, table, ref = R.case_data(case)
    pca = R.model_steps(model)[1]
    inputs = pca.components_.shape[1]
    last_block = 64 * ((inputs - 1) // 64)
    tol = R.proba_tolerance(case)
    found = {}
    for row in sorted({0, last_block, inputs - 1}):
        found['row %d of components_.T' % row] = moved(R.with_zeroed_component_row(model, row), table, ref)
    found['shift'] = float(np.abs(R.reference_proba(model, table, drop_shift=True) - ref).max())
    if pca.whiten:
        found['whitening scale'] = float(np.abs(R.reference_proba(model, table, drop_scale=True) - ref).max())
    found['input %d' % last_block] = moved(model, R.knocked_out(model, table, last_block), ref)
    for what, by in found.items():
        assert by > 1e-3 and by > 1e6 * tol, (what, by)


@pytest.mark.parametrize('case', R.BAYES_CASES, ids=R.case_id)
def test_the_bayesian_constants_move_the_reference(case):
    model, table, ref = R.case_data(case)
    by = float(np.abs(R.reference_proba(model, table, drop_bayes=True) - ref).max())
    assert by > 1e-3 and by > 1e6 * R.proba_tolerance(case)


@pytest.mark.parametrize('case', ALL_CASES, ids=R.case_id)
def test_device_model_is_built_with_the_values_of_scikit_learn(case):
    """fails before the device evaluated these models: DeviceGmm raised TypeError for a PCA step and for a Bayesian mixture"""
    from sklearn.mixture import BayesianGaussianMixture
    from sklearn.mixture._gaussian_mixture import _estimate_log_gaussian_prob
    from pyimsegm_amd import _hip
    model, table, _ = R.case_data(case)
    scaler, pca, mix = R.model_steps(model)
    gmm = _hip.DeviceGmm(model)
    n_comp, n_feat = mix.means_.shape
    inputs = pca.components_.shape[1] if pca is not None else n_feat
    assert (gmm.n_inputs, gmm.n_features, gmm.n_classes) == (inputs, n_feat, n_comp) and table.shape[1] == inputs
    par = gmm.params
    assert (par.n_features, par.n_classes, par.n_inputs) == (n_feat, n_comp, inputs if pca is not None else 0)
    assert gmm.prec_chol.shape == (n_comp, n_feat, n_feat) and gmm.mu_proj.shape == (n_comp, n_feat)
    assert gmm.log_det.shape == gmm.log_weights.shape == (n_comp, )
    if scaler is None:
        assert gmm.scaler_mean is None and gmm.scaler_scale is None and not par.scaler_mean and not par.scaler_scale
    else:
        assert np.array_equal(gmm.scaler_mean, scaler.mean_) and np.array_equal(gmm.scaler_scale, scaler.scale_)
        assert gmm.scaler_mean.shape == (inputs, )
    if pca is None:
        assert gmm.pca_components_t is None and not par.pca_components_t and not par.pca_shift and not par.pca_scale
    else:
        assert gmm.pca_components_t.shape == (inputs, n_feat) and gmm.pca_components_t.flags.c_contiguous
        assert np.array_equal(gmm.pca_components_t, pca.components_.T)
        assert gmm.pca_shift.shape == (n_feat, )
        assert np.array_equal(gmm.pca_shift, (pca.mean_.reshape(1, -1) @ pca.components_.T)[0])
        if pca.whiten:
            assert np.array_equal(gmm.pca_scale, np.sqrt(pca.explained_variance_)) and par.pca_scale
        else:
            assert gmm.pca_scale is None and not par.pca_scale
        # scikit-learn's transform is those three arrays applied in its order (to rounding: BLAS adds up a product with a
        # transposed view in another order than one with its contiguous copy)
        front = table if scaler is None else scaler.transform(table)
        mine = front @ gmm.pca_components_t - gmm.pca_shift
        if pca.whiten:
            mine = mine / gmm.pca_scale
        assert np.allclose(mine, pca.transform(front), rtol=1e-11, atol=1e-11)
    if isinstance(mix, BayesianGaussianMixture):
        assert np.array_equal(gmm.log_weights, mix._estimate_log_weights())
        rows = R.reduced_rows(model, table).astype(np.float64)
        extra = mix._estimate_log_prob(rows) - _estimate_log_gaussian_prob(rows, mix.means_, mix.precisions_cholesky_, 'full')
        want = np.median(extra, axis=0)
        assert np.allclose(gmm.bayes_log_prob_const, want, rtol=1e-9, atol=1e-9)
        plain = np.sum(np.log(gmm.prec_chol.reshape(n_comp, -1)[:, ::n_feat + 1]), 1)
        assert np.array_equal(gmm.log_det, plain + gmm.bayes_log_prob_const)
    else:
        assert gmm.bayes_log_prob_const is None and np.array_equal(gmm.log_weights, np.log(mix.weights_))


def test_device_model_still_refuses_what_the_device_does_not_evaluate():
    from sklearn.decomposition import PCA
    from sklearn.pipeline import Pipeline
    from pyimsegm_amd import _hip
    model, _, _ = R.case_data(R.CASES[1])
    scaler, pca, mix = R.model_steps(model)
    for steps in ([pca, scaler, mix], [scaler, pca, pca, mix], [scaler, scaler, mix]):
        with pytest.raises(TypeError):
            _hip.DeviceGmm(Pipeline([('s%d' % i, st) for i, st in enumerate(steps)]))
    wrong = PCA(n_components=3)
    wrong.components_, wrong.mean_, wrong.explained_variance_ = np.eye(3, 9), np.zeros(9), np.ones(3)
    with pytest.raises(TypeError):
        _hip.DeviceGmm(Pipeline([('p', wrong), ('m', mix)]))           # (three columns out, the mixture works on two)
    import copy
    diag = copy.deepcopy(mix)
    diag.covariance_type = 'diag'
    with pytest.raises(TypeError):
        _hip.DeviceGmm(Pipeline([('p', pca), ('m', diag)]))


def test_fitted_models_of_estim_class_model_are_accepted():
    """the two model shapes ``estim_class_model`` builds from ``pca_coef`` and ``estim_model='BGM'``, fitted on a small table"""
    from pyimsegm_amd import _hip
    from pyimsegm_amd.graph_cuts import estim_class_model
    rng = np.random.RandomState(3)
    table = np.concatenate([rng.standard_normal((60, 9)) * np.linspace(0.2, 3, 9) + shift for shift in (0., 2.5, -3.)])
    np.random.seed(0)
    reduced = estim_class_model(table, 3, 'GMM', pca_coef=0.95, max_iter=9)
    gmm = _hip.DeviceGmm(reduced)
    assert gmm.n_inputs == 9 and 1 <= gmm.n_features < 9
    np.random.seed(0)
    bayes = estim_class_model(table, 3, 'BGM', max_iter=9)
    gmm = _hip.DeviceGmm(bayes)
    assert gmm.n_inputs == gmm.n_features == 9 and gmm.bayes_log_prob_const is not None
    for model in (reduced, bayes):
        ref = R.reference_proba(model, table)
        assert np.abs(model.predict_proba(table) - ref).max() <= 1e-9
