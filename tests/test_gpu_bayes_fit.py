"""The variational fit of the Bayesian mixture on the device (``fit_on='device'`` with ``estim_model='BGM'``: csrc/mixture_fit.hip
through ``_hip.bayes_mixture_em`` and ``graph_cuts.fit_bayes_mixture_device``) against scikit-learn on the CPU driven from the same
start (tests/bayes_fit_cases.py), its determinism, its fall-backs and the pipelines that take the keyword."""
import itertools
import logging

import numpy as np
import pytest

import bayes_fit_cases as BC
import mixture_fit_cases as MC

pytestmark = pytest.mark.gpu

CASES = [(name, prior_type) for name in BC.CASES for prior_type in BC.CASES[name][2]]

#: share of pixels on which two HOST fits of the 'BGM' model under ``np.random.seed(1)`` and ``np.random.seed(2)`` give the same
#: class map up to a permutation of the classes, measured on the GPU box with ``fit_on='host'`` on the inputs of
#: test_pipelines_with_device_fit
HOST_FITS_AGREE_IMAGE = 1.0
HOST_FITS_AGREE_VOLUME = 1.0

_CACHE = {}


def case(name):
    """table, scikit-learn's Lloyd labels of the restarts"""
    if name not in _CACHE:
        table = BC.load_table(name)
        _CACHE[name] = (table, BC.labels_of(name, table))
    return _CACHE[name]


def reference(name, prior_type, tol, max_iter):
    key = (name, prior_type, tol, max_iter)
    if key not in _CACHE:
        table, labels = case(name)
        _CACHE[key] = [BC.reference_bayes_em(table, lab, tol, max_iter, prior_type, n_components=BC.CASES[name][0]) for lab in labels]
    return _CACHE[key]


def priors_of(table, n_components, prior_type):
    """scikit-learn's own default priors for the table"""
    bgm = BC.estimator(n_components, prior_type)
    bgm._check_parameters(table)
    return (prior_type, bgm.weight_concentration_prior_, bgm.mean_precision_prior_, bgm.mean_prior_, bgm.degrees_of_freedom_prior_,
            bgm.covariance_prior_)


def device_fit(name, prior_type, labels=None, **kwargs):
    """the variational fit on the device on the table of ``name`` from host labels (any number of restarts)"""
    from pyimsegm_amd import _hip
    table, all_labels = case(name)
    labels = np.atleast_2d(all_labels if labels is None else labels)
    n_components = BC.CASES[name][0]
    _hip.kmeans_lloyd(table, table[None, :n_components], 1, 0., want_labels=False)          # (uploads the table)
    return _hip.bayes_mixture_em(len(labels), n_components, table.shape[1], *priors_of(table, n_components, prior_type),
                                 labels=labels, **kwargs)


def restart_of(fit, r):
    return {key: fit[key][r] for key in fit}


def assert_close_to_reference(name, fit, refs, what):
    for r, ref in enumerate(refs):
        assert not ref['failed'] and not fit['not_pd'][r], (name, what, r)
        dev = BC.deviation(restart_of(fit, r), ref)
        print('%s %s restart %d: deviation %.3g (tolerance %.3g)' % (name, what, r, dev, BC.BAYES_TOLERANCE[name]))
        assert dev <= BC.BAYES_TOLERANCE[name], (name, what, r, dev)


@pytest.mark.parametrize('name,prior_type', CASES)
def test_iteration_for_iteration(name, prior_type):
    for max_iter in (20, 1):             # (one iteration: the plans of estim_class_model with max_iter = 1)
        refs = reference(name, prior_type, 0., max_iter)
        fit = device_fit(name, prior_type, tol=0., max_iter=max_iter)
        assert fit['n_iter'].tolist() == [max_iter] * len(refs) and not fit['converged'].any()
        assert_close_to_reference(name, fit, refs, '%s tol=0 max_iter=%d' % (prior_type, max_iter))


@pytest.mark.parametrize('name', BC.GOLDEN_TABLES)
def test_stopping_rule(name):
    refs = reference(name, BC.PROCESS, 1e-3, 99)
    for ref in refs:                     # the inputs qualify: no decision of the reference is within 1e-6 of the threshold
        bounds = [-np.inf] + ref['bounds']
        for i in range(1, len(bounds)):
            assert abs(abs(bounds[i] - bounds[i - 1]) - 1e-3) > 1e-6
    fit = device_fit(name, BC.PROCESS, tol=1e-3, max_iter=99)
    assert fit['n_iter'].tolist() == [ref['n_iter'] for ref in refs]
    assert fit['converged'].tolist() == [ref['converged'] for ref in refs]
    assert_close_to_reference(name, fit, refs, 'tol=1e-3 max_iter=99')


def same_bytes(fit_a, fit_b, rows_a=slice(None), rows_b=slice(None)):
    return all(np.asarray(fit_a[key][rows_a]).tobytes() == np.asarray(fit_b[key][rows_b]).tobytes() for key in fit_a)


@pytest.mark.parametrize('name', ('reference_c5', 'dying'))
def test_determinism(name):
    from pyimsegm_amd import _hip
    table, labels = case(name)
    n_components = BC.CASES[name][0]
    for prior_type in BC.CASES[name][2]:
        fit = device_fit(name, prior_type, tol=1e-3, max_iter=99)
        assert same_bytes(fit, device_fit(name, prior_type, tol=1e-3, max_iter=99))
        for r in range(len(labels)):
            alone = device_fit(name, prior_type, labels[r], tol=1e-3, max_iter=99)
            assert same_bytes(alone, fit, slice(None), slice(r, r + 1)), r
            if fit['converged'][r]:          # frozen at its iteration: what a run of exactly that many iterations gives
                short = device_fit(name, prior_type, labels[r], tol=1e-3, max_iter=int(fit['n_iter'][r]))
                assert same_bytes(short, fit, slice(None), slice(r, r + 1)), r
        # another entry dirties the scratch of the context: Lloyd and EM of the plain mixture with other restarts
        seeds = MC.seeds_of(table, 11, 5, n_components)
        _hip.kmeans_lloyd(table, seeds, 300, 0.)
        _hip.mixture_em(5, n_components, table.shape[1], tol=0., max_iter=3)
        assert same_bytes(fit, device_fit(name, prior_type, tol=1e-3, max_iter=99))
        # one more iteration of scikit-learn from the device's state after five agrees with the device's six
        five = device_fit(name, prior_type, tol=0., max_iter=5)
        six = device_fit(name, prior_type, tol=0., max_iter=6)
        for r in range(len(labels)):
            bgm = BC.estimator(n_components, prior_type)
            bgm._check_parameters(table)
            concentration = five['weight_concentration'][r]
            concentration = (concentration[0], concentration[1]) if prior_type == BC.PROCESS else concentration[0]
            bgm._set_parameters((concentration, ) + tuple(five[key][r] for key in BC.PARAMETERS[1:]))
            log_prob_norm, log_resp = bgm._e_step(table)
            bgm._m_step(table, log_resp)
            step = BC.as_run(bgm._get_parameters())
            step['lower_bound'] = bgm._compute_lower_bound(log_resp, log_prob_norm)
            assert BC.deviation(restart_of(six, r), step) <= BC.BAYES_TOLERANCE[name], (prior_type, r)


def host_restatement(features, n_classes, random_state, max_iter=99):
    """seeds -> KMeans(init=seeds) -> variational loop, best of the restarts, all scikit-learn"""
    from sklearn.preprocessing import StandardScaler
    table = np.ascontiguousarray(StandardScaler().fit_transform(np.asarray(features, dtype=np.float64)))
    seeds = MC.seeds_of(table, random_state, max(1, int(np.sqrt(max_iter))), n_classes)
    labels = MC.reference_lloyd(table, seeds)[0]
    runs = [BC.reference_bayes_em(table, lab, 1e-3, max_iter, BC.PROCESS, n_components=n_classes) for lab in labels]
    return max(run['lower_bound'] for run in runs if not run['failed'])


FITTED = ('weight_concentration_', 'mean_precision_', 'means_', 'degrees_of_freedom_', 'covariances_', 'precisions_cholesky_',
          'weights_', 'precisions_')


def fitted_bytes(mixture):
    return b''.join(np.asarray(getattr(mixture, attribute)).tobytes() for attribute in FITTED)


@pytest.mark.parametrize('name', BC.GOLDEN_TABLES)
def test_whole_fit(name, caplog):
    from sklearn.mixture import BayesianGaussianMixture
    from sklearn.pipeline import Pipeline
    from pyimsegm_amd import graph_cuts
    file_name, key = {'reference_2048': ('reference_2048.npz', 'features'), 'reference_c5': ('reference_c5.npz', 'normed'),
                      'plan_features': ('class_models.npz', 'plan_features')}[name]
    features = np.asarray(np.load(MC.GOLDEN + '/' + file_name)[key], dtype=np.float64)
    np.random.seed(MC.SEED)                      # (estim_class_model leaves random_state at None: numpy's global stream)
    with caplog.at_level(logging.INFO):
        model = graph_cuts.estim_class_model(features, 3, 'BGM', fit_on='device')
    assert not any('on the host' in record.getMessage() for record in caplog.records)
    assert isinstance(model, Pipeline) and type(model.steps[-1][1]) is BayesianGaussianMixture
    mixture = model.steps[-1][1]
    assert all(hasattr(mixture, attribute) for attribute in FITTED + ('converged_', 'n_iter_', 'lower_bound_'))
    assert mixture.converged_ and mixture.n_features_in_ == features.shape[1] and mixture.weights_.shape == (3, )
    assert np.abs(graph_cuts.predict_proba(model, features) - model.predict_proba(features)).max() <= 1e-9
    np.random.seed(MC.SEED)
    reference = host_restatement(features, 3, np.random.mtrand._rand)
    print(name, 'lower bound', mixture.lower_bound_, 'host restatement', reference)
    assert abs(mixture.lower_bound_ - reference) / (1 + abs(reference)) <= BC.BAYES_TOLERANCE[name]
    np.random.seed(MC.SEED)
    again = graph_cuts.estim_class_model(features, 3, 'BGM', fit_on='device').steps[-1][1]
    assert fitted_bytes(again) == fitted_bytes(mixture)
    # behind a PCA the fit still runs on the device, on the reduced table
    np.random.seed(MC.SEED)
    with caplog.at_level(logging.INFO):
        caplog.clear()
        reduced = graph_cuts.estim_class_model(features, 3, 'BGM', pca_coef=0.95, fit_on='device')
    assert not any('on the host' in record.getMessage() for record in caplog.records)
    assert reduced.steps[-1][1].means_.shape[1] == reduced.steps[-2][1].n_components_
    assert np.abs(graph_cuts.predict_proba(reduced, features) - reduced.predict_proba(features)).max() <= 1e-9


def test_fall_backs_and_errors(caplog):
    from sklearn.mixture import BayesianGaussianMixture
    from pyimsegm_amd import _hip, graph_cuts

    def both(table, n_components, n_init=2):
        host = BayesianGaussianMixture(n_components=n_components, n_init=n_init, random_state=np.random.RandomState(11))
        graph_cuts.fit_mixture_restarts(host, table)
        device = BayesianGaussianMixture(n_components=n_components, n_init=n_init, random_state=np.random.RandomState(11))
        with caplog.at_level(logging.INFO):
            caplog.clear()
            graph_cuts.fit_bayes_mixture_device(device, table)
        assert fitted_bytes(host) == fitted_bytes(device)
        return ' '.join(record.getMessage() for record in caplog.records if record.levelno == logging.INFO)

    # fewer distinct rows than classes: a cluster stays empty, the device says so and the host path takes the fit -- which for
    # this table is scikit-learn's error (its covariance prior, the table's covariance, is singular), from the device call too
    few = np.repeat(np.array([[0., 0.], [1., 1.]]), 30, axis=0)
    assert _hip.kmeans_lloyd(few, few[None, [0, 30, 1]], 10, 0.)['empty'].tolist() == [True]
    with pytest.raises(ValueError, match='ill-defined empirical covariance'):
        graph_cuts.fit_mixture_restarts(BayesianGaussianMixture(n_components=3, n_init=2, random_state=np.random.RandomState(5)), few)
    with caplog.at_level(logging.INFO):
        caplog.clear()
        with pytest.raises(ValueError, match='ill-defined empirical covariance'):
            graph_cuts.fit_bayes_mixture_device(BayesianGaussianMixture(n_components=3, n_init=2, random_state=np.random.RandomState(5)), few)
        assert any('empty' in record.getMessage() for record in caplog.records)
    # the same in one column, where two distinct values have a regular covariance: the host fit's model, byte for byte
    assert 'empty' in both(few[:, :1], 3)
    # nine components: beyond the caps, from the entry itself and through graph_cuts
    table, labels = case('caps_edge')
    _hip.kmeans_lloyd(table, table[None, :8], 1, 0., want_labels=False)
    with pytest.raises(_hip.HipFitCapsError):
        _hip.bayes_mixture_em(2, 9, 16, *priors_of(table, 9, BC.PROCESS), labels=labels, tol=0., max_iter=2)
    assert 'caps' in both(table, 9)
    bad = np.random.RandomState(3).standard_normal((50, 3))
    bad[7, 1] = np.nan
    with pytest.raises(ValueError):
        graph_cuts.estim_class_model(bad, 3, 'BGM', use_scaler=False, fit_on='device')


def agreement(segm_a, segm_b, n_classes):
    """share of pixels with the same class up to the best permutation of the classes"""
    return max(np.mean(np.asarray(order)[segm_a] == segm_b) for order in itertools.permutations(range(n_classes)))


def test_pipelines_with_device_fit():
    from pyimsegm_amd import pipelines
    from pyimsegm_amd.utilities.synthetic import ellipsoid_volume, voronoi_image
    image = voronoi_image(256, 256, nb_seeds=12, seed=3)
    features = {'color': ['mean', 'std']}

    def image_segm(seed, fit_on):
        np.random.seed(seed)
        return pipelines.pipe_color2d_slic_features_model_graphcut(image, 3, features, sp_size=12, estim_model='BGM', fit_on=fit_on)

    host, _ = image_segm(1, 'host')
    segm, soft = image_segm(1, 'device')
    assert segm.shape == (256, 256) and soft.shape == (256, 256, 3) and soft.dtype == np.float64
    assert segm.dtype == host.dtype and set(np.unique(segm)) <= set(range(3))
    share = agreement(host, segm, 3)
    print('image: device fit agrees with the host fit on', share, '; host fits of seeds 1 and 2 on',
          agreement(host, image_segm(2, 'host')[0], 3))
    assert share >= HOST_FITS_AGREE_IMAGE - 0.01
    volume = ellipsoid_volume((16, 64, 64))

    def volume_segm(seed, fit_on):
        np.random.seed(seed)
        return np.asarray(pipelines.pipe_gray3d_slic_features_model_graphcut(volume, 3, {'color': ['mean']}, spacing=(2, 1, 1), sp_size=6,
                                                                             estim_model='BGM', fit_on=fit_on))

    host = volume_segm(1, 'host')
    segm = volume_segm(1, 'device')
    assert segm.shape == volume.shape and segm.dtype == host.dtype and set(np.unique(segm)) <= set(range(3))
    share = agreement(host, segm, 3)
    print('volume: device fit agrees with the host fit on', share, '; host fits of seeds 1 and 2 on',
          agreement(host, volume_segm(2, 'host'), 3))
    assert share >= HOST_FITS_AGREE_VOLUME - 0.01
