"""What of the variational fit on the device (``estim_class_model(..., 'BGM', fit_on='device')``) can be checked without a GPU: the
routing with the entry points of ``_hip`` replaced, the refusals on the restored random stream, the default and ``'host'`` bit for
bit, the declaration of the C entry, and the yardstick of the GPU tests against ``BayesianGaussianMixture.fit``."""
import logging
import os
import re

import numpy as np
import pytest

import bayes_fit_cases as BC
import mixture_fit_cases as MC

ATTRIBUTES = ('weight_concentration_', 'mean_precision_', 'means_', 'degrees_of_freedom_', 'covariances_', 'precisions_cholesky_',
              'weights_', 'precisions_')


def fitted_bytes(mixture):
    return b''.join(np.asarray(getattr(mixture, attribute)).tobytes() for attribute in ATTRIBUTES)


class FakeDevice(object):
    """``_hip.kmeans_lloyd`` / ``_hip.bayes_mixture_em`` computed by scikit-learn (tests/bayes_fit_cases.py), and what was asked"""

    def __init__(self, monkeypatch):
        from pyimsegm_amd import _hip
        self.calls = []
        monkeypatch.setattr(_hip, 'default_context', lambda: 'ctx')
        monkeypatch.setattr(_hip, 'kmeans_lloyd', self.kmeans_lloyd)
        monkeypatch.setattr(_hip, 'bayes_mixture_em', self.bayes_mixture_em)
        monkeypatch.setattr(_hip, 'mixture_em', lambda *args, **kwargs: pytest.fail('the plain EM was asked'))

    def kmeans_lloyd(self, table, seeds, max_iter, tol, want_labels=True, ctx=None):
        self.calls.append(('kmeans_lloyd', table.shape, seeds.shape, max_iter, tol))
        self.table, self.labels = table, MC.reference_lloyd(table, seeds)[0]
        return dict(labels=None, empty=np.zeros(len(seeds), dtype=bool))

    def bayes_mixture_em(self, n_restarts, n_components, n_features, prior_type, *priors, **kwargs):
        self.calls.append(('bayes_mixture_em', n_restarts, n_components, n_features, prior_type, priors, kwargs))
        runs = [BC.reference_bayes_em(self.table, lab, kwargs['tol'], kwargs['max_iter'], prior_type, kwargs['reg_covar'], n_components)
                for lab in self.labels]
        fit = {key: np.stack([np.asarray(run[key]) for run in runs]) for key in BC.PARAMETERS + ('lower_bound', 'n_iter', 'converged')}
        fit['not_pd'] = np.zeros(n_restarts, dtype=bool)
        return fit


def test_bgm_on_the_device_reaches_the_bayes_entry(monkeypatch):
    from sklearn.mixture import BayesianGaussianMixture
    from pyimsegm_amd import graph_cuts
    device = FakeDevice(monkeypatch)
    features = np.load(MC.GOLDEN + '/class_models.npz')['plan_features']
    for fit_on in ('device', 'device_wide'):
        del device.calls[:]
        np.random.seed(5)
        model = graph_cuts.estim_class_model(features, 3, 'BGM', fit_on=fit_on)
        assert [call[0] for call in device.calls] == ['kmeans_lloyd', 'bayes_mixture_em']
        assert device.calls[0][1:4] == (features.shape, (9, 3, features.shape[1]), 300)
        table = device.table
        assert device.calls[0][4] == 1e-4 * np.mean(np.var(table, axis=0))
        _, n_restarts, n_components, n_features, prior_type, priors, kwargs = device.calls[1]
        assert (n_restarts, n_components, n_features, prior_type) == (9, 3, features.shape[1], 'dirichlet_process')
        assert kwargs == dict(reg_covar=1e-6, tol=1e-3, max_iter=99, ctx='ctx')
        # the priors are scikit-learn's own for that table
        own = BayesianGaussianMixture(n_components=3)
        own._check_parameters(table)
        assert priors[0] == own.weight_concentration_prior_ and priors[1] == own.mean_precision_prior_
        assert priors[3] == own.degrees_of_freedom_prior_
        assert np.array_equal(priors[2], own.mean_prior_) and np.array_equal(priors[4], own.covariance_prior_)
        # the winner (first largest bound) in the ordinary estimator, weights_ and precisions_ from scikit-learn's arithmetic
        mixture = model.steps[-1][1]
        assert type(mixture) is BayesianGaussianMixture and all(hasattr(mixture, attribute) for attribute in ATTRIBUTES)
        runs = [BC.reference_bayes_em(table, lab, 1e-3, 99, 'dirichlet_process') for lab in device.labels]
        best = runs[int(np.argmax([run['lower_bound'] for run in runs]))]
        assert mixture.lower_bound_ == best['lower_bound'] and mixture.n_iter_ == best['n_iter'] and mixture.converged_
        assert mixture.means_.tobytes() == best['means'].tobytes() and mixture.n_features_in_ == features.shape[1]
        expected = BayesianGaussianMixture(n_components=3)
        expected._set_parameters(((best['weight_concentration'][0], best['weight_concentration'][1]), ) +
                                 tuple(best[key] for key in BC.PARAMETERS[1:]))
        assert fitted_bytes(mixture) == fitted_bytes(expected)
        assert np.isfinite(model.predict_proba(features)).all()
    # user-given priors and the other prior type go down as scikit-learn checked them
    del device.calls[:]
    table = BC.load_table('plan_features')
    given = BayesianGaussianMixture(n_components=3, n_init=2, weight_concentration_prior_type='dirichlet_distribution',
                                    weight_concentration_prior=0.25, mean_precision_prior=2., mean_prior=np.full(4, 0.5),
                                    degrees_of_freedom_prior=6., covariance_prior=np.eye(4) * 3, random_state=3)
    graph_cuts.fit_bayes_mixture_device(given, table)
    _, _, _, _, prior_type, priors, _ = device.calls[1]
    assert prior_type == 'dirichlet_distribution' and priors[:2] == (0.25, 2.) and priors[3] == 6.
    assert np.array_equal(priors[2], np.full(4, 0.5)) and np.array_equal(priors[4], np.eye(4) * 3)
    assert given.weight_concentration_.shape == (3, )
    with pytest.raises(ValueError):          # scikit-learn's own error for a bad prior
        graph_cuts.fit_bayes_mixture_device(BayesianGaussianMixture(n_components=3, degrees_of_freedom_prior=1.), table)


def host_and_device(monkeypatch, caplog, table, **params):
    """the log of a device fit that has to go to the host; its model equals fit_mixture_restarts from the same stream"""
    from sklearn.mixture import BayesianGaussianMixture
    from pyimsegm_amd import _hip, graph_cuts
    monkeypatch.setattr(_hip, 'default_context', lambda: 'ctx')
    monkeypatch.setattr(_hip, 'bayes_mixture_em', lambda *args, **kwargs: pytest.fail('the device was asked'))
    host = BayesianGaussianMixture(n_components=2, n_init=2, random_state=np.random.RandomState(11), **params)
    graph_cuts.fit_mixture_restarts(host, table)
    device = BayesianGaussianMixture(n_components=2, n_init=2, random_state=np.random.RandomState(11), **params)
    with caplog.at_level(logging.INFO):
        caplog.clear()
        graph_cuts.fit_bayes_mixture_device(device, table)
    assert fitted_bytes(host) == fitted_bytes(device)
    return ' '.join(record.getMessage() for record in caplog.records if record.levelno == logging.INFO)


def test_refusals_go_to_the_host_on_the_restored_stream(monkeypatch, caplog):
    from sklearn.mixture import GaussianMixture
    from pyimsegm_amd import graph_cuts
    rng = np.random.RandomState(3)
    table = rng.standard_normal((400, 3)) + (np.arange(400) % 2)[:, None] * 4
    assert 'float32' in host_and_device(monkeypatch, caplog, table.astype(np.float32))
    assert 'full' in host_and_device(monkeypatch, caplog, table, covariance_type='diag')
    assert 'k-means' in host_and_device(monkeypatch, caplog, table, init_params='random')
    assert 'warm' in host_and_device(monkeypatch, caplog, table, warm_start=True)
    wide = rng.standard_normal((400, 17)) + (np.arange(400) % 2)[:, None] * 4
    assert '16 features' in host_and_device(monkeypatch, caplog, wide)
    assert 'GaussianMixture' in graph_cuts._device_bayes_fit_refusal(GaussianMixture(2), table)
    assert 'fewer rows' in graph_cuts._device_bayes_fit_refusal(BC.estimator(5, BC.PROCESS), table[:4])
    assert graph_cuts._device_bayes_fit_refusal(BC.estimator(2, BC.PROCESS), table) is None


def test_wide_table_goes_to_the_host_through_estim_class_model(monkeypatch, caplog):
    from pyimsegm_amd import _hip, graph_cuts
    monkeypatch.setattr(_hip, 'default_context', lambda: pytest.fail('the device was asked'))
    wide = np.random.RandomState(4).standard_normal((300, 17)) + (np.arange(300) % 3)[:, None] * 4
    np.random.seed(5)
    host = graph_cuts.estim_class_model(wide, 3, 'BGM', fit_on='host').steps[-1][1]
    for fit_on in ('device', 'device_wide'):
        np.random.seed(5)
        with caplog.at_level(logging.INFO):
            caplog.clear()
            model = graph_cuts.estim_class_model(wide, 3, 'BGM', fit_on=fit_on).steps[-1][1]
        assert any('more than 16 features (17)' in record.getMessage() for record in caplog.records)
        assert fitted_bytes(model) == fitted_bytes(host)


@pytest.mark.parametrize('fit_on', ('host', None))
def test_host_and_default_are_the_parent_model(fit_on, monkeypatch):
    from sklearn.mixture import BayesianGaussianMixture
    from sklearn.preprocessing import StandardScaler
    from pyimsegm_amd import graph_cuts
    monkeypatch.delenv('IMSEGM_FIT_ON', raising=False)
    monkeypatch.setattr(graph_cuts, 'fit_bayes_mixture_device', lambda *args, **kwargs: pytest.fail('the device fit was asked'))
    features = np.load(MC.GOLDEN + '/class_models.npz')['plan_features']
    np.random.seed(5)
    table = StandardScaler().fit_transform(np.asarray(features, dtype=np.float64))
    expected = graph_cuts.fit_mixture_restarts(BayesianGaussianMixture(n_components=3, covariance_type='full', n_init=9, max_iter=99), table)
    np.random.seed(5)
    model = graph_cuts.estim_class_model(features, 3, 'BGM', fit_on=fit_on)
    assert fitted_bytes(model.steps[-1][1]) == fitted_bytes(expected)


def test_header_and_signature_table_declare_the_entry():
    from pyimsegm_amd import _hip
    header = open(os.path.join(os.path.dirname(MC.GOLDEN), os.pardir, 'include', 'imsegm_hip.h')).read()
    declaration = re.search(r'IMSEGM_API int imsegm_bayes_mixture_em\(([^;]*)\);', header)
    assert declaration is not None
    assert len(declaration.group(1).split(',')) == len(_hip._SIGNATURES['imsegm_bayes_mixture_em'][1]) == 23
    assert header.index('imsegm_mixture_em(') < declaration.start() < header.index('imsegm_kmeans_lloyd_wide(')


@pytest.mark.parametrize('prior_type', (BC.PROCESS, BC.DISTRIBUTION))
def test_reference_loop_reproduces_scikit_learn_fit(prior_type, monkeypatch):
    """the yardstick of the GPU tests: from the k-means labels ``fit`` itself started from, the loop gives ``fit``'s model"""
    import sklearn.cluster
    table = BC.load_table('plan_features')
    seen = []
    original = sklearn.cluster.KMeans.fit

    def watched(self, *args, **kwargs):
        fitted = original(self, *args, **kwargs)
        seen.append(fitted.labels_.copy())
        return fitted
    monkeypatch.setattr(sklearn.cluster.KMeans, 'fit', watched)
    bgm = BC.estimator(3, prior_type, tol=1e-3, max_iter=99)
    bgm.set_params(random_state=3, n_init=1)
    bgm.fit(table)
    assert len(seen) == 1
    run = BC.reference_bayes_em(table, seen[0], 1e-3, 99, prior_type, n_components=3)
    assert run['n_iter'] == bgm.n_iter_ and run['converged'] == bgm.converged_ and run['lower_bound'] == bgm.lower_bound_
    fitted = BC.as_run(bgm._get_parameters())
    for key in BC.PARAMETERS:
        assert np.asarray(run[key]).tobytes() == np.asarray(fitted[key]).tobytes(), key
