"""What of ``fit_on`` (graph_cuts.estim_class_model, the device fit of the class model) can be checked without a GPU: the default
and ``'host'`` are the host fit bit for bit, the environment variable, the errors, and the seeding of the device fit."""
import numpy as np
import pytest

import mixture_fit_cases as MC

ATTRIBUTES = ('weights_', 'means_', 'covariances_', 'precisions_cholesky_', 'precisions_')


def parent_model(features, n_classes, seed):
    """what estim_class_model built before it had the keyword: scaler, then fit_mixture_restarts on the mixture"""
    from sklearn.mixture import GaussianMixture
    from sklearn.preprocessing import StandardScaler
    from pyimsegm_amd import graph_cuts
    np.random.seed(seed)
    table = StandardScaler().fit_transform(np.asarray(features, dtype=np.float64))
    return graph_cuts.fit_mixture_restarts(GaussianMixture(n_classes, covariance_type='full', n_init=9, max_iter=99), table)


@pytest.mark.parametrize('fit_on', ('host', None))
def test_host_and_default_are_the_parent_model(fit_on, monkeypatch):
    from pyimsegm_amd import graph_cuts
    monkeypatch.delenv('IMSEGM_FIT_ON', raising=False)
    features = np.load(MC.GOLDEN + '/class_models.npz')['plan_features']
    expected = parent_model(features, 3, 5)
    np.random.seed(5)
    model = graph_cuts.estim_class_model(features, 3, fit_on=fit_on)
    for attribute in ATTRIBUTES:
        assert getattr(model.steps[-1][1], attribute).tobytes() == getattr(expected, attribute).tobytes()


def test_environment_variable_and_bad_values(monkeypatch):
    from pyimsegm_amd import graph_cuts
    features = np.load(MC.GOLDEN + '/class_models.npz')['plan_features']
    calls = []
    monkeypatch.setattr(graph_cuts, 'fit_mixture_device', lambda mixture, table, ctx=None: calls.append(table.shape) or mixture)
    monkeypatch.setenv('IMSEGM_FIT_ON', 'device')
    graph_cuts.estim_class_model(features, 3)
    assert calls == [features.shape]
    graph_cuts.estim_class_model(features, 3, fit_on='host')           # (the keyword wins)
    assert len(calls) == 1
    monkeypatch.setenv('IMSEGM_FIT_ON', 'gpu')
    with pytest.raises(ValueError):
        graph_cuts.estim_class_model(features, 3)
    monkeypatch.delenv('IMSEGM_FIT_ON')
    with pytest.raises(ValueError):
        graph_cuts.estim_class_model(features, 3, fit_on='gpu')


def test_no_library_is_an_error_not_a_host_fit(monkeypatch):
    from pyimsegm_amd import _hip, graph_cuts
    monkeypatch.setattr(_hip, '_lib', None)
    monkeypatch.setattr(_hip, 'LIB_PATH', '/nonexistent/libimsegm_hip.so')
    monkeypatch.setattr(_hip, '_default_ctx', {})
    features = np.load(MC.GOLDEN + '/class_models.npz')['plan_features']
    with pytest.raises(_hip.HipUnavailableError):
        graph_cuts.estim_class_model(features, 3, fit_on='device')


def test_non_finite_table_raises_before_the_device_is_asked(monkeypatch):
    from pyimsegm_amd import _hip, graph_cuts
    monkeypatch.setattr(_hip, 'default_context', lambda: pytest.fail('the device was asked'))
    table = np.random.RandomState(0).standard_normal((40, 3))
    table[3, 0] = np.inf
    with pytest.raises(ValueError):
        graph_cuts.estim_class_model(table, 2, use_scaler=False, fit_on='device')


def test_seeding_depends_on_the_stream_only_and_sees_few_rows(monkeypatch):
    import sklearn.cluster
    from pyimsegm_amd import graph_cuts
    table = np.random.RandomState(1).standard_normal((100000, 3))
    seen = []
    original = sklearn.cluster.kmeans_plusplus

    def watched(rows, *args, **kwargs):
        seen.append(len(rows))
        return original(rows, *args, **kwargs)
    monkeypatch.setattr(sklearn.cluster, 'kmeans_plusplus', watched)
    first = graph_cuts.device_fit_seeds(table, 3, 9, np.random.RandomState(7))
    again = graph_cuts.device_fit_seeds(table, 3, 9, np.random.RandomState(7))
    other = graph_cuts.device_fit_seeds(table, 3, 9, np.random.RandomState(8))
    assert first.shape == (9, 3, 3) and first.tobytes() == again.tobytes() and first.tobytes() != other.tobytes()
    assert len(seen) == 27 and max(seen) <= graph_cuts.DEVICE_FIT_SEEDING_ROWS and min(seen) > graph_cuts.DEVICE_FIT_SEEDING_ROWS // 2
    assert all((table == row).all(axis=1).any() for row in first.reshape(-1, 3))         # (seeds are rows of the table)
    small = graph_cuts.device_fit_seeds(table[:500], 3, 2, np.random.RandomState(7))
    assert seen[-1] == 500 and small.shape == (2, 3, 3)


def test_refusals_name_their_reason():
    from sklearn.mixture import BayesianGaussianMixture, GaussianMixture
    from pyimsegm_amd import graph_cuts
    table = np.zeros((10, 2))
    assert graph_cuts._device_fit_refusal(GaussianMixture(2), table) is None
    assert 'BayesianGaussianMixture' in graph_cuts._device_fit_refusal(BayesianGaussianMixture(n_components=2), table)
    assert 'warm' in graph_cuts._device_fit_refusal(GaussianMixture(2, warm_start=True), table)
    assert 'initial' in graph_cuts._device_fit_refusal(GaussianMixture(2, means_init=np.zeros((2, 2))), table)
    assert 'full' in graph_cuts._device_fit_refusal(GaussianMixture(2, covariance_type='diag'), table)
    assert 'k-means' in graph_cuts._device_fit_refusal(GaussianMixture(2, init_params='random'), table)
    assert 'float32' in graph_cuts._device_fit_refusal(GaussianMixture(2), table.astype(np.float32))
