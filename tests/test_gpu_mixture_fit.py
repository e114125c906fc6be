"""The mixture fit on the device (``fit_on='device'``: csrc/mixture_fit.hip through ``_hip.kmeans_lloyd`` / ``_hip.mixture_em`` and
``graph_cuts.fit_mixture_device``) against scikit-learn on the CPU driven from the same start (tests/mixture_fit_cases.py), its
determinism, its fall-backs and the pipelines that take the keyword."""
import itertools
import logging

import numpy as np
import pytest

import mixture_fit_cases as MC

pytestmark = pytest.mark.gpu

GOLDEN_TABLES = ('plan_features', 'reference_c5', 'reference_2048')
ALL_TABLES = GOLDEN_TABLES + ('synthetic_300k', )
PARAMETERS = ('weights', 'means', 'covariances', 'precisions_cholesky', 'lower_bound')

#: share of pixels on which two HOST fits with different ``random_state`` give the same class map up to a permutation of the
#: classes, measured on the GPU box with ``fit_on='host'`` on the inputs of test_pipelines_with_device_fit
HOST_FITS_AGREE_IMAGE = 1.0
HOST_FITS_AGREE_VOLUME = 1.0

_CACHE = {}


def case(name):
    """table, seeds, scikit-learn's Lloyd from them, the device's Lloyd from them"""
    if name not in _CACHE:
        from pyimsegm_amd import _hip
        table = MC.load_table(name)
        seeds = MC.seeds_of(table)
        tol = 1e-4 * np.mean(np.var(table, axis=0))
        _CACHE[name] = (table, seeds, MC.reference_lloyd(table, seeds), _hip.kmeans_lloyd(table, seeds, 300, tol))
    return _CACHE[name]


def device_em(name, labels, **kwargs):
    """EM on the device on the table of ``name`` from host labels (any number of restarts)"""
    from pyimsegm_amd import _hip
    table, seeds = case(name)[:2]
    labels = np.atleast_2d(labels)
    _hip.kmeans_lloyd(table, seeds[:1], 1, 0., want_labels=False)          # (uploads the table)
    return _hip.mixture_em(len(labels), MC.N_CLASSES, table.shape[1], labels=labels, **kwargs)


def restart_of(fit, r):
    return {key: fit[key][r] for key in fit}


def assert_close_to_reference(name, fit, refs, what):
    for r, ref in enumerate(refs):
        got = restart_of(fit, r)
        dev = MC.deviation(got, ref)
        print('%s %s restart %d: deviation %.3g (tolerance %.3g)' % (name, what, r, dev, MC.EM_TOLERANCE[name]))
        assert dev <= MC.EM_TOLERANCE[name], (name, what, r, dev)


@pytest.mark.parametrize('name', ALL_TABLES)
def test_lloyd_equals_scikit_learn_from_the_same_seeds(name):
    table, seeds, (labels, centres, inertia, n_iter), got = case(name)
    assert not got['empty'].any()
    differing = (got['labels'] != labels).sum(axis=1)
    print(name, 'rows with another label per restart', differing.tolist(), 'iterations', got['n_iter'].tolist(), n_iter.tolist())
    assert differing.tolist() == [0] * MC.N_RESTARTS
    assert got['n_iter'].tolist() == n_iter.tolist()
    tolerance = MC.EM_TOLERANCE[name]
    assert np.max(np.abs(got['centres'] - centres) / (1 + np.abs(centres))) <= tolerance
    assert np.max(np.abs(got['inertia'] - inertia) / (1 + np.abs(inertia))) <= tolerance


@pytest.mark.parametrize('name', ALL_TABLES)
def test_em_iteration_for_iteration(name):
    table, _, (labels, _, _, _), _ = case(name)
    refs = [MC.reference_em(table, lab, 0., 20) for lab in labels]
    fit = device_em(name, labels, tol=0., max_iter=20)
    for r, ref in enumerate(refs):
        if ref['failed']:                # scikit-learn raised in that iteration: the device stops there too and says so
            assert fit['not_pd'][r] and fit['n_iter'][r] == ref['n_iter'], (r, ref['failed'])
        else:
            assert fit['n_iter'][r] == 20 and not fit['converged'][r] and not fit['not_pd'][r]
    assert_close_to_reference(name, fit, refs, 'tol=0 max_iter=20')


@pytest.mark.parametrize('name', GOLDEN_TABLES)
def test_stopping_rule(name):
    table, _, (labels, _, _, _), _ = case(name)
    refs = [MC.reference_em(table, lab, 1e-3, 99) for lab in labels]
    for ref in refs:                     # the inputs qualify: the reference's decision is not within 1e-6 of the threshold
        bounds = [-np.inf] + ref['bounds']
        for i in range(max(1, len(bounds) - 2), len(bounds)):
            assert abs(abs(bounds[i] - bounds[i - 1]) - 1e-3) > 1e-6
    fit = device_em(name, labels, tol=1e-3, max_iter=99)
    assert fit['n_iter'].tolist() == [ref['n_iter'] for ref in refs]
    assert fit['converged'].tolist() == [ref['converged'] for ref in refs]
    assert_close_to_reference(name, fit, refs, 'tol=1e-3 max_iter=99')
    good = [r for r, ref in enumerate(refs) if not ref['failed']]
    best_ref = max(refs[r]['lower_bound'] for r in good)
    best = max(fit['lower_bound'][r] for r in good)
    assert abs(best - best_ref) / (1 + abs(best_ref)) <= MC.EM_TOLERANCE[name]


def same_bytes(fit_a, fit_b, rows_a=slice(None), rows_b=slice(None)):
    return all(np.asarray(fit_a[key][rows_a]).tobytes() == np.asarray(fit_b[key][rows_b]).tobytes() for key in fit_a)


@pytest.mark.parametrize('name', ('reference_c5', 'reference_2048'))
def test_determinism(name):
    from pyimsegm_amd import _hip
    table, seeds, (labels, _, _, _), lloyd = case(name)
    tol = 1e-4 * np.mean(np.var(table, axis=0))
    again = _hip.kmeans_lloyd(table, seeds, 300, tol)
    assert same_bytes(lloyd, again)
    fit = _hip.mixture_em(MC.N_RESTARTS, MC.N_CLASSES, table.shape[1], tol=1e-3, max_iter=99)       # (from the resident labels)
    assert same_bytes(fit, device_em(name, labels, tol=1e-3, max_iter=99))
    assert same_bytes(fit, device_em(name, labels, tol=1e-3, max_iter=99))
    for r in range(MC.N_RESTARTS):
        alone_lloyd = _hip.kmeans_lloyd(table, seeds[r:r + 1], 300, tol)
        assert same_bytes(alone_lloyd, lloyd, slice(None), slice(r, r + 1)), r
        alone = _hip.mixture_em(1, MC.N_CLASSES, table.shape[1], tol=1e-3, max_iter=99)
        assert same_bytes(alone, fit, slice(None), slice(r, r + 1)), r
        if fit['converged'][r]:          # frozen at its iteration: what a run of exactly that many iterations gives
            short = device_em(name, labels[r], tol=1e-3, max_iter=int(fit['n_iter'][r]))
            assert same_bytes(short, fit, slice(None), slice(r, r + 1)), r
    # start parameters instead of labels: one more iteration from the state after five equals six iterations
    five = device_em(name, labels, tol=0., max_iter=5)
    six = device_em(name, labels, tol=0., max_iter=6)
    ok = ~five['not_pd'] & ~six['not_pd']
    step = _hip.mixture_em(MC.N_RESTARTS, MC.N_CLASSES, table.shape[1], start=(five['weights'], five['means'], five['precisions_cholesky']),
                           tol=0., max_iter=1)
    for key in PARAMETERS:
        assert np.allclose(step[key][ok], six[key][ok], rtol=0, atol=MC.EM_TOLERANCE[name] * (1 + np.abs(six[key][ok]).max())), key


def host_restatement(features, n_classes, random_state, max_iter=99):
    """seeds -> KMeans(init=seeds) -> EM loop, best of the restarts, all scikit-learn"""
    from sklearn.preprocessing import StandardScaler
    table = np.ascontiguousarray(StandardScaler().fit_transform(np.asarray(features, dtype=np.float64)))
    seeds = MC.seeds_of(table, random_state, max(1, int(np.sqrt(max_iter))), n_classes)
    labels = MC.reference_lloyd(table, seeds)[0]
    runs = [MC.reference_em(table, lab, 1e-3, max_iter) for lab in labels]
    return max(run['lower_bound'] for run in runs if not run['failed'])


@pytest.mark.parametrize('name', GOLDEN_TABLES)
def test_whole_fit(name):
    from sklearn.mixture import GaussianMixture
    from sklearn.pipeline import Pipeline
    from pyimsegm_amd import graph_cuts
    file_name, key = {'reference_2048': ('reference_2048.npz', 'features'), 'reference_c5': ('reference_c5.npz', 'normed'),
                      'plan_features': ('class_models.npz', 'plan_features')}[name]
    features = np.asarray(np.load(MC.GOLDEN + '/' + file_name)[key], dtype=np.float64)
    np.random.seed(MC.SEED)                      # (estim_class_model leaves random_state at None: numpy's global stream)
    model = graph_cuts.estim_class_model(features, 3, fit_on='device')
    assert isinstance(model, Pipeline) and type(model.steps[-1][1]) is GaussianMixture
    mixture = model.steps[-1][1]
    assert mixture.converged_ and mixture.n_features_in_ == features.shape[1] and mixture.weights_.shape == (3, )
    assert np.allclose(mixture.precisions_, [p @ p.T for p in mixture.precisions_cholesky_], rtol=0, atol=0)
    assert np.abs(graph_cuts.predict_proba(model, features) - model.predict_proba(features)).max() <= 1e-9
    np.random.seed(MC.SEED)
    stream = np.random.mtrand._rand
    reference = host_restatement(features, 3, stream)
    print(name, 'lower bound', mixture.lower_bound_, 'host restatement', reference)
    assert abs(mixture.lower_bound_ - reference) / (1 + abs(reference)) <= MC.EM_TOLERANCE[name]
    np.random.seed(MC.SEED)
    again = graph_cuts.estim_class_model(features, 3, fit_on='device').steps[-1][1]
    for attribute in ('weights_', 'means_', 'covariances_', 'precisions_cholesky_', 'precisions_'):
        assert getattr(again, attribute).tobytes() == getattr(mixture, attribute).tobytes()
    np.random.seed(MC.SEED + 1)
    other = graph_cuts.estim_class_model(features, 3, fit_on='device').steps[-1][1]
    assert other.converged_
    # the estim_model plans keep working: one EM iteration on the device for the max_iter = 1 plans
    np.random.seed(MC.SEED)
    one = graph_cuts.estim_class_model(features, 3, 'kmeans', fit_on='device').steps[-1][1]
    assert one.n_iter_ == 1 and np.isfinite(one.lower_bound_)


def test_fall_backs_and_errors(caplog):
    from sklearn.mixture import GaussianMixture
    from pyimsegm_amd import _hip, graph_cuts
    rng = np.random.RandomState(3)

    def both(table, n_components, n_init=3):
        host = GaussianMixture(n_components, n_init=n_init, random_state=np.random.RandomState(11))
        graph_cuts.fit_mixture_restarts(host, table)
        device = GaussianMixture(n_components, n_init=n_init, random_state=np.random.RandomState(11))
        with caplog.at_level(logging.INFO):
            caplog.clear()
            graph_cuts.fit_mixture_device(device, table)
        for attribute in ('weights_', 'means_', 'covariances_', 'precisions_cholesky_'):
            assert getattr(host, attribute).tobytes() == getattr(device, attribute).tobytes()
        return ' '.join(record.getMessage() for record in caplog.records if record.levelno == logging.INFO)

    wide = rng.standard_normal((400, 17)) + (np.arange(400) % 2)[:, None] * 4
    with pytest.raises(_hip.HipFitCapsError):
        _hip.kmeans_lloyd(wide, wide[None, :2], 10, 0.)
    assert 'caps' in both(wide, 2)
    narrow = rng.standard_normal((600, 2)) + (np.arange(600) % 9)[:, None] * 6
    with pytest.raises(_hip.HipFitCapsError):
        _hip.kmeans_lloyd(narrow, narrow[None, :9], 10, 0.)
    assert 'caps' in both(narrow, 9)
    # fewer distinct rows than classes: a cluster stays empty, the device says so and the host path takes the fit
    few = np.repeat(np.array([[0., 0.], [1., 1.]]), 30, axis=0)
    assert _hip.kmeans_lloyd(few, few[None, [0, 30, 1]], 10, 0.)['empty'].tolist() == [True]
    device = GaussianMixture(3, n_init=2, random_state=np.random.RandomState(5))
    host = GaussianMixture(3, n_init=2, random_state=np.random.RandomState(5))
    with caplog.at_level(logging.INFO):
        caplog.clear()
        graph_cuts.fit_mixture_device(device, few)
        assert any('empty' in record.getMessage() for record in caplog.records)
    graph_cuts.fit_mixture_restarts(host, few)
    assert host.means_.tobytes() == device.means_.tobytes()
    bad = rng.standard_normal((50, 3))
    bad[7, 1] = np.nan
    with pytest.raises(ValueError):
        graph_cuts.estim_class_model(bad, 3, use_scaler=False, fit_on='device')
    with pytest.raises(ValueError):
        graph_cuts.estim_class_model(rng.standard_normal((50, 3)), 3, fit_on='gpu')
    # float32 tables and other mixtures are fitted on the host, and the log says why
    assert 'float32' in both(narrow.astype(np.float32), 2)


def agreement(segm_a, segm_b, n_classes):
    """share of pixels with the same class up to the best permutation of the classes"""
    return max(np.mean(np.asarray(order)[segm_a] == segm_b) for order in itertools.permutations(range(n_classes)))


def test_pipelines_with_device_fit():
    from pyimsegm_amd import pipelines
    from pyimsegm_amd.utilities.synthetic import ellipsoid_volume, voronoi_image
    image = voronoi_image(256, 256, nb_seeds=12, seed=3)
    features = {'color': ['mean', 'std']}
    np.random.seed(1)
    host, _ = pipelines.pipe_color2d_slic_features_model_graphcut(image, 3, features, sp_size=12, fit_on='host')
    np.random.seed(1)
    segm, soft = pipelines.pipe_color2d_slic_features_model_graphcut(image, 3, features, sp_size=12, fit_on='device')
    assert segm.shape == (256, 256) and soft.shape == (256, 256, 3) and soft.dtype == np.float64
    assert segm.dtype == host.dtype and set(np.unique(segm)) <= set(range(3))
    share = agreement(host, segm, 3)
    print('image: device fit agrees with the host fit on', share)
    assert share >= HOST_FITS_AGREE_IMAGE - 0.01
    volume = ellipsoid_volume((16, 64, 64))
    np.random.seed(1)
    host = pipelines.pipe_gray3d_slic_features_model_graphcut(volume, 3, {'color': ['mean']}, spacing=(2, 1, 1), sp_size=6, fit_on='host')
    np.random.seed(1)
    segm = pipelines.pipe_gray3d_slic_features_model_graphcut(volume, 3, {'color': ['mean']}, spacing=(2, 1, 1), sp_size=6, fit_on='device')
    assert segm.shape == volume.shape and segm.dtype == host.dtype and set(np.unique(segm)) <= set(range(3))
    share = agreement(np.asarray(host), np.asarray(segm), 3)
    print('volume: device fit agrees with the host fit on', share)
    assert share >= HOST_FITS_AGREE_VOLUME - 0.01
