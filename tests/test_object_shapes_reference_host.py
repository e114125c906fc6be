"""The numpy / scipy statement of ``compute_object_shapes`` (pyimsegm_amd/region_growing.py, on='host') and the shape model
functions against the reference's doctests and its recorded answers (tests/golden/object_shapes.npz).  No GPU."""
import importlib
import json
import os
import types

import numpy as np
import pytest

from tests import object_shapes_cases as C

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
#: finished rays: what tests/region_growing_cases.py (_check_rays) applies to the finished rays of ``compute_segm_object_shape`` --
#: equal, and within this where a ray left the image and was filled in by np.polyfit; the shifts are held to it everywhere
FILLED_RTOL = FILLED_ATOL = 1e-9
#: cumulative tables from recorded attributes: ten times the largest difference measured between this build container's scipy
#: 1.15.3 (``stats.norm.cdf``, ``gaussian_filter1d``) and the tables and smoothed means recorded under scipy 1.7.1 -- 1.78e-15 -- with the floor 1e-12
TABLE_TOL = 1e-12


@pytest.fixture(scope='module')
def rg():
    return importlib.import_module('pyimsegm_amd.region_growing')


@pytest.fixture(scope='module')
def fx():
    with np.load(os.path.join(GOLDEN, 'object_shapes.npz')) as data:
        return {key: data[key] for key in data.files}


def _doctest_maps():
    img = np.zeros((100, 100))
    img[20:70, 30:80] = 1
    img1 = np.zeros((100, 100))
    img1[20:50, 30:60] = 1
    img1[40:80, 50:90] = 2
    img2 = np.zeros((100, 100))
    img2[10:40, 20:50] = 1
    img2[50:80, 20:50] = 1
    img2[50:80, 60:90] = 1
    return img, [img1, img2]


def check_doctests(rg, on):
    """imsegm/region_growing.py:272-276 and :300-316"""
    img, list_imgs = _doctest_maps()
    list_rays, list_shifts = rg.compute_object_shapes([img], ray_step=45, on=on)
    assert [int(r * 10) for r in list_rays[0]] == [367, 260, 353, 250, 353, 250, 353, 260]
    list_rays, list_shifts = rg.compute_object_shapes(list_imgs, ray_step=45, on=on)
    assert np.array(list_rays).astype(int).tolist() == [[19, 17, 9, 17, 19, 14, 19, 14], [29, 21, 28, 20, 28, 20, 28, 21],
                                                        [22, 16, 21, 15, 21, 15, 21, 16], [22, 16, 21, 15, 21, 15, 21, 16],
                                                        [22, 16, 21, 15, 21, 15, 21, 16]]
    # (as the doctest compares: what numpy prints, eight significant digits)
    assert np.array2string(np.array(list_shifts) % 180) == np.array2string(np.array([135., 45., 45., 45., 45.]))


def test_doctests_on_the_host(rg):
    check_doctests(rg, 'host')


def _has_device():
    from pyimsegm_amd import _hip
    try:
        return _hip.device_count() > 0
    except _hip.HipUnavailableError:
        return False


@pytest.mark.parametrize('name', sorted(C.CASES))
def test_host_statement_against_the_reference(rg, fx, name):
    img, ray_step = C.case(name, int(fx['shapes_%s_seed' % name]))
    want = {key: fx['shapes_%s_%s' % (name, key)] for key in ('labels', 'centres', 'rays_raw', 'rays', 'shifts')}
    labels, moments, centres, raw = rg.object_shape_rays(img, ray_step, on='host')
    assert len(labels) == len(want['labels']) >= 1
    assert float(np.max(np.abs(labels.astype(np.int64) - want['labels']))) == 0.0
    assert float(np.max(np.abs(centres.astype(np.int64) - want['centres']))) == 0.0
    assert raw.dtype == np.float32 and float(np.max(np.abs(raw.astype(np.float64) - want['rays_raw'].astype(np.float64)))) == 0.0
    assert moments.dtype == np.int64 and moments.shape == (len(labels), 3)
    if len(np.unique(img)) > 2:
        rows, cols = np.indices(img.shape)
        assert moments.tolist() == [[int((img == v).sum()), int(rows[img == v].sum()), int(cols[img == v].sum())] for v in labels]
    list_rays, list_shifts = rg.compute_object_shapes([img], ray_step=ray_step, on='host')
    assert len(list_rays) == len(want['rays'])
    for k in range(len(list_rays)):
        if (raw[k] != -1).all():
            assert np.array_equal(list_rays[k], want['rays'][k]), k
        else:
            assert np.allclose(list_rays[k], want['rays'][k], rtol=FILLED_RTOL, atol=FILLED_ATOL), k
        # (the shift is the phase of an FFT bin and numpy's transform is not the same code in every version; it is an angle: a phase
        # of -1e-16 is 360 where one of +1e-16 is 0, so the two are compared around the circle)
        assert abs((list_shifts[k] - want['shifts'][k] + 180.) % 360. - 180.) <= FILLED_ATOL + FILLED_RTOL * 360., k


def test_fixture_has_a_ray_that_left_the_image(fx):
    assert any((fx['shapes_%s_rays_raw' % name] == -1).any() for name in C.CASES)


def test_histograms(rg, fx):
    """exact: integer bin centres and sums of eighths"""
    chist = rg.transform_rays_model_cdf_histograms(C.DOCTEST_RAYS, nb_bins=5)
    assert chist == [[1.0, 1.0, 1.0, 1.0, 0.75, 0.75, 0.75, 0.625, 0.625, 0.0, 0.0, 0.0],
                     [1.0, 1.0, 1.0, 1.0, 0.875, 0.875, 0.875, 0.375, 0.25, 0.25, 0.0, 0.0],
                     [1.0, 1.0, 1.0, 1.0, 1.0, 0.75, 0.625, 0.5, 0.375, 0.375, 0.0, 0.0]]
    for table_name, list_rays, nb_bins in (('doctest', C.DOCTEST_RAYS, 5), ('seeded0', C.ray_table(0), 10), ('seeded1', C.ray_table(1), 7)):
        got = np.array(rg.transform_rays_model_cdf_histograms(list_rays, nb_bins=nb_bins))
        assert np.array_equal(got, fx['histograms_' + table_name]), table_name


class _Fitted(object):
    """stands in for a scikit-learn estimator: carries the attributes the reference's run fitted"""

    def __init__(self, **attributes):
        self.__dict__.update(attributes)

    def fit(self, *args, **kwargs):
        return self


def _stand_ins(monkeypatch, rg, fx, function, table_name):
    """the module's estimator names give back the recorded attributes of one run of the reference"""
    def recorded(key):
        return fx['model_%s_%s_%s' % (function, table_name, key)]

    keys = [k.split('_%s_' % table_name, 1)[1] for k in fx if k.startswith('model_%s_%s_' % (function, table_name))]
    clusters = {'labels_': recorded('labels')} if 'labels' in keys else {}
    if 'centres' in keys:
        clusters['cluster_centers_'] = recorded('centres')
    blend = {}
    if 'means' in keys:
        blend = {'means_': recorded('means'), 'covariances_': recorded('covariances')}
        if 'weights' in keys:
            blend['weights_'] = recorded('weights')
    # (MeanShift's labels only count the clusters: as many distinct labels as the recorded fit has components)
    count = int(recorded('n_components')) if 'n_components' in keys else len(np.unique(clusters.get('labels_', [0])))
    monkeypatch.setattr(rg, 'cluster', types.SimpleNamespace(
        MeanShift=lambda *a, **k: _Fitted(labels_=np.arange(count)), KMeans=lambda *a, **k: _Fitted(**clusters),
        SpectralClustering=lambda *a, **k: _Fitted(**clusters)))
    monkeypatch.setattr(rg, 'mixture', types.SimpleNamespace(BayesianGaussianMixture=lambda *a, **k: _Fitted(**blend)))
    return recorded


def _table_gaps(monkeypatch, rg, fx):
    """(name, max |table from the recorded attributes - recorded table|) of every run the fixture holds"""
    gaps = []
    got = rg.compute_cumulative_distrib(np.array([[1, 2]]), np.array([[1.5, 0.5], [0.5, 1]]), np.array([0.5]), 6)
    assert np.round(got, 2).tolist() == [[1., 0.67, 0.34, 0.12, 0.03, 0., 0.], [1., 0.98, 0.5, 0.02, 0., 0., 0.]]
    gaps.append(('cumulative doctest', np.max(np.abs(got - fx['cumulative_doctest']))))
    for seed in (0, 1):
        got = rg.compute_cumulative_distrib(*C.cumulative_inputs(seed))
        want = fx['cumulative_seeded%d' % seed]
        assert got.shape == want.shape
        gaps.append(('cumulative seeded%d' % seed, np.max(np.abs(got - want))))
    for table_name, list_rays in (('doctest', C.DOCTEST_RAYS), ('seeded0', C.ray_table(0))):
        for function, call, args in (('cdf_mixture', 'transform_rays_model_cdf_mixture', ()),
                                     ('cdf_spectral', 'transform_rays_model_cdf_spectral', (3, )),
                                     ('cdf_kmeans', 'transform_rays_model_cdf_kmeans', ()),
                                     ('cdf_kmeans2', 'transform_rays_model_cdf_kmeans', (2, ))):
            recorded = _stand_ins(monkeypatch, rg, fx, function, table_name)
            model, table = getattr(rg, call)(list_rays, *args)
            assert isinstance(model, _Fitted) and isinstance(table, list)
            want = recorded('table')
            assert np.shape(table) == want.shape == (len(list_rays[0]), int(recorded('max_dist')[0]) + 1), (function, table_name)
            gaps.append(('%s %s' % (function, table_name), np.max(np.abs(np.array(table) - want))))
        for function, call in (('sets_mean_cdf_mixture', 'transform_rays_model_sets_mean_cdf_mixture'),
                               ('sets_mean_cdf_kmeans', 'transform_rays_model_sets_mean_cdf_kmeans')):
            recorded = _stand_ins(monkeypatch, rg, fx, function, table_name)
            model, pairs = getattr(rg, call)(list_rays, 2)
            assert isinstance(model, _Fitted) and len(pairs) == 2 == len(recorded('max_dist'))
            for i, (mean, table) in enumerate(pairs):
                want = recorded('table%d' % i)
                assert isinstance(mean, list) and table.shape == want.shape == (len(list_rays[0]), int(recorded('max_dist')[i]) + 1)
                gaps.append(('%s %s mean %d' % (function, table_name, i), np.max(np.abs(np.array(mean) - recorded('table_means')[i]))))
                gaps.append(('%s %s table %d' % (function, table_name, i), np.max(np.abs(table - want))))
    return gaps


def test_tables_from_recorded_attributes(rg, fx, monkeypatch):
    """``compute_cumulative_distrib`` and the numpy / scipy halves of the five scikit-learn variants, fed with what the
    reference's estimators had fitted"""
    gaps = _table_gaps(monkeypatch, rg, fx)
    for name, gap in gaps:
        print('%-50s max |here - recorded| %.3g' % (name, gap))
    print('largest: %.3g, tolerance %.3g' % (max(g for _, g in gaps), TABLE_TOL))
    assert len(gaps) >= 3 + 2 * (4 + 2 * 4)
    for name, gap in gaps:
        assert gap <= TABLE_TOL, (name, gap)


def test_installed_scikit_learn_runs_every_variant(rg):
    """one run of each variant with the scikit-learn that is installed: shapes, range and monotony only"""
    import warnings
    nb_angles = len(C.DOCTEST_RAYS[0])

    def check(table):
        table = np.asarray(table)
        assert table.ndim == 2 and table.shape[0] == nb_angles and table.shape[1] >= 2
        assert table.min() >= 1e-9 and table.max() <= 1 + 1e-9
        assert np.all(np.diff(table, axis=1) <= 0)

    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        for call, args in (('transform_rays_model_cdf_mixture', ()), ('transform_rays_model_cdf_spectral', (3, )),
                           ('transform_rays_model_cdf_kmeans', ()), ('transform_rays_model_cdf_kmeans', (2, ))):
            np.random.seed(0)
            model, table = getattr(rg, call)(C.DOCTEST_RAYS, *args)
            assert isinstance(table, list)
            check(table)
        for call in ('transform_rays_model_sets_mean_cdf_mixture', 'transform_rays_model_sets_mean_cdf_kmeans'):
            np.random.seed(0)
            model, pairs = getattr(rg, call)(C.DOCTEST_RAYS, 2)
            assert len(pairs) == 2
            for mean, table in pairs:
                assert len(mean) == nb_angles
                check(table)


def test_every_public_function_of_the_reference_is_defined(rg):
    with open(os.path.join(GOLDEN, 'region_growing_names.json')) as fp:
        names = json.load(fp)
    assert len(names) >= 25 and 'compute_object_shapes' in names
    missing = [name for name in names if not callable(getattr(rg, name, None))]
    assert not missing, missing


def test_fallbacks_and_refusals(rg, fx):
    img, ray_step = C.case('labels', int(fx['shapes_labels_seed']))
    want = rg.compute_object_shapes([img], ray_step=ray_step, on='host')
    # half-values keep order and equality of the labels: the same objects, but no int32 map -- whatever `on` says, the host statement
    assert rg._int32_map(img * 0.5) is None and rg._int32_map(img) is not None and rg._int32_map(img.astype(float)) is not None
    assert rg._int32_map(img.astype(np.int64) + 2**40) is None
    for on in ('host', None):
        if on is None and _has_device():
            continue                                     # (the same call with a device is part of tests/test_gpu_object_shapes.py)
        got = rg.compute_object_shapes([img * 0.5], ray_step=ray_step, on=on)
        assert got[0] == want[0] and got[1] == want[1]
    assert np.array_equal(np.array(want[0]), fx['shapes_labels_rays'])
    with pytest.raises(ValueError, match="on is 'host' or 'device'"):
        rg.compute_object_shapes([img], on='bogus')
    with pytest.raises(ValueError, match="on is 'host' or 'device'"):
        rg.object_shape_rays(img, on='bogus')


def test_host_statement_on_the_edge_maps(rg):
    """the reference's quirks: np.unique(...)[1:] drops the first value whatever it is"""
    from pyimsegm_amd.descriptors import _ray_directions
    directions = _ray_directions(45.)
    full = np.ones((6, 7), dtype=np.int32)
    assert len(rg._object_shape_rays_host(full, directions)[0]) == 0                      # one component, dropped
    assert len(rg._object_shape_rays_host(full * 0, directions)[0]) == 0
    two = full.copy()
    two[:, 3:] = 2
    assert len(rg._object_shape_rays_host(two, directions)[0]) == 0                       # {1, 2}: no 0, one component
    three = two.copy()
    three[0, 0] = 5
    labels, moments, centres, rays = rg._object_shape_rays_host(three, directions)       # {1, 2, 5}: 1 is no object
    assert labels.tolist() == [2, 5] and moments.tolist() == [[24, 60, 108], [1, 0, 0]] and centres.tolist() == [[2, 4], [0, 0]]
    ties = np.zeros((4, 3), dtype=np.int32)
    ties[0:2, 0] = 1
    ties[1:3, 2] = 2
    assert rg._object_shape_rays_host(ties, directions)[2].tolist() == [[0, 0], [2, 2]]   # 0.5 -> 0, 1.5 -> 2
