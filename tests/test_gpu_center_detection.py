"""``imsegm_dbscan_points`` (csrc/cluster.hip) behind pyimsegm_amd/center_detection.py:

* labels, cluster counts and centres of every case of tests/center_detection_cases.py, single and batched, equal the host statement
  (``cluster_center_candidates_host``, which tests/test_center_detection_reference_host.py holds against scikit-learn) with
  ``array_equal``; every call runs twice and gives equal bytes;
* the error status leaves the output arrays untouched; a request above the caps equals the host route;
* a small call after a large one on a context whose scratch holds stale data;
* end to end on a 256 x 384 image of six ellipses: ``detect_centers`` on the device equals the step-by-step composition with the
  clustering on the host, finds six centres, one inside each ellipse, and the batch form equals two single calls."""
import numpy as np
import pytest

import center_detection_cases as C

pytestmark = pytest.mark.gpu

_HOST = {}


@pytest.fixture(scope='module')
def hip():
    from pyimsegm_amd import _hip
    _hip.default_context()
    return _hip


@pytest.fixture(scope='module')
def detection():
    from pyimsegm_amd import center_detection
    return center_detection


def host(detection, name, settings=None):
    """the statement's answer for a case, computed once and shared"""
    key = (name, settings)
    if key not in _HOST:
        points, eps, min_samples = C.case(name)
        if settings is not None:
            eps, min_samples = settings
        if len(points) == 0:
            _HOST[key] = (np.array([]), np.zeros(0, dtype=np.int64))
        else:
            _HOST[key] = detection.cluster_center_candidates_host(points, eps, min_samples)
        for part in _HOST[key]:
            part.setflags(write=False)
    return _HOST[key]


def raw(hip, sets, eps, min_samples):
    """one ``imsegm_dbscan_points`` call on the sets; run twice, equal bytes"""
    offsets = np.zeros(len(sets) + 1, dtype=np.int32)
    offsets[1:] = np.cumsum([len(s) for s in sets])
    concat = np.ascontiguousarray(np.concatenate(sets, axis=0), dtype=np.float64).reshape(-1, 2)
    first = hip.dbscan_points(concat, offsets, eps, min_samples)
    again = hip.dbscan_points(concat, offsets, eps, min_samples)
    assert first is not None and all(C.same(a, b) for a, b in zip(first, again))
    return offsets, first


def check_set(labels, nb_clusters, centres, want):
    """one set's slice of the raw outputs against the statement's (centres, labels)"""
    want_centres, want_labels = want
    assert np.array_equal(labels, want_labels)
    assert nb_clusters == len(want_centres)
    assert np.array_equal(centres[:nb_clusters], want_centres.reshape(-1, 2))
    assert not centres[nb_clusters:].any()                # the slots behind the clusters are zeroed


@pytest.mark.parametrize('name', [name for name in C.CASES if name != 'size_cap_plus_1'])
def test_single_sets_equal_the_statement(hip, detection, name):
    points, eps, min_samples = C.case(name)
    offsets, (labels, counts, centres) = raw(hip, [points], eps, min_samples)
    assert labels.dtype == np.int32 and counts.dtype == np.int32 and centres.dtype == np.float64
    check_set(labels, counts[0], centres, host(detection, name))
    got = detection.cluster_center_candidates(points, eps, min_samples, on='device')
    assert C.same(got[0], host(detection, name)[0]) and C.same(got[1], host(detection, name)[1])


def test_mixed_batch_with_empty_sets(hip, detection):
    eps, min_samples = C.BATCH_SETTINGS
    sets = [C.case(name)[0] for name in C.BATCH]
    offsets, (labels, counts, centres) = raw(hip, sets, eps, min_samples)
    for k, name in enumerate(C.BATCH):
        check_set(labels[offsets[k]:offsets[k + 1]], counts[k], centres[offsets[k]:offsets[k + 1]], host(detection, name, C.BATCH_SETTINGS))
    got = detection.cluster_center_candidates_batch(sets, eps, min_samples, on='device')
    for name, points, (found, found_labels) in zip(C.BATCH, sets, got):
        if name == 'empty':
            assert len(found) == 0 and found_labels == []
        else:
            want = host(detection, name, C.BATCH_SETTINGS)
            assert C.same(found, want[0]) and C.same(found_labels, want[1])
    # nothing but empty sets, and no set at all
    labels, counts, centres = hip.dbscan_points(np.zeros((0, 2)), np.zeros(4, dtype=np.int32), eps, min_samples)
    assert len(labels) == 0 and counts.tolist() == [0, 0, 0] and centres.shape == (0, 2)
    assert hip.dbscan_points(np.zeros((0, 2)), np.zeros(1, dtype=np.int32), eps, min_samples)[1].shape == (0, )


def test_many_sets_in_one_call(hip, detection):
    # 1024 sets of seven points: the sets of a call do not see each other
    points, eps, min_samples = C.case('triangles_3_4_5')
    shifted = [points + 1000.0 * (k % 3) for k in range(1024)]
    offsets, (labels, counts, centres) = raw(hip, shifted, eps, min_samples)
    want_centres, want_labels = host(detection, 'triangles_3_4_5')
    assert np.array_equal(labels.reshape(1024, 7), np.tile(want_labels, (1024, 1)))
    assert np.all(counts == 2)
    for k in (0, 1, 2, 1023):
        assert np.array_equal(centres[7 * k:7 * k + 2], want_centres + 1000.0 * (k % 3))


def test_refused_input_leaves_the_outputs_untouched(hip, detection):
    good = np.array([[1., 2.], [3., 4.], [50., 60.]])
    offsets = np.array([0, 3], dtype=np.int32)
    bad = good.copy()
    bad[1, 1] = np.nan
    far = good.copy()
    far[2, 0] = -np.inf
    for points, eps, min_samples in ((bad, 5., 1), (far, 5., 1), (good, 0., 1), (good, -2., 1), (good, np.inf, 1), (good, np.nan, 1),
                                     (good, 5., 0), (good, 5., -3)):
        out = np.full(3, 77, dtype=np.int32), np.full(1, 78, dtype=np.int32), np.full((3, 2), 79.5)
        with pytest.raises(hip.HipClusterInputError) as refused:
            hip.dbscan_points(points, offsets, eps, min_samples, out=out)
        assert isinstance(refused.value, ValueError)
        assert np.all(out[0] == 77) and np.all(out[1] == 78) and np.all(out[2] == 79.5)
        with pytest.raises(ValueError):
            detection.cluster_center_candidates(points, eps, min_samples, on='device')
    # the context is as good as before
    labels, counts, _ = hip.dbscan_points(good, offsets, 5., 1)
    assert labels.tolist() == [0, 0, 1] and counts.tolist() == [2]


def test_above_the_caps_equals_the_host_route(hip, detection):
    points, eps, min_samples = C.case('size_cap_plus_1')
    assert len(points) == hip.DBSCAN_MAX_POINTS + 1
    assert hip.dbscan_points(points, np.array([0, len(points)], dtype=np.int32), eps, min_samples) is None
    got = detection.cluster_center_candidates(points, eps, min_samples, on='device')
    want = host(detection, 'size_cap_plus_1')
    assert C.same(got[0], want[0]) and C.same(got[1], want[1])
    # more sets than the cap: the status, and the host route behind the batch call
    one = np.array([[0., 0.], [1., 1.]])
    count = hip.DBSCAN_MAX_SETS + 1
    offsets = (np.arange(count + 1) * 2).astype(np.int32)
    assert hip.dbscan_points(np.tile(one, (count, 1)), offsets, 2., 1) is None
    # a table that is not P x 2
    table = np.random.RandomState(0).randint(0, 30, (80, 3)).astype(np.float64)
    got = detection.cluster_center_candidates(table, 6, 3, on='device')
    want = detection.cluster_center_candidates_host(table, 6, 3)
    assert C.same(got[0], want[0]) and C.same(got[1], want[1])


@pytest.mark.parametrize('word', [0x00000001, 0x7F7F7F7F, 0xFFFFFFFF])
def test_a_small_call_after_a_large_one_on_stale_scratch(hip, detection, word):
    ctx = hip.Context()
    try:
        points, eps, min_samples = C.case('size_cap')
        large = hip.dbscan_points(points, np.array([0, len(points)], dtype=np.int32), eps, min_samples, ctx=ctx)
        check_set(large[0], large[1][0], large[2], host(detection, 'size_cap'))
        assert ctx.poison(word) > 0
        for name in ('size_65', 'border_between_two', 'min_samples_above_size'):
            points, eps, min_samples = C.case(name)
            small = hip.dbscan_points(points, np.array([0, len(points)], dtype=np.int32), eps, min_samples, ctx=ctx)
            check_set(small[0], small[1][0], small[2], host(detection, name))
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------
# end to end
# ------------------------------------------------------------------------------------------------

PARAMS = {'slic_size': 10, 'DBSCAN_max_dist': 30, 'DBSCAN_min_samples': 2}


@pytest.fixture(scope='module')
def trained(detection):
    """image, class map and a forest fitted on the image's own candidate points"""
    from sklearn.ensemble import RandomForestClassifier
    from pyimsegm_amd import center_annotation
    eggs = C.ellipse_eggs()
    img = C.ellipse_image(eggs)
    levels, centres = center_annotation.create_annot_centers((eggs > 0).astype(np.uint8) * 255, on='device', sel_radius=5)
    assert len(centres) == 6 and levels.max() == 3
    segm = levels.astype(np.int64)
    params = dict(detection.CENTER_PARAMS, **detection.CLUSTER_PARAMS)
    params.update(PARAMS)
    _, slic, points, features, names = detection.estim_points_compute_features('eggs', img, segm, params)
    target = (np.asarray(detection.label_close_points(levels, points, params)) >= 2).astype(int)
    assert 6 <= target.sum() < len(target)
    classif = RandomForestClassifier(n_estimators=20, random_state=0, n_jobs=1).fit(features, target)
    return dict(eggs=eggs, img=img, segm=segm, levels=levels, params=params, classif=classif, slic=slic, points=points,
                features=features, names=names)


def same_result(a, b):
    assert sorted(a) == sorted(b) == ['candidates', 'centres', 'clust_labels', 'feature_names', 'features', 'labels', 'points', 'slic']
    return all(a[key] == b[key] if key in ('points', 'feature_names') else C.same(a[key], b[key]) for key in a)


def test_detect_centers_equals_the_composition(detection, trained):
    from pyimsegm_amd import classification
    assert classification.device_forest(trained['classif'])[0] is not None
    got = detection.detect_centers(trained['img'], trained['segm'], trained['classif'], PARAMS, on='device', classif_on='device')
    # step by step through the public functions, the clustering on the host
    params = trained['params']
    _, slic, points, features, names = detection.estim_points_compute_features('', trained['img'], trained['segm'], params)
    zones = np.array([0, 0, -1, 1])[trained['levels']]              # the reference's LUT_ANNOT_CENTER_RELABEL: level 2 does not count
    found = detection.detect_center_candidates(trained['segm'], zones, points, features, params, trained['classif'], classif_on='host')
    assert C.same(found['labels'], trained['classif'].predict(features))
    assert found['points all'] == int(np.sum(np.asarray(detection.label_close_points(zones, points, params)) != -1))
    assert found['points FP'] + found['points FN'] < found['points all'] and 0 < found['precision_binary'] <= 1
    centres, clust_labels = detection.cluster_center_candidates(found['candidates'], params['DBSCAN_max_dist'],
                                                                params['DBSCAN_min_samples'], on='host')
    want = {'slic': slic, 'points': points, 'features': features, 'feature_names': names, 'labels': found['labels'],
            'candidates': found['candidates'], 'clust_labels': clust_labels, 'centres': centres}
    assert same_result(got, want)
    assert C.same(slic, trained['slic']) and C.same(features, trained['features'])
    # six centres, each inside another ellipse
    assert got['centres'].shape == (6, 2)
    hit = [int(trained['eggs'][int(round(row)), int(round(col))]) for row, col in got['centres']]
    assert sorted(hit) == [1, 2, 3, 4, 5, 6]


def test_detect_centers_batch_equals_single_calls(detection, trained):
    single = detection.detect_centers(trained['img'], trained['segm'], trained['classif'], PARAMS, on='device', classif_on='device')
    both = detection.detect_centers_batch([trained['img'], trained['img'].copy()], [trained['segm'], trained['segm']],
                                          trained['classif'], PARAMS, on='device', classif_on='device')
    assert len(both) == 2 and same_result(both[0], single) and same_result(both[1], single)
