"""The host side of the centre detection (pyimsegm_amd/center_detection.py, ``descriptors.shift_ray_features_rows``), without a
device:

* ``dbscan_host`` / ``cluster_center_candidates_host`` -- the definition the device entry is tested against -- equal scikit-learn's
  ``DBSCAN`` and the reference's ``np.mean`` per cluster on every case of tests/center_detection_cases.py, labels and centres with
  ``array_equal`` (no case is dropped from the comparison), and every case reaches the branch it is named for;
* ``shift_ray_features_rows`` equals the row loop of ``shift_ray_features`` byte for byte, shifts as float bits;
* ``compute_points_features`` equals the hand-written composition with ``shifting=True`` (the descriptors have no host path: skipped
  without a device, as the sibling host tests are);
* ``label_close_points``, ``compute_statistic_eggs_centres`` against the reference's statements restated here;
* the ``ValueError``s and the ``(points, [])`` return."""
import numpy as np
import pytest

import center_detection_cases as C


@pytest.fixture(scope='module')
def detection():
    from pyimsegm_amd import center_detection
    return center_detection


@pytest.fixture(scope='module')
def descriptors():
    from pyimsegm_amd import descriptors
    return descriptors


def reference_clustering(points, max_dist, min_samples):
    """``cluster_center_candidates`` of the reference's run_center_clustering.py, restated"""
    from sklearn import cluster
    points = np.array(points)
    if not list(points):
        return points, []
    dbscan = cluster.DBSCAN(eps=max_dist, min_samples=min_samples)
    dbscan.fit(points)
    labels = dbscan.labels_.copy()
    centers = []
    for i in range(max(labels) + 1):
        clust = points[labels == i]
        if len(clust) > 0:
            centers.append(np.mean(clust, axis=0))
    return np.array(centers), labels


@pytest.mark.parametrize('name', list(C.CASES))
def test_statement_equals_scikit_learn_and_the_reference_means(detection, name):
    points, eps, min_samples = C.case(name)
    centres, labels = detection.cluster_center_candidates_host(points, eps, min_samples)
    want_centres, want_labels = reference_clustering(points, eps, min_samples)
    assert labels.dtype == np.int64 and np.array_equal(labels, want_labels)
    assert centres.dtype == np.float64 and centres.shape == want_centres.shape and np.array_equal(centres, want_centres)
    assert np.array_equal(labels, detection.dbscan_host(points, eps, min_samples))


def test_cases_reach_the_branches_they_are_named_for(detection):
    def facts(name):
        points, eps, min_samples = C.case(name)
        return C.facts(points, eps, min_samples, detection.dbscan_host(points, eps, min_samples))

    for name in ('size_63', 'size_65', 'size_1023', 'size_1025', 'size_cap', 'size_cap_plus_1', 'half_integer', 'uniform_float'):
        got = facts(name)
        assert got['border'] > 0 and got['noise'] > 0 and got['clusters'] > 1, name
    assert facts('size_cap')['at_eps'] > 0                            # an inclusive tie among random integer points
    assert facts('line_at_eps') == {'core': 300, 'border': 0, 'noise': 0, 'clusters': 1, 'at_eps': 299}
    assert facts('line_at_eps_min_2')['clusters'] == 1
    assert facts('line_beyond_eps')['clusters'] == 300 and facts('line_beyond_eps')['at_eps'] == 0
    assert facts('line_beyond_eps_min_2')['noise'] == 300
    for name in ('triangles_3_4_5', 'triangles_half_steps'):
        # two clusters that hold together through pairs at eps exactly; without the equality every point is noise
        points, eps, min_samples = C.case(name)
        assert facts(name)['at_eps'] == 5 and facts(name)['clusters'] == 2 and facts(name)['noise'] == 0
        assert np.all(detection.dbscan_host(points, np.nextafter(eps, 0), min_samples) == -1)
    points, eps, min_samples = C.case('duplicates')
    assert detection.dbscan_host(points, eps, min_samples).tolist() == [0, 0, 0, 0, -1, -1, 0, 1, 1, 1, -1]
    # the point between the clusters takes the lower number, and the numbers follow the indices
    assert detection.dbscan_host(*C.case('border_between_two')).tolist() == [0, 0, 0, 0, 0, 1, 1, 1, 1]
    assert detection.dbscan_host(*C.case('border_between_two_reversed')).tolist() == [0, 0, 0, 0, 1, 1, 1, 1, 0]
    assert facts('border_between_two')['border'] == 1 and facts('border_between_two_reversed')['border'] == 1
    centres, labels = detection.cluster_center_candidates_host(*C.case('min_samples_above_size'))
    assert centres.shape == (0, ) and centres.dtype == np.float64 and np.all(labels == -1)
    assert facts('reference_settings')['core'] == 200


def test_clustering_on_the_host_place(detection):
    points, eps, min_samples = C.case('size_65')
    centres, labels = detection.cluster_center_candidates(points, eps, min_samples, on='host')
    want = detection.cluster_center_candidates_host(points, eps, min_samples)
    assert C.same(centres, want[0]) and C.same(labels, want[1])
    # lists and integer tables as the reference takes them
    centres, labels = detection.cluster_center_candidates(points.astype(int).tolist(), eps, min_samples, on='host')
    assert C.same(centres, want[0]) and C.same(labels, want[1])
    sets = [C.case(name)[0] for name in C.BATCH]
    got = detection.cluster_center_candidates_batch(sets, *C.BATCH_SETTINGS, on='host')
    assert len(got) == len(sets)
    for points, (centres, labels) in zip(sets, got):
        if len(points) == 0:
            assert centres is not None and len(centres) == 0 and labels == []
        else:
            want = detection.cluster_center_candidates_host(points, *C.BATCH_SETTINGS)
            assert C.same(centres, want[0]) and C.same(labels, want[1])


def test_no_point_and_refused_input(detection, monkeypatch):
    points, labels = detection.cluster_center_candidates([], on='host')
    assert isinstance(points, np.ndarray) and len(points) == 0 and labels == []
    good = [[1., 2.], [3., 4.]]
    for on in ('host', None):
        if on is None:
            monkeypatch.setenv('IMSEGM_CENTER_DETECT_ON', 'host')
        for points, eps, min_samples in (([[1., np.nan], [3., 4.]], 5, 1), ([[1., np.inf], [3., 4.]], 5, 1), (good, 0, 1), (good, -1., 1),
                                         (good, np.inf, 1), (good, np.nan, 1), (good, 5, 0), ([1., 2., 3.], 5, 1)):
            with pytest.raises(ValueError):
                detection.cluster_center_candidates(points, eps, min_samples, on=on)
    with pytest.raises(ValueError):
        detection.dbscan_host(good, 0, 1)
    with pytest.raises(ValueError):
        detection.cluster_center_candidates(good, on='gpu')


def test_a_table_that_is_not_p_x_2_runs_the_statement(detection):
    from sklearn import cluster
    points = np.random.RandomState(0).randint(0, 30, (80, 3)).astype(np.float64)
    centres, labels = detection.cluster_center_candidates(points, 6, 3, on='host')
    assert np.array_equal(labels, cluster.DBSCAN(eps=6, min_samples=3).fit(points).labels_)
    assert centres.shape == (labels.max() + 1, 3)


def test_parameters_hold_the_settings_of_the_reference(detection):
    assert detection.CENTER_PARAMS == {'slic_size': 25, 'slic_regul': 0.3, 'fts_hist_diams': [10, 50, 100, 200, 300], 'fts_ray_step': 15,
                                       'fts_ray_types': [('up', [0])], 'fts_ray_closer': True, 'fts_ray_smooth': 0, 'center_dist_thr': 50}
    assert detection.CLUSTER_PARAMS == {'DBSCAN_max_dist': 50, 'DBSCAN_min_samples': 1}
    for name in detection.__all__:
        assert hasattr(detection, name), name


# ------------------------------------------------------------------------------------------------
# the rotation of all rows at once
# ------------------------------------------------------------------------------------------------


def _ray_tables():
    rng = np.random.RandomState(5)
    tables = {'random_int': rng.randint(0, 400, (97, 24)),
              'random_float32': rng.randint(0, 400, (97, 24)).astype(np.float32),
              'random_float64': rng.uniform(0, 400, (33, 72)),
              'odd_length': rng.randint(0, 90, (20, 7)),
              'constant_rows': np.full((5, 24), 17, dtype=np.int64),
              'zero_rows': np.zeros((4, 24), dtype=np.float32),
              'four_fold': np.tile(np.array([[9, 4, 1, 1, 4, 8]]), (3, 4)),
              'one_row': rng.randint(0, 50, (1, 12))}
    tables['mixed'] = np.vstack([tables['random_int'][:5], tables['constant_rows'][:2], np.zeros((1, 24), dtype=np.int64),
                                 tables['four_fold'][:1]])
    return tables


@pytest.mark.parametrize('name', list(_ray_tables()))
@pytest.mark.parametrize('method', ['phase', 'max'])
def test_rotation_of_all_rows_equals_the_row_loop(descriptors, name, method):
    rays = _ray_tables()[name]
    loop = [descriptors.shift_ray_features(row, method) for row in rays]
    want = np.array([row for row, _ in loop])
    got, shifts = descriptors.shift_ray_features_rows(rays, method)
    assert C.same(got, want)
    assert isinstance(shifts, list) and len(shifts) == len(loop)
    for (_, a), b in zip(loop, shifts):
        assert type(a) is type(b) and np.asarray(a).tobytes() == np.asarray(b).tobytes()


def test_rotation_of_an_empty_table(descriptors):
    for empty in (np.zeros((0, 24), dtype=np.float32), np.zeros((0, )), np.zeros((0, 0))):
        got, shifts = descriptors.shift_ray_features_rows(empty)
        assert C.same(got, empty) and shifts == []


# ------------------------------------------------------------------------------------------------
# the statements around the classifier
# ------------------------------------------------------------------------------------------------


def test_label_close_points_branches(detection):
    points = [(10, 10), (10, 60), (80, 80), (30, 50)]
    params = {'center_dist_thr': 50}
    labels = detection.label_close_points([(10, 20), (200, 200)], points, params)
    assert labels.dtype == np.bool_ and labels.tolist() == [True, True, False, True]        # (30, 50): 36.06 away; inclusive
    assert detection.label_close_points([(10, 60)], [(10, 10)], params).tolist() == [True]  # at the threshold exactly
    dist, idx = detection.compute_min_dist_2_centers([(10, 20), (90, 80)], points)
    assert dist.tolist() == [10., 40., 10., np.hypot(20, 30)] and idx.tolist() == [0, 0, 1, 0]
    zones = np.zeros((100, 100), dtype=np.uint8)
    zones[5:15, 5:15], zones[75:85, 75:85] = 3, 2
    assert detection.label_close_points(zones, points, params).tolist() == [3, 0, 2, 0]
    assert detection.label_close_points(None, points, params) == [-1] * 4
    assert detection.label_close_points((1, 2), points, params) == [-1] * 4


def reference_statistic_eggs_centres(points, labels, mask_eggs, col_prefix=''):
    """the loop of the reference's run_center_evaluation.py::compute_statistic_eggs_centres, restated"""
    from scipy import ndimage
    dict_case = {}
    unique_eggs = [int(lb) for lb in np.unique(mask_eggs) if lb != 0]
    dict_case[col_prefix + 'eggs annot.'] = len(unique_eggs)
    centers = np.array(points)[labels == 1].astype(int)
    labels_eggs = [1] * len(centers)
    dict_case[col_prefix + 'eggs missed'] = 0
    dict_case[col_prefix + 'eggs multiple'] = 0
    for lb in unique_eggs:
        mask = (mask_eggs == lb)
        inside = mask[centers[:, 0], centers[:, 1]]
        if sum(inside) == 0:
            pos = ndimage.center_of_mass(mask)
            dict_case[col_prefix + 'eggs missed'] += 1
            centers = np.vstack((centers, list(map(int, pos))))
            labels_eggs.append(-1)
        elif sum(inside) > 1:
            dict_case[col_prefix + 'eggs multiple'] += 1
    return dict_case, centers, np.array(labels_eggs)


def _egg_mask():
    mask = np.zeros((120, 160), dtype=np.int32)
    mask[10:40, 10:50] = 1                  # hit once
    mask[10:41, 70:111] = 2                 # hit twice
    mask[60:98, 20:64] = 4                 # missed (label 3 does not occur); its centre of mass has fractions
    mask[60:100, 90:150] = 7                # a ring, missed: its centre of mass lies in the egg inside it
    mask[70:90, 100:140] = 9                # hit by nothing but the centre the ring adds
    return mask


@pytest.mark.parametrize('prefix', ['', 'stage 2: '])
def test_statistic_of_eggs_and_centres_equals_the_reference_loop(detection, prefix):
    mask = _egg_mask()
    points = np.array([[20.7, 30.2], [15, 80], [30.9, 100.1], [50, 5], [99, 5], [25, 25]])
    labels = np.array([1, 1, 1, 1, 0, 0])
    want = reference_statistic_eggs_centres(points, labels, mask, prefix)
    got = detection.compute_statistic_eggs_centres(points, labels, mask, prefix)
    assert got[0] == want[0] and all(type(v) is int for v in got[0].values())
    assert want[0] == {prefix + 'eggs annot.': 5, prefix + 'eggs missed': 2, prefix + 'eggs multiple': 1}
    assert C.same(got[1], want[1]) and C.same(got[2], want[2])
    assert got[2].tolist() == [1, 1, 1, 1, -1, -1]
    # lists go in as arrays do; no detected centre at all
    got = detection.compute_statistic_eggs_centres(points.tolist(), labels.tolist(), mask, prefix)
    assert C.same(got[1], want[1])
    want = reference_statistic_eggs_centres(points, np.zeros(6, dtype=int), mask)
    got = detection.compute_statistic_eggs_centres(points, np.zeros(6, dtype=int), mask)
    assert got[0] == want[0] and C.same(got[1], want[1]) and C.same(got[2], want[2])


class _Votes(object):
    """a classifier the device does not take: predicts by the sign of the first column"""
    classes_ = np.array([0, 1])

    def predict(self, features):
        return (np.asarray(features)[:, 0] > 0).astype(int)


def test_detect_center_candidates_with_a_model_the_device_does_not_take(detection):
    points = [(10, 10), (10, 60), (80, 80), (30, 50)]
    features = np.array([[1.], [-1.], [2.], [3.]])
    params = {'center_dist_thr': 50}
    got = detection.detect_center_candidates(None, None, points, features, params, _Votes())
    assert sorted(got) == ['candidates', 'labels'] and got['labels'].tolist() == [1, 0, 1, 1]
    assert got['candidates'].tolist() == [[10, 10], [80, 80], [30, 50]]
    got = detection.detect_center_candidates(None, [(10, 20), (200, 200)], points, features, params, _Votes())
    assert got['points all'] == 4 and got['points FP'] == 1 and got['points FN'] == 1
    assert got['precision_binary'] == got['recall_binary'] == 2. / 3


def test_forest_labels_are_scikit_learns_predict(detection):
    from sklearn.ensemble import RandomForestClassifier
    rng = np.random.RandomState(1)
    features = rng.uniform(-1, 1, (300, 6))
    target = (features[:, 0] + 0.3 * rng.normal(size=300) > 0).astype(int) * 2 + 1          # classes 1 and 3
    classif = RandomForestClassifier(n_estimators=20, random_state=0, n_jobs=1).fit(features, target)
    fresh = rng.uniform(-1, 1, (200, 6))
    labels = detection.predict_candidates(classif, fresh, classif_on='host')
    assert C.same(labels, classif.predict(fresh))


def test_shapes_that_do_not_match(detection):
    from pyimsegm_amd.utilities import ImageDimensionError
    with pytest.raises(ImageDimensionError):
        detection.estim_points_compute_features('x', np.zeros((20, 30, 3), dtype=np.uint8), np.zeros((20, 31), dtype=int),
                                                detection.CENTER_PARAMS)


def test_points_features_equal_the_composition_with_shifting(detection, descriptors):
    from pyimsegm_amd import _hip
    try:
        present = _hip.device_count() > 0
    except _hip.HipUnavailableError:
        present = False
    if not present:
        pytest.skip('the point descriptors have no host path: needs a device')
    eggs = C.ellipse_eggs()
    segm = (eggs > 0).astype(np.int64) + (eggs > 3)
    points = [(40, 50), (128, 190), (200.6, 300.2), (5, 5), (64, 64)]
    for ray_types, closer in (([('up', [0])], True), ([('up', [0]), ('down', [1])], True), ([('up', [0]), ('down', [1])], False)):
        params = dict(detection.CENTER_PARAMS, fts_ray_types=ray_types, fts_ray_closer=closer, fts_hist_diams=[10, 50])
        features, names = detection.compute_points_features(segm, points, params)
        hist, want_names = descriptors.compute_label_histograms_positions(segm, points, diameters=[10, 50])
        tables = []
        for edge, border in ray_types:
            rays, _, ray_names = descriptors.compute_ray_features_positions(segm, points, angle_step=15, edge=edge, border_labels=border,
                                                                            smooth_ray=0, shifting=len(ray_types) == 1 or not closer)
            tables.append(rays)
            want_names = want_names + ray_names if len(ray_types) == 1 or not closer else want_names
        if len(ray_types) > 1 and closer:
            tables = [np.array([descriptors.shift_ray_features(ray)[0] for ray in np.min(np.array(tables), axis=0)])]
            want_names = want_names + ray_names
        assert C.same(features, np.hstack([hist] + tables)) and names == want_names
