"""The scoring functions of ``pyimsegm_amd.classification`` without a GPU: the eight names and their signatures, the reference's
doctest values and its recorded results on the small pairs of tests/scoring_cases.py (tests/golden/scoring.json, integers and lists
equal, floats at 1e-12), the table-to-metrics function against scikit-learn called on the vectors, and ``relabel=True`` applied to the
table's columns against the host route that relabels the pixels."""
import inspect
import json
import math
import os
import re
import warnings

import numpy as np
import pytest

import scoring_cases as cases
from pyimsegm_amd import _hip
from pyimsegm_amd import classification as clf

HERE = os.path.dirname(os.path.abspath(__file__))
RTOL = 1e-12


def golden(name):
    with open(os.path.join(HERE, 'golden', name)) as fp:
        return json.load(fp)


@pytest.fixture(scope='module')
def recorded():
    return golden('scoring.json')


@pytest.fixture(autouse=True)
def quiet():
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')          # scikit-learn's "ill-defined" warnings: the zeros they announce are compared
        yield


def own(function):
    assert function.__module__ == 'pyimsegm_amd.classification'
    return function


def same(got, want, where=''):
    """integers, strings, None and lists equal; floats within RTOL; 'nan' in the file is NaN"""
    if isinstance(want, dict):
        assert isinstance(got, dict) and list(got) == list(want), (where, list(got), list(want))
        for key in want:
            same(got[key], want[key], where + '/' + str(key))
    elif isinstance(want, (list, tuple)):
        assert len(got) == len(want), where
        for i, (g, w) in enumerate(zip(got, want)):
            same(g, w, where + '[%i]' % i)
    elif (isinstance(want, str) and want == 'nan') or (isinstance(want, float) and math.isnan(want)):
        assert isinstance(got, float) and math.isnan(got), (where, got)
    elif isinstance(want, float):
        assert isinstance(got, (float, np.floating)), (where, type(got))
        assert abs(got - want) <= RTOL * abs(want), (where, got, want)
    elif want is None or isinstance(want, str):
        assert got == want or (want is None and got is None), (where, got, want)
    else:
        assert isinstance(got, (int, np.integer)) and not isinstance(got, bool) and int(got) == want, (where, got, want)


def attempt(call, want):
    if isinstance(want, dict) and 'raises' in want:
        with pytest.raises(Exception) as caught:
            call()
        assert type(caught.value).__name__ == want['raises']
        return
    got = call()
    same(list(got) if isinstance(got, tuple) else got, want)


def test_names_and_signatures():
    names = golden('scoring_names.json')
    assert list(own_constant('METRIC_AVERAGES')) == names['constants']['METRIC_AVERAGES'] and isinstance(clf.METRIC_AVERAGES, tuple)
    assert len(names['functions']) == 7
    for name, parameters in names['functions'].items():
        function = own(getattr(clf, name))
        mine = [[key, None if p.default is inspect.Parameter.empty else p.default] for key, p in inspect.signature(function).parameters.items()]
        mine = [[key, list(default) if isinstance(default, tuple) else default] for key, default in mine]
        assert mine[:len(parameters)] == parameters, name
        # the one keyword this project adds, last (relabel_sequential is a table look-up on a list: it has no other place to run)
        assert mine[len(parameters):] == ([] if name == 'relabel_sequential' else [['on', None]]), name


def own_constant(name):
    assert name in vars(clf)                 # (defined in the module itself, not handed out by its __getattr__)
    return vars(clf)[name]


def test_kernel_constants_match_the_header():
    header = open(os.path.join(os.path.dirname(HERE), 'include', 'imsegm_hip.h')).read()
    declared = {name: int(value) for name, value in re.findall(r'#define IMSEGM_SCORE_(\w+) (\d+)', header)}
    for name in ('MAX_LABELS', 'MAX_DROP', 'THREADS', 'RUN', 'CHUNK_STEPS', 'WAVE_TABLE_LABELS'):
        assert getattr(_hip, 'SCORE_' + name) == declared[name], name
    assert _hip.SCORE_CHUNK_PIXELS == declared['THREADS'] * declared['RUN'] * declared['CHUNK_STEPS']
    assert 'imsegm_score_pairs' in _hip.EXPORTED_SYMBOLS


def test_doctest_values(recorded):
    doc = recorded['doctests']
    np.random.seed(0)
    y_true, y_pred = np.random.randint(0, 3, 25) * 2, np.random.randint(0, 2, 25) * 2
    metrics = own(clf.compute_classif_metrics)
    same(metrics(y_true, y_true, on='host'), doc['metrics_same'])
    same(metrics(y_true, y_pred, on='host'), doc['metrics'])
    same(metrics(y_pred, y_pred, on='host'), doc['metrics_pred'])
    assert doc['metrics']['confusion'] == [[3, 7, 0], [5, 5, 0], [1, 4, 0]] and doc['metrics_same']['accuracy'] == 1.0
    np.random.seed(0)
    annot, segm = np.random.randint(0, 2, (5, 10)), np.random.randint(0, 2, (5, 10))
    stat = own(clf.compute_classif_stat_segm_annot)
    same(stat((annot, annot, 'ttt'), relabel=True, drop_labels=[5], on='host'), doc['stat_same'])
    same(stat((annot, segm, 'ttt'), relabel=True, drop_labels=[5], on='host'), doc['stat'])
    same(stat((annot, segm + 1, 'ttt'), relabel=False, drop_labels=[0], on='host'), doc['stat_shifted'])
    assert doc['stat_shifted']['confusion'] == [[13, 17], [0, 0]] and doc['stat_same']['(TP+FP)/(TP+FN)'] == 1.0
    assert own(clf.relabel_sequential)([0, 0, 0, 5, 5, 5, 0, 5]) == doc['relabel_sequential'] == [0, 0, 0, 1, 1, 1, 0, 1]
    np.random.seed(0)
    annot, segm = np.random.randint(0, 2, (5, 7)) * 9, np.random.randint(0, 2, (5, 7)) * 9
    cells = own(clf.compute_tp_tn_fp_fn)
    same(list(cells(annot, annot, on='host')), doc['cells_same'])
    same(list(cells(annot, segm, on='host')), doc['cells'])
    same(list(cells(annot, np.ones((5, 7)), on='host')), doc['cells_ones'])
    same(list(cells(np.zeros((5, 7)), np.zeros((5, 7)), on='host')), doc['cells_zeros'])
    assert doc['cells'] == [9, 5, 11, 10] and doc['cells_zeros'] == [35, 0, 0, 0]
    np.random.seed(0)
    annot, segm = np.random.randint(0, 2, (50, 75)) * 3, np.random.randint(0, 2, (50, 75)) * 3
    same([own(clf.compute_metric_fpfn_tpfn)(annot, other, on='host') for other in (segm, annot, np.ones((50, 75)))], doc['fpfn_tpfn'])
    same([own(clf.compute_metric_tpfp_tpfn)(annot, other, on='host') for other in (segm, annot, np.ones((50, 75)), np.zeros((50, 75)))],
         doc['tpfp_tpfn'])


def test_doctest_values_per_image(recorded):
    pytest.importorskip('pandas')
    doc = recorded['doctests']
    np.random.seed(0)
    img_true, img_pred = np.random.randint(0, 3, (50, 100)), np.random.randint(0, 2, (50, 100))
    per_image = own(clf.compute_stat_per_image)
    frame = per_image([img_true], [img_true], nb_workers=2, relabel=True, on='host')
    assert frame.index.name == 'name' and list(frame.index) == ['0']
    same(frame.iloc[0].to_dict(), doc['per_image_same'])
    same(per_image([img_true], [img_pred], drop_labels=[-1], on='host').iloc[0].to_dict(), doc['per_image'])
    assert doc['per_image']['confusion'] == [[836, 826, 770], [836, 856, 876], [0, 0, 0]]
    with pytest.raises(RuntimeError):
        per_image([img_true], [], on='host')


@pytest.mark.parametrize('name', cases.GOLDEN)
def test_recorded_reference_results(recorded, name):
    annot, segm, drop = cases.CASES[name]
    want = recorded['cases'][name]
    y_true, y_pred = cases.kept(annot, segm, drop)
    stat = own(clf.compute_classif_stat_segm_annot)
    attempt(lambda: stat((annot, segm, name), drop_labels=drop, relabel=False, on='host'), want['stat'])
    attempt(lambda: stat((annot, segm, name), drop_labels=drop, relabel=True, on='host'), want['stat_relabel'])
    attempt(lambda: own(clf.compute_classif_metrics)(y_true, y_pred, metric_averages=cases.AVERAGES, on='host'), want['metrics'])
    attempt(lambda: own(clf.compute_tp_tn_fp_fn)(y_true, y_pred, on='host'), want['tp_tn_fp_fn'])
    attempt(lambda: own(clf.compute_metric_fpfn_tpfn)(y_true, y_pred, on='host'), want['fpfn_tpfn'])
    attempt(lambda: own(clf.compute_metric_tpfp_tpfn)(y_true, y_pred, on='host'), want['tpfp_tpfn'])


@pytest.mark.parametrize('name', sorted(cases.CASES))
def test_table_to_metrics_against_scikit_learn(name):
    """scikit-learn on the vectors at run time against the table route, the table counted by numpy: every float is a handful of fp64
    operations on exact integers, so at most the rounding of the last operations may differ"""
    from sklearn import metrics
    annot, segm, drop = cases.CASES[name]
    y_true, y_pred = cases.kept(annot, segm, drop)
    labels, table = cases.count(annot, segm, drop)
    host_labels, host_table = clf.contingency_host(y_true, y_pred)
    assert np.array_equal(host_labels, labels) and np.array_equal(host_table, table)
    got = clf._metrics_from_table(labels, table, cases.AVERAGES)
    if len(labels) <= 2:
        y_true, y_pred = np.searchsorted(labels, y_true), np.searchsorted(labels, y_pred)
    assert got['confusion'] == metrics.confusion_matrix(y_true, y_pred).tolist()
    same(got['ARS'], float(metrics.adjusted_rand_score(y_true, y_pred)), 'ARS')
    same(got['accuracy'], float(metrics.accuracy_score(y_true, y_pred)), 'accuracy')
    for average in cases.AVERAGES:
        try:
            want = metrics.precision_recall_fscore_support(y_true, y_pred, average=average)
        except ValueError:
            want = (-1, ) * 4
        for key, value in zip(('precision', 'recall', 'f1', 'support'), want):
            same(got['%s_%s' % (key, average)], value, key + '_' + average)
    # the whole dictionary, keys in order, against the module's own host statement
    same(got, clf._metrics_host(y_true, y_pred, cases.AVERAGES))
    # the binary cells and ratios from the table
    for positive in (None, int(labels[0]), 12345):
        want = clf.compute_tp_tn_fp_fn(*cases.kept(annot, segm, drop), label_positive=positive, on='host')
        same(list(clf._confusion_cells(labels, table, positive)), [value if value == value else 'nan' for value in want])


@pytest.mark.parametrize('name', sorted(cases.CASES))
def test_relabel_on_the_table_against_relabelled_pixels(name):
    annot, segm, drop = cases.CASES[name]
    y_true, y_pred = cases.kept(annot, segm, drop)
    labels, table = cases.count(annot, segm, drop)
    moved = clf._relabel_table(labels, table)
    if max(y_true.max(), y_pred.max()) > clf.RELABEL_MAX_LABEL or min(y_true.max(), y_pred.max()) < 0:
        assert moved is None
        return
    if y_pred.min() < -(y_pred.max() + 1):           # the reference's look-up table is too short for that label: IndexError
        assert moved is None
        with pytest.raises(IndexError):
            clf._relabel_host(y_true, y_pred)
        return
    want_labels, want_table = cases.count(y_true, clf._relabel_host(y_true, y_pred))
    assert np.array_equal(moved[0], want_labels) and np.array_equal(moved[1], want_table)
    got = clf._stat_from_table(labels, table, name, True)
    same(got, clf._stat_from_vectors(y_true, y_pred, name, None, True))
    same(clf._stat_from_table(labels, table, name, False), clf._stat_from_vectors(y_true, y_pred, name, None, False))


def test_relabel_refuses_large_dense_overlaps():
    labels, table = cases.count(np.array([0, 1, clf.RELABEL_MAX_LABEL + 1]), np.array([0, 1, 1]))
    assert clf._relabel_table(labels, table) is None
    labels, table = cases.count(np.array([-3, -3]), np.array([0, 1]))
    assert clf._relabel_table(labels, table) is None


def test_errors_and_host_only_inputs():
    from pyimsegm_amd.utilities import ImageDimensionError
    with pytest.raises(ValueError):
        clf.compute_classif_metrics([0, 1, 1], [0, 1], on='host')
    with pytest.raises(ImageDimensionError):
        clf.compute_classif_stat_segm_annot((np.zeros((3, 4), dtype=int), np.zeros((4, 3), dtype=int), 'x'), on='host')
    with pytest.raises(ValueError):
        clf.compute_classif_stat_segm_annot((np.zeros((3, 4), dtype=int), np.zeros((3, 4), dtype=int), 'x'), drop_labels=[0], on='host')
    with pytest.raises(ValueError):
        clf.compute_classif_metrics([0, 1], [0, 1], on='nowhere')
    # an average the table route does not restate: the four -1 of the reference
    got = clf.compute_classif_metrics([0, 1, 1], [0, 1, 0], metric_averages=['samples'], on='host')
    assert [got[key + '_samples'] for key in ('precision', 'recall', 'f1', 'support')] == [-1] * 4
    assert clf._device_vector(np.array([0.5, 1.])) is None and clf._device_vector(np.array([2 ** 31])) is None
    assert clf._device_vector(np.array([-2 ** 31, 2 ** 31 - 1])).dtype == np.int32
    assert clf._device_vector(np.zeros((2, 2), dtype=np.uint8)).dtype == np.uint8
    assert clf._device_drop([1.5]) is None and clf._device_drop([2 ** 31]) is None and clf._device_drop(range(65)) is None
    assert clf._device_drop(None).size == 0 and clf._device_drop([-1, 3]).tolist() == [-1, 3]


def test_without_a_device_the_host_statement_runs():
    if _hip.device_count() > 0:
        pytest.skip('a GPU is present')
    annot, segm, _ = cases.CASES['four_classes']
    same(clf.compute_classif_metrics(annot.ravel(), segm.ravel()), clf.compute_classif_metrics(annot.ravel(), segm.ravel(), on='host'))
    with pytest.raises(_hip.HipUnavailableError):
        clf.compute_classif_metrics(annot.ravel(), segm.ravel(), on='device')
