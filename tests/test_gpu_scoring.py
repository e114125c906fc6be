"""``imsegm_score_pairs`` (csrc/scoring.hip) and the scoring functions of ``pyimsegm_amd.classification`` on the device.  Labels and
tables are compared for equality with numpy's count (tests/scoring_cases.py ``count``), dictionaries with the host statement of the
same build (floats at 1e-12).  Sizes come from the kernels' constants: the pixels of a lane step, a wave step, a workgroup step and
a workgroup's chunk.  The grid is not capped -- one workgroup per chunk -- so no workgroup takes a second chunk; sizes of several
chunks make several workgroups share a pair's table instead.  No map is larger than 512 x 512."""
import math
import warnings

import numpy as np
import pytest

import scoring_cases as cases
from pyimsegm_amd import _hip
from pyimsegm_amd import classification as clf

pytestmark = pytest.mark.gpu

LANE = _hip.SCORE_RUN
WAVE = 64 * _hip.SCORE_RUN
STEP = _hip.SCORE_THREADS * _hip.SCORE_RUN
CHUNK = _hip.SCORE_CHUNK_PIXELS
SIZES = sorted({0, 1} | {base + off for base in (LANE, WAVE, STEP, CHUNK) for off in (-1, 0, 1)} | {3 * CHUNK + STEP + 5})
RTOL = 1e-12


@pytest.fixture(autouse=True)
def quiet():
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        yield


def own(function):
    assert function.__module__ == 'pyimsegm_amd.classification'
    return function


def vectors(rng, size, labels, agree=0.7, run=5):
    """flat int32 vectors over ``labels`` in runs of about ``run`` pixels"""
    labels = np.asarray(labels, dtype=np.int64)
    annot = labels[np.repeat(rng.integers(0, len(labels), size // run + 1), run)[:size]]
    segm = np.where(rng.random(size) < agree, annot, labels[rng.integers(0, len(labels), size)])
    return annot.astype(np.int32), segm.astype(np.int32)


def check(annot, segm, drop=None):
    """one pair through the device against numpy's count; returns the device's answer"""
    got = _hip.score_pairs([annot], [segm], drop)[0]
    labels, table = cases.count(annot, segm, drop)
    assert got != _hip.SCORE_TOO_MANY_LABELS
    assert got[0].dtype == np.int32 and got[1].dtype == np.int64
    assert np.array_equal(got[0], labels) and np.array_equal(got[1], table)
    return got


def same(got, want, where=''):
    if isinstance(want, dict):
        assert list(got) == list(want), (where, list(got), list(want))
        for key in want:
            same(got[key], want[key], where + '/' + str(key))
    elif isinstance(want, (list, tuple)):
        assert len(got) == len(want), where
        for g, w in zip(got, want):
            same(g, w, where)
    elif isinstance(want, (float, np.floating)):
        assert isinstance(got, (float, np.floating)), (where, type(got))
        assert (math.isnan(got) and math.isnan(want)) or abs(got - want) <= RTOL * abs(want), (where, got, want)
    else:
        assert type(got) is type(want) or isinstance(got, (int, np.integer)) and isinstance(want, (int, np.integer)), (where, got, want)
        assert got == want, (where, got, want)


@pytest.mark.parametrize('size', SIZES)
def test_sizes(size):
    rng = np.random.default_rng(size)
    annot, segm = vectors(rng, size, [0, 1, 2, 3])
    check(annot, segm)
    check(annot.astype(np.uint8), segm.astype(np.uint8))


LABEL_SETS = {'one': [7], 'binary': [0, 255], 'negative': [-1, 0, 3], 'extremes': [cases.INT32_MIN, 0, cases.INT32_MAX],
              'cap': list(range(-20, 172, 3)), 'below_threshold': list(range(_hip.SCORE_WAVE_TABLE_LABELS - 1)),
              'at_threshold': list(range(_hip.SCORE_WAVE_TABLE_LABELS)), 'above_threshold': list(range(_hip.SCORE_WAVE_TABLE_LABELS + 1))}


@pytest.mark.parametrize('name', sorted(LABEL_SETS))
def test_label_sets(name):
    labels = LABEL_SETS[name]
    assert name != 'cap' or len(labels) == _hip.SCORE_MAX_LABELS
    rng = np.random.default_rng(len(labels))
    annot, segm = vectors(rng, 2 * CHUNK + 77, labels)
    got = check(annot, segm)
    assert len(got[0]) == len(labels)


def test_too_many_labels_goes_to_the_host():
    rng = np.random.default_rng(65)
    annot, segm = vectors(rng, 2 * CHUNK + 77, list(range(_hip.SCORE_MAX_LABELS + 1)))
    assert len(np.unique(np.concatenate([annot, segm]))) == _hip.SCORE_MAX_LABELS + 1
    assert _hip.score_pairs([annot], [segm])[0] == _hip.SCORE_TOO_MANY_LABELS
    # far over the cap, in every workgroup
    wide = np.arange(3 * CHUNK, dtype=np.int32)
    assert _hip.score_pairs([wide], [wide])[0] == _hip.SCORE_TOO_MANY_LABELS
    same(own(clf.compute_classif_metrics)(annot, segm, on='device'), clf.compute_classif_metrics(annot, segm, on='host'))


def test_contention_and_run_merging():
    size = 2 * CHUNK + 3 * STEP + 11
    check(np.full(size, 4, dtype=np.int32), np.full(size, 9, dtype=np.int32))              # every pixel the same pair
    board = (np.arange(size) % 2).astype(np.int32)
    check(board, 1 - board)                                                                # no run is merged
    # runs of 13 and of CHUNK - 3 pixels: they straddle lane, wave and workgroup borders
    for run in (13, CHUNK - 3):
        annot = (np.arange(size) // run % 3).astype(np.int32)
        segm = (np.arange(size) // (run + 2) % 2).astype(np.int32)
        check(annot, segm)
        check(annot.astype(np.uint8), segm.astype(np.uint8))


def test_drop_labels():
    rng = np.random.default_rng(5)
    size = CHUNK + STEP + 3
    annot, segm = vectors(rng, size, [0, 1, 2, 5])
    only_annot = np.where(segm == 5, 0, segm).astype(np.int32)
    got = check(annot, only_annot, [5])                       # in one array only
    assert 5 not in got[0]
    got = check(annot, segm, [5, 2])                          # in both
    assert 5 not in got[0] and 2 not in got[0]
    check(annot, segm, [77])                                  # absent
    check(annot, segm, [])
    # a drop label that survives in the other array at other pixels must not appear
    annot2, segm2 = annot.copy(), segm.copy()
    annot2[:STEP], segm2[:STEP] = 1, 5
    got = check(annot2, segm2, [5])
    assert 5 not in got[0]
    # a list that drops every pixel
    labels, table = _hip.score_pairs([annot], [segm], [0, 1, 2, 5])[0]
    assert labels.shape == (0, ) and table.shape == (0, 0)
    with pytest.raises(ValueError) as device_error:
        own(clf.compute_classif_stat_segm_annot)((annot, segm, 'x'), drop_labels=[0, 1, 2, 5], on='device')
    with pytest.raises(ValueError) as host_error:
        clf.compute_classif_stat_segm_annot((annot, segm, 'x'), drop_labels=[0, 1, 2, 5], on='host')
    assert str(device_error.value) == str(host_error.value)
    check(annot, segm, list(range(100, 100 + _hip.SCORE_MAX_DROP)))


def batch():
    rng = np.random.default_rng(8)
    sets = [[0, 1], [0, 255], [-1, 0, 3], list(range(_hip.SCORE_MAX_LABELS + 6)), [7], [0, 1, 2, 3], list(range(40)), [5, 6]]
    sizes = [1, 512 * 384, STEP + 1, 3 * CHUNK, 0, 333 * 200, CHUNK, 17]
    return [vectors(rng, size, labels) for size, labels in zip(sizes, sets)]


def test_batch_equals_single_calls():
    pairs = batch()
    together = _hip.score_pairs([a for a, _ in pairs], [s for _, s in pairs], [3])
    assert together[3] == _hip.SCORE_TOO_MANY_LABELS and together[4][0].size == 0
    for (annot, segm), got in zip(pairs, together):
        alone = _hip.score_pairs([annot], [segm], [3])[0]
        if got == _hip.SCORE_TOO_MANY_LABELS:
            assert alone == _hip.SCORE_TOO_MANY_LABELS
            continue
        labels, table = cases.count(annot, segm, [3])
        assert np.array_equal(got[0], alone[0]) and np.array_equal(got[1], alone[1])
        assert np.array_equal(got[0], labels) and np.array_equal(got[1], table)


def test_batches_above_the_byte_budget_are_split(monkeypatch):
    pairs = batch()
    whole = _hip.score_pairs([a for a, _ in pairs], [s for _, s in pairs])
    monkeypatch.setattr(_hip, 'SCORE_BATCH_BYTES', 8 * CHUNK)
    split = _hip.score_pairs([a for a, _ in pairs], [s for _, s in pairs])
    assert len(split) == len(whole)
    for one, other in zip(whole, split):
        assert (one == other) if isinstance(one, str) or isinstance(other, str) else all(np.array_equal(x, y) for x, y in zip(one, other))


def test_types():
    rng = np.random.default_rng(9)
    annot, segm = vectors(rng, CHUNK + 9, [0, 1, 200, 255])
    wide = check(annot, segm)
    narrow = check(annot.astype(np.uint8), segm.astype(np.uint8))
    assert wide[0].tobytes() == narrow[0].tobytes() and wide[1].tobytes() == narrow[1].tobytes()
    host = clf.compute_classif_metrics(annot, segm, on='host')
    same(own(clf.compute_classif_metrics)(annot.astype(np.int64), segm.astype(np.int64), on='device'), host)
    same(clf.compute_classif_metrics(annot.astype(np.uint8), segm.astype(np.int16), on='device'), host)
    # int64 beyond int32 goes to the host: the device is not asked
    far = annot.astype(np.int64) * 2 ** 31
    assert clf._device_tables([(far, far)], None) == [None]
    same(clf.compute_classif_metrics(far, far, on='device'), clf.compute_classif_metrics(far, far, on='host'))


def test_stale_scratch():
    rng = np.random.default_rng(10)
    big = rng.integers(0, 2 ** 20, 512 * 512).astype(np.int32)
    _hip.labels_overlap(big, big, 1, 1)                       # another entry leaves the shared scratch full of labels
    pairs = batch()
    first = _hip.score_pairs([a for a, _ in pairs], [s for _, s in pairs], [3])
    small = pairs[5:]
    runs = [_hip.score_pairs([a for a, _ in small], [s for _, s in small], [3]) for _ in range(2)]
    for run in runs:
        for got, want in zip(run, first[5:]):
            assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
    again = _hip.score_pairs([a for a, _ in pairs], [s for _, s in pairs], [3])
    for got, want in zip(again, first):
        assert (got == want) if isinstance(want, str) else (got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes())


@pytest.mark.parametrize('relabel', [False, True])
@pytest.mark.parametrize('name', sorted(cases.CASES))
def test_stat_against_the_host_statement(name, relabel):
    annot, segm, drop = cases.CASES[name]
    stat = own(clf.compute_classif_stat_segm_annot)
    try:
        want = stat((annot, segm, name), drop_labels=drop, relabel=relabel, on='host')
    except (IndexError, MemoryError, ValueError) as refused:       # the reference's own refusals: a look-up table too short or too large
        with pytest.raises(type(refused)):
            stat((annot, segm, name), drop_labels=drop, relabel=relabel, on='device')
        return
    same(stat((annot, segm, name), drop_labels=drop, relabel=relabel, on='device'), want)
    same(stat((annot.astype(np.int32), segm.astype(np.int32), name), drop_labels=drop, relabel=relabel, on='device'), want)


@pytest.mark.parametrize('name', sorted(cases.CASES))
def test_metrics_and_cells_against_the_host_statement(name):
    annot, segm, drop = cases.CASES[name]
    y_true, y_pred = cases.kept(annot, segm, drop)
    for averages in (cases.AVERAGES, clf.METRIC_AVERAGES, ['micro'], ['binary']):
        same(own(clf.compute_classif_metrics)(y_true, y_pred, metric_averages=averages, on='device'),
             clf.compute_classif_metrics(y_true, y_pred, metric_averages=averages, on='host'))
    for positive in (None, int(y_true[0])):
        same(list(own(clf.compute_tp_tn_fp_fn)(y_true, y_pred, positive, on='device')), list(clf.compute_tp_tn_fp_fn(y_true, y_pred, positive, on='host')))
    for ratio in (clf.compute_metric_fpfn_tpfn, clf.compute_metric_tpfp_tpfn):
        try:
            want = own(ratio)(y_true, y_pred, on='host')
        except ZeroDivisionError:
            with pytest.raises(ZeroDivisionError):
                ratio(y_true, y_pred, on='device')
            continue
        same(ratio(y_true, y_pred, on='device'), want)


@pytest.mark.parametrize('relabel', [False, True])
def test_stat_per_image(relabel):
    pytest.importorskip('pandas')
    names = [name for name in sorted(cases.CASES) if name not in ('negative_kept', 'extremes')]
    annots, segms = [cases.CASES[name][0] for name in names], [cases.CASES[name][1] for name in names]
    per_image = own(clf.compute_stat_per_image)
    got = per_image(segms, annots, names, drop_labels=[-1], relabel=relabel, on='device')
    want = per_image(segms, annots, names, drop_labels=[-1], relabel=relabel, on='host')
    assert list(got.index) == list(want.index) == names and got.index.name == 'name' and list(got.columns) == list(want.columns)
    for name in names:
        mine, theirs = got.loc[name].to_dict(), want.loc[name].to_dict()
        for key in theirs:
            if isinstance(theirs[key], float) and math.isnan(theirs[key]):
                assert isinstance(mine[key], float) and math.isnan(mine[key]), (name, key)
            else:
                same(mine[key], theirs[key], name + '/' + key)
