"""Seeded (annotation, segmentation) pairs for the scoring tests (tests/test_scoring_reference_host.py, tests/test_gpu_scoring.py,
tests/golden/make_golden_scoring.py).  Small on purpose: a contingency table can go wrong at a label set or at a size, not at a scale.

``CASES`` maps a name to ``(annot, segm, drop_labels)``; the golden file holds what the reference's functions return on ``GOLDEN``.
"""
import numpy as np

INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1


def noisy(rng, shape, labels, agree=0.8):
    """a blocky annotation over ``labels`` and a segmentation that agrees with it on about ``agree`` of the pixels"""
    labels = np.asarray(labels, dtype=np.int64)
    coarse = rng.integers(0, len(labels), (-(-shape[0] // 4), -(-shape[1] // 4)))
    annot = labels[np.kron(coarse, np.ones((4, 4), dtype=np.int64))[:shape[0], :shape[1]]]
    other = labels[rng.integers(0, len(labels), shape)]
    return annot, np.where(rng.random(shape) < agree, annot, other)


def _cases():
    rng = np.random.default_rng(20240607)
    cases = {}
    cases['one_label'] = (np.full((9, 7), 7), np.full((9, 7), 7), None)
    cases['binary_0_255'] = noisy(rng, (33, 41), [0, 255]) + (None, )
    cases['binary_one_sided'] = (noisy(rng, (16, 16), [0, 1])[0], np.ones((16, 16), dtype=np.int64), None)
    cases['three_with_drop'] = noisy(rng, (40, 37), [-1, 0, 3]) + ([-1], )
    cases['three_no_drop'] = noisy(rng, (40, 37), [-1, 0, 3]) + (None, )
    cases['extremes'] = noisy(rng, (21, 19), [INT32_MIN, 0, INT32_MAX]) + (None, )
    cases['four_classes'] = noisy(rng, (64, 48), [0, 1, 2, 3]) + (None, )
    annot, segm = noisy(rng, (64, 48), [0, 1, 2, 3])
    cases['four_permuted'] = (annot, np.array([2, 0, 3, 1])[segm], None)                  # relabelling has work to do
    annot, segm = noisy(rng, (50, 50), [0, 1, 2])
    cases['segm_extra_labels'] = (annot, np.where(rng.random((50, 50)) < 0.1, 9, segm), None)
    annot, segm = noisy(rng, (50, 50), [0, 2, 5, 6])
    cases['annot_more_labels'] = (annot, np.minimum(segm, 2), [6])
    cases['drop_both_sides'] = noisy(rng, (30, 30), [0, 1, 2, 5], agree=0.5) + ([5, 2], )
    cases['drop_absent'] = noisy(rng, (30, 30), [0, 1, 2]) + ([77], )
    cases['many_labels'] = noisy(rng, (60, 60), list(range(0, 120, 3)), agree=0.6) + (None, )
    cases['negative_kept'] = noisy(rng, (30, 31), [-5, -1, 0, 1, 2]) + (None, )
    return cases


CASES = _cases()
#: the cases the golden file records the reference's own answers for (a dozen small pairs)
GOLDEN = ('one_label', 'binary_0_255', 'binary_one_sided', 'three_with_drop', 'three_no_drop', 'four_classes', 'four_permuted',
          'segm_extra_labels', 'annot_more_labels', 'drop_both_sides', 'drop_absent', 'many_labels')
#: the averages the table-to-metrics function restates
AVERAGES = ('macro', 'weighted', 'micro', 'binary')


def kept(annot, segm, drop_labels):
    """the flat vectors of the pixels where neither map carries a drop label"""
    y_true, y_pred = np.asarray(annot).ravel(), np.asarray(segm).ravel()
    keep = ~(np.isin(y_true, list(drop_labels or [])) | np.isin(y_pred, list(drop_labels or [])))
    return y_true[keep], y_pred[keep]


def count(annot, segm, drop_labels=None):
    """numpy's count: (labels int64 [U] ascending, table int64 [U, U]) over the pixels that stay"""
    y_true, y_pred = kept(annot, segm, drop_labels)
    labels = np.unique(np.concatenate([y_true, y_pred]))
    table = np.zeros((len(labels), len(labels)), dtype=np.int64)
    np.add.at(table, (np.searchsorted(labels, y_true), np.searchsorted(labels, y_pred)), 1)
    return labels.astype(np.int64), table
