"""Cases of the random-forest class model: seeded scikit-learn fits (CPU tests, tests/golden/make_golden_forest.py) and forests
built by hand from plain numpy arrays (GPU tests).  Nothing here needs a device."""
import collections

import numpy as np

#: a fit: the ensemble ('rf': the reference's RandForest parameters, 'et': extra trees, 'tree': one decision tree, 'bestfirst': one
#: tree from the best-first builder, whose scikit-learn layout is not preorder), a scaler in front or not, columns, classes, what
#: the labels are called, and whether column 0 is quantised to adjacent float32 values (ties ``x == threshold``)
Fit = collections.namedtuple('Fit', 'name kind scaler n_features n_classes labels ties')

FITS = tuple(Fit('%s_%s_F%d_C%d' % (kind, 'scaled' if scaler else 'plain', F, C), kind, scaler, F, C, None, False)
             for kind in ('rf', 'et', 'tree') for scaler in (True, False) for F, C in ((1, 2), (9, 3), (180, 8))) + (
    Fit('rf_ties', 'rf', False, 9, 3, None, True),
    Fit('et_ties', 'et', False, 9, 4, None, True),
    Fit('bestfirst', 'bestfirst', True, 9, 3, None, False),
    Fit('rf_labels_2_5_9', 'rf', True, 9, 3, (2, 5, 9), False),
)
#: the fits whose packed forests, tables and scikit-learn probabilities are kept in tests/golden/forest_proba.npz
GOLDEN = ('rf_scaled_F9_C3', 'et_plain_F180_C8', 'tree_scaled_F1_C2', 'rf_ties', 'bestfirst', 'rf_labels_2_5_9')
#: seeds of the data and of the estimators.  With them the 'rf_scaled_F9_C3' probabilities change bits when the trees are added
#: last to first and when every tree's row is divided before it is added (test_forest_reference_host.test_seeded_defects)
DATA_SEED, MODEL_SEED = 20261020, 7
TRAIN_ROWS, TABLE_ROWS = 400, 96


def fit_data(case, rows, seed):
    """(table [rows, F] float64, labels) of a fit: classes that depend on the first and the last column"""
    rng = np.random.RandomState(seed)
    table = rng.randn(rows, case.n_features) * 3. + 1.
    if case.ties:
        # adjacent float32 values around 1: scikit-learn's thresholds fall between two of them, the packed float32 ones on them
        table[:, 0] = np.float32(1.) + rng.randint(-6, 7, rows).astype(np.float32) * np.finfo(np.float32).eps
        score = (table[:, 0] - 1.) / np.finfo(np.float32).eps + table[:, -1]
    else:
        score = table[:, 0] * 1.7 + table[:, -1]
    labels = (np.abs(score) * 1.3).astype(int) % case.n_classes
    if case.labels is not None:
        labels = np.asarray(case.labels)[labels]
    return table, labels


def fit_model(case):
    """the fitted scikit-learn model of a case (``n_jobs=1``: the trees are added in their order)"""
    from sklearn.ensemble import ExtraTreesClassifier, RandomForestClassifier
    from sklearn.pipeline import Pipeline
    from sklearn.preprocessing import StandardScaler
    from sklearn.tree import DecisionTreeClassifier
    clf = {'rf': lambda: RandomForestClassifier(n_estimators=20, min_samples_leaf=2, min_samples_split=3, n_jobs=1, random_state=MODEL_SEED),
           'et': lambda: ExtraTreesClassifier(n_estimators=10, n_jobs=1, random_state=MODEL_SEED),
           'tree': lambda: DecisionTreeClassifier(random_state=MODEL_SEED),
           'bestfirst': lambda: DecisionTreeClassifier(max_leaf_nodes=16, random_state=MODEL_SEED)}[case.kind]()
    model = Pipeline([('scaler', StandardScaler()), ('classif', clf)]) if case.scaler else clf
    return model.fit(*fit_data(case, TRAIN_ROWS, DATA_SEED))


def fit_table(case):
    """the table a fitted case is evaluated on (other rows than it was trained on; the ties of a 'ties' case included)"""
    return fit_data(case, TABLE_ROWS, DATA_SEED + 1)[0]


def fit_by_name(name):
    return next(case for case in FITS if case.name == name)


# ---- forests by hand: (nodes, tree_start, leaf_values) of _hip.DeviceForest.from_arrays -------------------------------------------

def _node_array(thresholds, words):
    from pyimsegm_amd import _hip
    nodes = np.zeros(len(words), dtype=_hip.FOREST_NODE)
    nodes['threshold'], nodes['word'] = thresholds, words
    return nodes


def random_tree(rng, n_leaves, n_features, first_leaf):
    """a random binary tree with ``n_leaves`` leaves in preorder: (thresholds, words); its leaves take the rows from ``first_leaf``"""
    thresholds, words, leaf = [], [], [first_leaf]

    def build(count, first):
        at = len(words)
        if count == 1:
            thresholds.append(0.)
            words.append(~leaf[0])
            leaf[0] += 1
            return
        left = int(rng.randint(1, count))
        thresholds.append(float(np.float32(rng.randn())))
        words.append(0)
        build(left, first)
        words[at] = int(rng.randint(n_features)) | ((len(words) - first) << 8)      # (the right child, counted from the tree's root)
        build(count - left, first)

    build(n_leaves, len(words))
    return thresholds, words


def random_forest(n_trees, n_leaves, n_features, n_classes, seed, scaler=True):
    """``_hip.DeviceForest`` of ``n_trees`` random trees of ``n_leaves`` leaves each, random leaf rows, a random scaler or none"""
    from pyimsegm_amd import _hip
    rng = np.random.RandomState(seed)
    thresholds, words, starts = [], [], [0]
    for tree in range(n_trees):
        th, wo = random_tree(rng, n_leaves, n_features, tree * n_leaves)
        thresholds += th
        words += wo
        starts.append(len(words))
    values = rng.rand(n_trees * n_leaves, n_classes)
    values /= values.sum(axis=1, keepdims=True)
    mean = rng.randn(n_features) if scaler else None
    scale = 0.5 + rng.rand(n_features) if scaler else None
    return _hip.DeviceForest.from_arrays(_node_array(thresholds, words), starts, values, n_features, mean, scale)


def chain_forest(depth, n_features, n_classes, seed, side, threshold=-1.5):
    """one tree that is a chain of ``depth`` inner nodes, each with a leaf on the other side: ``side`` 'right' -- the chain goes down
    the right children (a row stops where ``z <= `` the node's threshold, drawn around ``threshold``) -- or 'left' (around
    ``-threshold``).  2 * depth + 1 nodes."""
    from pyimsegm_amd import _hip
    rng = np.random.RandomState(seed)
    count = 2 * depth + 1
    thresholds, words = np.zeros(count, dtype=np.float32), np.zeros(count, dtype=np.int64)
    features = rng.randint(n_features, size=depth)
    spread = threshold + 0.8 * rng.randn(depth)                 # (a row that passes a column at one node may stop at it further down)
    if side == 'right':
        inner = 2 * np.arange(depth)                             # inner 0, leaf 1, inner 2, leaf 3, ..., leaf 2 * depth
        words[inner] = features | ((inner + 2) << 8)
        thresholds[inner] = spread
        leaves = np.concatenate([inner + 1, [2 * depth]])
    else:
        inner = np.arange(depth)                                 # inner 0 .. depth - 1, then the leaves from the deepest one up
        words[inner] = features | ((2 * depth - inner) << 8)
        thresholds[inner] = -spread
        leaves = np.arange(depth, count)
    words[leaves] = ~np.arange(len(leaves))
    values = rng.rand(len(leaves), n_classes)
    values /= values.sum(axis=1, keepdims=True)
    return _hip.DeviceForest.from_arrays(_node_array(thresholds, words), [0, count], values, n_features)


def single_leaf_forest(n_features, n_classes):
    from pyimsegm_amd import _hip
    return _hip.DeviceForest.from_arrays(_node_array([0.], [~0]), [0, 1], np.full((1, n_classes), 1. / n_classes), n_features)


def hand_table(rows, n_features, seed):
    """random rows, with one row far below and one far above every threshold (they walk a chain to its end)"""
    table = np.random.RandomState(seed).randn(rows, n_features)
    if rows > 2:
        table[rows // 3], table[2 * rows // 3] = -10., 10.
    return table
