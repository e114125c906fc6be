"""What the supervised pipeline (``pipelines.train_classif_color2d_slic_features``, reference ``pipelines.py:292-379``)
needs from the reference's classifier toolbox ``imsegm/classification.py`` -- and nothing else of it.

The toolbox (a dozen classifiers, feature selection, ROC / export helpers, 1 700 lines) is scikit-learn glue that never
touches the device; SURVEY marks it out of scope.  Three of its names sit on the path between the device-computed superpixel
features and the trained model, so they exist here, written against scikit-learn directly:

* :func:`convert_set_features_labels_2_dataset` -- one training set out of the per-image features / labels
  (``classification.py:1416-1476``);
* :class:`CrossValidateGroups` -- folds that hold out whole images (``classification.py:1616-1700``);
* :func:`create_classif_search_train_export` -- scaler -> (PCA) -> classifier, trained once or after a search
  (``classification.py:656-759``).

Scoring class maps against annotations -- how every experiment ends -- is here too, with the reference's signatures, defaults,
return types, keys and error types (``classification.py:305-471, 635-655, 1265-1366``): :data:`METRIC_AVERAGES`,
:func:`relabel_sequential`, :func:`compute_classif_metrics`, :func:`compute_classif_stat_segm_annot`,
:func:`compute_stat_per_image`, :func:`compute_tp_tn_fp_fn`, :func:`compute_metric_fpfn_tpfn` and :func:`compute_metric_tpfp_tpfn`.
Everything they report is a function of the contingency table of the two maps over the labels present.  Each keeps a host
statement (scikit-learn and numpy on the vectors) and takes ``on=None | 'host' | 'device'`` (environment: ``IMSEGM_SCORING_ON``;
the rules of the switch are ``_hip.resolve_place``, and ``'device'`` without a device raises).  On the device one call of
``imsegm_score_pairs`` (csrc/scoring.hip) returns the sorted labels and the exact table of every pair, and the scores are a few
fp64 operations on its integers (:func:`_metrics_from_table`).  The host statement also answers, whatever ``on`` says, what the
device does not take: arrays that are not integers within int32, more than 64 labels in a pair, more than 64 drop labels or one
that is not an int32 integer, an average other than macro / weighted / micro / binary, ``relabel=True`` with a label above
:data:`RELABEL_MAX_LABEL` or without a non-negative label on either side, and inputs that leave no element.  With ``on=None`` the
functions named in :data:`HOST_BY_DEFAULT` run on the host although a device is present (tools/time_scoring.py).

The trained classifier is evaluated by :func:`predict_proba`: ``model.predict_proba`` on the host, or -- ``on='device'``, environment
``IMSEGM_CLASSIF_ON``, default 'host' -- a random forest, extra trees or a single decision tree behind an optional scaler on the
device (csrc/forest.hip), with the bytes of scikit-learn's ``n_jobs=1`` result.  :func:`forest_proba_host` is the numpy statement
of that evaluation on the packed arrays of :class:`_hip.DeviceForest` (DESIGN.md has the definition).

Every other name of the reference module resolves to the reference's own function when a reference package is installed
behind the ``imsegm`` overlay (module ``__getattr__``).
"""
import collections
import logging
import random

import numpy as np

from pyimsegm_amd import _hip
from pyimsegm_amd.labeling import max_overlap_unique_lut
from pyimsegm_amd.utilities import ImageDimensionError, reference_attribute

#: classifier the pipelines train when none is named (``classification.py:47``)
DEFAULT_CLASSIF_NAME = 'RandForest'
#: the 'unique' balancing compares feature vectors after rounding to this many digits (``classification.py:55``)
ROUND_UNIQUE_FTS_DIGITS = 3


def __getattr__(name):
    """names of the reference toolbox that are not part of the path: the reference's own, when one is installed"""
    return reference_attribute('classification', name)


def _classifier(name, nb_workers):
    """the classifiers of ``classification.py:98-123`` by name, with the parameters the reference gives them"""
    from sklearn import ensemble, linear_model, neighbors, svm, tree
    makers = {
        'RandForest': lambda: ensemble.RandomForestClassifier(n_estimators=20, min_samples_leaf=2, min_samples_split=3, n_jobs=nb_workers),
        'GradBoost': lambda: ensemble.GradientBoostingClassifier(subsample=0.25, warm_start=False, max_depth=6, min_samples_leaf=6,
                                                                 n_estimators=200, min_samples_split=7),
        'LogistRegr': lambda: linear_model.LogisticRegression(solver='sag', n_jobs=nb_workers),
        'KNN': lambda: neighbors.KNeighborsClassifier(n_jobs=nb_workers),
        'SVM': lambda: svm.SVC(kernel='rbf', probability=True, tol=2e-3, max_iter=5000),
        'DecTree': lambda: tree.DecisionTreeClassifier(),
        'AdaBoost': lambda: ensemble.AdaBoostClassifier(n_estimators=5),
    }
    if name not in makers:
        raise KeyError('unknown classifier %r (known: %s)' % (name, ', '.join(sorted(makers))))
    return makers[name]()


#: a compact search space per classifier (lists: they serve the grid and the randomised search alike)
_SEARCH_SPACES = {
    'RandForest': {'classif__n_estimators': [10, 20, 40, 80], 'classif__min_samples_split': [2, 3, 5, 9],
                   'classif__min_samples_leaf': [1, 2, 5], 'classif__criterion': ['gini', 'entropy']},
    'GradBoost': {'classif__n_estimators': [50, 100, 200], 'classif__max_depth': [2, 4, 6], 'classif__learning_rate': [0.03, 0.1, 0.3]},
    'LogistRegr': {'classif__C': [0.01, 0.1, 1., 10., 100.]},
    'KNN': {'classif__n_neighbors': [3, 5, 9, 15], 'classif__weights': ['uniform', 'distance']},
    'SVM': {'classif__C': [0.1, 1., 10., 100.], 'classif__gamma': ['scale', 0.01, 0.1, 1.]},
    'DecTree': {'classif__max_depth': [None, 4, 8, 16], 'classif__min_samples_leaf': [1, 2, 5]},
    'AdaBoost': {'classif__n_estimators': [5, 15, 50], 'classif__learning_rate': [0.1, 0.5, 1.]},
}


def create_classif_search_train_export(clf_name, features, labels, cross_val=10, nb_search_iter=100, search_type='random',
                                       eval_metric='f1', nb_workers=1, path_out=None, params=None, pca_coef=0.98,
                                       feature_names=None, label_names=None):
    """ ``Pipeline([StandardScaler, (PCA,) classifier])`` trained on the given samples -- at once, or (``nb_search_iter`` > 1
    or a grid search) refitted with the best parameters of a cross-validated search.  Signature and errors of
    ``classification.py:656-759``; the export to ``path_out`` is not part of this path (returned untouched).

    :return tuple(obj,str): trained pipeline, path_out
    """
    from sklearn import decomposition, metrics, model_selection, pipeline, preprocessing
    if not list(labels):
        raise RuntimeError('some labels has to be given')
    samples = np.nan_to_num(features)
    if len(samples) != len(labels):
        raise ValueError('features (%i) and labels (%i) should have equal length' % (len(samples), len(labels)))
    if samples.ndim != 2 or samples.shape[1] < 1:
        raise ValueError('at least one feature is required')
    stages = [('scaler', preprocessing.StandardScaler())]
    if pca_coef is not None:
        stages += [('reduce_dim', decomposition.PCA(pca_coef))]
    model = pipeline.Pipeline(stages + [('classif', _classifier(clf_name, -1))])
    if nb_search_iter > 1 or search_type == 'grid':
        space = _SEARCH_SPACES.get(clf_name, {})
        classes, dense = np.unique(labels, return_inverse=True)                 # the search sees labels 0 .. n-1
        score_fn = {'f1': metrics.f1_score, 'accuracy': metrics.accuracy_score, 'precision': metrics.precision_score,
                    'recall': metrics.recall_score}[eval_metric.lower()]
        scoring = metrics.make_scorer(score_fn, average='weighted' if len(classes) > 2 else 'binary')
        common = dict(scoring=scoring, cv=cross_val, n_jobs=nb_workers, refit=True)
        if search_type == 'grid':
            search = model_selection.GridSearchCV(model, space, **common)
        else:
            combinations = int(np.prod([len(v) for v in space.values()])) if space else 1
            search = model_selection.RandomizedSearchCV(model, space, n_iter=max(1, min(int(nb_search_iter), combinations)), **common)
        search.fit(samples, dense.tolist())
        logging.info('Best score: %r', search.best_score_)
        model = search.best_estimator_
    model.fit(samples, labels)            # with or without a search: (re)trained on the labels as given
    return model, path_out


def _balanced(samples, labels, how):
    """the samples of ONE image thinned per label (``classification.py:1344-1413``): 'random' / 'kmeans' down to the size of the
    rarest label, 'unique' to the distinct vectors after rounding; labels in ascending order, an unknown method only warns"""
    from sklearn import cluster
    samples, labels = np.array(samples), np.asarray(labels)
    target = min(collections.Counter(labels.tolist()).values())
    kind = how.lower()
    if kind not in ('random', 'kmeans', 'unique'):
        logging.warning('not defined balancing method "%s"', how)
    rows, tags = [], []
    for tag in np.unique(labels):
        block = samples[labels == tag, :]
        if kind == 'unique':
            rounded = np.round(np.asarray(block, dtype=np.float64), ROUND_UNIQUE_FTS_DIGITS)
            block = np.unique(rounded, axis=0).reshape(-1, rounded.shape[1])
        elif kind == 'random' and len(block) > target:
            order = list(range(len(block)))
            random.shuffle(order)
            block = block[order[:target], :]
        elif kind == 'kmeans' and len(block) > target:
            to_centres = cluster.KMeans(n_clusters=target, init='random', n_init=3, max_iter=5).fit_transform(block)
            block = block[np.argmin(to_centres, axis=0), :]        # the sample nearest to every centre
        rows += np.asarray(block).tolist()
        tags += [tag.item()] * len(block)
    return np.array(rows), tags


def convert_set_features_labels_2_dataset(imgs_features, imgs_labels, drop_labels=None, balance_type=None):
    """ the per-image features and labels as one training set: images in sorted key order, ``drop_labels`` removed,
    every image balanced on its own (``classification.py:1416-1476``)

    :return tuple(ndarray,ndarray,list(int)): features, labels, number of samples per image
    """
    if any(key not in imgs_labels for key in imgs_features):
        raise ValueError('missing some items of %r' % imgs_labels.keys())
    rows, tags, sizes = [], [], []
    for key in sorted(imgs_features):
        samples, labels = np.array(imgs_features[key]), np.array(imgs_labels[key]).astype(int)
        keep = ~np.isin(labels, list(drop_labels or []))
        samples, labels = samples[keep], labels[keep]
        if balance_type is not None and len(labels) > 0:
            samples, labels = _balanced(samples, labels, balance_type)
        rows += np.asarray(samples).tolist()
        tags += np.asarray(labels).tolist()
        sizes.append(len(labels))
    return np.array(rows), np.array(tags, dtype=int), sizes


# ---------------------------------------------------------------------------------------------------------------------
# evaluating the trained classifier: tree ensembles on the device, bit for bit
# ---------------------------------------------------------------------------------------------------------------------
def forest_proba_host(packed, table, _defect=None):
    """ the numpy statement of ``predict_proba`` for a packed forest (:class:`_hip.DeviceForest`): what the device computes and what
    ``model.predict_proba(table)`` of scikit-learn returns with ``n_jobs=1``, byte for byte.

    1. scale in float64, ``(x - mean_) / scale_``: two IEEE operations, a true division.  (A float32 table stays float32 inside
       ``StandardScaler.transform``: either operation is then rounded to float32 on its own; the device takes float64 tables.)
    2. round to float32, as scikit-learn's input validation does;
    3. per tree, in order: from node 0, left while ``z[feature] <= threshold`` -- the threshold the largest float32 that is not
       above scikit-learn's float64 one, which decides every float32 value the same way;
    4. the leaf's row of ``leaf_values``;
    5. summed over the trees in order, in float64, from zeros; one division by the number of trees.

    ``_defect`` (tests only) breaks one step: 'lt' compares with ``<``, 'reverse' adds the trees last to first, 'divide_per_tree'
    divides every row before it is added.

    :param packed: :class:`_hip.DeviceForest`
    :param ndarray table: n x F, float64 or float32
    :return ndarray: n x C float64
    """
    table = np.asarray(table)
    if table.ndim != 2 or table.shape[1] != packed.n_features:
        raise ValueError('the table is n x %d' % packed.n_features)
    narrow = table.dtype == np.float32
    scaled = table.astype(np.float64)
    if packed.scaler_mean is not None:
        scaled = scaled - packed.scaler_mean
        if narrow:
            scaled = scaled.astype(np.float32).astype(np.float64)
    if packed.scaler_scale is not None:
        scaled = scaled / packed.scaler_scale
    with np.errstate(over='ignore'):
        z = scaled.astype(np.float32)
    if not (np.isfinite(table).all() and np.isfinite(z).all()):
        raise ValueError('the table holds a value that is not finite in float32')
    rows = np.arange(len(z))
    total = np.zeros((len(z), packed.n_classes), dtype=np.float64)
    order = range(packed.n_trees)
    for tree in (reversed(order) if _defect == 'reverse' else order):
        nodes = packed.nodes[packed.tree_start[tree]:packed.tree_start[tree + 1]]
        threshold, word = nodes['threshold'], nodes['word'].astype(np.int64)
        at = np.zeros(len(z), dtype=np.int64)
        walking = rows[word[at] >= 0]
        for _ in range(len(nodes)):                # (a path visits a node once)
            if not len(walking):
                break
            here = word[at[walking]]
            value = z[walking, here & 0xff]
            left = value < threshold[at[walking]] if _defect == 'lt' else value <= threshold[at[walking]]
            at[walking] = np.where(left, at[walking] + 1, here >> 8)
            walking = walking[word[at[walking]] >= 0]
        contribution = packed.leaf_values[~word[at]]
        total += contribution / packed.n_trees if _defect == 'divide_per_tree' else contribution
    return total if _defect == 'divide_per_tree' else total / packed.n_trees


_device_forests = None


def device_forest(model):
    """:class:`_hip.DeviceForest` of a fitted model (cached per model object as long as its trees are the same objects), or None
    with the reason: ``(forest, reason)``"""
    global _device_forests
    import weakref
    if _device_forests is None:
        _device_forests = weakref.WeakKeyDictionary()
    try:
        steps = [st for _, st in model.steps] if hasattr(model, 'steps') else [model]
        clf = steps[-1]
        # (what the packed arrays are formed from: a refit replaces them)
        key = [getattr(steps[0], 'mean_', None), getattr(steps[0], 'scale_', None), getattr(clf, 'tree_', None)] \
            + list(getattr(clf, 'estimators_', ()))
        hit = _device_forests.get(model)
        if hit is not None and len(hit[0]) == len(key) and all(a is b for a, b in zip(hit[0], key)):
            return hit[1], None
        reason = _hip.forest_refusal(model)
        if reason is not None:
            return None, reason
        forest = _hip.DeviceForest(model)
        _device_forests[model] = (key, forest)
        return forest, None
    except Exception as ex:       # private scikit-learn layout changed, a model that cannot be weakly referenced ...
        return None, 'the model could not be packed: %s' % (ex, )


def classif_place(on):
    """'host' or 'device' for the ``on`` / ``classif_on`` keywords: None reads IMSEGM_CLASSIF_ON, unset means 'host'; any other value
    is a ValueError and 'device' without a device a :class:`_hip.HipUnavailableError` (``_hip.resolve_place``)"""
    place, explicit = _hip.resolve_place(on, 'IMSEGM_CLASSIF_ON', True)
    return place if explicit else 'host'


def device_table(forest, features):
    """``features`` as the float64 table the device takes for ``forest``, or None with the reason: ``(table, reason)``"""
    table = np.asarray(features)
    if table.ndim != 2 or table.dtype not in (np.float64, np.float32) or table.shape[1] != forest.n_features:
        return None, 'the table is not a dense n x %d array of float64 or float32' % forest.n_features
    if table.dtype == np.float32 and (forest.scaler_mean is not None or forest.scaler_scale is not None):
        return None, 'a float32 table is scaled in float32 by scikit-learn'
    return table.astype(np.float64, copy=False), None


def predict_proba(model, features, on=None):
    """ class probabilities of a trained classifier: ``model.predict_proba(features)``, or the same bytes (for ``n_jobs=1``; with
    more jobs scikit-learn adds the trees in the order its threads finish) from the device for the models :class:`_hip.DeviceForest`
    packs.  Asked for the device, a model or a table it does not take is evaluated on the host and the reason logged at INFO.

    :param obj model: fitted classifier or ``Pipeline``
    :param ndarray features: n x F
    :param str on: None, 'host' or 'device'; None: IMSEGM_CLASSIF_ON, unset: 'host'
    :return ndarray: n x C
    """
    if classif_place(on) == 'device':
        forest, reason = device_forest(model)
        table = None
        if forest is not None:
            table, reason = device_table(forest, features)
        if table is not None:
            try:
                return _hip.forest_proba(forest, table)
            except _hip.HipForestInputError as ex:
                reason = str(ex)
        logging.info('class model evaluated on the host: %s', reason)
    return model.predict_proba(features)


class CrossValidateGroups(object):
    """ cross-validation folds over whole sets (images): a fold tests on ``nb_hold_out`` consecutive sets -- a share of
    them when below one -- and trains on all others (``classification.py:1616-1700``)
    """

    def __init__(self, set_sizes, nb_hold_out, rand_seed=None):
        count = len(set_sizes)
        if nb_hold_out <= 0:
            raise ValueError('Number of holdout has to be positive number.')
        if count <= nb_hold_out:
            raise ValueError('Number of holdout has to be smaller then total size.')
        self._per_fold = max(1, int(np.round(count * nb_hold_out)) if nb_hold_out < 1 else int(nb_hold_out))
        ends = np.cumsum([int(size) for size in set_sizes])
        self.set_indexes = [list(range(end - int(size), end)) for end, size in zip(ends, set_sizes)]
        self._order = list(range(count))
        if rand_seed is not None and rand_seed is not False:
            np.random.RandomState(rand_seed).shuffle(self._order)

    def __len__(self):
        return -(-len(self._order) // self._per_fold)

    def _samples(self, sets):
        return [index for which in sorted(sets) for index in self.set_indexes[which]]

    def __iter__(self):
        for first in range(0, len(self._order), self._per_fold):
            held_out = self._order[first:first + self._per_fold]
            yield self._samples(set(self._order) - set(held_out)), self._samples(held_out)


# ---------------------------------------------------------------------------------------------------------------------
# scoring class maps against annotations (reference classification.py:305-471, 635-655, 1265-1366)
# ---------------------------------------------------------------------------------------------------------------------
#: averages ``compute_classif_metrics`` reports when none are named (``classification.py:69``)
METRIC_AVERAGES = ('macro', 'weighted')
#: averages :func:`_metrics_from_table` restates; any other one takes the host statement
_TABLE_AVERAGES = ('macro', 'weighted', 'micro', 'binary')
#: ``relabel=True`` from the table builds the dense overlap of the labels 0 .. max: above this label the host relabels the pixels
RELABEL_MAX_LABEL = 4095
#: functions that run on the host with ``on=None`` although a device is present (profiles/scoring_time.json); ``on='device'``
#: still takes the device
HOST_BY_DEFAULT = frozenset()


def _place(on, name):
    """'host' or 'device' for the public function ``name``: ``_hip.resolve_place`` on IMSEGM_SCORING_ON and -- when neither the
    keyword nor the variable says anything -- ``HOST_BY_DEFAULT``"""
    place, explicit = _hip.resolve_place(on, 'IMSEGM_SCORING_ON', True)
    return place if explicit or name not in HOST_BY_DEFAULT else 'host'


def relabel_sequential(labels, uq_labels=None):
    """ the labels numbered 0, 1, ... in the order of ``uq_labels`` (default: their sorted distinct values), as a list
    (``classification.py:635-653``)

    :param list(int) labels: all labels
    :param list(int) uq_labels: unique labels
    :return list:
    """
    labels = np.asarray(labels)
    if uq_labels is None:
        uq_labels = np.unique(labels)
    lut = np.zeros(np.max(uq_labels) + 1)
    for number, label in enumerate(uq_labels):
        lut[label] = number
    return lut[labels].astype(labels.dtype).tolist()


# ---- the table and what follows from it ----

def contingency_host(y_true, y_pred):
    """the numpy statement of ``imsegm_score_pairs`` for one pair of equally long integer vectors: (labels [U] ascending over
    both, int64 table [U, U] with ``table[a, b]`` = number of elements with ``y_true == labels[a]`` and ``y_pred == labels[b]``)"""
    y_true, y_pred = np.asarray(y_true).ravel(), np.asarray(y_pred).ravel()
    labels, dense = np.unique(np.concatenate([y_true, y_pred]), return_inverse=True)
    dense = dense.ravel()
    flat = dense[:len(y_true)].astype(np.int64) * len(labels) + dense[len(y_true):]
    return labels, np.bincount(flat, minlength=len(labels) ** 2).reshape(len(labels), len(labels)).astype(np.int64)


def _divide_or_zero(numerator, denominator):
    """scikit-learn's ``_prf_divide`` with its default ``zero_division``: 0 where nothing is in the denominator"""
    numerator, denominator = np.asarray(numerator, dtype=np.float64), np.asarray(denominator, dtype=np.float64)
    empty = denominator == 0.
    result = numerator / np.where(empty, 1., denominator)
    result[empty] = 0.
    return result


def _prf_from_table(table, average):
    """``metrics.precision_recall_fscore_support(y_true, y_pred, average=average)`` of scikit-learn 1.7 from the table over the
    labels present (for 'binary' over 0 / 1 with 1 the positive label): (precision, recall, f1, None); ValueError where
    scikit-learn raises one ('binary' with more than two labels)"""
    hits, true_sum, pred_sum = np.diag(table), table.sum(axis=1), table.sum(axis=0)
    if average == 'binary':
        if len(table) > 2:
            raise ValueError("Target is multiclass but average='binary'")
        # one label only: it is label 0 and the positive label 1 has no element
        hits, true_sum, pred_sum = (part[1:2] if len(table) == 2 else np.zeros(1, dtype=np.int64) for part in (hits, true_sum, pred_sum))
    elif average == 'micro':
        hits, true_sum, pred_sum = (np.array([part.sum()]) for part in (hits, true_sum, pred_sum))
    precision, recall = _divide_or_zero(hits, pred_sum), _divide_or_zero(hits, true_sum)
    f_score = _divide_or_zero(2. * hits.astype(np.float64), 1. * true_sum.astype(np.float64) + pred_sum.astype(np.float64))
    if average == 'weighted' and true_sum.sum() != 0:
        return tuple(float(np.average(part, weights=true_sum)) for part in (precision, recall, f_score)) + (None, )
    return tuple(float(np.nanmean(part)) for part in (precision, recall, f_score)) + (None, )


def _ars_from_table(table):
    """``metrics.adjusted_rand_score`` from the table: scikit-learn's pair-confusion formula on Python integers"""
    n_samples = int(table.sum())
    by_true, by_pred = [int(v) for v in table.sum(axis=1)], [int(v) for v in table.sum(axis=0)]
    cells = [[int(v) for v in row] for row in table]
    sum_squares = sum(v * v for row in cells for v in row)
    both = sum_squares - n_samples                                                       # pairs together in both maps
    pred_only = sum(v * by_pred[b] for row in cells for b, v in enumerate(row)) - sum_squares
    true_only = sum(v * by_true[a] for a, row in enumerate(cells) for v in row) - sum_squares
    neither = n_samples ** 2 - pred_only - true_only - sum_squares
    if true_only == 0 and pred_only == 0:
        return 1.0
    # (scikit-learn: tn = neither, fp = pred_only, fn = true_only, tp = both)
    return 2.0 * (both * neither - true_only * pred_only) / ((both + true_only) * (true_only + neither) + (both + pred_only) * (pred_only + neither))


def _metrics_from_table(labels, table, metric_averages):
    """the dictionary of :func:`compute_classif_metrics` from the sorted labels present and their contingency table (at least one
    element): every value is a few fp64 operations on exact integers.  At most two labels count as 0 / 1 (the reference relabels
    them so); an average scikit-learn refuses gives -1 four times (the reference catches it so)."""
    table = np.asarray(table, dtype=np.int64)
    result = {'ARS': _ars_from_table(table), 'accuracy': float(np.trace(table) / table.sum()), 'confusion': table.tolist()}
    for average in metric_averages:
        try:
            values = _prf_from_table(table, average)
        except ValueError:
            values = (-1, ) * 4
        result.update(zip(['%s_%s' % (name, average) for name in ('precision', 'recall', 'f1', 'support')], values))
    return result


def _confusion_cells(labels, table, label_positive=None):
    """:func:`compute_tp_tn_fp_fn` from the labels present and their table"""
    labels = [int(label) for label in labels]
    if len(labels) > 2:
        logging.debug('too many labels: %r', labels)
        return np.nan, np.nan, np.nan, np.nan
    if len(labels) < 2:
        logging.debug('only one label: %r', labels)
        return int(np.sum(table)), 0, 0, 0
    positive = labels.index(label_positive) if label_positive is not None and label_positive in labels else 1
    negative = 1 - positive
    # (the reference's names: "fp" counts the positive annotation with a negative segmentation, "fn" the other way round)
    return table[positive, positive], table[negative, negative], table[positive, negative], table[negative, positive]


def _ratio_fpfn_tpfn(tp, fp, fn):
    if tp == np.nan:                 # (never holds, as in the reference: NaN cells run through the division)
        return np.nan
    if (fp + fn) == 0:
        return 0.
    return float(fp + fn) / float(tp + fn)


def _ratio_tpfp_tpfn(tp, fp, fn):
    if tp == np.nan:
        return np.nan
    if (tp + fn) == 0:
        return 0.
    return float(tp + fp) / float(tp + fn)


def _present(labels, table):
    """labels and table without the labels no element carries on either side"""
    keep = (table.sum(axis=0) + table.sum(axis=1)) > 0
    return np.asarray(labels)[keep], table[np.ix_(keep, keep)]


def _relabel_table(labels, table):
    """``relabel_max_overlap_unique(y_true, y_pred, keep_bg=False)`` applied to the COLUMNS of the table instead of the pixels:
    (labels, table) of the relabelled pair, or None where the host has to relabel the pixels (no non-negative label on a side, a
    label above ``RELABEL_MAX_LABEL``)"""
    labels = np.asarray(labels, dtype=np.int64)
    in_true, in_pred = table.sum(axis=1) > 0, table.sum(axis=0) > 0
    top_true, top_pred = int(labels[in_true].max()), int(labels[in_pred].max())
    if min(top_true, top_pred) < 0 or max(top_true, top_pred) > RELABEL_MAX_LABEL:
        return None
    if int(labels[in_pred].min()) < -(top_pred + 1):
        return None                  # (the host's look-up has no entry that far from its end: the reference's IndexError is its to raise)
    overlap = np.zeros((top_true + 1, top_pred + 1), dtype=np.int64)
    counted = labels >= 0
    overlap[np.ix_(labels[counted & in_true], labels[counted & in_pred])] = table[np.ix_(counted & in_true, counted & in_pred)]
    lut = np.array(max_overlap_unique_lut(overlap, keep_bg=False), dtype=np.int64)
    renamed = np.where(labels < 0, labels, lut[np.clip(labels, 0, top_pred)])          # negative labels keep their column
    union = np.unique(np.concatenate([labels[in_true], renamed[in_pred]]))
    moved = np.zeros((len(union), len(union)), dtype=np.int64)
    rows, cols = np.searchsorted(union, labels[in_true]), np.searchsorted(union, renamed[in_pred])
    np.add.at(moved, np.ix_(rows, cols), table[np.ix_(in_true, in_pred)])
    return union, moved


def _device_vector(arr):
    """the array as the flat C-contiguous uint8 / int32 vector ``_hip.score_pairs`` takes, or None: not integers, outside int32"""
    arr = np.asarray(arr)
    if arr.dtype.kind not in 'iu':
        return None
    if arr.dtype != np.uint8:
        if arr.size and (arr.dtype.itemsize > 4 or arr.dtype == np.uint32) and (int(arr.min()) < -2 ** 31 or int(arr.max()) >= 2 ** 31):
            return None
        arr = arr.astype(np.int32, copy=False)
    return np.ascontiguousarray(arr).ravel()


def _device_drop(drop_labels):
    """the drop list as int32, or None where the device does not take it"""
    if drop_labels is None:
        return np.zeros(0, dtype=np.int32)
    try:
        drop = np.asarray(list(drop_labels))
    except TypeError:
        return None
    if drop.size == 0:
        return np.zeros(0, dtype=np.int32)
    if drop.ndim != 1 or drop.dtype.kind not in 'iu' or len(drop) > _hip.SCORE_MAX_DROP or drop.min() < -2 ** 31 or drop.max() >= 2 ** 31:
        return None
    return drop.astype(np.int32)


def _device_tables(pairs, drop_labels):
    """(labels, table) over the labels present per ``(y_true, y_pred)`` of ``pairs`` from ONE ``_hip.score_pairs`` call; None in
    place of a pair the host statement has to take: arrays the device does not take, too many labels, no element left"""
    results = [None] * len(pairs)
    drop = _device_drop(drop_labels)
    if drop is None:
        return results
    vectors = [(_device_vector(y_true), _device_vector(y_pred)) for y_true, y_pred in pairs]
    taken = [i for i, (v_true, v_pred) in enumerate(vectors) if v_true is not None and v_pred is not None and v_true.size == v_pred.size]
    if not taken:
        return results
    if any(vector.dtype != np.uint8 for i in taken for vector in vectors[i]):       # one dtype per call: int32 unless all are bytes
        vectors = [tuple(v if v is None else v.astype(np.int32, copy=False) for v in pair) for pair in vectors]
    scored = _hip.score_pairs([vectors[i][0] for i in taken], [vectors[i][1] for i in taken], drop)
    for i, answer in zip(taken, scored):
        if answer != _hip.SCORE_TOO_MANY_LABELS and len(answer[0]):
            results[i] = (answer[0].astype(np.int64), answer[1])
    return results


# ---- the public functions ----

def _metrics_host(y_true, y_pred, metric_averages):
    """the host statement of :func:`compute_classif_metrics`: scikit-learn on the vectors"""
    from sklearn import metrics
    logging.debug('unique lbs true: %r, predict %r', np.unique(y_true), np.unique(y_pred))
    present = np.unique(np.hstack((y_true, y_pred)))
    if len(present) <= 2:
        # pos_label=1 has to be a label: two labels count as 0 / 1 for the statistic
        y_true, y_pred = relabel_sequential(y_true, present), relabel_sequential(y_pred, present)
    result = {'ARS': metrics.adjusted_rand_score(y_true, y_pred), 'accuracy': metrics.accuracy_score(y_true, y_pred),
              'confusion': metrics.confusion_matrix(y_true, y_pred).tolist()}
    for average in metric_averages:
        keys = ['%s_%s' % (name, average) for name in ('precision', 'recall', 'f1', 'support')]
        try:
            values = metrics.precision_recall_fscore_support(y_true, y_pred, average=average)
        except Exception:
            logging.exception('metrics.precision_recall_fscore_support')
            values = [-1] * 4
        result.update(zip(keys, values))
    return result


def compute_classif_metrics(y_true, y_pred, metric_averages=METRIC_AVERAGES, on=None):
    """ standard metrics for multi-class classification (``classification.py:305-371``): ARS, accuracy, the confusion matrix over
    the labels present and precision / recall / F1 / support per average

    :param list(int) y_true: annotation
    :param list(int) y_pred: prediction
    :param str|list(str) metric_averages: averages of ``precision_recall_fscore_support``
    :param str on: None, 'host' or 'device'
    :return dict(float):
    """
    y_true, y_pred = np.array(y_true), np.array(y_pred)
    if y_true.shape != y_pred.shape:
        raise ValueError('prediction (%i) and annotation (%i) should be equal' % (len(y_true), len(y_pred)))
    if _place(on, 'compute_classif_metrics') == 'device' and all(average in _TABLE_AVERAGES for average in metric_averages):
        counted = _device_tables([(y_true, y_pred)], None)[0]
        if counted is not None:
            return _metrics_from_table(counted[0], counted[1], metric_averages)
    return _metrics_host(y_true, y_pred, metric_averages)


def _relabel_host(y_true, y_pred):
    """``relabel_max_overlap_unique(y_true, y_pred, keep_bg=False)`` on the vectors in numpy: overlap of the non-negative labels,
    the table of ``labeling.max_overlap_unique_lut``, negative labels stay"""
    extents = [int(np.max(y_true)) + 1, int(np.max(y_pred)) + 1]
    overlap = np.zeros(extents, dtype=np.int64)
    counted = (y_true >= 0) & (y_pred >= 0)
    np.add.at(overlap, (y_true[counted], y_pred[counted]), 1)
    renamed = np.array(max_overlap_unique_lut(overlap, keep_bg=False))[y_pred].astype(np.int64)
    renamed[y_pred < 0] = y_pred[y_pred < 0]
    return renamed


def _stat_from_vectors(y_true, y_pred, name, drop_labels, relabel):
    """the host statement of :func:`compute_classif_stat_segm_annot` on the flat vectors"""
    if drop_labels is not None:
        keep = np.ones(y_true.shape, dtype=bool)
        for label in drop_labels:
            keep[y_true == label] = False
            keep[y_pred == label] = False
        y_true, y_pred = y_true[keep], y_pred[keep]
    if relabel:
        y_pred = _relabel_host(y_true, y_pred)
    stat = _metrics_host(y_true, y_pred, ['macro'])
    if len(np.unique(y_pred)) == 2:
        stat['(FP+FN)/(TP+FN)'] = compute_metric_fpfn_tpfn(y_true, y_pred, on='host')
        stat['(TP+FP)/(TP+FN)'] = compute_metric_tpfp_tpfn(y_true, y_pred, on='host')
    stat['name'] = name
    return stat


def _stat_from_table(labels, table, name, relabel):
    """:func:`compute_classif_stat_segm_annot` from the labels present and their table, or None where the host has to relabel"""
    if relabel:
        moved = _relabel_table(labels, table)
        if moved is None:
            return None
        labels, table = moved
    stat = _metrics_from_table(labels, table, ['macro'])
    if np.count_nonzero(table.sum(axis=0)) == 2:
        tp, _, fp, fn = _confusion_cells(labels, table)
        stat['(FP+FN)/(TP+FN)'] = _ratio_fpfn_tpfn(tp, fp, fn)
        stat['(TP+FP)/(TP+FN)'] = _ratio_tpfp_tpfn(tp, fp, fn)
    stat['name'] = name
    return stat


def _stats(triples, drop_labels, relabel, place):
    """the dictionaries of all ``(annot, segm, name)``: the pairs the device takes in one call, the others by the host statement"""
    triples = list(triples)
    for annot, segm, _ in triples:
        if segm.shape != annot.shape:
            raise ImageDimensionError('dimension do not match for segm: %r - annot: %r' % (segm.shape, annot.shape))
    counted = _device_tables([(annot, segm) for annot, segm, _ in triples], drop_labels) if place == 'device' else [None] * len(triples)
    stats = []
    for (annot, segm, name), answer in zip(triples, counted):
        stat = _stat_from_table(answer[0], answer[1], name, relabel) if answer is not None else None
        stats.append(stat if stat is not None else _stat_from_vectors(annot.ravel(), segm.ravel(), name, drop_labels, relabel))
    return stats


def compute_classif_stat_segm_annot(annot_segm_name, drop_labels=None, relabel=False, on=None):
    """ classification statistic between an annotation and a segmentation (``classification.py:374-421``): the metrics with the
    macro average over the elements where neither map carries a drop label, the two binary ratios when the segmentation holds
    exactly two labels, and the name

    :param tuple(ndarray,ndarray,str) annot_segm_name: annotation, segmentation, name
    :param list(int) drop_labels: labels to be ignored
    :param bool relabel: relabel the segmentation such that its labels match the annotation's best
    :param str on: None, 'host' or 'device'
    :return dict:
    """
    annot, segm, name = annot_segm_name
    return _stats([(annot, segm, name)], drop_labels, relabel, _place(on, 'compute_classif_stat_segm_annot'))[0]


def compute_stat_per_image(segms, annots, names=None, nb_workers=2, drop_labels=None, relabel=False, on=None):
    """ statistic over several segmentations with annotations (``classification.py:424-471``): one row per image, indexed by
    its name.  On the device all pairs go through one ``score_pairs`` call.

    :param list(ndarray) segms: segmentations
    :param list(ndarray) annots: annotations
    :param list(str) names: list of names
    :param int nb_workers: accepted for the reference's callers; neither place starts workers
    :param list(int) drop_labels: labels to be ignored
    :param bool relabel: whether relabel
    :param str on: None, 'host' or 'device'
    :return DF:
    """
    import pandas as pd
    if len(segms) != len(annots):
        raise RuntimeError('size of segment. (%i) amd annot. (%i) should be equal' % (len(segms), len(annots)))
    if not names:
        names = map(str, range(len(segms)))
    frame = pd.DataFrame(_stats(zip(annots, segms, names), drop_labels, relabel, _place(on, 'compute_stat_per_image')))
    frame.set_index('name', inplace=True)
    return frame


def compute_tp_tn_fp_fn(annot, segm, label_positive=None, on=None):
    """ TruePositive, TrueNegative, FalsePositive, FalseNegative of two maps with two labels between them
    (``classification.py:1265-1310``); four NaN for more labels, ``(size, 0, 0, 0)`` for one.  As in the reference "FP" counts the
    positive annotation under a negative segmentation and "FN" the other way round.

    :param ndarray annot: annotation
    :param ndarray segm: segmentation
    :param int label_positive: the positive label (default and when absent: the larger one)
    :param str on: None, 'host' or 'device'
    :return tuple(float,float,float,float):
    """
    y_true, y_pred = np.asarray(annot).ravel(), np.asarray(segm).ravel()
    if _place(on, 'compute_tp_tn_fp_fn') == 'device' and y_true.shape == y_pred.shape:
        counted = _device_tables([(y_true, y_pred)], None)[0]
        if counted is not None:
            return _confusion_cells(counted[0], counted[1], label_positive)
    present = np.unique([y_true, y_pred]).tolist()
    if len(present) > 2:
        logging.debug('too many labels: %r', present)
        return np.nan, np.nan, np.nan, np.nan
    if len(present) < 2:
        logging.debug('only one label: %r', present)
        return len(y_true), 0, 0, 0
    if label_positive is None or label_positive not in present:
        label_positive = present[-1]
    present.remove(label_positive)
    label_negative = present[0]
    tp = np.sum((y_true == label_positive) & (y_pred == label_positive))
    tn = np.sum((y_true == label_negative) & (y_pred == label_negative))
    fp = np.sum((y_true == label_positive) & (y_pred == label_negative))
    fn = np.sum((y_true == label_negative) & (y_pred == label_positive))
    return tp, tn, fp, fn


def compute_metric_fpfn_tpfn(annot, segm, label_positive=None, on=None):
    """ the measure (FP + FN) / (TP + FN) of :func:`compute_tp_tn_fp_fn` (``classification.py:1313-1337``)

    :param ndarray annot: annotation
    :param ndarray segm: segmentation
    :param int label_positive: the positive label
    :param str on: None, 'host' or 'device'
    :return float:
    """
    tp, _, fp, fn = compute_tp_tn_fp_fn(annot, segm, label_positive, on=on)
    return _ratio_fpfn_tpfn(tp, fp, fn)


def compute_metric_tpfp_tpfn(annot, segm, label_positive=None, on=None):
    """ the measure (TP + FP) / (TP + FN) of :func:`compute_tp_tn_fp_fn` (``classification.py:1340-1366``)

    :param ndarray annot: annotation
    :param ndarray segm: segmentation
    :param int label_positive: the positive label
    :param str on: None, 'host' or 'device'
    :return float:
    """
    tp, _, fp, fn = compute_tp_tn_fp_fn(annot, segm, label_positive, on=on)
    return _ratio_tpfp_tpfn(tp, fp, fn)
