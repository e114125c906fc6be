"""Detection of egg centres: the reference's ``experiments_ovary_centres`` chain -- ``run_center_candidate_training.py``,
``run_center_prediction.py``, ``run_center_clustering.py``, ``run_center_evaluation.py`` -- as library functions under the
reference's names and defaults, without its files, pandas tables and figures.

* :func:`estim_points_compute_features` / :func:`compute_points_features` -- SLIC centres as candidate points and their ring
  histograms and ray distances (one launch each for all points, :mod:`pyimsegm_amd.descriptors`);
* :func:`predict_candidates` / :func:`detect_center_candidates` -- the classifier's labels (on the device for the forests
  :func:`pyimsegm_amd.classification.device_forest` takes) and the reference's statistics against annotated centres;
* :func:`cluster_center_candidates` / :func:`cluster_center_candidates_batch` -- DBSCAN of the positive candidates and one mean per
  cluster; all sets of a batch in ONE device call (``imsegm_dbscan_points``, one workgroup per set);
* :func:`compute_statistic_eggs_centres`, :func:`label_close_points`, :func:`compute_min_dist_2_centers` -- the evaluation statements;
* :func:`detect_centers` / :func:`detect_centers_batch` -- the whole chain for one image or several.

:func:`dbscan_host` is the definition of the clustering ("Centre detection"), in numpy; it equals scikit-learn's
``DBSCAN(eps, min_samples).fit(points).labels_``, whose scan expands one cluster completely before it starts the next.  Where the
clustering runs: ``on='host' | 'device'`` or the environment variable ``IMSEGM_CENTER_DETECT_ON``; with nothing asked, on the device
when one is present.  What ``imsegm_dbscan_points`` does not take runs the statement silently: a set of more than 4096 points, more
than 4096 sets or 2^20 points in a call, a point table that is not P x 2."""
import logging

import numpy as np

from . import _hip, classification, descriptors, superpixels
from .utilities import ImageDimensionError

#: the numeric and feature settings of the reference's ``CENTER_PARAMS``
CENTER_PARAMS = {
    'slic_size': 25,
    'slic_regul': 0.3,
    'fts_hist_diams': [10, 50, 100, 200, 300],
    'fts_ray_step': 15,
    'fts_ray_types': [('up', [0])],
    'fts_ray_closer': True,
    'fts_ray_smooth': 0,
    'center_dist_thr': 50,
}
#: the reference's ``CLUSTER_PARAMS``: the largest distance is about three sampling distances
CLUSTER_PARAMS = {
    'DBSCAN_max_dist': 50,
    'DBSCAN_min_samples': 1,
}

__all__ = ['CENTER_PARAMS', 'CLUSTER_PARAMS', 'dbscan_host', 'cluster_center_candidates_host', 'cluster_center_candidates',
           'cluster_center_candidates_batch', 'compute_points_features', 'estim_points_compute_features', 'compute_min_dist_2_centers',
           'label_close_points', 'predict_candidates', 'detect_center_candidates', 'compute_statistic_eggs_centres', 'detect_centers',
           'detect_centers_batch']


def _place(on):
    """'host' or 'device': ``_hip.resolve_place`` on IMSEGM_CENTER_DETECT_ON ('device' without a device raises)"""
    return _hip.resolve_place(on, 'IMSEGM_CENTER_DETECT_ON', True)[0]


def _check_dbscan(points, eps, min_samples):
    """what scikit-learn's DBSCAN answers with a ValueError; the points as a float64 table P x D"""
    points = np.asarray(points)
    if points.ndim != 2 or points.dtype.kind not in 'biuf':
        raise ValueError('the points have to be a 2-D numeric table, not %s %r' % (points.dtype, points.shape))
    points = np.ascontiguousarray(points, dtype=np.float64)
    if not np.isfinite(points).all():
        raise ValueError('a coordinate is not finite')
    try:
        eps_ok = bool(np.isfinite(eps)) and eps > 0
    except TypeError:
        eps_ok = False
    if not eps_ok:
        raise ValueError('eps must be positive and finite, not %r' % (eps, ))
    if not min_samples >= 1:
        raise ValueError('min_samples must be at least 1, not %r' % (min_samples, ))
    return points


# ------------------------------------------------------------------------------------------------
# the host statements
# ------------------------------------------------------------------------------------------------


def dbscan_host(points, eps, min_samples):
    """ the definition of the clustering, in numpy:

    * ``a`` and ``b`` are *near* when ``dx * dx + dy * dy <= eps * eps`` in float64 (every product and the sum rounded on its own;
      every point is near itself);
    * a point is *core* when at least ``min_samples`` points are near it;
    * clusters are the connected components of the core points under *near*, numbered 0, 1, ... in ascending order of their
      smallest core index;
    * a point that is not core takes the smallest cluster number among the core points near it, -1 (noise) without one.

    :param ndarray points: P x D, numeric and finite
    :param float eps: the largest distance of two near points
    :param int min_samples: near points (itself included) that make a point core
    :return ndarray: int64 [P]
    """
    points = _check_dbscan(points, eps, min_samples)
    count = len(points)
    eps2 = np.float64(eps) * np.float64(eps)
    near = np.empty((count, count), dtype=bool)
    for start in range(0, count, 512):
        dist2 = None
        for axis in range(points.shape[1]):
            diff = points[start:start + 512, None, axis] - points[None, :, axis]
            dist2 = diff * diff if dist2 is None else dist2 + diff * diff
        near[start:start + 512] = dist2 <= eps2 if dist2 is not None else True
    core = np.flatnonzero(near.sum(axis=1) >= min_samples)
    among_core = near[np.ix_(core, core)]
    cluster = np.full(len(core), -1, dtype=np.int64)
    nb_clusters = 0
    for seed in range(len(core)):
        if cluster[seed] >= 0:
            continue
        cluster[seed] = nb_clusters
        frontier = np.array([seed])
        while len(frontier):
            reached = among_core[frontier].any(axis=0) & (cluster < 0)
            cluster[reached] = nb_clusters
            frontier = np.flatnonzero(reached)
        nb_clusters += 1
    labels = np.full(count, -1, dtype=np.int64)
    labels[core] = cluster
    other = np.setdiff1d(np.arange(count), core)
    if len(other) and len(core):
        to_core = near[np.ix_(other, core)]
        labels[other] = np.where(to_core.any(axis=1), np.where(to_core, cluster[None, :], nb_clusters).min(axis=1), -1)
    return labels


def cluster_center_candidates_host(points, max_dist=100, min_samples=1):
    """the numpy statement of :func:`cluster_center_candidates`: :func:`dbscan_host` and ``np.mean(points[labels == i], axis=0)`` per
    cluster -- the sum of the cluster's points in index order over their count"""
    points = np.array(points)
    if not list(points):
        return points, []
    labels = dbscan_host(points, max_dist, min_samples)
    points = np.asarray(points, dtype=np.float64)
    centers = [np.mean(points[labels == i], axis=0) for i in range(max(labels) + 1)]
    return np.array(centers), labels


# ------------------------------------------------------------------------------------------------
# clustering
# ------------------------------------------------------------------------------------------------


def _device_takes(tables):
    """the caps of ``imsegm_dbscan_points`` that show before the call"""
    return (len(tables) <= _hip.DBSCAN_MAX_SETS and sum(len(t) for t in tables) <= _hip.DBSCAN_MAX_TOTAL
            and all(t.ndim == 2 and t.shape[1] == 2 and len(t) <= _hip.DBSCAN_MAX_POINTS and t.dtype.kind in 'biuf' for t in tables))


def _cluster_sets(tables, max_dist, min_samples, on):
    """(centres, labels) of every non-empty table of ``tables``: one device call, or the statement set by set"""
    if tables and _place(on) == 'device' and _device_takes(tables):
        offsets = np.zeros(len(tables) + 1, dtype=np.int32)
        offsets[1:] = np.cumsum([len(t) for t in tables])
        concat = np.ascontiguousarray(np.concatenate(tables, axis=0), dtype=np.float64)
        got = _hip.dbscan_points(concat, offsets, max_dist, min_samples)
        if got is not None:
            labels, counts, centres = got
            out = []
            for start, stop, nb_clusters in zip(offsets[:-1], offsets[1:], counts):
                found = centres[start:start + nb_clusters].copy() if nb_clusters else np.array([])
                out.append((found, labels[start:stop].astype(np.int64)))
            return out
    return [cluster_center_candidates_host(t, max_dist, min_samples) for t in tables]


def cluster_center_candidates(points, max_dist=100, min_samples=1, on=None):
    """ cluster centre candidates by density (the reference's ``cluster_center_candidates``): DBSCAN with ``eps=max_dist`` and one
    mean per cluster.  On the device (``imsegm_dbscan_points``) by default when one is present; ``on='host'`` or
    ``IMSEGM_CENTER_DETECT_ON=host`` runs :func:`cluster_center_candidates_host`, and so does what the entry does not take.
    Coordinates that are not finite, ``max_dist`` that is not positive and finite and ``min_samples`` below 1 raise ``ValueError``
    on both places, as scikit-learn does.

    :param list(list(float)) points: points as (row, col)
    :param float max_dist: the largest distance of two near points
    :param int min_samples: near points that make a core point
    :return tuple(ndarray,ndarray): centres float64 (C, 2) -- shape (0,) without a cluster --, labels int64;
        ``(points, [])`` for no point
    """
    return cluster_center_candidates_batch([points], max_dist, min_samples, on)[0]


def cluster_center_candidates_batch(list_points, max_dist=100, min_samples=1, on=None):
    """ :func:`cluster_center_candidates` of several point sets -- the candidates of several images -- with ONE device call for all
    of them (one workgroup per set).  Empty sets are allowed anywhere and give ``(points, [])``.

    :param list(ndarray) list_points: point sets as (row, col) rows
    :return list(tuple(ndarray,ndarray)): (centres, labels) per set
    """
    tables = [np.array(points) for points in list_points]
    full = [i for i, table in enumerate(tables) if list(table)]
    found = _cluster_sets([tables[i] for i in full], max_dist, min_samples, on)
    out = [(table, []) for table in tables]
    for i, pair in zip(full, found):
        out[i] = pair
    return out


# ------------------------------------------------------------------------------------------------
# candidate points and their features
# ------------------------------------------------------------------------------------------------


def compute_points_features(segm, points, params):
    """ for each point in the segmentation compute the features ``params`` ask for (the reference's ``compute_points_features``):
    the ring histograms of ``fts_hist_diams``, then per entry of ``fts_ray_types`` the ray distances at ``fts_ray_step`` degrees,
    rotated to their main direction -- with ``fts_ray_closer`` and more than one ray type, the element-wise minimum of the tables,
    rotated.  The rays are asked for without the rotation and rotated by :func:`descriptors.shift_ray_features_rows`, all rows in one
    transform; the columns are what ``shifting=True`` returns.

    :param ndarray segm: segmentation
    :param list(tuple(int,int)) points: positions in the image
    :param dict params: parameters
    :return tuple(ndarray,list(str)): features P x F, names
    """
    features, feature_names = np.empty((len(points), 0)), []
    if params.get('fts_hist_diams') is not None:
        features_hist, names_hist = descriptors.compute_label_histograms_positions(segm, points, diameters=params['fts_hist_diams'])
        features = np.hstack((features, features_hist))
        feature_names += names_hist
    names_ray = []
    if params.get('fts_ray_step') is not None:
        list_features_ray = []
        perform_closer = all((params.get('fts_ray_closer', False), len(params['fts_ray_types']) > 1))
        for ray_edge, ray_border in params['fts_ray_types']:
            features_ray, _, names_ray = descriptors.compute_ray_features_positions(
                segm, points, angle_step=params['fts_ray_step'], edge=ray_edge, border_labels=ray_border,
                smooth_ray=params['fts_ray_smooth'], shifting=False)
            if perform_closer:
                list_features_ray.append(features_ray)
            else:
                features = np.hstack((features, descriptors.shift_ray_features_rows(features_ray)[0]))
                feature_names += names_ray
        if perform_closer:
            features_ray = descriptors.shift_ray_features_rows(np.min(np.array(list_features_ray), axis=0))[0]
            features = np.hstack((features, features_ray))
            feature_names += names_ray
    return features, feature_names


def estim_points_compute_features(name, img, segm, params):
    """ determine the points (centre candidates) with SLIC and compute for each its feature vector (the reference's
    ``estim_points_compute_features``)

    :param str name: handed through
    :param ndarray img: image
    :param ndarray segm: segmentation of the same height and width
    :param dict params: parameters
    :return tuple(str,ndarray,list(tuple(int,int)),ndarray,list(str)): name, superpixels, their centres, features, names
    """
    if np.shape(img)[:2] != np.shape(segm)[:2]:
        raise ImageDimensionError('not matching shapes: %r : %r' % (np.shape(img), np.shape(segm)))
    slic = superpixels.segment_slic_img2d(img, params['slic_size'], params['slic_regul'])
    slic_centers = superpixels.superpixel_centers(slic)
    features, feature_names = compute_points_features(segm, slic_centers, params)
    return name, slic, slic_centers, features, feature_names


def compute_min_dist_2_centers(centers, points):
    """ the distance of every point to its closest centre and which centre that is (the reference's statement:
    ``scipy.spatial.distance.cdist`` on the host -- a few thousand by a few dozen distances do not pay for a launch)

    :return tuple(ndarray,ndarray): distances, indexes
    """
    from scipy import spatial
    dists = spatial.distance.cdist(np.array(points), np.array(centers), metric='euclidean')
    return np.min(dists, axis=1), np.argmin(dists, axis=1)


def label_close_points(centers, points, params):
    """ label the points that are close to a centre (the reference's statement, on the host like
    :func:`compute_min_dist_2_centers`, which does not pay for a launch): for a list of centres by ``center_dist_thr``, for a map of
    centre zones by its value at the point, -1 for anything else

    :param ndarray|list(tuple(int,int)) centers: centres or a map of them
    :param list(tuple(int,int)) points: positions in the image
    :param dict params: parameters
    :return list(int)|ndarray:
    """
    if isinstance(centers, list):
        min_dist, _ = compute_min_dist_2_centers(centers, points)
        labels = (min_dist <= params['center_dist_thr'])
    elif isinstance(centers, np.ndarray):
        mx_points = np.array(points, dtype=int)
        labels = centers[mx_points[:, 0], mx_points[:, 1]]
    else:
        logging.warning('not relevant centers info of type "%s"', type(centers))
        labels = [-1] * len(points)
    if len(points) != len(labels):
        raise RuntimeError('not equal lengths of points (%i) and labels (%i)' % (len(points), len(labels)))
    return labels


# ------------------------------------------------------------------------------------------------
# classification of the candidates
# ------------------------------------------------------------------------------------------------


def predict_candidates(classif, features, classif_on=None):
    """ the classifier's label of every candidate.  For a model :func:`classification.device_forest` accepts: the class of the
    largest of :func:`classification.predict_proba` (``classif_on``: where it runs) -- scikit-learn's own forest ``predict`` on the
    same probability bytes; for any other model ``classif.predict(features)``.

    :return ndarray: labels [P]
    """
    forest, _ = classification.device_forest(classif)
    if forest is None:
        return classif.predict(features)
    proba = classification.predict_proba(classif, features, on=classif_on)
    return classif.classes_.take(np.argmax(proba, axis=1), axis=0)


def _statistic_centers(centers_gt, points, labels, params):
    """the reference's ``compute_statistic_centers`` without the figure"""
    labels_gt = np.asarray(label_close_points(centers_gt, points, params))
    mask_valid = (labels_gt != -1)
    labels = np.asarray(labels)[mask_valid]
    labels_gt = labels_gt[mask_valid].astype(int)
    stat = dict(classification.compute_classif_metrics(labels_gt, labels, metric_averages=['binary']))
    stat['points all'] = len(labels)
    stat['points FP'] = np.sum(np.logical_and(labels == 1, labels_gt == 0))
    stat['points FN'] = np.sum(np.logical_and(labels == 0, labels_gt == 1))
    return stat


def detect_center_candidates(segm, centers_gt, points, features, params, classif, classif_on=None):
    """ classify the centre candidates and, where an annotation is given, validate the result (the reference's
    ``detect_center_candidates`` and ``compute_statistic_centers`` without files and figures)

    :param ndarray segm: segmentation (kept for the reference's signature)
    :param centers_gt: None, a list of centres or a map of centre zones (:func:`label_close_points`)
    :param list(tuple(int,int)) points: candidate positions
    :param ndarray features: their features
    :param dict params: parameters
    :param obj classif: fitted classifier
    :return dict: 'candidates' (the points labelled 1), 'labels' and, with ``centers_gt``, the metrics of
        ``compute_classif_metrics(..., metric_averages=['binary'])``, 'points all', 'points FP', 'points FN'
    """
    labels = predict_candidates(classif, features, classif_on)
    dict_centers = {'candidates': np.asarray(points)[np.asarray(labels) == 1], 'labels': labels}
    if centers_gt is not None:
        dict_centers.update(_statistic_centers(centers_gt, points, labels, params))
    return dict_centers


def compute_statistic_eggs_centres(points, labels, mask_eggs, col_prefix=''):
    """ count the annotated eggs that no detected centre hits and those that several hit (the reference's
    ``compute_statistic_eggs_centres`` without the figure).  The reference takes one ``mask_eggs == lb`` pass and one
    ``ndimage.center_of_mass`` per egg; here ONE gather of the map at the centres, one ``np.bincount`` of it and one pair of exact
    integer coordinate sums per label serve all eggs (on the host).  A missed egg adds its truncated centre of mass to the centres,
    and -- as in the reference's loop -- that centre counts for the eggs that come after it.

    :param list(list(float)) points: positions as (row, col)
    :param list(int) labels: 1 marks a detected centre
    :param ndarray mask_eggs: map of annotated eggs, 0 background
    :param str col_prefix: prefix of the keys
    :return tuple(dict,ndarray,ndarray): the counts 'eggs annot.', 'eggs missed', 'eggs multiple'; the centres with those of the
        missed eggs behind them (int); their labels, 1 detected and -1 added
    """
    mask_eggs = np.asarray(mask_eggs)
    centers = np.array(points).reshape(-1, 2)[np.asarray(labels) == 1].astype(int)
    values, inverse = np.unique(mask_eggs, return_inverse=True)
    inverse = inverse.reshape(mask_eggs.shape)
    hits = np.bincount(inverse[centers[:, 0], centers[:, 1]], minlength=len(values))
    pixels = np.bincount(inverse.ravel(), minlength=len(values))
    rows, cols = np.divmod(np.arange(mask_eggs.size), mask_eggs.shape[1])
    # (float64 weights: exact below 2^53)
    sum_rows = np.bincount(inverse.ravel(), weights=rows, minlength=len(values))
    sum_cols = np.bincount(inverse.ravel(), weights=cols, minlength=len(values))
    dict_case = {col_prefix + 'eggs annot.': int(np.sum(values != 0)), col_prefix + 'eggs missed': 0, col_prefix + 'eggs multiple': 0}
    added = []
    for k, value in enumerate(values):
        if value == 0:
            continue
        if hits[k] == 0:
            pos = [int(sum_rows[k] / float(pixels[k])), int(sum_cols[k] / float(pixels[k]))]
            dict_case[col_prefix + 'eggs missed'] += 1
            added.append(pos)
            hits[inverse[pos[0], pos[1]]] += 1
        elif hits[k] > 1:
            dict_case[col_prefix + 'eggs multiple'] += 1
    labels_eggs = np.array([1] * len(centers) + [-1] * len(added))
    if added:
        centers = np.vstack((centers, np.array(added, dtype=centers.dtype)))
    return dict_case, centers, labels_eggs


# ------------------------------------------------------------------------------------------------
# the whole chain
# ------------------------------------------------------------------------------------------------


def _detect_candidates(img, segm, classif, params, classif_on):
    _, slic, points, features, feature_names = estim_points_compute_features('', img, segm, params)
    labels = predict_candidates(classif, features, classif_on)
    return {'slic': slic, 'points': points, 'features': features, 'feature_names': feature_names, 'labels': labels,
            'candidates': np.asarray(points)[np.asarray(labels) == 1]}


def _params(params):
    merged = dict(CENTER_PARAMS)
    merged.update(CLUSTER_PARAMS)
    merged.update(params or {})
    return merged


def detect_centers(img, segm, classif, params=None, on=None, classif_on=None):
    """ the egg centres of one image: superpixels, their centres as candidate points, the features, the classifier's labels, the
    candidates (label 1) and their clustering

    :param ndarray img: image H x W x 3
    :param ndarray segm: its class map H x W
    :param obj classif: fitted classifier of the candidates
    :param dict params: what differs from :data:`CENTER_PARAMS` and :data:`CLUSTER_PARAMS`
    :param str on: where the clustering runs (None, 'host', 'device')
    :param str classif_on: where the classifier runs (:func:`classification.predict_proba`)
    :return dict: 'slic', 'points', 'features', 'feature_names', 'labels', 'candidates', 'clust_labels' and 'centres' as (row, col)
    """
    return detect_centers_batch([img], [segm], classif, params, on, classif_on)[0]


def detect_centers_batch(imgs, segms, classif, params=None, on=None, classif_on=None):
    """ :func:`detect_centers` of several images: the stages per image in turn, the candidates of all images clustered in ONE device
    call

    :return list(dict): per image what :func:`detect_centers` returns
    """
    if len(imgs) != len(segms):
        raise ValueError('one class map per image: %i and %i' % (len(imgs), len(segms)))
    params = _params(params)
    found = [_detect_candidates(img, segm, classif, params, classif_on) for img, segm in zip(imgs, segms)]
    clustered = cluster_center_candidates_batch([one['candidates'] for one in found], params['DBSCAN_max_dist'],
                                                params['DBSCAN_min_samples'], on)
    for one, (centres, clust_labels) in zip(found, clustered):
        one['centres'], one['clust_labels'] = centres, clust_labels
    return found
