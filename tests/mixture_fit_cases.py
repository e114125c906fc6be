"""Shared by tests/test_gpu_mixture_fit.py and tests/test_mixture_fit_host.py: the tables of the device-fit tests and the
scikit-learn side of every comparison -- ``KMeans`` from given seeds and the private EM loop of ``GaussianMixture`` that
``graph_cuts.fit_mixture_restarts`` also drives -- so that no expected number ever comes from the device code."""
import os
import warnings

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
N_CLASSES, N_RESTARTS, SEED = 3, 9, 7

#: The tolerance of every parameter comparison, per table: scikit-learn's OWN sensitivity to the order of its sums -- the largest
#: deviation (weights, means, covariances, precision factors relative to 1 + |value|, lower bound) between the EM loop on the table
#: and on a row-permuted copy, tol = 0, 20 iterations from the same one-hot labels, five permutations x nine restarts -- times 16 for
#: the device's different reduction tree, floor 1e-12.  Measured with :func:`reference_sensitivity` (scikit-learn 1.7.2, CPU); the
#: raw deviations are in DESIGN.md section 5.
EM_TOLERANCE = {
    'reference_2048': 16 * 1.167e-07,                # measured 1.167e-07 (two components of this table are nearly singular)
    'reference_c5': 16 * 2.514e-12,                  # measured 2.514e-12
    'plan_features': max(16 * 1.107e-14, 1e-12),     # measured 1.107e-14: the floor
    'synthetic_300k': max(16 * 4.702e-14, 1e-12),    # measured 4.702e-14 (two permutations: 150 s of scikit-learn): the floor
}


def load_table(name):
    from sklearn.preprocessing import StandardScaler
    if name == 'synthetic_300k':
        rng = np.random.RandomState(20261016)
        means = np.array([[0., 0., 0.], [2.5, 1., -1.], [-1., 3., 2.]])
        scales = np.array([[1., .8, 1.2], [.7, 1.1, .9], [1.3, .6, 1.]])
        which = rng.randint(0, 3, 300000)
        raw = means[which] + rng.standard_normal((300000, 3)) * scales[which]
    else:
        file_name, key = {'reference_2048': ('reference_2048.npz', 'features'), 'reference_c5': ('reference_c5.npz', 'normed'),
                          'plan_features': ('class_models.npz', 'plan_features')}[name]
        raw = np.load(os.path.join(GOLDEN, file_name))[key]
    return np.ascontiguousarray(StandardScaler().fit_transform(np.asarray(raw, dtype=np.float64)))


def seeds_of(table, seed=SEED, n_restarts=N_RESTARTS, n_classes=N_CLASSES):
    from sklearn.utils import check_random_state
    from pyimsegm_amd import graph_cuts
    stream = seed if isinstance(seed, np.random.RandomState) else np.random.RandomState(seed)
    return graph_cuts.device_fit_seeds(table, n_classes, n_restarts, check_random_state(stream))


def reference_lloyd(table, seeds):
    """KMeans(algorithm='lloyd') from each restart's seeds: labels R x n, centres, inertia, iterations"""
    from sklearn.cluster import KMeans
    runs = []
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        for start in seeds:
            km = KMeans(len(start), init=start, n_init=1, algorithm='lloyd').fit(table)
            runs.append((km.labels_, km.cluster_centers_, km.inertia_, km.n_iter_))
    return tuple(np.array(v) for v in zip(*runs))


def reference_em(table, labels, tol, max_iter, reg_covar=1e-6):
    """scikit-learn's EM loop (``BaseMixture.fit_predict``) for one restart from one-hot responsibilities.  Returns a dict of the
    parameters after the last completed iteration, the bounds of all iterations, n_iter, converged and ``failed`` (the iteration in
    which scikit-learn raised for a covariance that is not positive definite, else 0)."""
    from sklearn.mixture import GaussianMixture
    n_comp = int(labels.max()) + 1
    gm = GaussianMixture(n_comp, covariance_type='full', tol=tol, max_iter=max_iter, reg_covar=reg_covar)
    resp = np.zeros((len(table), n_comp))
    resp[np.arange(len(table)), labels] = 1
    gm._initialize(table, resp)
    bound, bounds, converged, n_iter, failed = -np.inf, [], False, 0, 0
    kept = gm._get_parameters()
    for n_iter in range(1, max_iter + 1):
        before = bound
        try:
            log_prob_norm, log_resp = gm._e_step(table)
            gm._m_step(table, log_resp)
        except ValueError:
            failed, n_iter = n_iter, n_iter - 1
            gm._set_parameters(kept)
            break
        kept = gm._get_parameters()
        bound = gm._compute_lower_bound(log_resp, log_prob_norm)
        bounds.append(bound)
        if abs(bound - before) < tol:
            converged = True
            break
    weights, means, cov, prec = kept[0], kept[1], kept[2], kept[3]
    return dict(weights=weights, means=means, covariances=cov, precisions_cholesky=prec, lower_bound=bounds[-1] if bounds else -np.inf,
                bounds=bounds, n_iter=n_iter, converged=converged, failed=failed)


def deviation(run_a, run_b):
    """largest difference of two runs' parameters relative to 1 + |value|, and of their lower bounds"""
    worst = 0.
    for key in ('weights', 'means', 'covariances', 'precisions_cholesky', 'lower_bound'):
        a, b = np.asarray(run_a[key], dtype=float), np.asarray(run_b[key], dtype=float)
        worst = max(worst, float(np.max(np.abs(a - b) / (1 + np.abs(b)))))
    return worst


def reference_sensitivity(table, labels, n_permutations=5, max_iter=20):
    """the measurement behind EM_TOLERANCE: scikit-learn against itself on row-permuted copies of the table"""
    rng = np.random.RandomState(1)
    worst = 0.
    plain = [reference_em(table, lab, 0., max_iter) for lab in labels]
    for _ in range(n_permutations):
        order = rng.permutation(len(table))
        moved = np.ascontiguousarray(table[order])
        for lab, run in zip(labels, plain):
            other = reference_em(moved, lab[order], 0., max_iter)
            if other['n_iter'] == run['n_iter']:
                worst = max(worst, deviation(other, run))
    return worst
