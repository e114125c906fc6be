"""Shared by tests/test_gpu_bayes_fit.py and tests/test_bayes_fit_host.py: the tables of the tests of the variational fit on the
device and the scikit-learn side of every comparison -- the private loop of ``BayesianGaussianMixture`` from one-hot
responsibilities, as tests/mixture_fit_cases.py has it for ``GaussianMixture`` -- so that no expected number ever comes from the
device code."""
import numpy as np

import mixture_fit_cases as MC

PROCESS, DISTRIBUTION = 'dirichlet_process', 'dirichlet_distribution'
GOLDEN_TABLES = ('plan_features', 'reference_c5', 'reference_2048')
#: table -> (components, restarts, prior types)
CASES = {
    'plan_features': (3, 9, (PROCESS, DISTRIBUTION)),
    'reference_c5': (3, 9, (PROCESS, )),
    'reference_2048': (3, 9, (PROCESS, )),
    'one_feature': (2, 3, (PROCESS, )),
    'caps_edge': (8, 2, (PROCESS, )),
    'dying': (5, 3, (PROCESS, DISTRIBUTION)),
}
PARAMETERS = ('weight_concentration', 'mean_precision', 'means', 'degrees_of_freedom', 'covariances', 'precisions_cholesky')

#: The tolerance of every comparison, per table, built as MC.EM_TOLERANCE is: scikit-learn's OWN sensitivity to the order of its
#: sums -- the largest deviation (the six parameter arrays and the lower bound, relative to 1 + |value|) between the variational
#: loop on the table and on a row-permuted copy, tol = 0, 20 iterations from the same one-hot labels, five permutations x all
#: restarts x the table's prior types -- times 16 for the device's different reduction tree, floor 1e-12.  Measured with
#: :func:`reference_sensitivity` (scikit-learn 1.7.2, CPU), twice with the same result; the raw deviations are in DESIGN.md section 5.
BAYES_TOLERANCE = {
    'plan_features': max(16 * 1.125e-14, 1e-12),     # measured 1.125e-14: the floor
    'reference_c5': 16 * 1.181e-12,                  # measured 1.181e-12
    'reference_2048': 16 * 2.032e-08,                # measured 2.032e-08 (two components of this table are nearly singular)
    'one_feature': max(16 * 1.2e-14, 1e-12),         # measured 1.200e-14: the floor
    'caps_edge': max(16 * 1.315e-15, 1e-12),         # measured 1.315e-15: the floor
    'dying': 16 * 1.361e-13,                         # measured 1.361e-13 (components down to nk = 5e-9 after 20 iterations)
}


def load_table(name):
    """the standardised table of a case (the golden ones are MC.load_table's)"""
    if name in GOLDEN_TABLES:
        return MC.load_table(name)
    if name == 'one_feature':
        rng = np.random.RandomState(20261021)
        raw = np.concatenate([rng.standard_normal(170) * 0.6 - 2., rng.standard_normal(130) * 1.1 + 3.])[:, None]
    elif name == 'caps_edge':
        rng = np.random.RandomState(20261022)
        raw = rng.standard_normal((700, 16)) + (rng.standard_normal((8, 16)) * 4.)[np.arange(700) % 8]
    elif name == 'dying':
        rng = np.random.RandomState(20261023)
        raw = rng.standard_normal((600, 2)) * np.array([1., 0.7]) + np.array([[-8., 0.], [8., 3.]])[np.arange(600) % 2]
    else:
        raise KeyError(name)
    from sklearn.preprocessing import StandardScaler
    return np.ascontiguousarray(StandardScaler().fit_transform(raw))


def seeds_of(name, table):
    n_classes, n_restarts, _ = CASES[name]
    return MC.seeds_of(table, MC.SEED, n_restarts, n_classes)


def labels_of(name, table):
    """the start labels of a case's restarts, R x n: scikit-learn's Lloyd from the case's seeds.  ``dying`` has one restart more,
    from a Lloyd of TWO clusters: three of its five components are empty from the start (nk = 10 eps exactly)"""
    labels = MC.reference_lloyd(table, seeds_of(name, table))[0]
    if name == 'dying':
        labels = np.concatenate([labels, MC.reference_lloyd(table, MC.seeds_of(table, MC.SEED, 1, 2))[0]])
    return np.ascontiguousarray(labels, dtype=np.int32)


def estimator(n_components, prior_type, tol=1e-3, max_iter=100, reg_covar=1e-6):
    from sklearn.mixture import BayesianGaussianMixture
    return BayesianGaussianMixture(n_components=n_components, covariance_type='full', tol=tol, max_iter=max_iter, reg_covar=reg_covar,
                                   weight_concentration_prior_type=prior_type)


def as_run(parameters):
    """the six parameters of ``_get_parameters`` under the names of ``_hip.bayes_mixture_em`` (weight concentration 2 x C: rows a, b
    of the process; row 0 of the distribution, row 1 zero)"""
    concentration = parameters[0]
    if isinstance(concentration, tuple):
        concentration = np.stack(concentration)
    else:
        concentration = np.stack([concentration, np.zeros_like(concentration)])
    return dict(zip(PARAMETERS, (concentration, ) + tuple(np.array(v) for v in parameters[1:])))


def reference_bayes_em(table, labels, tol, max_iter, prior_type, reg_covar=1e-6, n_components=None):
    """scikit-learn's variational loop (``BaseMixture.fit_predict``) for one restart from one-hot responsibilities.  Returns a dict
    of the six parameters after the last completed iteration, the bounds of all iterations, n_iter, converged and ``failed`` (the
    iteration in which scikit-learn raised for a covariance that is not positive definite, else 0)."""
    n_comp = int(labels.max()) + 1 if n_components is None else n_components
    bgm = estimator(n_comp, prior_type, tol, max_iter, reg_covar)
    bgm._check_parameters(table)
    resp = np.zeros((len(table), n_comp))
    resp[np.arange(len(table)), labels] = 1
    bgm._initialize(table, resp)
    bound, bounds, converged, n_iter, failed = -np.inf, [], False, 0, 0
    kept = bgm._get_parameters()
    for n_iter in range(1, max_iter + 1):
        before = bound
        try:
            log_prob_norm, log_resp = bgm._e_step(table)
            bgm._m_step(table, log_resp)
        except ValueError:
            failed, n_iter = n_iter, n_iter - 1
            bgm._set_parameters(kept)
            break
        kept = bgm._get_parameters()
        bound = bgm._compute_lower_bound(log_resp, log_prob_norm)
        bounds.append(bound)
        if abs(bound - before) < tol:
            converged = True
            break
    run = as_run(kept)
    run.update(lower_bound=bounds[-1] if bounds else -np.inf, bounds=bounds, n_iter=n_iter, converged=converged, failed=failed)
    return run


def deviation(run_a, run_b):
    """largest difference of two runs' six parameter arrays and lower bounds, relative to 1 + |value|"""
    worst = 0.
    for key in PARAMETERS + ('lower_bound', ):
        a, b = np.asarray(run_a[key], dtype=float), np.asarray(run_b[key], dtype=float)
        worst = max(worst, float(np.max(np.abs(a - b) / (1 + np.abs(b)))))
    return worst


def reference_sensitivity(name, n_permutations=5, max_iter=20):
    """the measurement behind BAYES_TOLERANCE: scikit-learn against itself on row-permuted copies of the table"""
    table = load_table(name)
    labels = labels_of(name, table)
    n_comp = CASES[name][0]
    worst = 0.
    for prior_type in CASES[name][2]:
        rng = np.random.RandomState(1)
        plain = [reference_bayes_em(table, lab, 0., max_iter, prior_type, n_components=n_comp) for lab in labels]
        for _ in range(n_permutations):
            order = rng.permutation(len(table))
            moved = np.ascontiguousarray(table[order])
            for lab, run in zip(labels, plain):
                other = reference_bayes_em(moved, lab[order], 0., max_iter, prior_type, n_components=n_comp)
                if other['n_iter'] == run['n_iter']:
                    worst = max(worst, deviation(other, run))
    return worst
