"""Shared by tests/test_gpu_mixture_fit_wide.py and tests/test_mixture_fit_wide_host.py: the tables of the WIDE device fit
(17 to 256 features) and their tolerances.  The scikit-learn side of every comparison is that of tests/mixture_fit_cases.py, so
that no expected number ever comes from the device code."""
import os

import numpy as np

from mixture_fit_cases import GOLDEN, deviation, reference_em, reference_lloyd, reference_sensitivity, seeds_of       # noqa: F401

SEED = 7

#: name -> (components, restarts).  The feature counts cross the hand-overs of the kernels' tile counts (17: the first width
#: beyond the narrow fit, two 16-column tiles; 65, 129: one column into a fifth and a ninth tile; 180: the Leung-Malik table;
#: 256: the cap, where the staged rows pass 64 KB of LDS); the row counts are ragged against 256, all but one against 16 and 32.
CASES = {'c3_full': (3, 3), 'c3_17': (3, 3), 'c3_65': (2, 2), 'synth_129': (3, 2), 'synth_256': (2, 2)}

#: The tolerance of every parameter comparison, per case: scikit-learn's OWN sensitivity to the order of its sums (the rule of
#: ``mixture_fit_cases.EM_TOLERANCE``: five row permutations x 20 iterations, tol = 0, from the same one-hot labels, every
#: restart) times 16 for the device's different reduction tree, floor 1e-12.  Measured with ``reference_sensitivity``
#: (scikit-learn 1.7.2, CPU); the raw deviations are in DESIGN.md section 5.
EM_TOLERANCE = {
    'c3_full': 16 * 1.474e-06,       # measured 1.474e-06 (clusters of 110 rows < 180 features: positive definite through reg_covar only)
    'c3_17': 16 * 2.166e-11,         # measured 2.166e-11
    'c3_65': 16 * 1.276e-07,         # measured 1.276e-07 (clusters of 73 and 90 rows on 65 features)
    'synth_129': 16 * 2.370e-11,     # measured 2.370e-11
    'synth_256': 16 * 6.953e-12,     # measured 6.953e-12
}

#: centres and inertia of the Lloyd iterations against scikit-learn's, relative to 1 + |value| (the project's measure)
LLOYD_TOLERANCE = 1e-12

_TABLES = {}


def synthetic(n_rows, n_features, n_components):
    """rows dealt round-robin to Gaussian components with dense covariances: per component A = randn(F, F) / sqrt(F) + I and
    mean 1.5 randn(F), row i = mean + randn(F) @ A of component i mod C"""
    rng = np.random.RandomState(5)
    mixing, means = [], []
    for _ in range(n_components):
        mixing.append(rng.standard_normal((n_features, n_features)) / np.sqrt(n_features) + np.eye(n_features))
        means.append(1.5 * rng.standard_normal(n_features))
    noise = rng.standard_normal((n_rows, n_features))
    which = np.arange(n_rows) % n_components
    return np.stack([means[c] + noise[i] @ mixing[c] for i, c in enumerate(which)])


def raw_table(name):
    if name.startswith('c3'):
        features = np.asarray(np.load(os.path.join(GOLDEN, 'reference_c3.npz'))['features'], dtype=np.float64)
        return {'c3_full': features, 'c3_17': features[:, :17], 'c3_65': features[::3, :65]}[name]
    return {'synth_129': synthetic(600, 129, 3), 'synth_256': synthetic(1200, 256, 2)}[name]


def load_table(name):
    """the case's table through StandardScaler, as ``mixture_fit_cases.load_table`` does"""
    from sklearn.preprocessing import StandardScaler
    if name not in _TABLES:
        _TABLES[name] = np.ascontiguousarray(StandardScaler().fit_transform(raw_table(name)))
    return _TABLES[name]


def case_seeds(name):
    n_components, n_restarts = CASES[name]
    return seeds_of(load_table(name), SEED, n_restarts, n_components)


def lloyd_tol(table):
    return 1e-4 * np.mean(np.var(table, axis=0))


_HOST = {}


def host_lloyd(name):
    """scikit-learn's Lloyd from the case's seeds, computed once: (labels R x n, centres, inertia, iterations)"""
    if name not in _HOST:
        _HOST[name] = reference_lloyd(load_table(name), case_seeds(name))
    return _HOST[name]
