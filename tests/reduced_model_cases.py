"""Shared by tests/test_reduced_model_reference_host.py and tests/test_gpu_reduced_model.py: class models with a PCA between the
scaler and the mixture, and Bayesian Gaussian mixtures, assembled from chosen parameters (tests/terms_cases.py says why not fitted
ones), their raw feature tables, and an 80-bit (``numpy.longdouble``) restatement of ``predict_proba`` for both -- so that no
expected number comes from the device code or from scikit-learn's fp64.

Construction of a PCA case I -> F: ``terms_cases.overlapping_model`` gives a mixture of overlapping classes and rows Z IN THE
REDUCED SPACE; ``components_`` are F orthonormal rows (QR of a seeded I x I matrix), ``mean_`` and ``explained_variance_`` are
drawn; the rows in front of the PCA are mean_ + (Z * scale) @ components_ (the pseudo-inverse of an orthonormal projection is its
transpose) plus a part orthogonal to the components, which the projection has to cancel; the raw table is the inverse transform
of the scaler on top.  Bayesian cases: the same mixtures with degrees of freedom, mean precisions and weight concentrations of
their own, which differ between the classes (a constant shared by all classes cancels in the probabilities)."""
import numpy as np

import terms_cases as T

LD = T.LD
LONGDOUBLE_OK, LONGDOUBLE_REASON = T.LONGDOUBLE_OK, T.LONGDOUBLE_REASON

#: (inputs I, mixture dimension F, classes C, rows K, whiten, scaler): both sides of every hand-over of k_pca_project (64, 128, 192
#: inputs: <1,1>, <2,4>, <3,4>, <4,4>) and of k_gmm_proba behind it (64 outputs), one output, as many outputs as inputs, 256 of
#: both (the limit), sixteen classes; K = 1, 2, 3 modulo 4 beyond 64 inputs (the last wave of the four-rows-per-wave form).  The
#: four cases at the hand-overs come a second time without the scaler (both null-pointer branches of the kernel).
CASES = [(3, 1, 2, 9, False, True), (9, 2, 3, 37, True, True), (9, 9, 3, 37, False, True), (63, 5, 7, 64, False, True),
         (64, 63, 4, 130, True, True), (65, 64, 2, 131, False, True), (129, 65, 4, 66, True, True), (193, 7, 16, 65, False, True),
         (256, 256, 16, 133, False, True), (256, 1, 2, 67, True, True),
         (64, 63, 4, 130, True, False), (65, 64, 2, 131, False, False), (129, 65, 4, 66, True, False), (193, 7, 16, 65, False, False)]
#: K = TERMS_WIDE_FROM: the terms behind the class model are computed by the whole device (the path of volumes)
WIDE_CASE = (9, 3, 3, 16384, False, True)

#: (inputs I or None, mixture dimension F, classes C, rows K, weight_concentration_prior_type)
BAYES_CASES = [(None, 3, 2, 9, 'dirichlet_process'), (None, 9, 3, 37, 'dirichlet_distribution'),
               (None, 65, 16, 131, 'dirichlet_process'), (9, 3, 3, 37, 'dirichlet_process')]

#: condition number of the shared covariance in the reduced space (terms_cases: 1e2 or 1e6; one value here)
COND = 1e2

#: seed of every case's construction, chosen before any measurement ...
SEED = 20261019
#: ... but for the cases that left fewer than 70 % of their rows with a probability in (0.01, 0.99): the next seeds were tried in
#: order on the reference alone until the condition held (tests/test_reduced_model_reference_host.py proves it for what stands
#: here).  Both are mixtures of two classes in ONE dimension, where the two means easily come to lie far apart: 20261019 left 6 of 9
#: and 45 of 67 rows open (70 % asks for 7 and 47), 20261020 3 and 29; 20261021 leaves 8 and 66.
CASE_SEED = {'I3-F1-C2-K9-n': 20261021, 'I256-F1-C2-K67-w': 20261021}


def case_id(case):
    if len(case) == 6:
        return 'I%d-F%d-C%d-K%d-%s%s' % (case[:4] + ('w' if case[4] else 'n', '' if case[5] else '-bare'))
    return 'bayes-%sF%d-C%d-K%d-%s' % (('I%d-' % case[0]) if case[0] else '', case[1], case[2], case[3], case[4].split('_')[1])


#: max |scikit-learn fp64 - longdouble| of ``model.predict_proba`` per case over all rows, measured on the CPU (scikit-learn 1.7.2,
#: OpenBLAS) and measured again by tests/test_reduced_model_reference_host.py::test_fp64_sensitivity_is_the_recorded_one
PROBA_DEVIATION = {
    'I3-F1-C2-K9-n': 3.997e-14,
    'I9-F2-C3-K37-w': 3.174e-16,
    'I9-F9-C3-K37-n': 1.439e-11,
    'I63-F5-C7-K64-n': 1.234e-15,
    'I64-F63-C4-K130-w': 1.083e-14,
    'I65-F64-C2-K131-n': 7.356e-15,
    'I129-F65-C4-K66-w': 7.904e-15,
    'I193-F7-C16-K65-n': 1.115e-15,
    'I256-F256-C16-K133-n': 3.162e-14,
    'I256-F1-C2-K67-w': 6.009e-16,
    'I64-F63-C4-K130-w-bare': 1.219e-14,
    'I65-F64-C2-K131-n-bare': 9.030e-15,
    'I129-F65-C4-K66-w-bare': 8.353e-15,
    'I193-F7-C16-K65-n-bare': 1.550e-15,
    'I9-F3-C3-K16384-n': 2.207e-15,
    'bayes-F3-C2-K9-process': 1.771e-13,
    'bayes-F9-C3-K37-distribution': 8.556e-12,
    'bayes-F65-C16-K131-process': 2.095e-14,
    'bayes-I9-F3-C3-K37-process': 7.570e-16,
}


def proba_tolerance(case):
    """the project's rule: 16 x the reference's own fp64 sensitivity, floor 1e-12"""
    return max(16 * PROBA_DEVIATION[case_id(case)], 1e-12)


# ---- digamma in longdouble
_ASYMPTOTIC = [(1, 12), (-1, 120), (1, 252), (-1, 240), (1, 132), (-691, 32760), (1, 12)]     # B_2n / (2 n), n = 1 .. 7


def digamma_ld(x):
    """psi(x) for x > 0 in longdouble: psi(x) = psi(x + 1) - 1 / x upwards until x >= 20, there the asymptotic series
    log x - 1 / (2 x) - sum_n B_2n / (2 n x^2n) up to x^-14 (the first term left out is 3617 / 8160 x^-16 < 1e-21)"""
    x = np.array(x, dtype=LD, ndmin=1).copy()
    acc = np.zeros_like(x)
    while True:
        low = x < 20
        if not low.any():
            break
        acc[low] -= 1 / x[low]
        x[low] += 1
    inv2 = 1 / (x * x)
    series, power = np.zeros_like(x), inv2.copy()
    for num, den in _ASYMPTOTIC:
        series += LD(num) / LD(den) * power
        power = power * inv2
    return acc + np.log(x) - 1 / (2 * x) - series


# ---- construction
def _pca(rng, I, F, whiten):
    from sklearn.decomposition import PCA
    basis, _ = np.linalg.qr(rng.standard_normal((I, I)))
    pca = PCA(n_components=F, whiten=whiten)
    pca.components_ = np.ascontiguousarray(basis[:, :F].T)
    pca.mean_ = 2 * rng.standard_normal(I)
    pca.explained_variance_ = np.sort(np.exp(rng.uniform(-1, 2, F)))[::-1].copy()
    pca.n_components_, pca.n_features_in_, pca.n_samples_ = F, I, 1000
    return pca, np.ascontiguousarray(basis[:, F:])


def _scaler(rng, I, K):
    from sklearn.preprocessing import StandardScaler
    front = StandardScaler()
    front.mean_, front.scale_ = 3 * rng.standard_normal(I), np.exp(rng.standard_normal(I))
    front.var_ = front.scale_**2
    front.n_features_in_, front.n_samples_seen_ = I, K
    return front


def _behind_pca(rng, pca, rest, rows):
    """rows in front of the PCA whose projection is ``rows``: the pseudo-inverse plus a part orthogonal to every component"""
    scale = np.sqrt(pca.explained_variance_) if pca.whiten else 1.
    off = rng.standard_normal((rows.shape[0], rest.shape[1])) @ rest.T if rest.shape[1] else 0.
    return pca.mean_ + (rows * scale) @ pca.components_ + off


def build_case(case, seed=None):
    """(Pipeline([scaler,] PCA, GaussianMixture), raw K x I table) of a case of :data:`CASES`"""
    from sklearn.pipeline import Pipeline
    I, F, C, K, whiten, scaler = case
    seed = CASE_SEED.get(case_id(case), SEED) if seed is None else seed
    inner, rows = T.overlapping_model(F, C, K, seed, COND, scaler=False)
    rng = np.random.RandomState([seed, I, F, C, 1])
    pca, rest = _pca(rng, I, F, whiten)
    table = _behind_pca(rng, pca, rest, rows)
    steps = [('reduce_dim', pca), ('GMM', inner.steps[-1][1])]
    if scaler:
        front = _scaler(rng, I, K)
        table = table * front.scale_ + front.mean_
        steps.insert(0, ('scaler', front))
    return Pipeline(steps), np.ascontiguousarray(table)


def build_bayes_case(case, seed=None):
    """(Pipeline([scaler, [PCA,]] BayesianGaussianMixture), raw table) of a case of :data:`BAYES_CASES`"""
    from sklearn.mixture import BayesianGaussianMixture
    from sklearn.pipeline import Pipeline
    I, F, C, K, kind = case
    seed = CASE_SEED.get(case_id(case), SEED) if seed is None else seed
    inner, rows = T.overlapping_model(F, C, K, seed, COND, scaler=False)
    gmm = inner.steps[-1][1]
    rng = np.random.RandomState([seed, I or 0, F, C, 2])
    bgm = BayesianGaussianMixture(n_components=C, covariance_type='full', weight_concentration_prior_type=kind)
    for name in ('weights_', 'means_', 'covariances_', 'precisions_cholesky_', 'precisions_', 'converged_', 'n_iter_', 'lower_bound_',
                 'n_features_in_'):
        setattr(bgm, name, getattr(gmm, name))
    # per class: the derivative of the constant with respect to the degrees of freedom grows with F; steps of 1 / F keep the
    # classes within a few units of log-probability of each other
    bgm.degrees_of_freedom_ = F + 2 + 3 * rng.uniform(0, 1, C) / F
    bgm.mean_precision_ = rng.uniform(0.5, 4, C) * max(1., F / 4.)
    if kind == 'dirichlet_process':
        bgm.weight_concentration_ = (1 + 20 * rng.uniform(0, 1, C), 1 + 30 * rng.uniform(0, 1, C))
    else:
        bgm.weight_concentration_ = 0.5 + 20 * rng.dirichlet(2 * np.ones(C))
    width = I or F
    table, steps = rows, [('BGM', bgm)]
    if I:
        pca, rest = _pca(rng, I, F, True)
        table = _behind_pca(rng, pca, rest, rows)
        steps.insert(0, ('reduce_dim', pca))
    front = _scaler(rng, width, K)
    table = table * front.scale_ + front.mean_
    return Pipeline([('scaler', front)] + steps), np.ascontiguousarray(table)


def build(case, seed=None):
    return build_case(case, seed) if len(case) == 6 else build_bayes_case(case, seed)


# ---- the reference
def model_steps(model):
    """(scaler or None, PCA or None, mixture)"""
    from sklearn.decomposition import PCA
    from sklearn.preprocessing import StandardScaler
    steps = [st for _, st in model.steps]
    scaler = next((st for st in steps if isinstance(st, StandardScaler)), None)
    pca = next((st for st in steps if isinstance(st, PCA)), None)
    return scaler, pca, steps[-1]


def reduced_rows(model, table, drop_shift=False, drop_scale=False):
    """longdouble rows the mixture sees: StandardScaler.transform, then X @ components_.T - mean_ @ components_.T, then the
    division by sqrt(explained_variance_) (whiten)"""
    scaler, pca, _ = model_steps(model)
    x = np.asarray(table, dtype=np.float64).astype(LD)
    if scaler is not None:
        if scaler.with_mean:
            x = x - scaler.mean_.astype(LD)
        if scaler.with_std:
            x = x / scaler.scale_.astype(LD)
    if pca is not None:
        comp_t = pca.components_.astype(LD).T
        y = x @ comp_t
        if not drop_shift:
            y = y - pca.mean_.astype(LD) @ comp_t
        if pca.whiten and not drop_scale:
            y = y / np.sqrt(pca.explained_variance_.astype(LD))
        x = y
    return x


def bayes_constants(mix):
    """(per-class constant of _estimate_log_prob, _estimate_log_weights) of a BayesianGaussianMixture in longdouble"""
    n_feat = mix.means_.shape[1]
    nu, kappa = mix.degrees_of_freedom_.astype(LD), mix.mean_precision_.astype(LD)
    psi = digamma_ld((LD(0.5) * (nu[None, :] - np.arange(n_feat, dtype=LD)[:, None])).ravel()).reshape(n_feat, -1)
    log_lambda = n_feat * np.log(LD(2)) + psi.sum(axis=0)
    const = -LD(0.5) * n_feat * np.log(nu) + LD(0.5) * (log_lambda - n_feat / kappa)
    if mix.weight_concentration_prior_type == 'dirichlet_process':
        a, b = (np.asarray(v, dtype=np.float64).astype(LD) for v in mix.weight_concentration_)
        psi_sum, psi_a, psi_b = digamma_ld(a + b), digamma_ld(a), digamma_ld(b)
        log_w = psi_a - psi_sum + np.concatenate([np.zeros(1, LD), np.cumsum(psi_b - psi_sum)[:-1]])
    else:
        conc = np.asarray(mix.weight_concentration_, dtype=np.float64).astype(LD)
        log_w = digamma_ld(conc) - digamma_ld(np.sum(conc)[None])
    return const, log_w


def reference_proba(model, table, drop_shift=False, drop_scale=False, drop_bayes=False):
    """``predict_proba`` of scaler -> PCA -> mixture in longdouble (the ``drop_*`` switches leave a step out: the host test shows
    that each of them moves the probabilities far beyond the tolerance)"""
    from sklearn.mixture import BayesianGaussianMixture
    mix = model_steps(model)[2]
    x = reduced_rows(model, table, drop_shift, drop_scale)
    n_feat = x.shape[1]
    log_w = np.log(mix.weights_.astype(LD))
    const = np.zeros(len(mix.weights_), LD)
    if isinstance(mix, BayesianGaussianMixture) and not drop_bayes:
        const, log_w = bayes_constants(mix)
    out = []
    for c in range(len(mix.weights_)):
        fac = mix.precisions_cholesky_[c].astype(LD)
        y = x @ fac - mix.means_[c].astype(LD) @ fac
        maha = np.sum(y * y, axis=1)
        log_det = np.sum(np.log(np.diagonal(fac)))
        out.append(-LD(0.5) * (n_feat * np.log(2 * LD(np.pi)) + maha) + log_det + const[c] + log_w[c])
    wl = np.stack(out, axis=1)
    top = wl.max(axis=1, keepdims=True)
    lse = np.log(np.sum(np.exp(wl - top), axis=1, keepdims=True)) + top
    return np.exp(wl - lse)


def with_zeroed_component_row(model, row):
    """a copy of the model whose ``components_.T`` has row ``row`` (what input column ``row`` contributes) set to zero"""
    import copy
    other = copy.deepcopy(model)
    model_steps(other)[1].components_[:, row] = 0.
    return other


def knocked_out(model, table, f):
    """the table with input column ``f`` at the scaler's mean (0 without a scaler): it contributes nothing to the projection"""
    scaler = model_steps(model)[0]
    out = np.array(table)
    out[:, f] = scaler.mean_[f] if scaler is not None else 0.
    return out


def undecided_share(ref):
    """share of the rows with a probability in (0.01, 0.99)"""
    top = np.asarray(ref).max(axis=1)
    return float(np.mean((top > 0.01) & (top < 0.99)))


_CACHE = {}


def case_data(case):
    """(model, raw table, longdouble reference probabilities) of a case, computed once per process and never modified"""
    if case not in _CACHE:
        model, table = build(case)
        table.setflags(write=False)
        ref = reference_proba(model, table)
        ref.setflags(write=False)
        _CACHE[case] = (model, table, ref)
    return _CACHE[case]
