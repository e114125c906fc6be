"""Shared by tests/test_terms_reference_host.py and tests/test_gpu_terms_reference.py: class models the tests choose themselves
(not fitted ones), their feature tables, and an 80-bit (``numpy.longdouble``) restatement of ``predict_proba`` and of the graph-cut
terms -- so that no expected number ever comes from the device code or from the project's fp64 mirror (graph_cuts.py).

Why chosen models: a mixture fitted on real superpixel features of 64 columns and more separates its classes so far that every
probability is 0 or 1 to 1e-76; a kernel that drops a 64-feature block, a lane or a class still returns those zeros and ones.  Here
the components share one covariance (up to a factor close to one) and their means lie about 1.5 apart in Mahalanobis distance
whatever F is, so most rows have probabilities in the middle of (0, 1) and every feature and every class moves them."""
import numpy as np

#: x87 extended precision (eps 1.08e-19); where ``longdouble`` is the fp64 of the platform the reference is no reference
LONGDOUBLE_OK = bool(np.finfo(np.longdouble).eps < 1e-18)
LONGDOUBLE_REASON = 'numpy.longdouble is not an 80-bit format here (eps %.3g)' % float(np.finfo(np.longdouble).eps)

LD = np.longdouble

#: (features F, classes C, rows K, condition number of the shared covariance): every hand-over of terms.hip launch_gc_terms --
#: k_gmm_proba<1,1> up to 64 features, <2,4> to 128, <3,4> to 192, <4,4> to 256 --, both sides of each; one class, two, sixteen
#: (the model's limit); K = 1, 2, 3 modulo 4 beyond 64 features (the last wave of the four-rows-per-wave form).  A descriptor group
#: is three columns wide, so imsegm_image2d_features_place cannot lay out a table of one or two columns: F starts at 3.
CASES = [(3, 1, 5, 1e2), (3, 2, 9, 1e6), (9, 3, 37, 1e2), (63, 7, 64, 1e6), (64, 16, 130, 1e2), (65, 2, 131, 1e6),
         (128, 5, 129, 1e2), (129, 4, 66, 1e6), (192, 3, 67, 1e2), (193, 16, 65, 1e6), (256, 16, 133, 1e6)]
#: the whole-device terms (K >= TERMS_WIDE_FROM = 16384)
WIDE_CASE = (9, 3, 16384, 1e2)

EDGE_TYPES = ['model', 'model_l1', 'model_l2', 'model_lT', 'spatial', 'features', '', 'const']
EDGE_COSTS = [1.0, 2.75]
GC_REGUL = 1.5

#: seed of every case's construction (one for all, chosen before any measurement; the host test proves the conditions for it)
SEED = 20261017
#: ... but for the nine rows of (3, 2): two of them are the mean and the outlier, and the first seed left only six rows with a
#: probability in (0.01, 0.99); the next seeds were tried in order on the reference alone until seven were (condition 1)
CASE_SEED = {'F3-C2-K9': 20261020}


def case_id(case):
    return 'F%d-C%d-K%d' % case[:3]


#: max |scikit-learn fp64 - longdouble| of predict_proba per case over all rows, the larger of ``model.predict_proba`` and
#: ``graph_cuts.predict_proba``: measured on the CPU (scikit-learn 1.7.2, OpenBLAS) and measured again by
#: tests/test_terms_reference_host.py::test_fp64_sensitivity_is_the_recorded_one.  (The outlier row's weighted log-probabilities are
#: -4e3 .. -2e9, but the classes lie so far apart there that the row is 0 / 1 in every precision: it adds nothing to the figure.)
PROBA_DEVIATION = {
    'F3-C1-K5': 0.,              # one class: the probability is exp(0) in every precision
    'F3-C2-K9': 1.583e-16,
    'F9-C3-K37': 1.338e-15,
    'F63-C7-K64': 7.435e-14,
    'F64-C16-K130': 6.521e-15,
    'F65-C2-K131': 4.381e-14,
    'F128-C5-K129': 1.416e-14,
    'F129-C4-K66': 1.451e-13,
    'F192-C3-K67': 3.109e-14,
    'F193-C16-K65': 2.445e-13,
    'F256-C16-K133': 2.355e-13,
    'F9-C3-K16384': 2.975e-15,
}

#: max relative |host mirror fp64 - longdouble| of unary cost and edge weights per case over all edge types and edge costs
#: (test_host_mirror_agrees_with_the_reference measures it)
TERMS_DEVIATION = {
    'F3-C1-K5': 2.253e-16,
    'F3-C2-K9': 2.040e-15,
    'F9-C3-K37': 1.439e-15,
    'F63-C7-K64': 1.483e-15,
    'F64-C16-K130': 1.871e-15,
    'F65-C2-K131': 1.489e-15,
    'F128-C5-K129': 2.615e-15,
    'F129-C4-K66': 1.456e-15,
    'F192-C3-K67': 1.853e-15,
    'F193-C16-K65': 1.673e-15,
    'F256-C16-K133': 2.480e-15,
    'F9-C3-K16384': 2.482e-15,
}


def proba_tolerance(case):
    """the project's rule: 16 x the reference's own fp64 sensitivity -- the factor covers another order of
    the sums --, floor 1e-12"""
    return max(16 * PROBA_DEVIATION[case_id(case)], 1e-12)


def terms_tolerance(case):
    """relative; the same rule with floor 1e-13"""
    return max(16 * TERMS_DEVIATION[case_id(case)], 1e-13)


def build_case(case, **variant):
    """(model, raw table) of a case of :data:`CASES` with its seed"""
    F, C, K, cond = case
    return overlapping_model(F, C, K, CASE_SEED.get(case_id(case), SEED), cond, **variant)


def overlapping_model(F, C, K, seed=SEED, cond=1e2, with_mean=True, with_std=True, scaler=True):
    """(Pipeline([StandardScaler,] GaussianMixture('full')) assembled from chosen parameters, raw K x F feature table).

    One SPD base covariance (random orthogonal basis, eigenvalues log-uniform over ``cond``, geometric mean one), per class scaled by
    1 + 0.02 c / F; means a step of length ~1.5 in Mahalanobis distance from a common point; rows drawn from the mixture; row 0 sits
    on the mean of class 0, row 1 is a far outlier; the scaler has a mean and a scale of its own, and the raw table is the inverse
    transform of the rows."""
    from sklearn.mixture import GaussianMixture
    from sklearn.pipeline import Pipeline
    from sklearn.preprocessing import StandardScaler
    rng = np.random.RandomState([seed, F, C])
    basis, _ = np.linalg.qr(rng.standard_normal((F, F)))
    eig = np.exp(rng.uniform(0, np.log(cond), F)) / np.sqrt(cond)
    base = (basis * eig) @ basis.T
    base = 0.5 * (base + base.T)
    low = np.linalg.cholesky(base)
    centre = rng.standard_normal(F)
    means = centre + (rng.standard_normal((C, F)) * 1.5 / np.sqrt(F)) @ low.T
    factors = 1 + 0.02 * np.arange(C) / F
    covs = base[None] * factors[:, None, None]
    weights = rng.dirichlet(5 * np.ones(C))
    which = rng.choice(C, size=K, p=weights)
    rows = means[which] + rng.standard_normal((K, F)) @ low.T
    rows[0] = means[0]
    if K > 1:
        rows[1] = 50 * np.abs(rows[1]) + 30
    sc_mean, sc_scale = 3 * rng.standard_normal(F), np.exp(rng.standard_normal(F))
    gmm = GaussianMixture(n_components=C, covariance_type='full')
    gmm.weights_, gmm.means_, gmm.covariances_ = weights, means, covs
    inv_low = np.linalg.inv(low)
    gmm.precisions_cholesky_ = np.ascontiguousarray([inv_low.T / np.sqrt(f) for f in factors])
    gmm.precisions_ = np.array([pc @ pc.T for pc in gmm.precisions_cholesky_])
    gmm.converged_, gmm.n_iter_, gmm.lower_bound_ = True, 1, 0.
    gmm.n_features_in_ = F
    if not scaler:
        return Pipeline([('GMM', gmm)]), np.ascontiguousarray(rows)
    front = StandardScaler(with_mean=with_mean, with_std=with_std)
    front.mean_ = sc_mean if with_mean else None
    front.scale_ = sc_scale if with_std else None
    front.var_ = sc_scale**2 if with_std else None
    front.n_features_in_, front.n_samples_seen_ = F, K
    raw = rows * (sc_scale if with_std else 1.) + (sc_mean if with_mean else 0.)
    return Pipeline([('scaler', front), ('GMM', gmm)]), np.ascontiguousarray(raw)


def model_parts(model):
    """(scaler mean or None, scaler scale or None, mixture) of the pipeline"""
    steps = [st for _, st in model.steps]
    mean = scale = None
    if len(steps) == 2:
        mean = steps[0].mean_ if steps[0].with_mean else None
        scale = steps[0].scale_ if steps[0].with_std else None
    return mean, scale, steps[-1]


def weighted_log_prob(model, table, classes=None):
    """longdouble K x C: log N(x; mu_c, Sigma_c) + log w_c from the model's own parameters (means, precision factors, weights)"""
    mean, scale, gmm = model_parts(model)
    x = np.asarray(table, dtype=np.float64).astype(LD)
    if mean is not None:
        x = x - mean.astype(LD)
    if scale is not None:
        x = x / scale.astype(LD)
    n_feat = x.shape[1]
    out = []
    for c in (range(len(gmm.weights_)) if classes is None else classes):
        fac = gmm.precisions_cholesky_[c].astype(LD)
        y = x @ fac - gmm.means_[c].astype(LD) @ fac
        maha = np.sum(y * y, axis=1)
        log_det = np.sum(np.log(np.diagonal(fac)))
        out.append(-LD(0.5) * (n_feat * np.log(2 * LD(np.pi)) + maha) + log_det + np.log(LD(gmm.weights_[c])))
    return np.stack(out, axis=1)


def reference_proba(model, table, classes=None):
    """``predict_proba`` in longdouble: scaler, x P_c - mu_c P_c, squared norm, -0.5 (F log 2 pi + .) + sum log diag P_c + log w_c,
    log-sum-exp shifted by the row's maximum, exp.  (``np.pi`` is the fp64 constant, as in scikit-learn.)"""
    wl = weighted_log_prob(model, table, classes)
    top = wl.max(axis=1, keepdims=True)
    lse = np.log(np.sum(np.exp(wl - top), axis=1, keepdims=True)) + top
    return np.exp(wl - lse)


# ---- the graph the GPU tests use: label k is a 2 x 2 block of pixels, the blocks in h x w row-major order
def block_labels(h, w, block=2):
    grid = np.arange(h * w, dtype=np.int32).reshape(h, w)
    return np.ascontiguousarray(np.repeat(np.repeat(grid, block, axis=0), block, axis=1))


def grid_shape(K):
    """h x w = K with w the largest divisor up to sqrt(K) ... swapped so that w >= h (a prime K is one row)"""
    h = max(d for d in range(1, int(np.sqrt(K)) + 1) if K % d == 0)
    return h, K // h


def grid_graph(h, w, block=2):
    """(edges E x 2 int32 with a < b ordered by (b, a), centres K x 2 float64 as (row, column)) of :func:`block_labels`"""
    idx = np.arange(h * w).reshape(h, w)
    pairs = np.concatenate([np.stack([idx[:, :-1].ravel(), idx[:, 1:].ravel()], 1), np.stack([idx[:-1].ravel(), idx[1:].ravel()], 1)])
    order = np.lexsort((pairs[:, 0], pairs[:, 1]))
    rows, cols = np.divmod(np.arange(h * w), w)
    half = (block - 1) / 2.
    centres = np.stack([rows * block + half, cols * block + half], 1).astype(np.float64)
    return pairs[order].astype(np.int32).reshape(-1, 2), centres


def pairwise_cost(C, gc_regul=GC_REGUL):
    """``compute_pairwise_cost`` for a scalar: gc_regul off the diagonal"""
    return (np.ones((C, C)) - np.eye(C)) * gc_regul


# ---- the terms in longdouble
_SPATIAL = ('model', 'features', 'spatial')


def _pop_std(v):
    return np.sqrt(np.mean((v - np.mean(v))**2))


def reference_terms(proba, edges, centres, features, edge_type, edge_cost, pairwise):
    """unary cost, edge weights and pyGCO's scaled values in longdouble from fp64 inputs (the reference's graph_cuts.py and
    gco-wrapper's pygco.cut_general_graph restated):
      unary   |-log(clip(p, 0.01, 1 - 0.01))|
      dist    model / model_lT: max_c (dp)^2; model_l1: sum |dp|; model_l2: sqrt(sum dp^2); features: l2 of the columns standardised
              by their own mean and population std (zero std -> 1); else none
      weight  exp(-dist / (2 std(dist)^2)) (population std of the distance vector) or 1; for 'model', 'features', 'spatial' divided by
              the centre distance relative to its mean; clipped to [1e-3, 1e3]; times edge_cost
      pygco   dwf = max(|unary|.max(), |w|.max() * pairwise.max() if there are edges) + 1e-10; unary / dwf * 1e5 and w / dwf * 1e3
              are truncated towards zero
    A distance vector of equal entries has std 0: numpy's 0 / 0 = NaN stays NaN through the clips (comparisons with NaN are
    false), d / 0 = inf gives exp(-inf) = 0 -> 1e-3.  Returns a dict of longdouble arrays: unary, weights, unary_scaled,
    weights_scaled (before truncation), dist, std, dwf."""
    p = np.asarray(proba, dtype=np.float64).astype(LD)
    edges = np.asarray(edges).reshape(-1, 2)
    a, b = edges[:, 0], edges[:, 1]
    unary = np.abs(-np.log(np.clip(p, LD(0.01), LD(1 - 0.01))))
    kind, _, metric = edge_type.partition('_')
    n_edges = len(edges)
    dist, std = np.zeros(n_edges, LD), LD(0)
    with np.errstate(all='ignore'):
        if kind == 'model':
            dp = p[a] - p[b]
            metric = metric or 'lT'
            dist = {'l1': lambda: np.abs(dp).sum(axis=1), 'l2': lambda: np.sqrt((dp * dp).sum(axis=1)),
                    'lT': lambda: (dp * dp).max(axis=1) if dp.shape[0] else np.zeros(0, LD)}[metric]()
        elif edge_type == 'features':
            x = np.asarray(features, dtype=np.float64).astype(LD)
            mean = x.mean(axis=0)
            sd = np.sqrt(np.mean((x - mean)**2, axis=0))
            sd[sd == 0] = 1
            z = (x - mean) / sd
            dz = z[a] - z[b]
            dist = np.sqrt((dz * dz).sum(axis=1))
        if kind == 'model' or edge_type == 'features':
            std = _pop_std(dist) if n_edges else LD(0)
            weights = np.exp(-(dist / (2 * std**2)))
        else:
            weights = np.ones(n_edges, LD)
        if edge_type in _SPATIAL and n_edges:
            c = np.asarray(centres, dtype=np.float64).astype(LD)
            d = c[a] - c[b]
            length = np.sqrt((d * d).sum(axis=1))
            weights = weights / (length / np.mean(length))
        low = LD(1. / 1e3)
        weights = np.where(weights < low, low, weights)
        weights = np.where(weights > 1e3, LD(1e3), weights)
        weights = weights * LD(edge_cost)
        umax = np.abs(unary).max()
        wmax = np.abs(weights).max() if n_edges else LD(0)          # (numpy: NaN if a weight is NaN -> the comparison is false)
        pmax = LD(np.max(pairwise))
        dwf = (wmax * pmax if (n_edges and wmax * pmax > umax) else umax) + LD(1e-10)
        return dict(unary=unary, weights=weights, unary_scaled=(unary / dwf) * 100000, weights_scaled=(weights / dwf) * 1000,
                    dist=dist, std=std, dwf=dwf)


def truncated(scaled):
    """the integers pygco forms (truncation towards zero); NaN positions -> 0 here, callers mask them"""
    v = np.where(np.isfinite(scaled), scaled, 0)
    return np.trunc(v).astype(np.int64)


def ambiguous(scaled, rel_tol):
    """elements whose scaled value lies within the tolerance of an integer: a value that differs from the reference by ``rel_tol``
    (relative) may truncate to the neighbouring integer there.  The dwf carries the same relative tolerance: twice ``rel_tol``."""
    v = np.where(np.isfinite(scaled), scaled, 0.5)
    return np.abs(v - np.rint(v)) <= 2 * rel_tol * np.maximum(np.abs(v), 1)


def mpmath_proba(model, table, digits=50):
    """the same probabilities by mpmath at ``digits`` decimal digits: a spot check of the longdouble reference on a small case"""
    import mpmath
    mean, scale, gmm = model_parts(model)
    with mpmath.workdps(digits):
        out = []
        for row in np.asarray(table, dtype=np.float64):
            x = [mpmath.mpf(float(v)) for v in row]
            if mean is not None:
                x = [v - mpmath.mpf(float(m)) for v, m in zip(x, mean)]
            if scale is not None:
                x = [v / mpmath.mpf(float(s)) for v, s in zip(x, scale)]
            wl = []
            for c in range(len(gmm.weights_)):
                fac = gmm.precisions_cholesky_[c]
                n = len(x)
                maha = mpmath.mpf(0)
                for j in range(n):
                    y = mpmath.fsum((x[f] - mpmath.mpf(float(gmm.means_[c][f]))) * mpmath.mpf(float(fac[f, j])) for f in range(n))
                    maha += y * y
                log_det = mpmath.fsum(mpmath.log(mpmath.mpf(float(fac[j, j]))) for j in range(n))
                wl.append(-(n * mpmath.log(2 * mpmath.mpf(float(np.pi))) + maha) / 2 + log_det + mpmath.log(mpmath.mpf(float(gmm.weights_[c]))))
            top = max(wl)
            lse = mpmath.log(mpmath.fsum(mpmath.exp(w - top) for w in wl)) + top
            out.append([float(mpmath.exp(w - lse)) for w in wl])
        return np.array(out)


_CACHE = {}


def case_data(case):
    """(model, raw table, longdouble reference probabilities) of a case, computed once per process and never modified"""
    if case not in _CACHE:
        model, table = build_case(case)
        table.setflags(write=False)
        ref = reference_proba(model, table)
        ref.setflags(write=False)
        _CACHE[case] = (model, table, ref)
    return _CACHE[case]


def knocked_out(model, table, f):
    """the table with feature ``f`` replaced by the scaler's mean: the value at which the feature contributes nothing"""
    out = np.array(table)
    out[:, f] = model_parts(model)[0][f]
    return out
