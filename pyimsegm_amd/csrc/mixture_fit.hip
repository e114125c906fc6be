// mixture_fit.hip -- the class model's fit on the device: Lloyd k-means and EM for full covariances over one resident n x F
// table, all R restarts at once (imsegm_kmeans_lloyd, imsegm_mixture_em of include/imsegm_hip.h).
//
// What is restated (scikit-learn 1.x): sklearn/cluster/_kmeans.py `_kmeans_single_lloyd` (labels by argmin of |c|^2 - 2 x.c, ties
// to the lowest index; centres = sums / counts; stop on unchanged labels or on a summed squared centre shift <= tol, then one
// more labelling; `_inertia_dense`), and sklearn/mixture/_gaussian_mixture.py `_estimate_gaussian_parameters` with
// `_estimate_gaussian_covariances_full` (centred form, two passes), `_compute_precision_cholesky`, `_estimate_log_gaussian_prob`,
// `_compute_log_det_cholesky`, and sklearn/mixture/_base.py `_estimate_log_prob_resp` / the loop of `fit_predict`.
//
// Shape.  ONE pass kernel serves the four passes over the table (template MODE).  A workgroup owns a contiguous run of rows --
// the split depends on n alone, never on R --, a thread loads its row into registers ONCE and loops over the restarts; the
// parameters of the (restart, component) are wave-uniform loads.  Per (restart, component) the 1 + F (sums) or F (F + 1) / 2
// (centred products) values of the 256 rows are summed sixteen at a time by the transposed DPP row reduction of common.h, the
// sixteen row totals are added in a fixed order by one thread and kept in LDS across the workgroup's rows; at the end the
// workgroup writes its sums to its own slot of `partial`.  NO atomics: a finalising workgroup per restart adds the slots in a
// fixed order (sixteen strided sub-sums, then those in order) and does the small dense algebra.  Every restart's arithmetic is
// its own, so a restart gives the same bits alone and in a batch, and the same call gives the same bits every time.
// A restart that is done (converged, out of iterations, flagged) is skipped by every kernel: its parameters and outputs freeze.
//
// The variational fit (imsegm_bayes_mixture_em; sklearn/mixture/_bayesian_mixture.py `_initialize`, `_m_step`, `_estimate_log_prob`,
// `_estimate_log_weights`, `_compute_lower_bound` for covariance_type='full') is the template parameter BAYES of the two EM passes
// and their finalisers: the row passes are the same, the finaliser of the covariance pass does the posterior updates, folds the
// per-component constant of the E step (digamma, fit_digamma below) into the log-weight slot of `params` and forms the lower bound
// (lgamma of the device library) from the entropy sum of the E step's pass.  The BAYES = false instantiations are what they were.
#include "mixture_fit.h"

#include <cmath>
#include <limits>

namespace imsegm {

enum { FIT_KM_ASSIGN = 0, FIT_KM_FINAL = 1, FIT_EM_SUMS = 2, FIT_EM_COV = 3 };
constexpr int FIT_MAX_F = 16, FIT_MAX_BLOCKS = 256;      // (the caps and flags shared with the wide fit: mixture_fit.h)

struct FitArgs {
    const double *X;
    int n, F, C, R, G, L;       // G workgroups of L rows each (L a multiple of 256)
    int r0, r1;                 // the restarts of this launch (their sums must fit the LDS of a workgroup)
    int NG, PS;                 // groups of 16 values per (restart, component); doubles per (workgroup, restart) in `partial`
    int from_labels;            // EM: responsibilities are the one-hot labels (the M step of init_params='kmeans')
    int max_iter;
    double tol, reg;
    int32_t *labels;            // [R][n]
    double *centres;            // [R][C][F]
    double *params;             // [R][PP]: log weights C | log det C | means C F | means @ prec_chol C F | prec_chol C F F
    double *means_new;          // [R][C][F]
    double *nk;                 // [R][C]
    double *partial;            // [G][R][PS]
    int *done, *strict, *n_iter, *flags, *pending, *converged;      // [R] each
    double *bound, *inertia;    // [R] each
    double *out_w, *out_means, *out_cov, *out_prec;
    // the variational fit (imsegm_bayes_mixture_em) only
    int prior_type;             // 0: dirichlet_process, 1: dirichlet_distribution
    double wc_prior, mp_prior, dof_prior;
    const double *prior;        // mean_prior F | covariance_prior F F
    double *bstate;             // [R][4 C]: weight concentration a C | b C | mean precision C | degrees of freedom C
    double *entropy;            // [R]: sum over rows and components of resp log resp of the last E step
};

__host__ __device__ inline int fit_params_size(int C, int F) { return 2 * C + 2 * C * F + C * F * F; }

// (row, column) of element p of a packed lower triangle, p = a (a + 1) / 2 + b with b <= a: a table the unrolled loops index
// with constants
struct TriTable {
    int row[144], col[144];
    constexpr TriTable() : row(), col()
    {
        int a = 0, b = 0;
        for (int p = 0; p < 144; ++p) {
            row[p] = a;
            col[p] = b;
            if (++b > a) {
                ++a;
                b = 0;
            }
        }
    }
};

__device__ __forceinline__ void fit_group_store(const double (&v)[16], double *red, int g, int tid)
{
    red[g * 256 + tid] = row16_reduce16_f64(v, tid & 63);      // lane j of each 16-lane row: the row's total of value j
}
// the sixteen row totals of `ngroups` x 16 values, added in row order into the workgroup's running sums
__device__ __forceinline__ void fit_group_combine(double *slot, const double *red, int ngroups, int tid)
{
    __syncthreads();
    if (tid < ngroups * 16) {
        const int g = tid >> 4, j = tid & 15;
        double s = 0.0;
#pragma unroll
        for (int row = 0; row < 16; ++row) s += red[g * 256 + row * 16 + j];
        slot[tid] += s;
    }
    __syncthreads();
}

template <int FP> __device__ __forceinline__ int fit_nearest(const double (&x)[FP], const double *cen, int C, int F)
{
    int best = 0;
    double bd = INFINITY;
    for (int c = 0; c < C; ++c) {
        double cc = 0.0, xc = 0.0;
#pragma unroll
        for (int f = 0; f < FP; ++f)
            if (f < F) {
                const double cv = cen[c * F + f];
                cc += cv * cv;
                xc += x[f] * cv;
            }
        const double d = cc - 2.0 * xc;
        if (d < bd) {
            bd = d;
            best = c;
        }
    }
    return best;
}

// digamma of a positive argument: the recurrence up to 10, then the asymptotic series through x^-16 (the next term is below
// 4e-18 there)
__device__ inline double fit_digamma(double x)
{
    double r = 0.0;
    while (x < 10.0) {
        r -= 1.0 / x;
        x += 1.0;
    }
    const double i = 1.0 / x, i2 = i * i;
    const double s = i2 * (1.0 / 12 - i2 * (1.0 / 120 - i2 * (1.0 / 252 - i2 * (1.0 / 240 - i2 * (1.0 / 132 - i2 * (691.0 / 32760
                     - i2 * (1.0 / 12 - i2 * (3617.0 / 8160))))))));
    return r + ((log(x) - 0.5 * i) - s);
}

// BAYES: the variational fit of BayesianGaussianMixture -- the same row passes; the per-row extra of the E step is the entropy
// term sum_k resp log resp instead of log_prob_norm (sklearn/mixture/_bayesian_mixture.py `_compute_lower_bound`)
template <int MODE, int FP, bool BAYES = false> __global__ __launch_bounds__(256) void k_fit_pass(const FitArgs a)
{
    extern __shared__ double fit_lds[];
    const int tid = threadIdx.x;
    const int F = a.F, C = a.C, NG = a.NG, PS = a.PS, nr = a.r1 - a.r0;
    double *acc = fit_lds, *red = fit_lds + nr * PS;
    for (int k = tid; k < nr * PS; k += 256) acc[k] = 0.0;
    __syncthreads();
    const long row0 = (long)blockIdx.x * a.L;
    const long row1 = row0 + a.L < (long)a.n ? row0 + a.L : (long)a.n;
    for (long base = row0; base < row1; base += 256) {
        const long i = base + tid;
        const bool valid = i < row1;
        double x[FP];
#pragma unroll
        for (int f = 0; f < FP; ++f) x[f] = (valid && f < F) ? a.X[i * F + f] : 0.0;
        for (int r = a.r0; r < a.r1; ++r) {
            if (MODE == FIT_KM_FINAL ? a.flags[r] != 0 : a.done[r] != 0) continue;
            double *slot_r = acc + (r - a.r0) * PS;
            double resp[FIT_MAX_C];
            double extra = 0.0;
#pragma unroll
            for (int c = 0; c < FIT_MAX_C; ++c) resp[c] = 0.0;
            if (MODE == FIT_KM_ASSIGN || MODE == FIT_KM_FINAL) {
                const double *cen = a.centres + (size_t)r * C * F;
                int32_t *lab = a.labels + (size_t)r * a.n;
                int best = valid ? lab[i] : 0;
                if (MODE == FIT_KM_ASSIGN || !a.strict[r]) {
                    const int now = fit_nearest<FP>(x, cen, C, F);
                    if (valid) {
                        extra = now != best ? 1.0 : 0.0;
                        lab[i] = now;
                    }
                    best = now;
                }
                if (MODE == FIT_KM_FINAL) {
                    extra = 0.0;
                    if (valid) {
#pragma unroll
                        for (int f = 0; f < FP; ++f)
                            if (f < F) {
                                const double d = x[f] - cen[best * F + f];
                                extra += d * d;
                            }
                    }
                } else {
#pragma unroll
                    for (int c = 0; c < FIT_MAX_C; ++c) resp[c] = (valid && best == c) ? 1.0 : 0.0;
                }
            } else if (a.from_labels) {
                const int lab = valid ? a.labels[(size_t)r * a.n + i] : -1;
#pragma unroll
                for (int c = 0; c < FIT_MAX_C; ++c) resp[c] = lab == c ? 1.0 : 0.0;
            } else {
                // _estimate_log_gaussian_prob + log weights, then _estimate_log_prob_resp
                const double *par = a.params + (size_t)r * fit_params_size(C, F);
                const double *logw = par, *logdet = par + C, *muproj = par + 2 * C + C * F, *prec = par + 2 * C + 2 * C * F;
                double lp[FIT_MAX_C];
                double top = -INFINITY;
#pragma unroll
                for (int c = 0; c < FIT_MAX_C; ++c) {
                    lp[c] = -INFINITY;
                    if (c < C) {
                        const double *P = prec + (size_t)c * F * F;
                        double maha = 0.0;
#pragma unroll
                        for (int j = 0; j < FP; ++j)
                            if (j < F) {
                                double s = 0.0;
#pragma unroll
                                for (int k = 0; k <= j; ++k) s += x[k] * P[k * F + j];
                                const double y = s - muproj[c * F + j];
                                maha += y * y;
                            }
                        lp[c] = (-0.5 * ((double)F * 1.8378770664093453 + maha) + logdet[c]) + logw[c];
                        top = fmax(top, lp[c]);
                    }
                }
                double sum = 0.0;
#pragma unroll
                for (int c = 0; c < FIT_MAX_C; ++c)
                    if (c < C) sum += exp(lp[c] - top);
                const double lpn = top + log(sum);
#pragma unroll
                for (int c = 0; c < FIT_MAX_C; ++c) resp[c] = (valid && c < C) ? exp(lp[c] - lpn) : 0.0;
                if constexpr (BAYES) {
                    if (MODE == FIT_EM_SUMS && valid) {
#pragma unroll
                        for (int c = 0; c < FIT_MAX_C; ++c)
                            if (c < C) extra += resp[c] * (lp[c] - lpn);
                    }
                } else {
                    if (MODE == FIT_EM_SUMS && valid) extra = lpn;
                }
            }

            if (MODE != FIT_KM_FINAL) {
                for (int c = 0; c < C; ++c) {
                    double rc = 0.0;
#pragma unroll
                    for (int q = 0; q < FIT_MAX_C; ++q) rc = q == c ? resp[q] : rc;
                    if (MODE == FIT_EM_COV) {
                        const double *mu = a.means_new + ((size_t)r * C + c) * F;
                        double d[FP];
#pragma unroll
                        for (int f = 0; f < FP; ++f) d[f] = f < F ? x[f] - mu[f] : 0.0;
                        constexpr int GROUPS = (FP * (FP + 1) / 2 + 15) / 16;
                        constexpr TriTable tri;
#pragma unroll
                        for (int g = 0; g < GROUPS; ++g)
                            if (g < NG) {
                                double v[16];
#pragma unroll
                                for (int k = 0; k < 16; ++k) {
                                    const int ra = tri.row[g * 16 + k], rb = tri.col[g * 16 + k];
                                    v[k] = ra < FP ? (rc * d[ra < FP ? ra : 0]) * d[rb < FP ? rb : 0] : 0.0;
                                }
                                fit_group_store(v, red, g, tid);
                            }
                    } else {
                        constexpr int GROUPS = (FP + 1 + 15) / 16;
#pragma unroll
                        for (int g = 0; g < GROUPS; ++g)
                            if (g < NG) {
                                double v[16];
#pragma unroll
                                for (int k = 0; k < 16; ++k) {
                                    const int p = g * 16 + k;
                                    v[k] = p == 0 ? rc : (p - 1 < FP ? rc * x[p - 1 < FP ? (p > 0 ? p - 1 : 0) : 0] : 0.0);
                                }
                                fit_group_store(v, red, g, tid);
                            }
                    }
                    fit_group_combine(slot_r + c * NG * 16, red, NG, tid);
                }
            }
            if (MODE != FIT_EM_COV) {
                double v[16];
#pragma unroll
                for (int k = 0; k < 16; ++k) v[k] = k == 0 ? extra : 0.0;
                fit_group_store(v, red, 0, tid);
                fit_group_combine(slot_r + C * NG * 16, red, 1, tid);
            }
        }
    }
    __syncthreads();
    double *out = a.partial + ((size_t)blockIdx.x * a.R + a.r0) * PS;
    for (int k = tid; k < nr * PS; k += 256) out[k] = acc[k];
}

// one workgroup per restart: the slots of `partial` in a fixed order, then what the pass was for
// BAYES (FIT_EM_SUMS, FIT_EM_COV): the posterior updates of `_m_step`, the per-component constant of `_estimate_log_prob` +
// `_estimate_log_weights` folded into the log-weight slot of `params`, and the lower bound with the parameters after the M step
template <int MODE, bool BAYES = false> __global__ __launch_bounds__(256) void k_fit_final(const FitArgs a)
{
    __shared__ double tot[FIT_MAX_C * 144 + 16];
    __shared__ double tmp[256];
    __shared__ double mat[FIT_MAX_C][2][FIT_MAX_F * FIT_MAX_F];
    __shared__ double sh[FIT_MAX_C];
    __shared__ int shi[FIT_MAX_C];
    const int tid = threadIdx.x, r = blockIdx.x;
    const int F = a.F, C = a.C, PS = a.PS, NG16 = a.NG * 16;
    if (MODE == FIT_KM_FINAL ? a.flags[r] != 0 : a.done[r] != 0) return;
    for (int v0 = 0; v0 < PS; v0 += 16) {
        const int v = v0 + (tid >> 4), s = tid & 15;
        double sub = 0.0;
        if (v < PS)
            for (int b = s; b < a.G; b += 16) sub += a.partial[((size_t)b * a.R + r) * PS + v];
        tmp[tid] = sub;
        __syncthreads();
        if (tid < 16 && v0 + tid < PS) {
            double t = 0.0;
#pragma unroll
            for (int q = 0; q < 16; ++q) t += tmp[tid * 16 + q];
            tot[v0 + tid] = t;
        }
        __syncthreads();
    }
    const int c = tid;
    if (MODE == FIT_KM_ASSIGN) {
        if (c < C) {
            double *cen = a.centres + ((size_t)r * C + c) * F;
            const double count = tot[c * NG16];
            double shift = 0.0;
            shi[c] = count == 0.0;
            if (count != 0.0)
                for (int f = 0; f < F; ++f) {
                    const double nv = tot[c * NG16 + 1 + f] / count, d = nv - cen[f];
                    shift += d * d;
                    cen[f] = nv;
                }
            const double norm = sqrt(shift);
            sh[c] = norm * norm;
        }
        __syncthreads();
        if (tid == 0) {
            double shift_tot = 0.0;
            int empty = 0;
            for (int q = 0; q < C; ++q) {
                shift_tot += sh[q];
                empty |= shi[q];
            }
            const int it = a.n_iter[r] + 1;
            a.n_iter[r] = it;
            if (empty) {
                a.flags[r] |= FIT_FLAG_EMPTY;
                a.done[r] = 1;
            } else if (tot[C * NG16] == 0.0) {
                a.strict[r] = 1;
                a.done[r] = 1;
            } else if (shift_tot <= a.tol || it >= a.max_iter) {
                a.done[r] = 1;
            }
        }
    } else if (MODE == FIT_KM_FINAL) {
        if (tid == 0) a.inertia[r] = tot[0];
    } else if (MODE == FIT_EM_SUMS) {
        if (c < C) {
            const double nk = tot[c * NG16] + 10.0 * 2.220446049250313e-16;
            a.nk[r * C + c] = nk;
            for (int f = 0; f < F; ++f) a.means_new[((size_t)r * C + c) * F + f] = tot[c * NG16 + 1 + f] / nk;
        }
        if constexpr (BAYES) {
            if (tid == 0 && !a.from_labels) a.entropy[r] = tot[C * NG16];
        } else if (tid == 0 && !a.from_labels) {
            const double now = tot[C * NG16] / (double)a.n;
            a.pending[r] = fabs(now - a.bound[r]) < a.tol;
            a.bound[r] = now;
        }
    } else {
        double *par = a.params + (size_t)r * fit_params_size(C, F);
        __shared__ double bc[4][FIT_MAX_C];      // BAYES: E-step constant | log Wishart norm | mean precision | degrees of freedom
        if (c < C) {
            double *A = mat[c][0], *Z = mat[c][1];
            const double nk = a.nk[r * C + c];
            double *cov = a.out_cov + ((size_t)r * C + c) * F * F;
            double mp = 0.0, dof = 0.0, scale = 0.0;
            if constexpr (BAYES) {
                // `_estimate_means`: the posterior mean replaces the weighted mean the covariance pass was centred on; the
                // difference to the prior mean waits in Z's first row for the covariance below
                mp = a.mp_prior + nk;
                dof = a.dof_prior + nk;
                scale = nk * a.mp_prior / mp;
                double *mn = a.means_new + ((size_t)r * C + c) * F;
                for (int f = 0; f < F; ++f) {
                    const double xk = mn[f];
                    Z[f] = xk - a.prior[f];
                    mn[f] = (a.mp_prior * a.prior[f] + nk * xk) / mp;
                }
            }
            for (int i = 0; i < F; ++i)
                for (int j = 0; j <= i; ++j) {
                    double v = tot[c * NG16 + i * (i + 1) / 2 + j] / nk;
                    if (i == j) v += a.reg;
                    if constexpr (BAYES)        // `_estimate_wishart_full`
                        v = ((a.prior[F + i * F + j] + nk * v) + scale * (Z[i] * Z[j])) / dof;
                    A[i * FIT_MAX_F + j] = v;
                    cov[i * F + j] = v;
                    cov[j * F + i] = v;
                }
            // lower Cholesky factor in place, then its inverse by forward substitution (_compute_precision_cholesky)
            bool bad = false;
            for (int j = 0; j < F && !bad; ++j) {
                double s = A[j * FIT_MAX_F + j];
                for (int k = 0; k < j; ++k) s -= A[j * FIT_MAX_F + k] * A[j * FIT_MAX_F + k];
                if (!(s > 0.0) || !(s < INFINITY)) {
                    bad = true;
                    break;
                }
                const double ljj = sqrt(s);
                A[j * FIT_MAX_F + j] = ljj;
                for (int i = j + 1; i < F; ++i) {
                    double t = A[i * FIT_MAX_F + j];
                    for (int k = 0; k < j; ++k) t -= A[i * FIT_MAX_F + k] * A[j * FIT_MAX_F + k];
                    A[i * FIT_MAX_F + j] = t / ljj;
                }
            }
            shi[c] = bad;
            if (!bad) {
                for (int j = 0; j < F; ++j) {
                    Z[j * FIT_MAX_F + j] = 1.0 / A[j * FIT_MAX_F + j];
                    for (int i = j + 1; i < F; ++i) {
                        double s = 0.0;
                        for (int k = j; k < i; ++k) s += A[i * FIT_MAX_F + k] * Z[k * FIT_MAX_F + j];
                        Z[i * FIT_MAX_F + j] = -s / A[i * FIT_MAX_F + i];
                    }
                }
                double *P = par + 2 * C + 2 * C * F + (size_t)c * F * F, *Pout = a.out_prec + ((size_t)r * C + c) * F * F;
                double *mu = par + 2 * C + c * F, *muproj = par + 2 * C + C * F + c * F;
                const double *mnew = a.means_new + ((size_t)r * C + c) * F;
                double logdet = 0.0;
                for (int i = 0; i < F; ++i) {
                    logdet += log(Z[i * FIT_MAX_F + i]);
                    mu[i] = mnew[i];
                    a.out_means[((size_t)r * C + c) * F + i] = mnew[i];
                    for (int j = 0; j < F; ++j) {
                        const double v = j >= i ? Z[j * FIT_MAX_F + i] : 0.0;
                        P[i * F + j] = v;
                        Pout[i * F + j] = v;
                    }
                }
                for (int j = 0; j < F; ++j) {
                    double s = 0.0;
                    for (int i = 0; i <= j; ++i) s += mnew[i] * Z[j * FIT_MAX_F + i];
                    muproj[j] = s;
                }
                par[C + c] = logdet;
                if constexpr (BAYES) {
                    double dg = 0.0, lg = 0.0;
                    for (int i = 0; i < F; ++i) {
                        dg += fit_digamma(0.5 * (dof - i));
                        lg += lgamma(0.5 * (dof - i));
                    }
                    const double half_f_log_dof = 0.5 * F * log(dof), ld = logdet - half_f_log_dof;
                    bc[0][c] = -half_f_log_dof + 0.5 * ((F * 0.6931471805599453 + dg) - F / mp);
                    bc[1][c] = -((dof * ld + dof * F * 0.5 * 0.6931471805599453) + lg);
                    bc[2][c] = mp;
                    bc[3][c] = dof;
                }
            }
        }
        __syncthreads();
        if (tid == 0) {
            int bad = 0;
            for (int q = 0; q < C; ++q) bad |= shi[q];
            if (bad) {
                a.flags[r] |= FIT_FLAG_NOT_PD;
                a.done[r] = 1;
            } else if constexpr (BAYES) {
                double *bs = a.bstate + (size_t)r * 4 * C;
                const double *nk = a.nk + r * C;
                double log_norm_weight = 0.0, wishart = 0.0, log_mp = 0.0;
                if (a.prior_type == 0) {        // stick breaking: `_estimate_weights`, `_estimate_log_weights`, -sum betaln
                    double tail = 0.0, run = 0.0;
                    for (int q = C - 1; q >= 0; --q) {
                        bs[q] = 1.0 + nk[q];
                        bs[C + q] = a.wc_prior + tail;
                        tail += nk[q];
                    }
                    for (int q = 0; q < C; ++q) {
                        const double wa = bs[q], wb = bs[C + q];
                        const double dsum = fit_digamma(wa + wb), da = fit_digamma(wa), db = fit_digamma(wb);
                        par[q] = bc[0][q] + ((da - dsum) + run);
                        run += db - dsum;
                        log_norm_weight -= (lgamma(wa) + lgamma(wb)) - lgamma(wa + wb);
                    }
                } else {
                    double csum = 0.0, lsum = 0.0;
                    for (int q = 0; q < C; ++q) {
                        bs[q] = a.wc_prior + nk[q];
                        bs[C + q] = 0.0;
                        csum += bs[q];
                        lsum += lgamma(bs[q]);
                    }
                    const double dsum = fit_digamma(csum);
                    for (int q = 0; q < C; ++q) par[q] = bc[0][q] + (fit_digamma(bs[q]) - dsum);
                    log_norm_weight = lgamma(csum) - lsum;
                }
                for (int q = 0; q < C; ++q) {
                    bs[2 * C + q] = bc[2][q];
                    bs[3 * C + q] = bc[3][q];
                    wishart += bc[1][q];
                    log_mp += log(bc[2][q]);
                }
                if (!a.from_labels) {
                    const double now = ((-a.entropy[r] - wishart) - log_norm_weight) - 0.5 * F * log_mp;
                    const bool settled = fabs(now - a.bound[r]) < a.tol;
                    a.bound[r] = now;
                    const int it = a.n_iter[r] + 1;
                    a.n_iter[r] = it;
                    if (settled) {
                        a.converged[r] = 1;
                        a.done[r] = 1;
                    } else if (it >= a.max_iter) {
                        a.done[r] = 1;
                    }
                }
            } else {
                double w[FIT_MAX_C], wsum = 0.0;
                for (int q = 0; q < C; ++q) {
                    w[q] = a.nk[r * C + q] / (double)a.n;
                    wsum += w[q];
                }
                for (int q = 0; q < C; ++q) {
                    const double wq = w[q] / wsum;
                    a.out_w[r * C + q] = wq;
                    par[q] = log(wq);
                }
                if (!a.from_labels) {
                    const int it = a.n_iter[r] + 1;
                    a.n_iter[r] = it;
                    if (a.pending[r]) {
                        a.converged[r] = 1;
                        a.done[r] = 1;
                    } else if (it >= a.max_iter) {
                        a.done[r] = 1;
                    }
                }
            }
        }
    }
}

// start parameters given by the caller (weights, means, precision Cholesky factors in the output arrays): what the E step reads
__global__ void k_fit_set_params(const FitArgs a)
{
    const int r = blockIdx.x, c = threadIdx.x, F = a.F, C = a.C;
    if (c >= C) return;
    double *par = a.params + (size_t)r * fit_params_size(C, F);
    const double *P = a.out_prec + ((size_t)r * C + c) * F * F, *mu = a.out_means + ((size_t)r * C + c) * F;
    double logdet = 0.0;
    for (int i = 0; i < F; ++i) {
        logdet += log(P[i * F + i]);
        par[2 * C + c * F + i] = mu[i];
        for (int j = 0; j < F; ++j) par[2 * C + 2 * C * F + ((size_t)c * F + i) * F + j] = P[i * F + j];
    }
    for (int j = 0; j < F; ++j) {
        double s = 0.0;
        for (int i = 0; i < F; ++i) s += mu[i] * P[i * F + j];
        par[2 * C + C * F + c * F + j] = s;
    }
    par[c] = log(a.out_w[r * C + c]);
    par[C + c] = logdet;
}

}  // namespace imsegm

// ---------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------
namespace {

struct FitLayout {
    size_t o_labels, o_centres, o_params, o_means_new, o_nk, o_partial, o_ints, o_dbl, o_w, o_means, o_cov, o_prec, o_bayes, bytes;
    int G, L, ps_max;
};

inline int fit_groups(int values) { return (values + 15) / 16; }

FitLayout fit_layout(int n, int F, int C, int R)
{
    FitLayout lay;
    const int batches = cdiv(n, 256);
    const int per = cdiv(batches, FIT_MAX_BLOCKS);
    lay.L = per * 256;
    lay.G = cdiv(batches, per);
    const int ng_max = std::max(fit_groups(1 + F), fit_groups(F * (F + 1) / 2));
    lay.ps_max = C * ng_max * 16 + 16;
    size_t at = 0;
    auto take = [&](size_t bytes) {
        const size_t here = at;
        at += (bytes + 255) & ~(size_t)255;
        return here;
    };
    lay.o_labels = take((size_t)R * n * 4);
    lay.o_centres = take((size_t)R * C * F * 8);
    lay.o_params = take((size_t)R * fit_params_size(C, F) * 8);
    lay.o_means_new = take((size_t)R * C * F * 8);
    lay.o_nk = take((size_t)R * C * 8);
    lay.o_partial = take((size_t)lay.G * R * lay.ps_max * 8);
    lay.o_ints = take((size_t)6 * R * 4);
    lay.o_dbl = take((size_t)2 * R * 8);
    lay.o_w = take((size_t)R * C * 8);
    lay.o_means = take((size_t)R * C * F * 8);
    lay.o_cov = take((size_t)R * C * F * F * 8);
    lay.o_prec = take((size_t)R * C * F * F * 8);
    lay.o_bayes = take(((size_t)R * (4 * C + 1) + F + F * F) * 8);      // state R 4 C | entropy R | priors F + F F
    lay.bytes = at;
    return lay;
}

FitArgs fit_args(imsegm_ctx *ctx, const FitLayout &lay, int C, int R)
{
    FitArgs a;
    memset(&a, 0, sizeof(a));
    unsigned char *w = ctx->fit_work.as<unsigned char>();
    a.X = ctx->fit_table.as<double>();
    a.n = ctx->fit_n;
    a.F = ctx->fit_F;
    a.C = C;
    a.R = R;
    a.G = lay.G;
    a.L = lay.L;
    a.labels = reinterpret_cast<int32_t *>(w + lay.o_labels);
    a.centres = reinterpret_cast<double *>(w + lay.o_centres);
    a.params = reinterpret_cast<double *>(w + lay.o_params);
    a.means_new = reinterpret_cast<double *>(w + lay.o_means_new);
    a.nk = reinterpret_cast<double *>(w + lay.o_nk);
    a.partial = reinterpret_cast<double *>(w + lay.o_partial);
    int *ints = reinterpret_cast<int *>(w + lay.o_ints);
    a.done = ints;
    a.strict = ints + R;
    a.n_iter = ints + 2 * R;
    a.flags = ints + 3 * R;
    a.pending = ints + 4 * R;
    a.converged = ints + 5 * R;
    double *dbl = reinterpret_cast<double *>(w + lay.o_dbl);
    a.bound = dbl;
    a.inertia = dbl + R;
    a.out_w = reinterpret_cast<double *>(w + lay.o_w);
    a.out_means = reinterpret_cast<double *>(w + lay.o_means);
    a.out_cov = reinterpret_cast<double *>(w + lay.o_cov);
    a.out_prec = reinterpret_cast<double *>(w + lay.o_prec);
    a.bstate = reinterpret_cast<double *>(w + lay.o_bayes);
    a.entropy = a.bstate + (size_t)R * 4 * C;
    a.prior = a.entropy + R;
    return a;
}

template <int MODE, bool BAYES = false> int fit_pass(FitArgs a, hipStream_t st)
{
    const int F = a.F, C = a.C;
    const int values = MODE == FIT_KM_FINAL ? 0 : MODE == FIT_EM_COV ? F * (F + 1) / 2 : 1 + F;
    a.NG = fit_groups(values);
    a.PS = C * a.NG * 16 + 16;
    // the running sums of the restarts of one launch live in a workgroup's LDS: as many restarts per launch as fit 60 KB
    const size_t red_bytes = (size_t)std::max(a.NG, 1) * 256 * 8, per_restart = (size_t)a.PS * 8;
    const int block = std::max(1, (int)std::min<size_t>((size_t)a.R, (60 * 1024 - red_bytes) / per_restart));
    for (int r0 = 0; r0 < a.R; r0 += block) {
        a.r0 = r0;
        a.r1 = std::min(a.R, r0 + block);
        const size_t lds = (size_t)(a.r1 - a.r0) * per_restart + red_bytes;
        if (F <= 4)
            hipLaunchKernelGGL((k_fit_pass<MODE, 4, BAYES>), dim3(a.G), dim3(256), lds, st, a);
        else if (F <= 8)
            hipLaunchKernelGGL((k_fit_pass<MODE, 8, BAYES>), dim3(a.G), dim3(256), lds, st, a);
        else
            hipLaunchKernelGGL((k_fit_pass<MODE, 16, BAYES>), dim3(a.G), dim3(256), lds, st, a);
        HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL((k_fit_final<MODE, BAYES>), dim3(a.R), dim3(256), 0, st, a);
    HIP_TRY(hipGetLastError());
    return 0;
}

int fit_caps(const char *who, long n, int F, int C, int R)
{
    if (n < 1 || F < 1 || C < 1 || R < 1) {
        set_error(std::string(who) + ": bad arguments");
        return -1;
    }
    if (F > FIT_MAX_F || C > FIT_MAX_C || R > FIT_MAX_R || n >= 2147483647L) {
        set_error(std::string(who) + ": outside the caps of the device fit (features <= 16, components <= 8, restarts <= 16, rows < 2^31)");
        return IMSEGM_E_FIT_CAPS;
    }
    return 0;
}

}  // namespace

extern "C" {

int imsegm_kmeans_lloyd(imsegm_ctx *ctx, const double *table, long n_rows, int n_features, const double *seeds, int n_restarts,
                        int n_clusters, int max_iter, double tol, int32_t *labels_out, double *centres_out, double *inertia_out,
                        int32_t *n_iter_out, int32_t *empty_out)
{
    if (bind(ctx)) return -1;
    if (!table || !seeds || max_iter < 1) {
        set_error("kmeans_lloyd: bad arguments");
        return -1;
    }
    if (const int rc = fit_caps("kmeans_lloyd", n_rows, n_features, n_clusters, n_restarts)) return rc;
    const int n = (int)n_rows, F = n_features, C = n_clusters, R = n_restarts;
    hipStream_t st = ctx->stream;
    ctx->fit_n = ctx->fit_F = ctx->fit_label_restarts = 0;
    if (ctx->fit_table.ensure((size_t)n * F * 8)) return -1;
    const FitLayout lay = fit_layout(n, F, C, R);
    if (ctx->fit_work.ensure(lay.bytes)) return -1;
    ctx->fit_n = n;
    ctx->fit_F = F;
    FitArgs a = fit_args(ctx, lay, C, R);
    a.max_iter = max_iter;
    a.tol = tol;
    unsigned char *w = ctx->fit_work.as<unsigned char>();
    HIP_TRY(hipMemcpyAsync(ctx->fit_table.p, table, (size_t)n * F * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(a.centres, seeds, (size_t)R * C * F * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(a.labels, 0xff, (size_t)R * n * 4, st));          // no row has a label yet (-1)
    HIP_TRY(hipMemsetAsync(w + lay.o_ints, 0, (size_t)6 * R * 4, st));
    HIP_TRY(hipMemsetAsync(w + lay.o_dbl, 0, (size_t)2 * R * 8, st));
    if (fit_iterate(a.done, a.R, max_iter, st, [&]() { return fit_pass<FIT_KM_ASSIGN>(a, st); })) return -1;
    if (fit_pass<FIT_KM_FINAL>(a, st)) return -1;
    int ints[6 * FIT_MAX_R];
    HIP_TRY(hipMemcpyAsync(ints, w + lay.o_ints, (size_t)6 * R * 4, hipMemcpyDeviceToHost, st));
    if (labels_out) HIP_TRY(hipMemcpyAsync(labels_out, a.labels, (size_t)R * n * 4, hipMemcpyDeviceToHost, st));
    if (centres_out) HIP_TRY(hipMemcpyAsync(centres_out, a.centres, (size_t)R * C * F * 8, hipMemcpyDeviceToHost, st));
    if (inertia_out) HIP_TRY(hipMemcpyAsync(inertia_out, a.inertia, (size_t)R * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (int r = 0; r < R; ++r) {
        if (n_iter_out) n_iter_out[r] = ints[2 * R + r];
        if (empty_out) empty_out[r] = (ints[3 * R + r] & FIT_FLAG_EMPTY) != 0;
    }
    ctx->fit_label_restarts = R;
    ctx->fit_label_classes = C;
    return 0;
}

int imsegm_mixture_em(imsegm_ctx *ctx, int n_restarts, int n_components, const int32_t *labels, const double *weights_init,
                      const double *means_init, const double *prec_chol_init, double reg_covar, double tol, int max_iter,
                      double *weights_out, double *means_out, double *covariances_out, double *prec_chol_out, double *lower_bound_out,
                      int32_t *n_iter_out, int32_t *converged_out, int32_t *not_pd_out)
{
    if (bind(ctx)) return -1;
    if (ctx->fit_n < 1) {
        set_error("mixture_em: no resident table (imsegm_kmeans_lloyd uploads it)");
        return -1;
    }
    const int n = ctx->fit_n, F = ctx->fit_F, C = n_components, R = n_restarts;
    if (const int rc = fit_caps("mixture_em", n, F, C, R)) return rc;
    const bool from_params = weights_init && means_init && prec_chol_init;
    if (max_iter < 0 || (!from_params && (weights_init || means_init || prec_chol_init))) {
        set_error("mixture_em: bad arguments (start parameters are weights, means and precision factors together)");
        return -1;
    }
    if (!from_params && !labels && (ctx->fit_label_restarts != R || ctx->fit_label_classes != C)) {
        set_error("mixture_em: no resident labels of that many restarts and classes (imsegm_kmeans_lloyd leaves them)");
        return -1;
    }
    hipStream_t st = ctx->stream;
    const FitLayout lay = fit_layout(n, F, C, R);
    if (!from_params && !labels && ctx->fit_work.cap < lay.bytes) {
        set_error("mixture_em: the resident labels are gone");
        return -1;
    }
    if ((from_params || labels) && (ctx->fit_label_restarts != R || ctx->fit_label_classes != C || ctx->fit_work.cap < lay.bytes))
        ctx->fit_label_restarts = 0;           // (the buffers of another layout overwrite labels that were resident)
    if (ctx->fit_work.ensure(lay.bytes)) return -1;
    FitArgs a = fit_args(ctx, lay, C, R);
    a.max_iter = max_iter;
    a.tol = tol;
    a.reg = reg_covar;
    unsigned char *w = ctx->fit_work.as<unsigned char>();
    HIP_TRY(hipMemsetAsync(w + lay.o_ints, 0, (size_t)6 * R * 4, st));
    double start[2 * FIT_MAX_R];
    for (int r = 0; r < 2 * R; ++r) start[r] = r < R ? -std::numeric_limits<double>::infinity() : 0.0;
    HIP_TRY(hipMemcpyAsync(w + lay.o_dbl, start, (size_t)2 * R * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(a.out_cov, 0, (size_t)R * C * F * F * 8, st));
    if (from_params) {
        HIP_TRY(hipMemcpyAsync(a.out_w, weights_init, (size_t)R * C * 8, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(a.out_means, means_init, (size_t)R * C * F * 8, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(a.out_prec, prec_chol_init, (size_t)R * C * F * F * 8, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_fit_set_params, dim3(R), dim3(64), 0, st, a);
        HIP_TRY(hipGetLastError());
    } else {
        if (labels) {
            ctx->fit_label_restarts = 0;
            HIP_TRY(hipMemcpyAsync(a.labels, labels, (size_t)R * n * 4, hipMemcpyHostToDevice, st));
        }
        a.from_labels = 1;      // the M step of the initialisation: no iteration is counted, no bound formed
        if (fit_pass<FIT_EM_SUMS>(a, st) || fit_pass<FIT_EM_COV>(a, st)) return -1;
        a.from_labels = 0;
    }
    HIP_TRY(hipStreamSynchronize(st));          // (pageable sources are free again)
    if (fit_iterate(a.done, a.R, max_iter, st, [&]() { return fit_pass<FIT_EM_SUMS>(a, st) || fit_pass<FIT_EM_COV>(a, st) ? -1 : 0; })) return -1;
    int ints[6 * FIT_MAX_R];
    double bounds[2 * FIT_MAX_R];
    HIP_TRY(hipMemcpyAsync(ints, w + lay.o_ints, (size_t)6 * R * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(bounds, w + lay.o_dbl, (size_t)2 * R * 8, hipMemcpyDeviceToHost, st));
    if (weights_out) HIP_TRY(hipMemcpyAsync(weights_out, a.out_w, (size_t)R * C * 8, hipMemcpyDeviceToHost, st));
    if (means_out) HIP_TRY(hipMemcpyAsync(means_out, a.out_means, (size_t)R * C * F * 8, hipMemcpyDeviceToHost, st));
    if (covariances_out) HIP_TRY(hipMemcpyAsync(covariances_out, a.out_cov, (size_t)R * C * F * F * 8, hipMemcpyDeviceToHost, st));
    if (prec_chol_out) HIP_TRY(hipMemcpyAsync(prec_chol_out, a.out_prec, (size_t)R * C * F * F * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (int r = 0; r < R; ++r) {
        if (lower_bound_out) lower_bound_out[r] = bounds[r];
        if (n_iter_out) n_iter_out[r] = ints[2 * R + r];
        if (converged_out) converged_out[r] = ints[5 * R + r];
        if (not_pd_out) not_pd_out[r] = (ints[3 * R + r] & FIT_FLAG_NOT_PD) != 0;
    }
    return 0;
}

int imsegm_bayes_mixture_em(imsegm_ctx *ctx, int n_restarts, int n_components, const int32_t *labels, int prior_type,
                            double weight_concentration_prior, double mean_precision_prior, const double *mean_prior,
                            double degrees_of_freedom_prior, const double *covariance_prior, double reg_covar, double tol,
                            int max_iter, double *weight_concentration_out, double *mean_precision_out, double *means_out,
                            double *degrees_of_freedom_out, double *covariances_out, double *prec_chol_out, double *lower_bound_out,
                            int32_t *n_iter_out, int32_t *converged_out, int32_t *not_pd_out)
{
    if (bind(ctx)) return -1;
    if (ctx->fit_n < 1) {
        set_error("bayes_mixture_em: no resident table (imsegm_kmeans_lloyd uploads it)");
        return -1;
    }
    const int n = ctx->fit_n, F = ctx->fit_F, C = n_components, R = n_restarts;
    if (const int rc = fit_caps("bayes_mixture_em", n, F, C, R)) return rc;
    if (max_iter < 0 || !mean_prior || !covariance_prior || (prior_type != 0 && prior_type != 1)) {
        set_error("bayes_mixture_em: bad arguments (the priors are given, the prior type is 0 or 1)");
        return -1;
    }
    if (!labels && (ctx->fit_label_restarts != R || ctx->fit_label_classes != C)) {
        set_error("bayes_mixture_em: no resident labels of that many restarts and classes (imsegm_kmeans_lloyd leaves them)");
        return -1;
    }
    hipStream_t st = ctx->stream;
    const FitLayout lay = fit_layout(n, F, C, R);
    if (!labels && ctx->fit_work.cap < lay.bytes) {
        set_error("bayes_mixture_em: the resident labels are gone");
        return -1;
    }
    if (labels) ctx->fit_label_restarts = 0;           // (host labels overwrite the resident ones)
    if (ctx->fit_work.ensure(lay.bytes)) return -1;
    FitArgs a = fit_args(ctx, lay, C, R);
    a.max_iter = max_iter;
    a.tol = tol;
    a.reg = reg_covar;
    a.prior_type = prior_type;
    a.wc_prior = weight_concentration_prior;
    a.mp_prior = mean_precision_prior;
    a.dof_prior = degrees_of_freedom_prior;
    unsigned char *w = ctx->fit_work.as<unsigned char>();
    double *prior = a.entropy + R;
    HIP_TRY(hipMemsetAsync(w + lay.o_ints, 0, (size_t)6 * R * 4, st));
    double start[2 * FIT_MAX_R];
    for (int r = 0; r < 2 * R; ++r) start[r] = r < R ? -std::numeric_limits<double>::infinity() : 0.0;
    HIP_TRY(hipMemcpyAsync(w + lay.o_dbl, start, (size_t)2 * R * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(a.out_cov, 0, (size_t)R * C * F * F * 8, st));
    HIP_TRY(hipMemsetAsync(a.bstate, 0, (size_t)R * (4 * C + 1) * 8, st));
    HIP_TRY(hipMemcpyAsync(prior, mean_prior, (size_t)F * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(prior + F, covariance_prior, (size_t)F * F * 8, hipMemcpyHostToDevice, st));
    if (labels) HIP_TRY(hipMemcpyAsync(a.labels, labels, (size_t)R * n * 4, hipMemcpyHostToDevice, st));
    a.from_labels = 1;          // `_initialize`: the M step from the one-hot responsibilities, no iteration counted, no bound
    if (fit_pass<FIT_EM_SUMS, true>(a, st) || fit_pass<FIT_EM_COV, true>(a, st)) return -1;
    a.from_labels = 0;
    HIP_TRY(hipStreamSynchronize(st));          // (pageable sources are free again)
    if (fit_iterate(a.done, a.R, max_iter, st,
                    [&]() { return fit_pass<FIT_EM_SUMS, true>(a, st) || fit_pass<FIT_EM_COV, true>(a, st) ? -1 : 0; }))
        return -1;
    int ints[6 * FIT_MAX_R];
    double bounds[2 * FIT_MAX_R], state[FIT_MAX_R * 4 * FIT_MAX_C];
    HIP_TRY(hipMemcpyAsync(ints, w + lay.o_ints, (size_t)6 * R * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(bounds, w + lay.o_dbl, (size_t)2 * R * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(state, a.bstate, (size_t)R * 4 * C * 8, hipMemcpyDeviceToHost, st));
    if (means_out) HIP_TRY(hipMemcpyAsync(means_out, a.out_means, (size_t)R * C * F * 8, hipMemcpyDeviceToHost, st));
    if (covariances_out) HIP_TRY(hipMemcpyAsync(covariances_out, a.out_cov, (size_t)R * C * F * F * 8, hipMemcpyDeviceToHost, st));
    if (prec_chol_out) HIP_TRY(hipMemcpyAsync(prec_chol_out, a.out_prec, (size_t)R * C * F * F * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (int r = 0; r < R; ++r) {
        const double *s = state + (size_t)r * 4 * C;
        for (int q = 0; q < C; ++q) {
            if (weight_concentration_out) {
                weight_concentration_out[(r * 2 + 0) * C + q] = s[q];
                weight_concentration_out[(r * 2 + 1) * C + q] = s[C + q];
            }
            if (mean_precision_out) mean_precision_out[r * C + q] = s[2 * C + q];
            if (degrees_of_freedom_out) degrees_of_freedom_out[r * C + q] = s[3 * C + q];
        }
        if (lower_bound_out) lower_bound_out[r] = bounds[r];
        if (n_iter_out) n_iter_out[r] = ints[2 * R + r];
        if (converged_out) converged_out[r] = ints[5 * R + r];
        if (not_pd_out) not_pd_out[r] = (ints[3 * R + r] & FIT_FLAG_NOT_PD) != 0;
    }
    return 0;
}

}  // extern "C"
