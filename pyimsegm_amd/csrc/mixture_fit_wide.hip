// mixture_fit_wide.hip -- the class model's fit on the device for WIDE tables, 17 to 256 features: Lloyd k-means and EM for full
// covariances over one resident table, all R restarts at once (imsegm_kmeans_lloyd_wide, imsegm_mixture_em_wide of
// include/imsegm_hip.h).  The scikit-learn functions restated are the ones the header comment of mixture_fit.hip names.
//
// Shape.  A table row no longer fits a thread's registers, so every pass is a dense fp64 product on 16 x 16 tiles of the matrix
// instruction v_mfma_f64_16x16x4_f64.  The table is kept PADDED on the device, n x Fp with Fp = F rounded up to 16 and zeros
// behind column F, and so are the centres, the means and the precision factors: no kernel tests a column bound, the padding
// contributes exact zeros.  A workgroup (four waves) stages 32 table rows in LDS -- all loads requested, one barrier -- and every
// wave reads its A fragments from there; the B fragments (centres, precision factors) come from global memory, which L2 holds.
//   Lloyd    k_wide_assign   32 rows x all R C centres: |c|^2 - 2 x.c, argmin per (row, restart), one-hot responsibilities
//            k_wide_sums     sum r and sum r x per (restart, component) and row group       (also the first M-step pass of EM)
//            k_wide_lloyd_update                          centres = sums / counts, the stopping rule of _kmeans_single_lloyd
//   EM       k_wide_estep    y = x @ prec_chol - mu @ prec_chol per (restart, component), upper-triangular tiles only, then
//                            log density, log-sum-exp, responsibilities (n x C per restart, in HBM) and log_prob_norm
//            k_wide_sums, k_wide_means                    nk, means
//            k_wide_cov      sum r (x - mu)(x - mu)^T: lower-triangle tiles, diagonal tiles whole; k_wide_cov_reduce
//            k_wide_chol     one workgroup per (restart, component): blocked right-looking Cholesky (16-column panel in LDS,
//                            trailing update from global memory), then the triangular inverse
//            k_wide_install, k_wide_book                  parameters for the next E step; iteration count, flags, `done`
// Determinism.  No floating-point atomics (the one atomic is the integer count of changed labels).  Row ranges depend on n
// alone; a workgroup writes its partial sums to its own slot and a fixed-order pass adds the slots; every (restart, component)
// has its own arithmetic, so a restart gives the same bytes alone and in a batch.  Kernel boundaries order the passes: no
// grid-wide barrier, no waiting on memory, every loop's trip count is fixed by n, F, C, R.
// A restart that is done is skipped by every kernel: its parameters and outputs freeze.
#include "mixture_fit.h"

#include <cmath>
#include <limits>

namespace imsegm {

constexpr int WIDE_MIN_F = 17, WIDE_MAX_F = 256, WIDE_ROWS = 32, WIDE_XPAD = 4, WIDE_MAX_GROUPS = 16, WIDE_COV_TILES = 32;

typedef double wide_d4 __attribute__((ext_vector_type(4)));

// D (16 x 16) += A (16 x 4) B (4 x 16).  Lane l gives A[l & 15][l >> 4] and B[l >> 4][l & 15] and holds
// D[(l >> 4) + 4 reg][l & 15] in reg = 0..3 (the f64 map, not the f32 one).
__device__ __forceinline__ wide_d4 wide_mma(double a, double b, wide_d4 acc)
{
    return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
}

struct WideArgs {
    const double *X;            // [n][Fp]
    int n, F, Fp, TP, C, R, RC, RCp;      // TP = Fp / 16; RCp = R C rounded up to 16
    int G, G2, L2, T;           // G tiles of 32 rows; G2 row groups of L2 rows (a multiple of 32); T = TP (TP + 1) / 2 lower tiles
    int from_labels, max_iter;
    double tol, reg;
    int32_t *labels;            // [R][n]
    double *resp;               // [RC][n]
    double *centres, *cnorm;    // [RCp][Fp], [RCp]
    double *P;                  // [RC][Fp][Fp] precision Cholesky factors (upper triangular), what the E step reads
    double *muproj, *logw, *logdet;       // [RC][Fp], [RC], [RC]
    double *means_new, *nk;     // [RC][Fp], [RC]
    double *psum, *pnk;         // [G2][RC][Fp], [G2][RC]
    double *pcov;               // [G2][RC][T][256]
    double *A, *Z;              // [RC][Fp][Fp]: covariance -> its Cholesky factor (lower); the factor's inverse (lower)
    double *covs;               // [RC][Fp][Fp]: the covariance (lower half) until its factorisation has succeeded
    double *prow;               // [R][G]: per row tile, the sum of log_prob_norm (EM) or of squared distances (inertia)
    int *changed, *bad;         // [R], [RC]
    int *done, *strict, *n_iter, *flags, *pending, *converged;      // [R] each
    double *bound, *inertia, *bound_prev;                            // [R] each
    double *out_w, *out_means, *out_cov, *out_prec;
};

// 32 table rows from row0 on into LDS (row stride Fp + 4), zeros behind row n; optionally minus a mean
__device__ __forceinline__ void wide_stage(const WideArgs &a, double *xs, long row0, const double *minus, int tid)
{
    const int Fp = a.Fp, stride = Fp + WIDE_XPAD;
    for (int e = tid; e < WIDE_ROWS * Fp; e += 256) {
        const int row = e / Fp, col = e - row * Fp;
        const long i = row0 + row;
        double v = i < (long)a.n ? a.X[i * Fp + col] : 0.0;
        if (minus) v -= minus[col];
        xs[row * stride + col] = v;
    }
}

// the sum of `count` values in a fixed order: 256 strided sub-sums, then those in order (thread 0 returns it)
__device__ __forceinline__ double wide_ordered_sum(const double *p, int count, double *tmp, int tid)
{
    double sub = 0.0;
    for (int b = tid; b < count; b += 256) sub += p[b];
    tmp[tid] = sub;
    __syncthreads();
    double t = 0.0;
    if (tid == 0)
        for (int q = 0; q < 256; ++q) t += tmp[q];
    __syncthreads();
    return t;
}

__global__ void k_wide_cnorm(const WideArgs a)
{
    const int col = blockIdx.x * blockDim.x + threadIdx.x;
    if (col >= a.RCp) return;
    double s = 0.0;
    for (int f = 0; f < a.F; ++f) s += a.centres[(size_t)col * a.Fp + f] * a.centres[(size_t)col * a.Fp + f];
    a.cnorm[col] = s;
}

// FINAL = 0: one Lloyd labelling (labels, changed count, one-hot responsibilities) of the restarts that are not done.
// FINAL = 1: the labelling after the loop (not for a restart that stopped on unchanged labels) and the inertia's row-tile sums.
template <int FINAL> __global__ __launch_bounds__(256) void k_wide_assign(const WideArgs a)
{
    extern __shared__ double wide_lds[];
    const int tid = threadIdx.x, Fp = a.Fp, stride = Fp + WIDE_XPAD, RCp = a.RCp, C = a.C, R = a.R;
    double *xs = wide_lds, *dist = xs + WIDE_ROWS * stride, *ine = dist + WIDE_ROWS * RCp;      // ine: [R][32]
    const long row0 = (long)blockIdx.x * WIDE_ROWS;
    wide_stage(a, xs, row0, nullptr, tid);
    __syncthreads();
    const int w = tid >> 6, l = tid & 63, h = w & 1, q = w >> 1, g = l >> 4, c16 = l & 15, NCT = RCp >> 4;
    wide_d4 acc[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) acc[s] = (wide_d4){0.0, 0.0, 0.0, 0.0};
    const double *xrow = xs + (h * 16 + c16) * stride + g * 4;
    for (int kt = 0; kt < a.TP; ++kt) {
        double av[4];
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) av[kk] = xrow[kt * 16 + kk];
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int ct = q + 2 * s;
            if (ct < NCT) {
                const double *crow = a.centres + (size_t)(ct * 16 + c16) * Fp + kt * 16 + g * 4;
#pragma unroll
                for (int kk = 0; kk < 4; ++kk) acc[s] = wide_mma(av[kk], crow[kk], acc[s]);
            }
        }
    }
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const int ct = q + 2 * s;
        if (ct < NCT) {
            const int col = ct * 16 + c16;
            const double cc = a.cnorm[col];
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) dist[(h * 16 + g + 4 * reg) * RCp + col] = cc - 2.0 * acc[s][reg];
        }
    }
    __syncthreads();
    for (int p = tid; p < WIDE_ROWS * R; p += 256) {
        const int row = p & (WIDE_ROWS - 1), r = p / WIDE_ROWS;
        const long i = row0 + row;
        double sq = 0.0;
        const bool active = i < (long)a.n && (FINAL ? a.flags[r] == 0 : a.done[r] == 0);
        if (active) {
            int32_t *lab = a.labels + (size_t)r * a.n + i;
            int best = *lab;
            if (!FINAL || !a.strict[r]) {
                int now = 0;
                double bd = INFINITY;
                for (int c = 0; c < C; ++c) {
                    const double d = dist[row * RCp + r * C + c];
                    if (d < bd) {
                        bd = d;
                        now = c;
                    }
                }
                if (!FINAL && now != best) atomicAdd(a.changed + r, 1);
                *lab = now;
                best = now;
            }
            if (FINAL) {
                const double *cen = a.centres + (size_t)(r * C + best) * Fp;
                for (int f = 0; f < a.F; ++f) {
                    const double d = xs[row * stride + f] - cen[f];
                    sq += d * d;
                }
            } else {
                for (int c = 0; c < C; ++c) a.resp[(size_t)(r * C + c) * a.n + i] = c == best ? 1.0 : 0.0;
            }
        }
        if (FINAL) ine[r * WIDE_ROWS + row] = sq;
    }
    if (FINAL) {
        __syncthreads();
        if (tid < R) {
            double s = 0.0;
            for (int row = 0; row < WIDE_ROWS; ++row) s += ine[tid * WIDE_ROWS + row];
            a.prow[(size_t)tid * a.G + blockIdx.x] = s;
        }
    }
}

// one-hot responsibilities from labels (the M step of init_params='kmeans')
__global__ void k_wide_onehot(const WideArgs a)
{
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const int r = blockIdx.y;
    if (i >= (long)a.n) return;
    const int lab = a.labels[(size_t)r * a.n + i];
    for (int c = 0; c < a.C; ++c) a.resp[(size_t)(r * a.C + c) * a.n + i] = lab == c ? 1.0 : 0.0;
}

// sum r and sum r x of one row group for one (restart, component): thread f owns column f
__global__ __launch_bounds__(256) void k_wide_sums(const WideArgs a)
{
    const int tid = threadIdx.x, g2 = blockIdx.x, rc = blockIdx.y, Fp = a.Fp;
    if (a.done[rc / a.C]) return;
    const long i0 = (long)g2 * a.L2, i1 = i0 + a.L2 < (long)a.n ? i0 + a.L2 : (long)a.n;
    const double *resp = a.resp + (size_t)rc * a.n;
    const int f = tid < Fp ? tid : 0;
    double s = 0.0, cnt = 0.0;
    long i = i0;
    for (; i + 4 <= i1; i += 4) {
        double rv[4], xv[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            rv[k] = resp[i + k];
            xv[k] = a.X[(i + k) * Fp + f];
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            s += rv[k] * xv[k];
            cnt += rv[k];
        }
    }
    for (; i < i1; ++i) {
        const double rv = resp[i];
        s += rv * a.X[i * Fp + f];
        cnt += rv;
    }
    if (tid < Fp) a.psum[((size_t)g2 * a.RC + rc) * Fp + tid] = s;
    if (tid == 0) a.pnk[(size_t)g2 * a.RC + rc] = cnt;
}

// one workgroup per restart: centres = sums / counts, the centre shift, and the stopping rule
__global__ __launch_bounds__(256) void k_wide_lloyd_update(const WideArgs a)
{
    __shared__ double sh[FIT_MAX_C][WIDE_MAX_F];
    __shared__ double sq[FIT_MAX_C][WIDE_MAX_F];
    __shared__ int empty[FIT_MAX_C];
    const int tid = threadIdx.x, r = blockIdx.x, C = a.C, F = a.F, Fp = a.Fp;
    if (a.done[r]) return;
    for (int c = 0; c < C; ++c) {
        const int rc = r * C + c;
        double count = 0.0, tot = 0.0;
        for (int g2 = 0; g2 < a.G2; ++g2) {
            count += a.pnk[(size_t)g2 * a.RC + rc];
            if (tid < F) tot += a.psum[((size_t)g2 * a.RC + rc) * Fp + tid];
        }
        if (tid == 0) empty[c] = count == 0.0;
        if (tid < F) {
            double *cen = a.centres + (size_t)rc * Fp + tid;
            double d = 0.0, nv = *cen;
            if (count != 0.0) {
                nv = tot / count;
                d = nv - *cen;
                *cen = nv;
            }
            sh[c][tid] = d * d;
            sq[c][tid] = nv * nv;
        }
    }
    __syncthreads();
    if (tid < C) {
        double shift = 0.0, norm2 = 0.0;
        for (int f = 0; f < F; ++f) {
            shift += sh[tid][f];
            norm2 += sq[tid][f];
        }
        a.cnorm[r * C + tid] = norm2;
        const double norm = sqrt(shift);
        sh[tid][0] = norm * norm;
    }
    __syncthreads();
    if (tid == 0) {
        double shift_tot = 0.0;
        int any_empty = 0;
        for (int c = 0; c < C; ++c) {
            shift_tot += sh[c][0];
            any_empty |= empty[c];
        }
        const int it = a.n_iter[r] + 1, changed = a.changed[r];
        a.n_iter[r] = it;
        a.changed[r] = 0;
        if (any_empty) {
            a.flags[r] |= FIT_FLAG_EMPTY;
            a.done[r] = 1;
        } else if (changed == 0) {
            a.strict[r] = 1;
            a.done[r] = 1;
        } else if (shift_tot <= a.tol || it >= a.max_iter) {
            a.done[r] = 1;
        }
    }
}

__global__ __launch_bounds__(256) void k_wide_inertia(const WideArgs a)
{
    __shared__ double tmp[256];
    const int r = blockIdx.x;
    if (a.flags[r]) return;
    const double t = wide_ordered_sum(a.prow + (size_t)r * a.G, a.G, tmp, threadIdx.x);
    if (threadIdx.x == 0) a.inertia[r] = t;
}

// E step of 32 rows for one restart: _estimate_log_gaussian_prob + log weights, _estimate_log_prob_resp
__global__ __launch_bounds__(256) void k_wide_estep(const WideArgs a)
{
    extern __shared__ double wide_lds[];
    const int tid = threadIdx.x, r = blockIdx.y, Fp = a.Fp, stride = Fp + WIDE_XPAD, C = a.C;
    if (a.done[r]) return;
    double *xs = wide_lds, *mh = xs + WIDE_ROWS * stride, *lp = mh + 2 * WIDE_ROWS;      // mh: [2][32], lp: [C][32]
    const long row0 = (long)blockIdx.x * WIDE_ROWS;
    wide_stage(a, xs, row0, nullptr, tid);
    __syncthreads();
    const int w = tid >> 6, l = tid & 63, h = w & 1, q = w >> 1, g = l >> 4, c16 = l & 15;
    const double *xrow = xs + (h * 16 + c16) * stride + g * 4;
    for (int c = 0; c < C; ++c) {
        const int rc = r * C + c;
        const double *P = a.P + (size_t)rc * Fp * Fp, *mp = a.muproj + (size_t)rc * Fp;
        double s4[4] = {0.0, 0.0, 0.0, 0.0};
        for (int jt = q; jt < a.TP; jt += 2) {
            wide_d4 acc = (wide_d4){0.0, 0.0, 0.0, 0.0};
            const double *pcol = P + (size_t)(g * 4) * Fp + jt * 16 + c16;
            for (int kt = 0; kt <= jt; ++kt) {          // (the factor is upper triangular: tiles below the diagonal are zero)
#pragma unroll
                for (int kk = 0; kk < 4; ++kk) acc = wide_mma(xrow[kt * 16 + kk], pcol[(size_t)(kt * 16 + kk) * Fp], acc);
            }
            const double m = mp[jt * 16 + c16];
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const double y = acc[reg] - m;
                s4[reg] += y * y;
            }
        }
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            double v = s4[reg];
            v += __shfl_xor(v, 8);
            v += __shfl_xor(v, 4);
            v += __shfl_xor(v, 2);
            v += __shfl_xor(v, 1);
            if (c16 == 0) mh[q * WIDE_ROWS + h * 16 + g + 4 * reg] = v;
        }
        __syncthreads();
        if (tid < WIDE_ROWS) {
            const double maha = mh[tid] + mh[WIDE_ROWS + tid];
            lp[c * WIDE_ROWS + tid] = (-0.5 * ((double)a.F * 1.8378770664093453 + maha) + a.logdet[rc]) + a.logw[rc];
        }
        __syncthreads();
    }
    if (tid < WIDE_ROWS) {
        const long i = row0 + tid;
        double lpn = 0.0;
        if (i < (long)a.n) {
            double top = -INFINITY, sum = 0.0;
            for (int c = 0; c < C; ++c) top = fmax(top, lp[c * WIDE_ROWS + tid]);
            for (int c = 0; c < C; ++c) sum += exp(lp[c * WIDE_ROWS + tid] - top);
            lpn = top + log(sum);
            for (int c = 0; c < C; ++c) a.resp[(size_t)(r * C + c) * a.n + i] = exp(lp[c * WIDE_ROWS + tid] - lpn);
        }
        mh[tid] = lpn;
    }
    __syncthreads();
    if (tid == 0) {
        double s = 0.0;
        for (int row = 0; row < WIDE_ROWS; ++row) s += mh[row];
        a.prow[(size_t)r * a.G + blockIdx.x] = s;
    }
}

// one workgroup per (restart, component): nk and the means from the row groups' sums; component 0 also forms the lower bound
__global__ __launch_bounds__(256) void k_wide_means(const WideArgs a)
{
    __shared__ double tmp[256];
    const int tid = threadIdx.x, rc = blockIdx.x, r = rc / a.C, Fp = a.Fp;
    if (a.done[r]) return;
    double count = 0.0, tot = 0.0;
    for (int g2 = 0; g2 < a.G2; ++g2) {
        count += a.pnk[(size_t)g2 * a.RC + rc];
        if (tid < Fp) tot += a.psum[((size_t)g2 * a.RC + rc) * Fp + tid];
    }
    const double nk = count + 10.0 * 2.220446049250313e-16;
    if (tid < Fp) a.means_new[(size_t)rc * Fp + tid] = tot / nk;
    if (tid == 0) a.nk[rc] = nk;
    if (rc == r * a.C && !a.from_labels) {
        const double t = wide_ordered_sum(a.prow + (size_t)r * a.G, a.G, tmp, tid);
        if (tid == 0) {
            const double now = t / (double)a.n;
            a.pending[r] = fabs(now - a.bound[r]) < a.tol;
            a.bound_prev[r] = a.bound[r];
            a.bound[r] = now;
        }
    }
}

__device__ __forceinline__ void wide_tile_of(int t, int &ti, int &tj)
{
    int row = 0;
    while ((row + 1) * (row + 2) / 2 <= t) ++row;
    ti = row;
    tj = t - row * (row + 1) / 2;
}

// the centred weighted products of one row group for one (restart, component): up to 32 lower-triangle tiles per workgroup,
// eight per wave, a rank-32 update per staged chunk of rows
__global__ __launch_bounds__(256) void k_wide_cov(const WideArgs a)
{
    extern __shared__ double wide_lds[];
    const int tid = threadIdx.x, g2 = blockIdx.y, rc = blockIdx.z, Fp = a.Fp, stride = Fp + WIDE_XPAD;
    if (a.done[rc / a.C]) return;
    double *xs = wide_lds, *rs = xs + WIDE_ROWS * stride;
    const int w = tid >> 6, l = tid & 63, g = l >> 4, c16 = l & 15;
    int ti[8], tj[8];
    wide_d4 acc[8];
#pragma unroll
    for (int s = 0; s < 8; ++s) {
        const int t = blockIdx.x * WIDE_COV_TILES + s * 4 + w;
        wide_tile_of(t < a.T ? t : 0, ti[s], tj[s]);
        acc[s] = (wide_d4){0.0, 0.0, 0.0, 0.0};
    }
    const long i0 = (long)g2 * a.L2, i1 = i0 + a.L2 < (long)a.n ? i0 + a.L2 : (long)a.n;
    const double *mu = a.means_new + (size_t)rc * Fp, *resp = a.resp + (size_t)rc * a.n;
    for (long base = i0; base < i1; base += WIDE_ROWS) {
        __syncthreads();
        wide_stage(a, xs, base, mu, tid);
        if (tid < WIDE_ROWS) rs[tid] = base + tid < i1 ? resp[base + tid] : 0.0;
        __syncthreads();
#pragma unroll
        for (int s = 0; s < 8; ++s) {
            if (blockIdx.x * WIDE_COV_TILES + s * 4 + w < a.T) {
#pragma unroll
                for (int k = 0; k < WIDE_ROWS / 4; ++k) {
                    const int row = (k >> 2) * 16 + g * 4 + (k & 3);
                    const double *xr = xs + row * stride;
                    acc[s] = wide_mma(rs[row] * xr[ti[s] * 16 + c16], xr[tj[s] * 16 + c16], acc[s]);
                }
            }
        }
    }
#pragma unroll
    for (int s = 0; s < 8; ++s) {
        const int t = blockIdx.x * WIDE_COV_TILES + s * 4 + w;
        if (t < a.T) {
            double *out = a.pcov + (((size_t)g2 * a.RC + rc) * a.T + t) * 256;
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) out[(g + 4 * reg) * 16 + c16] = acc[s][reg];
        }
    }
}

// the row groups' tiles in order, / nk, + reg_covar: the covariance (lower half, staged: k_wide_install writes the output once
// the factorisation has succeeded) and the matrix to factor (lower half; behind F the identity)
__global__ __launch_bounds__(256) void k_wide_cov_reduce(const WideArgs a)
{
    const int tid = threadIdx.x, t = blockIdx.x, rc = blockIdx.y, F = a.F, Fp = a.Fp;
    if (a.done[rc / a.C]) return;
    int ti, tj;
    wide_tile_of(t, ti, tj);
    const int i = ti * 16 + (tid >> 4), j = tj * 16 + (tid & 15);
    if (j > i) return;
    double v = 0.0;
    for (int g2 = 0; g2 < a.G2; ++g2) v += a.pcov[(((size_t)g2 * a.RC + rc) * a.T + t) * 256 + tid];
    v /= a.nk[rc];
    if (i == j) v += a.reg;
    if (i >= F) v = i == j ? 1.0 : 0.0;
    a.A[((size_t)rc * Fp + i) * Fp + j] = v;
    a.covs[((size_t)rc * Fp + i) * Fp + j] = v;
}

// one workgroup per (restart, component): lower Cholesky factor of A in place (blocked, right-looking), then its inverse Z by
// forward substitution, a column per thread (_compute_precision_cholesky: precisions_cholesky_ = solve_triangular(L, I).T)
__global__ __launch_bounds__(256) void k_wide_chol(const WideArgs a)
{
    __shared__ double Dg[16][17];
    __shared__ double Lp[WIDE_MAX_F][17];
    __shared__ double Lrow[2][WIDE_MAX_F];
    __shared__ int bad;
    const int tid = threadIdx.x, rc = blockIdx.x, Fp = a.Fp, F = a.F;
    if (a.done[rc / a.C]) return;
    double *A = a.A + (size_t)rc * Fp * Fp, *Z = a.Z + (size_t)rc * Fp * Fp;
    const int w = tid >> 6, l = tid & 63, g = l >> 4, c16 = l & 15, da = tid >> 4, db = tid & 15;
    if (tid == 0) bad = 0;
    for (int p = 0; p < a.TP; ++p) {
        const int k0 = p * 16;
        Dg[da][db] = A[(size_t)(k0 + da) * Fp + k0 + db];
        __syncthreads();
        for (int j = 0; j < 16; ++j) {
            if (tid == 0) {
                const double s = Dg[j][j];
                if (!(s > 0.0) || !(s < INFINITY))
                    bad = 1;
                else
                    Dg[j][j] = sqrt(s);
            }
            __syncthreads();
            if (bad) break;
            if (tid > j && tid < 16) Dg[tid][j] = Dg[tid][j] / Dg[j][j];
            __syncthreads();
            if (da > j && db > j && db <= da) Dg[da][db] -= Dg[da][j] * Dg[db][j];
            __syncthreads();
        }
        if (bad) break;
        if (db <= da) A[(size_t)(k0 + da) * Fp + k0 + db] = Dg[da][db];
        const int below = Fp - k0 - 16;           // rows under the diagonal block
        if (tid < below) {
            double *arow = A + (size_t)(k0 + 16 + tid) * Fp + k0;
            double v[16];
#pragma unroll
            for (int b = 0; b < 16; ++b) v[b] = arow[b];
#pragma unroll
            for (int b = 0; b < 16; ++b) {
                double t = v[b];
#pragma unroll
                for (int k = 0; k < b; ++k) t -= v[k] * Dg[b][k];
                v[b] = t / Dg[b][b];
            }
#pragma unroll
            for (int b = 0; b < 16; ++b) {
                arow[b] = v[b];
                Lp[tid][b] = v[b];
            }
        }
        __syncthreads();
        const int m = below >> 4, cnt = m * (m + 1) / 2;
        for (int t = w; t < cnt; t += 4) {
            int ti, tj;
            wide_tile_of(t, ti, tj);
            double *tile = A + (size_t)(k0 + 16 + ti * 16) * Fp + k0 + 16 + tj * 16;
            wide_d4 acc;
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) acc[reg] = tile[(size_t)(g + 4 * reg) * Fp + c16];
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) acc = wide_mma(-Lp[ti * 16 + c16][g * 4 + kk], Lp[tj * 16 + c16][g * 4 + kk], acc);
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) tile[(size_t)(g + 4 * reg) * Fp + c16] = acc[reg];
        }
        __syncthreads();
    }
    if (tid == 0) a.bad[rc] = bad;
    if (bad) return;
    for (int i = 0; i < F; ++i) {
        double *buf = Lrow[i & 1];
        if (tid <= i) buf[tid] = A[(size_t)i * Fp + tid];
        __syncthreads();
        if (tid == i) {
            Z[(size_t)i * Fp + i] = 1.0 / buf[i];
        } else if (tid < i) {
            double s = 0.0;
            for (int k = tid; k < i; ++k) s += buf[k] * Z[(size_t)k * Fp + tid];
            Z[(size_t)i * Fp + tid] = -s / buf[i];
        }
    }
}

// one workgroup per (restart, component): what the E step reads, and the outputs.  START = 0: from the M step that just ran
// (nothing is written, the covariance included, when a component of the restart was not positive definite); START = 1: from the
// caller's start parameters in the output arrays (of the precision factors the upper triangle, which is all a Cholesky factor has).
template <int START> __global__ __launch_bounds__(256) void k_wide_install(const WideArgs a)
{
    __shared__ double lg[WIDE_MAX_F];
    const int tid = threadIdx.x, rc = blockIdx.x, r = rc / a.C, F = a.F, Fp = a.Fp;
    if (a.done[r]) return;
    if (!START)
        for (int c = 0; c < a.C; ++c)
            if (a.bad[r * a.C + c]) return;
    double *P = a.P + (size_t)rc * Fp * Fp, *Pout = a.out_prec + (size_t)rc * F * F;
    const double *Z = a.Z + (size_t)rc * Fp * Fp, *covs = a.covs + (size_t)rc * Fp * Fp;
    double *cov = a.out_cov + (size_t)rc * F * F;
    for (int e = tid; e < Fp * Fp; e += 256) {
        const int i = e / Fp, j = e - i * Fp;
        double v = 0.0;
        if (i < F && j < F) {
            if (START) {
                v = j >= i ? Pout[(size_t)i * F + j] : 0.0;
            } else {
                v = j >= i ? Z[(size_t)j * Fp + i] : 0.0;
                Pout[(size_t)i * F + j] = v;
                cov[(size_t)i * F + j] = j <= i ? covs[(size_t)i * Fp + j] : covs[(size_t)j * Fp + i];
            }
        }
        P[e] = v;
    }
    double *mout = a.out_means + (size_t)rc * F;
    if (!START && tid < F) mout[tid] = a.means_new[(size_t)rc * Fp + tid];
    __syncthreads();
    if (tid < Fp) {
        double s = 0.0;
        if (tid < F)
            for (int i = 0; i <= tid; ++i) s += mout[i] * P[(size_t)i * Fp + tid];
        a.muproj[(size_t)rc * Fp + tid] = s;
        lg[tid] = tid < F ? log(P[(size_t)tid * Fp + tid]) : 0.0;
    }
    __syncthreads();
    if (tid == 0) {
        double logdet = 0.0;
        for (int i = 0; i < F; ++i) logdet += lg[i];
        a.logdet[rc] = logdet;
        if (START) a.logw[rc] = log(a.out_w[rc]);
    }
}

// per restart, after the M step: the flag of a covariance that was not positive definite, or the weights and the iteration's end
__global__ void k_wide_book(const WideArgs a)
{
    const int r = threadIdx.x, C = a.C;
    if (r >= a.R || a.done[r]) return;
    int bad = 0;
    for (int c = 0; c < C; ++c) bad |= a.bad[r * C + c];
    if (bad) {
        a.flags[r] |= FIT_FLAG_NOT_PD;
        a.done[r] = 1;
        if (!a.from_labels) a.bound[r] = a.bound_prev[r];        // (the iteration did not complete)
        return;
    }
    double wq[FIT_MAX_C], wsum = 0.0;
    for (int c = 0; c < C; ++c) {
        wq[c] = a.nk[r * C + c] / (double)a.n;
        wsum += wq[c];
    }
    for (int c = 0; c < C; ++c) {
        const double v = wq[c] / wsum;
        a.out_w[r * C + c] = v;
        a.logw[r * C + c] = log(v);
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

}  // namespace imsegm

// ---------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------
namespace {

using namespace imsegm;

struct WideLayout {
    size_t o_labels, o_resp, o_centres, o_cnorm, o_P, o_muproj, o_small, o_means_new, o_psum, o_pnk, o_pcov, o_A, o_Z, o_covs, o_prow, o_ints,
        o_dbl, o_w, o_means, o_cov, o_prec, bytes;
    int Fp, TP, RC, RCp, G, G2, L2, T;
};

constexpr int WIDE_INTS = 8, WIDE_DBLS = 3;       // bookkeeping words per restart (bad: per component, behind them)

WideLayout wide_layout(int n, int F, int C, int R)
{
    WideLayout lay;
    lay.Fp = (F + 15) & ~15;
    lay.TP = lay.Fp / 16;
    lay.RC = R * C;
    lay.RCp = (lay.RC + 15) & ~15;
    lay.G = cdiv(n, WIDE_ROWS);
    const int per = cdiv(lay.G, WIDE_MAX_GROUPS);
    lay.L2 = per * WIDE_ROWS;
    lay.G2 = cdiv(lay.G, per);
    lay.T = lay.TP * (lay.TP + 1) / 2;
    size_t at = 0;
    auto take = [&](size_t bytes) {
        const size_t here = at;
        at += (bytes + 255) & ~(size_t)255;
        return here;
    };
    const size_t Fp = lay.Fp, RC = lay.RC;
    lay.o_labels = take((size_t)R * n * 4);
    lay.o_resp = take(RC * n * 8);
    lay.o_centres = take((size_t)lay.RCp * Fp * 8);
    lay.o_cnorm = take((size_t)lay.RCp * 8);
    lay.o_P = take(RC * Fp * Fp * 8);
    lay.o_muproj = take(RC * Fp * 8);
    lay.o_small = take(RC * 3 * 8);                 // logw, logdet, nk
    lay.o_means_new = take(RC * Fp * 8);
    lay.o_psum = take((size_t)lay.G2 * RC * Fp * 8);
    lay.o_pnk = take((size_t)lay.G2 * RC * 8);
    lay.o_pcov = take((size_t)lay.G2 * RC * lay.T * 256 * 8);
    lay.o_A = take(RC * Fp * Fp * 8);
    lay.o_Z = take(RC * Fp * Fp * 8);
    lay.o_covs = take(RC * Fp * Fp * 8);
    lay.o_prow = take((size_t)R * lay.G * 8);
    lay.o_ints = take(((size_t)WIDE_INTS * R + RC) * 4);
    lay.o_dbl = take((size_t)WIDE_DBLS * R * 8);
    lay.o_w = take(RC * 8);
    lay.o_means = take(RC * F * 8);
    lay.o_cov = take(RC * F * F * 8);
    lay.o_prec = take(RC * F * F * 8);
    lay.bytes = at;
    return lay;
}

WideArgs wide_args(imsegm_ctx *ctx, const WideLayout &lay, int C, int R)
{
    WideArgs a;
    memset(&a, 0, sizeof(a));
    unsigned char *w = ctx->fit_work.as<unsigned char>();
    auto dbl = [&](size_t off) { return reinterpret_cast<double *>(w + off); };
    a.X = ctx->fit_table.as<double>();
    a.n = ctx->fit_n;
    a.F = ctx->fit_F;
    a.Fp = lay.Fp;
    a.TP = lay.TP;
    a.C = C;
    a.R = R;
    a.RC = lay.RC;
    a.RCp = lay.RCp;
    a.G = lay.G;
    a.G2 = lay.G2;
    a.L2 = lay.L2;
    a.T = lay.T;
    a.labels = reinterpret_cast<int32_t *>(w + lay.o_labels);
    a.resp = dbl(lay.o_resp);
    a.centres = dbl(lay.o_centres);
    a.cnorm = dbl(lay.o_cnorm);
    a.P = dbl(lay.o_P);
    a.muproj = dbl(lay.o_muproj);
    a.logw = dbl(lay.o_small);
    a.logdet = a.logw + lay.RC;
    a.nk = a.logw + 2 * lay.RC;
    a.means_new = dbl(lay.o_means_new);
    a.psum = dbl(lay.o_psum);
    a.pnk = dbl(lay.o_pnk);
    a.pcov = dbl(lay.o_pcov);
    a.A = dbl(lay.o_A);
    a.Z = dbl(lay.o_Z);
    a.covs = dbl(lay.o_covs);
    a.prow = dbl(lay.o_prow);
    int *ints = reinterpret_cast<int *>(w + lay.o_ints);
    a.done = ints;
    a.strict = ints + R;
    a.n_iter = ints + 2 * R;
    a.flags = ints + 3 * R;
    a.pending = ints + 4 * R;
    a.converged = ints + 5 * R;
    a.changed = ints + 6 * R;
    a.bad = ints + WIDE_INTS * R;
    a.bound = dbl(lay.o_dbl);
    a.inertia = a.bound + R;
    a.bound_prev = a.bound + 2 * R;
    a.out_w = dbl(lay.o_w);
    a.out_means = dbl(lay.o_means);
    a.out_cov = dbl(lay.o_cov);
    a.out_prec = dbl(lay.o_prec);
    return a;
}

int wide_caps(const char *who, long n, int F, int C, int R)
{
    if (n < 1 || F < 1 || C < 1 || R < 1) {
        set_error(std::string(who) + ": bad arguments");
        return -1;
    }
    if (F < WIDE_MIN_F || F > WIDE_MAX_F || C > FIT_MAX_C || R > FIT_MAX_R || n >= 2147483647L) {
        set_error(std::string(who) + ": outside the caps of the wide device fit (17 <= features <= 256, components <= 8, restarts <= 16, "
                                     "rows < 2^31)");
        return IMSEGM_E_FIT_CAPS;
    }
    return 0;
}

size_t wide_stage_bytes(const WideArgs &a) { return (size_t)WIDE_ROWS * (a.Fp + WIDE_XPAD) * 8; }

// (a workgroup's staged rows pass 64 KB at 256 features: the kernels with dynamic LDS are told their largest size once per call)
template <typename K> int wide_allow_lds(K kernel, size_t bytes)
{
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    return 0;
}

size_t wide_assign_lds(const WideArgs &a) { return wide_stage_bytes(a) + (size_t)WIDE_ROWS * a.RCp * 8 + (size_t)FIT_MAX_R * WIDE_ROWS * 8; }

template <int FINAL> int wide_assign(const WideArgs &a, hipStream_t st)
{
    const size_t lds = wide_assign_lds(a);
    hipLaunchKernelGGL((k_wide_assign<FINAL>), dim3(a.G), dim3(256), lds, st, a);
    HIP_TRY(hipGetLastError());
    return 0;
}

int wide_sums(const WideArgs &a, hipStream_t st)
{
    hipLaunchKernelGGL(k_wide_sums, dim3(a.G2, a.RC), dim3(256), 0, st, a);
    HIP_TRY(hipGetLastError());
    return 0;
}

int wide_lloyd_step(const WideArgs &a, hipStream_t st)
{
    if (wide_assign<0>(a, st) || wide_sums(a, st)) return -1;
    hipLaunchKernelGGL(k_wide_lloyd_update, dim3(a.R), dim3(256), 0, st, a);
    HIP_TRY(hipGetLastError());
    return 0;
}

// nk, means, centred products, factorisation, the next E step's parameters, bookkeeping
int wide_m_step(const WideArgs &a, hipStream_t st)
{
    if (wide_sums(a, st)) return -1;
    hipLaunchKernelGGL(k_wide_means, dim3(a.RC), dim3(256), 0, st, a);
    HIP_TRY(hipGetLastError());
    const size_t lds = wide_stage_bytes(a) + WIDE_ROWS * 8;
    hipLaunchKernelGGL(k_wide_cov, dim3(cdiv(a.T, WIDE_COV_TILES), a.G2, a.RC), dim3(256), lds, st, a);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_wide_cov_reduce, dim3(a.T, a.RC), dim3(256), 0, st, a);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_wide_chol, dim3(a.RC), dim3(256), 0, st, a);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL((k_wide_install<0>), dim3(a.RC), dim3(256), 0, st, a);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_wide_book, dim3(1), dim3(64), 0, st, a);
    HIP_TRY(hipGetLastError());
    return 0;
}

int wide_em_step(const WideArgs &a, hipStream_t st)
{
    const size_t lds = wide_stage_bytes(a) + (size_t)(2 + FIT_MAX_C) * WIDE_ROWS * 8;
    hipLaunchKernelGGL(k_wide_estep, dim3(a.G, a.R), dim3(256), lds, st, a);
    HIP_TRY(hipGetLastError());
    return wide_m_step(a, st);
}

}  // namespace

extern "C" {

int imsegm_kmeans_lloyd_wide(imsegm_ctx *ctx, const double *table, long n_rows, int n_features, const double *seeds, int n_restarts,
                             int n_clusters, int max_iter, double tol, int32_t *labels_out, double *centres_out, double *inertia_out,
                             int32_t *n_iter_out, int32_t *empty_out)
{
    if (bind(ctx)) return -1;
    if (!table || !seeds || max_iter < 1) {
        set_error("kmeans_lloyd_wide: bad arguments");
        return -1;
    }
    if (const int rc = wide_caps("kmeans_lloyd_wide", n_rows, n_features, n_clusters, n_restarts)) return rc;
    const int n = (int)n_rows, F = n_features, C = n_clusters, R = n_restarts;
    hipStream_t st = ctx->stream;
    ctx->fit_n = ctx->fit_F = ctx->fit_label_restarts = 0;
    const WideLayout lay = wide_layout(n, F, C, R);
    const size_t Fp = lay.Fp;
    if (ctx->fit_table.ensure((size_t)n * Fp * 8)) return -1;
    if (ctx->fit_work.ensure(lay.bytes)) return -1;
    ctx->fit_n = n;
    ctx->fit_F = F;
    WideArgs a = wide_args(ctx, lay, C, R);
    a.max_iter = max_iter;
    a.tol = tol;
    unsigned char *w = ctx->fit_work.as<unsigned char>();
    // the table and the seeds in their padded form: zeros behind column F
    if (Fp != (size_t)F) HIP_TRY(hipMemsetAsync(ctx->fit_table.p, 0, (size_t)n * Fp * 8, st));
    HIP_TRY(hipMemcpy2DAsync(ctx->fit_table.p, Fp * 8, table, (size_t)F * 8, (size_t)F * 8, n, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(a.centres, 0, (size_t)lay.RCp * Fp * 8, st));
    HIP_TRY(hipMemcpy2DAsync(a.centres, Fp * 8, seeds, (size_t)F * 8, (size_t)F * 8, (size_t)R * C, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(a.labels, 0xff, (size_t)R * n * 4, st));          // no row has a label yet (-1)
    HIP_TRY(hipMemsetAsync(w + lay.o_ints, 0, ((size_t)WIDE_INTS * R + lay.RC) * 4, st));
    HIP_TRY(hipMemsetAsync(w + lay.o_dbl, 0, (size_t)WIDE_DBLS * R * 8, st));
    if (wide_allow_lds(k_wide_assign<0>, wide_assign_lds(a)) || wide_allow_lds(k_wide_assign<1>, wide_assign_lds(a))) return -1;
    hipLaunchKernelGGL(k_wide_cnorm, dim3(cdiv(lay.RCp, 64)), dim3(64), 0, st, a);
    HIP_TRY(hipGetLastError());
    if (fit_iterate(a.done, R, max_iter, st, [&]() { return wide_lloyd_step(a, st); })) return -1;
    if (wide_assign<1>(a, st)) return -1;
    hipLaunchKernelGGL(k_wide_inertia, dim3(R), dim3(256), 0, st, a);
    HIP_TRY(hipGetLastError());
    int ints[WIDE_INTS * FIT_MAX_R];
    HIP_TRY(hipMemcpyAsync(ints, w + lay.o_ints, (size_t)WIDE_INTS * R * 4, hipMemcpyDeviceToHost, st));
    if (labels_out) HIP_TRY(hipMemcpyAsync(labels_out, a.labels, (size_t)R * n * 4, hipMemcpyDeviceToHost, st));
    if (centres_out)
        HIP_TRY(hipMemcpy2DAsync(centres_out, (size_t)F * 8, a.centres, Fp * 8, (size_t)F * 8, (size_t)R * C, hipMemcpyDeviceToHost, st));
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

int imsegm_mixture_em_wide(imsegm_ctx *ctx, int n_restarts, int n_components, const int32_t *labels, const double *weights_init,
                           const double *means_init, const double *prec_chol_init, double reg_covar, double tol, int max_iter,
                           double *weights_out, double *means_out, double *covariances_out, double *prec_chol_out,
                           double *lower_bound_out, int32_t *n_iter_out, int32_t *converged_out, int32_t *not_pd_out)
{
    if (bind(ctx)) return -1;
    if (ctx->fit_n < 1) {
        set_error("mixture_em_wide: no resident table (imsegm_kmeans_lloyd_wide uploads it)");
        return -1;
    }
    const int n = ctx->fit_n, F = ctx->fit_F, C = n_components, R = n_restarts;
    if (const int rc = wide_caps("mixture_em_wide", n, F, C, R)) return rc;
    const bool from_params = weights_init && means_init && prec_chol_init;
    if (max_iter < 0 || (!from_params && (weights_init || means_init || prec_chol_init))) {
        set_error("mixture_em_wide: bad arguments (start parameters are weights, means and precision factors together)");
        return -1;
    }
    if (!from_params && !labels && (ctx->fit_label_restarts != R || ctx->fit_label_classes != C)) {
        set_error("mixture_em_wide: no resident labels of that many restarts and classes (imsegm_kmeans_lloyd_wide leaves them)");
        return -1;
    }
    hipStream_t st = ctx->stream;
    const WideLayout lay = wide_layout(n, F, C, R);
    if (!from_params && !labels && ctx->fit_work.cap < lay.bytes) {
        set_error("mixture_em_wide: the resident labels are gone");
        return -1;
    }
    if ((from_params || labels) && (ctx->fit_label_restarts != R || ctx->fit_label_classes != C || ctx->fit_work.cap < lay.bytes))
        ctx->fit_label_restarts = 0;           // (the buffers of another layout overwrite labels that were resident)
    if (ctx->fit_work.ensure(lay.bytes)) return -1;
    WideArgs a = wide_args(ctx, lay, C, R);
    a.max_iter = max_iter;
    a.tol = tol;
    a.reg = reg_covar;
    unsigned char *w = ctx->fit_work.as<unsigned char>();
    const size_t RC = lay.RC;
    if (wide_allow_lds(k_wide_estep, wide_stage_bytes(a) + (size_t)(2 + FIT_MAX_C) * WIDE_ROWS * 8)) return -1;
    if (wide_allow_lds(k_wide_cov, wide_stage_bytes(a) + WIDE_ROWS * 8)) return -1;
    HIP_TRY(hipMemsetAsync(w + lay.o_ints, 0, ((size_t)WIDE_INTS * R + RC) * 4, st));
    double start[WIDE_DBLS * FIT_MAX_R];
    for (int r = 0; r < WIDE_DBLS * R; ++r) start[r] = r < R || r >= 2 * R ? -std::numeric_limits<double>::infinity() : 0.0;
    HIP_TRY(hipMemcpyAsync(w + lay.o_dbl, start, (size_t)WIDE_DBLS * R * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(a.out_cov, 0, RC * F * F * 8, st));
    if (from_params) {
        HIP_TRY(hipMemcpyAsync(a.out_w, weights_init, RC * 8, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(a.out_means, means_init, RC * F * 8, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(a.out_prec, prec_chol_init, RC * F * F * 8, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL((k_wide_install<1>), dim3(lay.RC), dim3(256), 0, st, a);
        HIP_TRY(hipGetLastError());
    } else {
        // (a restart whose first M step fails returns zeros, not what an earlier call left in the buffer)
        HIP_TRY(hipMemsetAsync(a.out_w, 0, RC * 8, st));
        HIP_TRY(hipMemsetAsync(a.out_means, 0, RC * F * 8, st));
        HIP_TRY(hipMemsetAsync(a.out_prec, 0, RC * F * F * 8, st));
        if (labels) {
            ctx->fit_label_restarts = 0;
            HIP_TRY(hipMemcpyAsync(a.labels, labels, (size_t)R * n * 4, hipMemcpyHostToDevice, st));
        }
        a.from_labels = 1;      // the M step of the initialisation: no iteration is counted, no bound formed
        hipLaunchKernelGGL(k_wide_onehot, dim3(cdiv(n, 256), R), dim3(256), 0, st, a);
        HIP_TRY(hipGetLastError());
        if (wide_m_step(a, st)) return -1;
        a.from_labels = 0;
    }
    HIP_TRY(hipStreamSynchronize(st));          // (pageable sources are free again)
    if (fit_iterate(a.done, R, max_iter, st, [&]() { return wide_em_step(a, st); })) return -1;
    int ints[WIDE_INTS * FIT_MAX_R];
    double bounds[WIDE_DBLS * FIT_MAX_R];
    HIP_TRY(hipMemcpyAsync(ints, w + lay.o_ints, (size_t)WIDE_INTS * R * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(bounds, w + lay.o_dbl, (size_t)WIDE_DBLS * R * 8, hipMemcpyDeviceToHost, st));
    if (weights_out) HIP_TRY(hipMemcpyAsync(weights_out, a.out_w, RC * 8, hipMemcpyDeviceToHost, st));
    if (means_out) HIP_TRY(hipMemcpyAsync(means_out, a.out_means, RC * F * 8, hipMemcpyDeviceToHost, st));
    if (covariances_out) HIP_TRY(hipMemcpyAsync(covariances_out, a.out_cov, RC * F * F * 8, hipMemcpyDeviceToHost, st));
    if (prec_chol_out) HIP_TRY(hipMemcpyAsync(prec_chol_out, a.out_prec, RC * F * F * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (int r = 0; r < R; ++r) {
        if (lower_bound_out) lower_bound_out[r] = bounds[r];
        if (n_iter_out) n_iter_out[r] = ints[2 * R + r];
        if (converged_out) converged_out[r] = ints[5 * R + r];
        if (not_pd_out) not_pd_out[r] = (ints[3 * R + r] & FIT_FLAG_NOT_PD) != 0;
    }
    return 0;
}

}  // extern "C"
