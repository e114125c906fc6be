// region_growing.hip -- the kernels behind the growth loop of imsegm/region_growing.py (region_growing_shape_slic_greedy :1155,
// region_growing_shape_slic_graphcut :1482) on the resident state of api_region_growing.hip: the shape prior of every (object,
// superpixel) pair (compute_shape_prior_table_cdf :591-652), the ray distances of every object's mask (compute_segm_object_shape
// :259-286 through computeRayFeaturesBinary2d), the candidates of an iteration with their energy changes (:1346-1371) and the
// criterion (compute_rg_crit :1114-1133).  All fp64 (the rays float32, as the .pyx), every operation rounds on its own
// (-ffp-contract=off), sums in a fixed order, no floating-point atomics.  The numpy statement of the same definitions is
// pyimsegm_amd/region_growing.py (on='host').
#include "raywalk.h"
#include "region_growing.h"
#include "slic.h"

#include <math.h>

namespace imsegm {

constexpr int RG_THREADS = 256;
constexpr double RG_MIN_SHAPE_PROB = 0.01;           // MIN_SHAPE_PROB
constexpr double RG_REPLACE_INF = 1e5;               // GC_REPLACE_INF

// np.round(centres).astype(int): half to even; a label without pixels has the centre (-1, -1) and keeps it
__global__ __launch_bounds__(RG_THREADS) void k_rg_points(const double *__restrict__ centres, int K, int32_t *__restrict__ points)
{
    const int i = blockIdx.x * RG_THREADS + threadIdx.x;
    if (i < 2 * K) points[i] = (int32_t)rint(centres[i]);
}

// Python's a % 360 for floats (numpy's npy_divmod): the sign follows the divisor
__device__ __forceinline__ double py_mod360(double a)
{
    double m = fmod(a, 360.0);
    if (m != 0.0) {
        if (m < 0.0) m += 360.0;
    } else {
        m = 0.0;
    }
    return m;
}

// compute_shape_prior_table_cdf for one point, operation by operation; table: A x D row-major, row A is row 0 again
__device__ __forceinline__ double rg_shape_prior(double px, double py, double cx, double cy, double shift, const double *__restrict__ table,
                                                 int A, int D)
{
    const double angle_step = 360.0 / (double)A;
    const double dx = px - cx, dy = py - cy;
    const double dist = sqrt(dx * dx + dy * dy);
    double angle = atan2(dy, dx) * 57.29577951308232;               // np.rad2deg: x * (180 / pi)
    angle = py_mod360((810.0 - angle) - shift);
    const double angle_norm = angle / angle_step;
    if (dist >= (double)(D - 1)) {
        int row = (int)rint(angle_norm);                            // Python's round: half to even
        if (row >= A) row = 0;
        return table[(size_t)row * D + (D - 1)];
    }
    int a0 = (int)floor(angle_norm);
    double ta = angle_norm - (double)a0;
    if (a0 >= A) {                                                  // the modulus rounded to 360.0 itself: row 0, weight 0
        a0 = 0;
        ta = 0.0;
    }
    const int a1 = a0 + 1 >= A ? 0 : a0 + 1;
    const int d0 = (int)floor(dist);                                // dist < D - 1, so d0 + 1 <= D - 1
    const double td = dist - (double)d0;
    const double v00 = table[(size_t)a0 * D + d0], v01 = table[(size_t)a0 * D + d0 + 1];
    const double v10 = table[(size_t)a1 * D + d0], v11 = table[(size_t)a1 * D + d0 + 1];
    const double low = v00 + (v01 - v00) * td, high = v10 + (v11 - v10) * td;
    return low + (high - low) * ta;
}

// One lane per (selected object, superpixel): lut_shape[s, object + 1] = -log(prior + MIN_SHAPE_PROB), +-inf replaced.
__global__ __launch_bounds__(RG_THREADS) void k_rg_shape_cost(const int32_t *__restrict__ points, int K, int n_obj,
                                                              const int32_t *__restrict__ objects, const double *__restrict__ centres,
                                                              const double *__restrict__ shifts, const int32_t *__restrict__ dims,
                                                              const long long *__restrict__ offsets,
                                                              const double *__restrict__ tables, double *__restrict__ lut_shape,
                                                              double *__restrict__ proba)
{
    const int j = blockIdx.y;
    const int s = blockIdx.x * RG_THREADS + threadIdx.x;
    if (s >= K) return;
    const int obj = objects[j], A = dims[2 * j], D = dims[2 * j + 1];
    const double p = rg_shape_prior((double)points[2 * s], (double)points[2 * s + 1], centres[2 * j], centres[2 * j + 1], shifts[j],
                                    tables + offsets[j], A, D);
    double cost = -log(p + RG_MIN_SHAPE_PROB);
    if (isinf(cost)) cost = RG_REPLACE_INF;
    lut_shape[(size_t)s * (n_obj + 1) + obj + 1] = cost;
    if (proba) proba[(size_t)j * K + s] = p;
}

// computeRayFeaturesBinary2d (the walk of raywalk.h) with edge 'down' on the mask labels[slic[y][x]] == object + 1, which is never
// materialised.  One wave per object, one lane per angle.
__global__ __launch_bounds__(64) void k_rg_object_rays(const int32_t *__restrict__ slic, int H, int W, const int32_t *__restrict__ labels,
                                                       int K, const int32_t *__restrict__ positions, const float *__restrict__ grad,
                                                       int A, float *__restrict__ out)
{
    const int o = blockIdx.x, obj = o + 1;
    const int py = positions[2 * o], px = positions[2 * o + 1];
    const bool inside = py >= 0 && py < H && px >= 0 && px < W;
    auto mask = [&](int y, int x) -> bool {
        const int l = slic[(size_t)y * W + x];
        return (unsigned)l < (unsigned)K && labels[l] == obj;
    };
    const bool start = inside ? mask(py, px) : false;
    const int diag = ray_walk_limit(H, W);
    for (int a = threadIdx.x; a < A; a += 64)
        out[(size_t)o * A + a] = ray_walk(py, px, inside, start, grad[2 * a], grad[2 * a + 1], H, W, diag, -1, mask);
}

// get_neighboring_candidates for every object at once: one lane per (object, superpixel); the pair qualifies when the superpixel
// has a neighbour labelled with the object and is itself not of the object (allow_obj_swap) or background (otherwise).
__global__ __launch_bounds__(RG_THREADS) void k_rg_candidates(const int32_t *__restrict__ labels, const int32_t *__restrict__ nb_off,
                                                              const int32_t *__restrict__ nb, int K, int allow_obj_swap,
                                                              uint8_t *__restrict__ flags, int32_t *__restrict__ slots)
{
    const int obj = blockIdx.y + 1;
    const int s = blockIdx.x * RG_THREADS + threadIdx.x;
    if (s >= K) return;
    const int own = labels[s];
    bool found = false;
    if (allow_obj_swap ? own != obj : own == 0)
        for (int e = nb_off[s]; e < nb_off[s + 1] && !found; ++e) found = labels[nb[e]] == obj;
    const size_t at = (size_t)blockIdx.y * K + s;
    flags[at] = found;
    slots[at] = found;
}

__device__ __forceinline__ double rg_penalty(int a, int b, double pen_bg, double pen_fg)
{
    return a == b ? 0.0 : ((a == 0 || b == 0) ? pen_bg : pen_fg);
}

// The flagged pairs in the reference's order (object-major, superpixels ascending: `slots` is the exclusive scan of the flags)
// and what relabelling the superpixel would take off the criterion, in its delta form.
__global__ __launch_bounds__(RG_THREADS) void k_rg_scores(const int32_t *__restrict__ labels, const int32_t *__restrict__ nb_off,
                                                          const int32_t *__restrict__ nb, const long long *__restrict__ sums,
                                                          const double *__restrict__ lut_data, const double *__restrict__ lut_shape,
                                                          int K, int n_obj, RgCoefs c, int with_scores,
                                                          const uint8_t *__restrict__ flags, const int32_t *__restrict__ slots,
                                                          int32_t *__restrict__ cand_obj, int32_t *__restrict__ cand_sp,
                                                          double *__restrict__ cand_change)
{
    const int obj = blockIdx.y + 1;
    const int s = blockIdx.x * RG_THREADS + threadIdx.x;
    if (s >= K) return;
    const size_t at = (size_t)blockIdx.y * K + s;
    if (!flags[at]) return;
    const int slot = slots[at];
    cand_obj[slot] = obj;
    cand_sp[slot] = s;
    if (!with_scores) return;
    const int old = labels[s];
    const size_t row = (size_t)s * (n_obj + 1);
    const double unary = c.data * (lut_data[row + old] - lut_data[row + obj]) + c.shape * (lut_shape[row + old] - lut_shape[row + obj]);
    double change = (double)sums[3 * (size_t)s] * unary;
    if (c.pairwise > 0.0) {
        double pair = 0.0;
        for (int e = nb_off[s]; e < nb_off[s + 1]; ++e) {
            const int other = labels[nb[e]];
            pair += rg_penalty(old, other, c.pen_bg, c.pen_fg) - rg_penalty(obj, other, c.pen_bg, c.pen_fg);
        }
        change = change + c.pairwise * pair;
    }
    cand_change[slot] = change;
}

// the 256 partial sums of a workgroup in a fixed tree: butterfly inside a wave, the four waves in one expression
__device__ __forceinline__ double rg_block_sum(double acc, double *part)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
    __syncthreads();
    return (part[0] + part[1]) + (part[2] + part[3]);
}

// compute_rg_crit: one workgroup; lane i adds the superpixels (then the edges) i, i + 256, ... in that order, two trees that
// depend on K and E alone: the same labels give the same bytes.
__global__ __launch_bounds__(RG_THREADS) void k_rg_crit(const int32_t *__restrict__ labels, const long long *__restrict__ sums,
                                                        const double *__restrict__ lut_data, const double *__restrict__ lut_shape,
                                                        const int32_t *__restrict__ edges, int K, int n_obj, int E, RgCoefs c,
                                                        double *__restrict__ crit)
{
    __shared__ double part[RG_THREADS / 64];
    double acc = 0.0;
    for (int s = threadIdx.x; s < K; s += RG_THREADS) {
        const size_t at = (size_t)s * (n_obj + 1) + labels[s];
        acc += (double)sums[3 * (size_t)s] * (c.data * lut_data[at] + c.shape * lut_shape[at]);
    }
    double total = rg_block_sum(acc, part);
    if (c.pairwise > 0.0) {                                         // (uniform)
        acc = 0.0;
        for (int e = threadIdx.x; e < E; e += RG_THREADS) acc += rg_penalty(labels[edges[2 * e]], labels[edges[2 * e + 1]], c.pen_bg, c.pen_fg);
        total = total + c.pairwise * rg_block_sum(acc, part);
    }
    if (threadIdx.x == 0) *crit = total;
}

int launch_rg_points(const double *centres, int K, int32_t *points, hipStream_t st)
{
    hipLaunchKernelGGL(k_rg_points, cdiv(2 * (long)K, RG_THREADS), RG_THREADS, 0, st, centres, K, points);
    HIP_TRY(hipGetLastError());
    return 0;
}

int launch_rg_shape_cost(const RgView &v, const RgShapeJob &job, int n_sel, hipStream_t st)
{
    if (n_sel < 1) return 0;
    hipLaunchKernelGGL(k_rg_shape_cost, dim3(cdiv(v.K, RG_THREADS), n_sel), RG_THREADS, 0, st, v.points, v.K, v.n_obj, job.objects,
                       job.centres, job.shifts, job.dims, job.offsets, job.tables, v.lut_shape, job.proba);
    HIP_TRY(hipGetLastError());
    return 0;
}

int launch_rg_object_rays(const RgView &v, const int32_t *positions, const float *directions, int A, float *out, hipStream_t st)
{
    hipLaunchKernelGGL(k_rg_object_rays, v.n_obj, 64, 0, st, v.slic, v.H, v.W, v.labels, v.K, positions, directions, A, out);
    HIP_TRY(hipGetLastError());
    return 0;
}

int launch_rg_candidates(const RgView &v, int allow_obj_swap, hipStream_t st)
{
    hipLaunchKernelGGL(k_rg_candidates, dim3(cdiv(v.K, RG_THREADS), v.n_obj), RG_THREADS, 0, st, v.labels, v.nb_off, v.nb, v.K,
                       allow_obj_swap, v.flags, v.slots);
    HIP_TRY(hipGetLastError());
    launch_exclusive_scan(v.slots, v.n_obj * v.K, v.slots + (size_t)v.n_obj * v.K, st);
    HIP_TRY(hipGetLastError());
    return 0;
}

int launch_rg_scores(const RgView &v, const RgCoefs &c, bool with_scores, hipStream_t st)
{
    hipLaunchKernelGGL(k_rg_scores, dim3(cdiv(v.K, RG_THREADS), v.n_obj), RG_THREADS, 0, st, v.labels, v.nb_off, v.nb, v.sums, v.lut_data,
                       v.lut_shape, v.K, v.n_obj, c, with_scores ? 1 : 0, v.flags, v.slots, v.cand_obj, v.cand_sp, v.cand_change);
    HIP_TRY(hipGetLastError());
    return 0;
}

int launch_rg_crit(const RgView &v, const RgCoefs &c, hipStream_t st)
{
    hipLaunchKernelGGL(k_rg_crit, 1, RG_THREADS, 0, st, v.labels, v.sums, v.lut_data, v.lut_shape, v.edges, v.K, v.n_obj, v.E, c, v.crit);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // namespace imsegm
