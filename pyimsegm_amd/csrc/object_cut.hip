// object_cut.hip -- the front of a graph cut on a pixel grid (object_cut.h): grid arcs in closed form, pyGCO's float -> integer
// conversion, the unary costs of object_segmentation_graphcut_pixels.  All of them stream: what counts is the bytes they write
// (4 K (C + 1) of integer unary costs, 40 bytes of arcs per site).  The library is built with -ffp-contract=off: the division and
// the multiplication of the conversion round one after the other as they do on the host (csrc/terms.hip does the same).
#include "object_cut.h"

namespace imsegm {

// ---------------------------------------------------------------------------------------------------
// arcs of the 4-connected grid.  The host loop of imsegm_cut_general_graph gives every site its arcs in the order of the edges it
// is part of; with pyGCO's edge order (vertical edges row-major, then the horizontal ones) that is: up, down, left, right.
// ---------------------------------------------------------------------------------------------------
// arcs of all sites in front of (r, c) in row-major order; (H, 0) gives their total
__device__ __forceinline__ int grid_arc_start(int r, int c, int H, int W)
{
    const int vertical = W * (max(r - 1, 0) + min(r, H - 1)) + c * ((r > 0) + (r < H - 1));
    const int horizontal = r * 2 * (W - 1) + max(c - 1, 0) + min(c, W - 1);
    return vertical + horizontal;
}

__global__ void k_grid_arcs(int H, int W, GridArcs g)
{
    const int K = H * W;
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s > K) return;
    if (s == K) {
        g.arc_start[K] = grid_arc_start(H, 0, H, W);
        return;
    }
    const int r = s / W, c = s - r * W;
    const int base = grid_arc_start(r, c, H, W);
    g.arc_start[s] = base;
    const int rows = (r > 0) + (r < H - 1);          // vertical arcs of every site of this row (the row below has its `up` first)
    if (r < H - 1) {                                  // vertical edge j = s: (r, c) - (r + 1, c)
        const int b = s + W, ia = base + (r > 0), ib = grid_arc_start(r + 1, c, H, W);
        g.edges[2 * (size_t)s] = s;
        g.edges[2 * (size_t)s + 1] = b;
        g.arc_to[ia] = b;
        g.arc_to[ib] = s;
        g.arc_rev[ia] = ib;
        g.arc_rev[ib] = ia;
        g.edge_arc[2 * (size_t)s] = ia;
        g.edge_arc[2 * (size_t)s + 1] = ib;
    }
    if (c < W - 1) {                                  // horizontal edge j = (H - 1) W + r (W - 1) + c: (r, c) - (r, c + 1)
        const size_t j = (size_t)(H - 1) * W + (size_t)r * (W - 1) + c;
        const int b = s + 1, ia = base + rows + (c > 0), ib = grid_arc_start(r, c + 1, H, W) + rows;
        g.edges[2 * j] = s;
        g.edges[2 * j + 1] = b;
        g.arc_to[ia] = b;
        g.arc_to[ib] = s;
        g.arc_rev[ia] = ib;
        g.arc_rev[ib] = ia;
        g.edge_arc[2 * j] = ia;
        g.edge_arc[2 * j + 1] = ib;
    }
}

int launch_grid_arcs(int H, int W, GridArcs g, hipStream_t st)
{
    const long K = (long)H * W;
    hipLaunchKernelGGL(k_grid_arcs, cdiv(K + 1, 256), 256, 0, st, H, W, g);
    HIP_TRY(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------------------------------------------
// pyGCO's conversion: a maximum (exact in any order), then the truncation
// ---------------------------------------------------------------------------------------------------
// the maximum of a workgroup of 256 into one word: shuffles inside a wave, four values through the LDS, one atomic
__device__ __forceinline__ void block_max_to(double m, unsigned long long *word)
{
    __shared__ double waves[4];
    m = wave_max_f64(m);
    if ((threadIdx.x & 63) == 0) waves[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        m = fmax(fmax(waves[0], waves[1]), fmax(waves[2], waves[3]));
        if (m > 0) atomicMax(word, (unsigned long long)__double_as_longlong(m));
    }
}

__global__ void __launch_bounds__(256) k_max_abs(const double *x, size_t n, unsigned long long *word)
{
    double m = 0;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const double v = fabs(x[i]);
        if (v > m) m = v;
    }
    block_max_to(m, word);
}

int launch_max_abs(const double *x, size_t n, unsigned long long *red, int slot, hipStream_t st)
{
    if (n == 0) return 0;
    const int blocks = (int)std::min<size_t>((n + 2047) / 2048, 2048);
    hipLaunchKernelGGL(k_max_abs, blocks, 256, 0, st, x, n, red + slot);
    HIP_TRY(hipGetLastError());
    return 0;
}

__device__ __forceinline__ double gc_down_weight_factor(const unsigned long long *red, double pairwise_max, int have_edges)
{
    const double mu = __longlong_as_double((long long)red[GC_RED_MU]), mw = __longlong_as_double((long long)red[GC_RED_MW]);
    return ((have_edges && mw * pairwise_max > mu) ? mw * pairwise_max : mu) + 1e-10;
}

__global__ void __launch_bounds__(256) k_gc_convert(const double *unary, size_t n_unary, const double *w, int E, int have_edges,
                                                    double pairwise_max, unsigned long long *red, int32_t *unary_i, int32_t *w_i)
{
    const double dwf = gc_down_weight_factor(red, pairwise_max, have_edges);
    const size_t n = n_unary + (size_t)E;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        if (i < n_unary) {
            unary_i[i] = (int32_t)((unary[i] / dwf) * 100000);
        } else {
            const size_t j = i - n_unary;
            w_i[j] = (int32_t)(((w ? w[j] : 1.0) / dwf) * 1000);
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        // (the conversion is monotone in |w|: the largest |integer weight| is the one of the largest |w|)
        const double mw = __longlong_as_double((long long)red[GC_RED_MW]);
        red[GC_RED_DWF] = (unsigned long long)__double_as_longlong(dwf);
        red[GC_RED_WMAX] = (unsigned long long)(long long)(int32_t)((mw / dwf) * 1000);
    }
}

int launch_gc_convert(const double *unary, size_t n_unary, const double *w, int E, bool have_edges, double pairwise_max,
                      unsigned long long *red, int32_t *unary_i, int32_t *w_i, hipStream_t st)
{
    if (!unary) n_unary = 0;
    const size_t n = n_unary + (size_t)E;
    const int blocks = (int)std::min<size_t>(std::max<size_t>((n + 1023) / 1024, 1), 4096);
    hipLaunchKernelGGL(k_gc_convert, blocks, 256, 0, st, unary, n_unary, w, E, have_edges ? 1 : 0, pairwise_max, red, unary_i, w_i);
    HIP_TRY(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------------------------------------------
// object unary costs.  A workgroup takes OBJ_TILE pixels: their classes and the tables in LDS, then the OBJ_TILE * (C + 1) costs
// of the tile thread after thread, so that a wave writes consecutive words.
// ---------------------------------------------------------------------------------------------------
constexpr int OBJ_TILE = 1024;

struct ObjectTables {
    const double *a_bg, *a_fg, *s_bg, *b;
    const int32_t *centres;
};

__device__ __forceinline__ ObjectTables object_tables_to_lds(const ObjectUnary &o, unsigned char *lds)
{
    double *t = reinterpret_cast<double *>(lds);
    const int L = o.n_labels;
    for (int i = threadIdx.x; i < L; i += blockDim.x) {
        t[i] = o.a_bg[i];
        t[L + i] = o.a_fg[i];
        t[2 * L + i] = o.s_bg[i];
    }
    for (int i = threadIdx.x; i < o.n_dist; i += blockDim.x) t[3 * L + i] = o.b[i];
    int32_t *cen = reinterpret_cast<int32_t *>(t + 3 * L + o.n_dist);
    for (int i = threadIdx.x; i < 4 * o.n_centres; i += blockDim.x) cen[i] = o.centres[i];
    return { t, t + L, t + 2 * L, t + 3 * L, cen };
}

// floor(sqrt(v)) of an integer: what numpy's sqrt(...).astype(int) gives for it
__device__ __forceinline__ int isqrt_i64(long long v)
{
    long long d = (long long)sqrt((double)v);
    while (d * d > v) --d;
    while ((d + 1) * (d + 1) <= v) ++d;
    return (int)d;
}

__device__ __forceinline__ double object_unary(const ObjectUnary &o, const ObjectTables &t, int raw, int r, int c, int column)
{
    int l = raw < 0 ? raw + o.n_labels : raw;
    l = min(max(l, 0), o.n_labels - 1);               // (the host has refused classes outside the tables)
    const bool shape = o.coef_shape > 0;
    if (column == 0) {
        const double u = t.a_bg[l];
        return shape ? u - o.coef_shape * t.s_bg[l] : u;
    }
    const int32_t *cen = t.centres + 4 * (column - 1);
    const int sr = r - cen[2], sc = c - cen[3];
    if (o.seed_size > 0) {
        if (abs(sr) <= o.seed_size && abs(sc) <= o.seed_size && sr * sr + sc * sc <= o.seed_size * o.seed_size && raw > 0) return 0.0;
    } else if (sr == 0 && sc == 0) {
        return 0.0;
    }
    const double u = t.a_fg[l];
    if (!shape) return u;
    const long long dr = r - cen[0], dc = c - cen[1];
    const int d = min(isqrt_i64(dr * dr + dc * dc), o.n_dist - 1);
    return u - o.coef_shape * t.b[d];
}

template <bool WRITE>
__global__ void __launch_bounds__(256) k_object_unary(ObjectUnary o, unsigned long long *red, int32_t *unary_i)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    __shared__ int32_t s_segm[OBJ_TILE];
    const ObjectTables t = object_tables_to_lds(o, lds);
    const size_t K = (size_t)o.H * o.W, first = (size_t)blockIdx.x * OBJ_TILE;
    const int pixels = K - first < (size_t)OBJ_TILE ? (int)(K - first) : OBJ_TILE, C = o.n_centres + 1;
    for (int i = threadIdx.x; i < pixels; i += 256) s_segm[i] = o.segm[first + i];
    __syncthreads();
    const double dwf = WRITE ? __longlong_as_double((long long)red[GC_RED_DWF]) : 1.0;
    const int row0 = (int)(first / o.W), col0 = (int)(first - (size_t)row0 * o.W);       // the tile's first pixel: one wide division
    double m = 0;
    for (int j = threadIdx.x; j < pixels * C; j += 256) {
        const int p = j / C, column = j - p * C;
        const int q = col0 + p, r = row0 + q / o.W, c = q % o.W;
        const double u = object_unary(o, t, s_segm[p], r, c, column);
        if (WRITE) {
            unary_i[first * C + j] = (int32_t)((u / dwf) * 100000);
        } else {
            const double v = fabs(u);
            if (v > m) m = v;
        }
    }
    if (!WRITE) block_max_to(m, red + GC_RED_MU);
}

static int object_unary_launch(const ObjectUnary &o, unsigned long long *red, int32_t *unary_i, hipStream_t st)
{
    const size_t dyn = object_unary_lds_bytes(o.n_labels, o.n_dist, o.n_centres);
    if (dyn > OBJECT_UNARY_LDS_MAX) {
        set_error("object_cut_pixels: the tables do not fit the LDS");
        return -1;
    }
    const size_t K = (size_t)o.H * o.W;
    const int blocks = (int)((K + OBJ_TILE - 1) / OBJ_TILE);
    if (unary_i)
        hipLaunchKernelGGL(k_object_unary<true>, blocks, 256, dyn, st, o, red, unary_i);
    else
        hipLaunchKernelGGL(k_object_unary<false>, blocks, 256, dyn, st, o, red, unary_i);
    HIP_TRY(hipGetLastError());
    return 0;
}

int launch_object_unary_max(const ObjectUnary &o, unsigned long long *red, hipStream_t st) { return object_unary_launch(o, red, nullptr, st); }

int launch_object_unary_int(const ObjectUnary &o, const unsigned long long *red, int32_t *unary_i, hipStream_t st)
{
    return object_unary_launch(o, const_cast<unsigned long long *>(red), unary_i, st);
}

}  // namespace imsegm
