// center_annotation.hip -- centre-level annotations from maps of annotated eggs on the device: the reference's
// experiments_ovary_centres/run_create_annotation.py (load_correct_segm :68-83, segm_set_center_levels :100-132,
// compute_eggs_center :52-65) for all objects of a map at once.
//
//   correction   threshold; the opening is morphology.hip's; ONE 4-connected labelling of the mask with the pixel count of every
//                root and a removal pass; ONE 8-connected labelling of what stays.  Both are the forest of unionfind.h (smallest index
//                = root), so a component's root is its first pixel in raster order and its number is the rank of that root: a count
//                per 2048-pixel chunk, the exclusive scan of scan.hip, block_stable_slot inside the chunk.
//   distances    the squared distance of every pixel to the nearest pixel of ANOTHER label, one transform for the whole map: the
//                column pass gives g = the distance along the column to the nearest pixel whose label differs (NONE when the run of
//                equal labels reaches both ends of the column); the row pass of a pixel of label A minimises k^2 + f(x +- k)^2 with
//                f = g inside A and 0 outside it -- it never passes the first foreign pixel on a side, since k^2 alone ends the
//                search there.  The image border is no background.  uint32 throughout, as boundary.hip.
//   reductions   max d2, pixel count, row and column sums per label: a lane that opens a run of equal labels adds the run's exact
//                sums once (cut_objects.hip's rule), the maximum comes from a segmented shuffle reduction over the run.
//   code         sqrt(d2) / sqrt(max2) > level in fp64 -- the two roots and the quotient numpy takes, nothing reformulated -- as one
//                bit per level in a byte per pixel, and the count of every (label, level): one ballot per level, one atomic per run.
//   discs        bit i >= 1 cleared outside scikit-image's disc of (label, i) (ellipse_place.h's inside test on draw.disk's offsets).
// The opening of every level is morphology.hip's label-aware erosion and dilation.  fp64 only where numpy has it; the library is
// built with -ffp-contract=off.
#include "center_annotation.h"
#include "ellipse_place.h"
#include "scan.h"
#include "slic.h"
#include "unionfind.h"

namespace imsegm {

namespace {

constexpr uint32_t CA_NONE = 0xffffffffu;
constexpr int CA_CHUNK = 2048;                       // the chunk of launch_compact_count (slic.h)

__device__ __forceinline__ bool ca_set(uint8_t v) { return v != 0; }

template <typename T> __global__ void __launch_bounds__(256) k_ca_threshold(const T *__restrict__ img, size_t n, uint8_t *__restrict__ out)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = img[i] > 0;
}

// ---- labelling: workgroup (c, y) covers pixels 256 c .. 256 c + 255 of row y (the run rule of unionfind.h) -------------------
__global__ void __launch_bounds__(256) k_ca_cc_init(const uint8_t *__restrict__ mask, int32_t *__restrict__ parent, int W)
{
    run_label_init(mask, parent, blockIdx.y, blockIdx.x * 256 + threadIdx.x, W, ca_set);
}

// EIGHT: the two diagonal neighbours of the row above as well; a diagonal needs a union only where the pixel above is not set
// (otherwise it ties the two already)
template <bool EIGHT> __global__ void __launch_bounds__(256) k_ca_cc_merge(const uint8_t *__restrict__ mask, int32_t *parent, int W)
{
    const int y = blockIdx.y, x = blockIdx.x * 256 + threadIdx.x;
    run_label_merge(mask, parent, y, x, W, ca_set);
    if (!EIGHT || x >= W || y == 0) return;
    const size_t p = (size_t)y * W + x;
    if (!mask[p] || mask[p - W]) return;
    if (x > 0 && mask[p - W - 1]) uf_union_pair(parent, (int)p, (int)(p - W - 1));
    if (x + 1 < W && mask[p - W + 1]) uf_union_pair(parent, (int)p, (int)(p - W + 1));
}

// the pixel count of every root: the lane that opens a run of set pixels adds the run's length once
__global__ void __launch_bounds__(256) k_ca_sizes(const uint8_t *__restrict__ mask, const int32_t *__restrict__ parent, int W,
                                                  int32_t *__restrict__ size)
{
    const int y = blockIdx.y, x = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63;
    const bool sel = x < W && mask[(size_t)y * W + x];
    const unsigned long long z = __ballot(sel);
    if (!sel || (lane > 0 && ((z >> (lane - 1)) & 1ull))) return;
    const unsigned long long gaps = ~(z >> lane);      // (the bits shifted in are gaps: a run ends at lane 63 at the latest)
    const int length = gaps ? __ffsll((long long)gaps) - 1 : 64;
    atomicAdd(&size[uf_find(parent, (int)((size_t)y * W + x))], length);
}

__global__ void __launch_bounds__(256) k_ca_keep(const uint8_t *__restrict__ mask, const int32_t *__restrict__ parent,
                                                 const int32_t *__restrict__ size, size_t n, int min_size, uint8_t *__restrict__ kept)
{
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (p < n) kept[p] = mask[p] && size[uf_find(parent, (int)p)] >= min_size;
}

__global__ void __launch_bounds__(256) k_ca_roots(const uint8_t *__restrict__ kept, const int32_t *__restrict__ parent, size_t n,
                                                  uint8_t *__restrict__ roots)
{
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (p < n) roots[p] = kept[p] && parent[p] == (int32_t)p;
}

// number[root] = 1 + the number of roots in front of it (offsets: the exclusive chunk offsets of launch_compact_count)
__global__ void __launch_bounds__(256) k_ca_number(const uint8_t *__restrict__ roots, size_t n, const uint32_t *__restrict__ offsets,
                                                   int32_t *__restrict__ number)
{
    const size_t start = (size_t)blockIdx.x * CA_CHUNK;
    uint32_t base = offsets[blockIdx.x];
    for (int it = 0; it < CA_CHUNK / 256; ++it) {
        const size_t i = start + (size_t)it * 256 + threadIdx.x;
        const bool set = i < n && roots[i];
        const uint32_t at = block_stable_slot(set, &base);
        if (set) number[i] = (int32_t)at + 1;
    }
}

__global__ void __launch_bounds__(256) k_ca_write_labels(const uint8_t *__restrict__ kept, const int32_t *__restrict__ parent,
                                                         const int32_t *__restrict__ number, size_t n, int32_t *__restrict__ labels)
{
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (p < n) labels[p] = kept[p] ? number[uf_find(parent, (int)p)] : 0;
}

// ---- distances -------------------------------------------------------------------------------------------------------------------
// column pass: threads along x, down and up again; *foreign is raised when the map holds two values
__global__ void __launch_bounds__(64) k_ca_columns(const int32_t *__restrict__ labels, int H, int W, uint32_t *__restrict__ g,
                                                   int *__restrict__ foreign)
{
    const int x = blockIdx.x * 64 + threadIdx.x;
    const bool valid = x < W;
    bool differs = false;
    if (valid) {
        const int32_t first = labels[0];
        const int32_t *l = labels + x;
        uint32_t *gx = g + x;
        uint32_t d = CA_NONE;
        int32_t prev = l[0];
#pragma unroll 4
        for (int y = 0; y < H; ++y) {
            const int32_t v = l[(size_t)y * W];
            d = v != prev ? 1u : (d == CA_NONE ? CA_NONE : d + 1u);
            differs |= v != first;
            gx[(size_t)y * W] = d;
            prev = v;
        }
        d = CA_NONE;
#pragma unroll 4
        for (int y = H - 1; y >= 0; --y) {
            const int32_t v = l[(size_t)y * W];
            d = v != prev ? 1u : (d == CA_NONE ? CA_NONE : d + 1u);
            if (d < gx[(size_t)y * W]) gx[(size_t)y * W] = d;
            prev = v;
        }
    }
    if (__ballot(differs) != 0 && threadIdx.x == 0) atomicOr(foreign, 1);
}

// row pass: boundary.hip's outward search in staged windows (k_edt_rows), the windows holding the labels beside g
constexpr int CA_B = 256, CA_T = 256;

__global__ void __launch_bounds__(CA_B) k_ca_rows(const int32_t *__restrict__ labels, const uint32_t *__restrict__ g, int H, int W,
                                                  int max_label, const int *__restrict__ foreign, uint32_t *__restrict__ d2_out)
{
    __shared__ uint32_t s_gl[CA_T + CA_B], s_gr[CA_T + CA_B];
    __shared__ int32_t s_ll[CA_T + CA_B], s_lr[CA_T + CA_B];
    const int t = threadIdx.x, x0 = blockIdx.x * CA_B, x = x0 + t, y = blockIdx.y;
    const uint32_t *grow = g + (size_t)y * W;
    const int32_t *lrow = labels + (size_t)y * W;
    const bool inside = x < W;
    const int32_t own = inside ? lrow[x] : 0;
    uint32_t best = 0;
    bool done = true;
    if (inside && own >= 1 && own <= max_label) {
        if (*foreign == 0) {                           // (uniform over the grid)
            best = (uint32_t)(y + 1) * (uint32_t)(y + 1) + (uint32_t)x * (uint32_t)x;
        } else {
            const uint32_t g0 = grow[x];
            best = g0 != CA_NONE ? g0 * g0 : CA_NONE;
            done = false;
        }
    }
    for (int r = 0;; ++r) {
        const int base = r * CA_T;                     // this round: k = base + 1 .. base + T
        const int left0 = x0 - base - CA_T, right0 = x0 + base;
        const bool windows_in_row = left0 + CA_T + CA_B - 1 > 0 || right0 + 1 < W;
        if (!windows_in_row || !__syncthreads_or(!done)) break;
        for (int i = t; i < CA_T + CA_B; i += CA_B) {
            const int xl = left0 + i, xr = right0 + i;
            const bool inl = xl >= 0 && xl < W, inr = xr >= 0 && xr < W;
            s_gl[i] = inl ? grow[xl] : CA_NONE;
            s_ll[i] = inl ? lrow[xl] : 0;
            s_gr[i] = inr ? grow[xr] : CA_NONE;
            s_lr[i] = inr ? lrow[xr] : 0;
        }
        __syncthreads();
        if (!done) {
            for (int kk = 1; kk <= CA_T; ++kk) {
                const int k = base + kk;
                const uint32_t k2 = (uint32_t)k * (uint32_t)k;
                const bool in_left = x - k >= 0, in_right = x + k < W;
                if (k2 >= best || (!in_left && !in_right)) {
                    done = true;
                    break;
                }
                if (in_left) {
                    const uint32_t gl = s_gl[t + CA_T - kk];
                    if (s_ll[t + CA_T - kk] != own)
                        best = k2;                     // (k2 < best here)
                    else if (gl != CA_NONE)
                        best = min(best, k2 + gl * gl);
                }
                if (in_right) {
                    const uint32_t gr = s_gr[t + kk];
                    if (s_lr[t + kk] != own)
                        best = min(best, k2);
                    else if (gr != CA_NONE)
                        best = min(best, k2 + gr * gr);
                }
            }
        }
        __syncthreads();                               // the next round overwrites the windows
    }
    if (inside) d2_out[(size_t)y * W + x] = best;
}

// ---- runs of equal labels inside a wave ---------------------------------------------------------------------------------------
// head: the lane opens a run; end: the lane behind the last one of the run of this lane (every lane of the wave calls)
__device__ __forceinline__ void ca_runs(int32_t v, bool valid, bool &head, int &end)
{
    const int lane = threadIdx.x & 63;
    const int32_t left = __shfl_up(v, 1, 64);
    head = valid && (lane == 0 || left != v);
    const unsigned long long stops = __ballot(head) | ~__ballot(valid);
    const unsigned long long after = lane == 63 ? 0ull : stops & ~((2ull << lane) - 1ull);
    end = after ? __ffsll((long long)after) - 1 : 64;
}

__global__ void __launch_bounds__(256) k_ca_reduce(const int32_t *__restrict__ labels, const uint32_t *__restrict__ d2, int W, int chunks,
                                                   int max_label, uint32_t *__restrict__ max2, unsigned long long *__restrict__ sums)
{
    const int y = blockIdx.x / chunks, x = (blockIdx.x % chunks) * 256 + threadIdx.x, lane = threadIdx.x & 63;
    const bool valid = x < W;                          // (the valid lanes of a wave are its first ones)
    const int32_t v = valid ? labels[(size_t)y * W + x] : 0;
    bool head;
    int end;
    ca_runs(v, valid, head, end);
    uint32_t m = valid && d2 ? d2[(size_t)y * W + x] : 0u;
    if (d2) {
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t other = __shfl_down(m, off, 64);
            if (lane + off < end) m = max(m, other);
        }
    }
    if (!head || v < 1 || v > max_label) return;
    const long long L = end - lane;
    if (d2) atomicMax(max2 + v, m);
    atomicAdd(sums + 3 * (size_t)v, (unsigned long long)L);
    atomicAdd(sums + 3 * (size_t)v + 1, (unsigned long long)((long long)y * L));
    atomicAdd(sums + 3 * (size_t)v + 2, (unsigned long long)(L * x + L * (L - 1) / 2));
}

__global__ void __launch_bounds__(256) k_ca_code(const int32_t *__restrict__ labels, const uint32_t *__restrict__ d2, int W, int chunks,
                                                 int max_label, const uint32_t *__restrict__ max2, const double *__restrict__ levels,
                                                 int n_levels, uint8_t *__restrict__ code, uint32_t *__restrict__ counts)
{
    const int y = blockIdx.x / chunks, x = (blockIdx.x % chunks) * 256 + threadIdx.x, lane = threadIdx.x & 63;
    const bool valid = x < W;
    const size_t p = (size_t)y * W + x;
    const int32_t v = valid ? labels[p] : 0;
    const bool own = valid && v >= 1 && v <= max_label;
    bool head;
    int end;
    ca_runs(v, valid, head, end);
    unsigned bits = 0;
    if (own) {
        const double probab = sqrt((double)d2[p]) / sqrt((double)max2[v]);
        for (int i = 0; i < n_levels; ++i)
            if (probab > levels[i]) bits |= 1u << i;
    }
    if (valid) code[p] = (uint8_t)bits;
    const unsigned long long mine = (end == 64 ? ~0ull : (1ull << end) - 1ull) & ~((1ull << lane) - 1ull);
    for (int i = 0; i < n_levels; ++i) {
        const unsigned long long votes = __ballot((bits >> i) & 1u);
        const int c = __popcll(votes & mine);
        if (head && own && c) atomicAdd(counts + (size_t)v * CA_MAX_LEVELS + i, (uint32_t)c);
    }
}

__global__ void __launch_bounds__(256) k_ca_discs(const int32_t *__restrict__ labels, int W, size_t n, int max_label,
                                                  const CaDisc *__restrict__ discs, int n_levels, uint8_t *__restrict__ code,
                                                  uint8_t *__restrict__ out)
{
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    unsigned bits = code[p];
    if (bits > 1u) {                                   // (a bit is only ever set for a label with a slot)
        const int32_t v = labels[p];
        const int row = (int)(p / (size_t)W), col = (int)(p % (size_t)W);
        for (int i = 1; i < n_levels; ++i) {
            if (!((bits >> i) & 1u)) continue;
            const CaDisc d = discs[(size_t)v * CA_MAX_LEVELS + i];
            const bool in = row >= d.r0 && row <= d.r1 && col >= d.c0 && col <= d.c1 &&
                            ellipse_inside_offsets((double)(row - d.r0) - d.r_org, (double)(col - d.c0) - d.c_org, 0.0, 1.0, d.radius, d.radius);
            if (!in) bits &= ~(1u << i);
        }
        code[p] = (uint8_t)bits;
    }
    out[p] = (uint8_t)(bits & 1u);
}

int ca_row_grid(int H, int W, int &chunks)
{
    chunks = cdiv(W, 256);
    if (H > 65535 || (size_t)chunks * (size_t)H > 0x7fffffffull) {
        set_error("center annotation: the map is too large for one launch");
        return -1;
    }
    return 0;
}

}  // namespace

int launch_ca_threshold(const void *img, int is_i32, size_t n, uint8_t *out, hipStream_t st)
{
    const unsigned blocks = (unsigned)((n + 255) / 256);
    if (is_i32)
        hipLaunchKernelGGL(k_ca_threshold<int32_t>, blocks, 256, 0, st, static_cast<const int32_t *>(img), n, out);
    else
        hipLaunchKernelGGL(k_ca_threshold<uint8_t>, blocks, 256, 0, st, static_cast<const uint8_t *>(img), n, out);
    HIP_TRY(hipGetLastError());
    return 0;
}

int launch_ca_label(const uint8_t *mask, int H, int W, int min_size, int32_t *parent, int32_t *size, uint8_t *roots, uint32_t *counts,
                    uint8_t *kept, int32_t *labels, hipStream_t st)
{
    int chunks;
    if (ca_row_grid(H, W, chunks)) return -1;
    const size_t n = (size_t)H * W;
    if (compact_count_words(n) != (n + CA_CHUNK - 1) / CA_CHUNK + 1) {
        set_error("center annotation: internal error, the chunk of the compaction has changed");
        return -1;
    }
    const dim3 rows(chunks, H);
    const unsigned flat = (unsigned)((n + 255) / 256);
    HIP_TRY(hipMemsetAsync(size, 0, n * 4, st));
    hipLaunchKernelGGL(k_ca_cc_init, rows, 256, 0, st, mask, parent, W);
    hipLaunchKernelGGL(k_ca_cc_merge<false>, rows, 256, 0, st, mask, parent, W);
    hipLaunchKernelGGL(k_ca_sizes, rows, 256, 0, st, mask, parent, W, size);
    hipLaunchKernelGGL(k_ca_keep, flat, 256, 0, st, mask, parent, size, n, min_size, kept);
    hipLaunchKernelGGL(k_ca_cc_init, rows, 256, 0, st, kept, parent, W);
    hipLaunchKernelGGL(k_ca_cc_merge<true>, rows, 256, 0, st, kept, parent, W);
    hipLaunchKernelGGL(k_ca_roots, flat, 256, 0, st, kept, parent, n, roots);
    if (launch_compact_count(roots, n, counts, st)) return -1;
    hipLaunchKernelGGL(k_ca_number, (unsigned)(compact_count_words(n) - 1), 256, 0, st, roots, n, counts, size);
    hipLaunchKernelGGL(k_ca_write_labels, flat, 256, 0, st, kept, parent, size, n, labels);
    HIP_TRY(hipGetLastError());
    return 0;
}

int launch_ca_distances(const int32_t *labels, int H, int W, int max_label, uint32_t *g, int *foreign, uint32_t *d2, hipStream_t st)
{
    if (!edt_size_ok(H, W)) return -1;
    if (H > 65535) {                                   // (gridDim.y of the row pass)
        set_error("center annotation: more than 65535 rows");
        return -1;
    }
    HIP_TRY(hipMemsetAsync(foreign, 0, sizeof(int), st));
    hipLaunchKernelGGL(k_ca_columns, cdiv(W, 64), 64, 0, st, labels, H, W, g, foreign);
    hipLaunchKernelGGL(k_ca_rows, dim3(cdiv(W, CA_B), H), CA_B, 0, st, labels, g, H, W, max_label, foreign, d2);
    HIP_TRY(hipGetLastError());
    return 0;
}

int launch_ca_reduce(const int32_t *labels, const uint32_t *d2, int H, int W, int max_label, uint32_t *max2,
                     unsigned long long *sums, hipStream_t st)
{
    int chunks;
    if (ca_row_grid(H, W, chunks)) return -1;
    hipLaunchKernelGGL(k_ca_reduce, chunks * H, 256, 0, st, labels, d2, W, chunks, max_label, max2, sums);
    HIP_TRY(hipGetLastError());
    return 0;
}

int launch_ca_code(const int32_t *labels, const uint32_t *d2, int H, int W, int max_label, const uint32_t *max2, const double *levels,
                   int n_levels, uint8_t *code, uint32_t *counts, hipStream_t st)
{
    int chunks;
    if (ca_row_grid(H, W, chunks)) return -1;
    hipLaunchKernelGGL(k_ca_code, chunks * H, 256, 0, st, labels, d2, W, chunks, max_label, max2, levels, n_levels, code, counts);
    HIP_TRY(hipGetLastError());
    return 0;
}

int launch_ca_discs(const int32_t *labels, int H, int W, int max_label, const CaDisc *discs, int n_levels, uint8_t *code, uint8_t *out,
                    hipStream_t st)
{
    const size_t n = (size_t)H * W;
    hipLaunchKernelGGL(k_ca_discs, (unsigned)((n + 255) / 256), 256, 0, st, labels, W, n, max_label, discs, n_levels, code, out);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // namespace imsegm
