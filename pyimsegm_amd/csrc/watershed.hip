// watershed.hip -- the marker flood of segment_watershed (experiments_ovary_detect/run_ovary_egg-segmentation.py:259 of the
// reference: morphology.watershed(-distance, markers, mask=seg_binary)) and the stages of its clean-up (:265-274) that
// work on one plane per label, all labels in one launch.  Integers only.
//
// The flood (DESIGN.md section 4 "Watershed"; pyimsegm_amd/egg_segmentation.py watershed_markers_host is the definition) runs in
// rounds: the frontier pixels with the smallest key spread at once, an unlabelled 4-neighbour takes the smallest label among its
// spreading neighbours and joins the frontier.  Floods never cross components of the mask, so ONE workgroup owns a component and
// no launch-wide synchronisation exists.  Its frontier is a compacted list in global scratch (two halves of count words each, count =
// the pixels of the component: a pixel enters the frontier once).  A round is
//   (A) the workgroup minimum of the frontier keys: 64-lane wave reductions, one LDS step across the waves;
//   (B) every list entry either moves to the other half (key above the minimum) or spreads: atomicMin(state[q], WS_CLAIM + label)
//       on its four neighbours -- a settled label and the 0 outside the mask are smaller and stay, an unlabelled pixel holds WS_FREE
//       and the lane that finds WS_FREE appends it to the other half.  All claimants of a round have stored before (C) runs, so
//       the smallest label wins whatever the order;
//   (C) the claims of the round lose their WS_CLAIM bit.
// The state words of a component are touched by its workgroup only, always by atomics (they go to L2: no stale copy in the vector
// L1).  Every loop is bounded by the pixel count of the component and every append by the size of its half: a defect ends in a
// wrong map, never in a hang or a store outside the arena.
#include "morphology.h"
#include "scan.h"
#include "slic.h"
#include "unionfind.h"
#include "watershed.h"

namespace imsegm {

namespace {

__global__ void __launch_bounds__(256) k_ws_mask(const uint8_t *__restrict__ background, size_t n, uint8_t *__restrict__ mask,
                                                 int *__restrict__ any_background)
{
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    const bool bg = p < n && background[p] != 0;
    if (p < n) mask[p] = !bg;
    if (__ballot(bg) != 0 && (threadIdx.x & 63) == 0) atomicOr(any_background, 1);
}

__global__ void __launch_bounds__(256) k_ws_negate(uint32_t *__restrict__ d2, size_t n)
{
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (p < n) reinterpret_cast<int32_t *>(d2)[p] = -(int32_t)d2[p];
}

// state[p] = WS_FREE inside the mask, 0 outside; count[c] = the pixels of component c (one atomic per wave where its lanes agree)
__global__ void __launch_bounds__(256) k_ws_count(const int32_t *__restrict__ comp, size_t n, int32_t *__restrict__ state,
                                                  uint32_t *__restrict__ count)
{
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    int c = p < n ? comp[p] : 0;
    if (c < 0 || (size_t)c > n) c = 0;
    if (p < n) state[p] = c ? WS_FREE : 0;
    const int c0 = __builtin_amdgcn_readfirstlane(c);
    const unsigned long long same = __ballot(c == c0);
    if (c == c0) {
        if (c && (threadIdx.x & 63) == __ffsll((long long)same) - 1) atomicAdd(&count[c], (uint32_t)__popcll(same));
    } else if (c) {
        atomicAdd(&count[c], 1u);
    }
}

// the two halves of component c in the arena; fill[c] = 0
__global__ void __launch_bounds__(256) k_ws_alloc(const uint32_t *__restrict__ n_comp, const uint32_t *__restrict__ count, size_t n,
                                                  uint32_t *__restrict__ base, uint32_t *__restrict__ fill, uint32_t *__restrict__ top)
{
    const size_t c = (size_t)blockIdx.x * 256 + threadIdx.x + 1;
    if (c > n || c > *n_comp) return;
    base[c] = atomicAdd(top, 2u * count[c]);
    fill[c] = 0;
}

__global__ void __launch_bounds__(256) k_ws_seed(const int32_t *__restrict__ comp, size_t n, const int32_t *__restrict__ seed_pixels,
                                                 const int32_t *__restrict__ seed_labels, int n_seeds, const uint32_t *__restrict__ n_comp,
                                                 const uint32_t *__restrict__ count, const uint32_t *__restrict__ base,
                                                 uint32_t *__restrict__ fill, uint32_t *__restrict__ arena, int32_t *__restrict__ state)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_seeds) return;
    const int p = seed_pixels[i], label = seed_labels[i];
    if (p < 0 || (size_t)p >= n || label < 1 || label > WS_MAX_LABELS) return;
    const int c = comp[p];
    if (c < 1 || (uint32_t)c > *n_comp || (size_t)c > n) return;
    const uint32_t slot = atomicAdd(&fill[c], 1u);
    if (slot >= count[c] || (size_t)base[c] + 2 * (size_t)count[c] > 2 * n) return;
    arena[base[c] + slot] = (uint32_t)p;
    state[p] = label;
}

__device__ __forceinline__ int wave_min_i32(int v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = min(v, __shfl_xor(v, off, 64));
    return v;
}

__device__ __forceinline__ int ws_load(const int32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__global__ void __launch_bounds__(WS_THREADS) k_ws_flood(const uint32_t *__restrict__ n_comp, const int32_t *__restrict__ keys, int H, int W,
                                                         const uint32_t *__restrict__ count, const uint32_t *__restrict__ base,
                                                         const uint32_t *__restrict__ fill, uint32_t *__restrict__ arena,
                                                         int32_t *__restrict__ state)
{
    __shared__ int s_min[WS_THREADS / 64];
    __shared__ uint32_t s_next;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t n = (size_t)H * W;
    const uint32_t comps = min(*n_comp, (uint32_t)min(n, (size_t)0x7fffffff));
    for (uint32_t c = blockIdx.x + 1; c <= comps; c += gridDim.x) {
        const uint32_t cnt = count[c];
        uint32_t m = min(fill[c], cnt);
        if (m == 0 || (size_t)base[c] + 2 * (size_t)cnt > 2 * n) continue;       // (uniform over the workgroup)
        uint32_t *cur = arena + base[c], *nxt = cur + cnt;
        for (uint32_t round = 0; round < cnt && m > 0; ++round) {
            // (A)
            int k = 0x7fffffff;
            for (uint32_t i = tid; i < m; i += WS_THREADS) {
                const uint32_t p = cur[i];
                if (p < n) k = min(k, keys[p]);
            }
            k = wave_min_i32(k);
            if (lane == 0) s_min[wave] = k;
            if (tid == 0) s_next = 0;
            __syncthreads();
            int kmin = s_min[0];
#pragma unroll
            for (int w = 1; w < WS_THREADS / 64; ++w) kmin = min(kmin, s_min[w]);
            // (B)
            for (uint32_t i = tid; i < m; i += WS_THREADS) {
                const uint32_t p = cur[i];
                if (p >= n) continue;
                if (keys[p] != kmin) {
                    const uint32_t slot = atomicAdd(&s_next, 1u);
                    if (slot < cnt) nxt[slot] = p;
                    continue;
                }
                const int label = ws_load(&state[p]);
                if (label < 1 || label >= WS_CLAIM) continue;
                const int y = (int)(p / (uint32_t)W), x = (int)(p - (uint32_t)y * (uint32_t)W);
                const uint32_t q4[4] = { p - (uint32_t)W, p + (uint32_t)W, p - 1u, p + 1u };
                const bool in4[4] = { y > 0, y < H - 1, x > 0, x < W - 1 };
#pragma unroll
                for (int d = 0; d < 4; ++d) {
                    if (!in4[d]) continue;
                    if (atomicMin(&state[q4[d]], WS_CLAIM + label) == WS_FREE) {
                        const uint32_t slot = atomicAdd(&s_next, 1u);
                        if (slot < cnt) nxt[slot] = q4[d];
                    }
                }
            }
            __syncthreads();
            const uint32_t m2 = min(s_next, cnt);
            // (C)
            for (uint32_t i = tid; i < m2; i += WS_THREADS) {
                const uint32_t q = nxt[i];
                if (q < n) atomicAnd(&state[q], WS_CLAIM - 1);
            }
            __syncthreads();
            uint32_t *const t = cur;
            cur = nxt;
            nxt = t;
            m = m2;
        }
        __syncthreads();
    }
}

__global__ void __launch_bounds__(256) k_ws_finish(const int32_t *state, size_t n, int32_t *out)
{
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    const int v = state[p];
    out[p] = v > 0 && v <= WS_MAX_LABELS ? v : 0;
}

// ---- the clean-up: glue around launch_disc_morph and launch_fill_holes_split on the box of one label ---------------------------

__global__ void __launch_bounds__(256) k_ws_boxes_init(int32_t *__restrict__ boxes, int max_label)
{
    const int l = blockIdx.x * 256 + threadIdx.x;
    if (l > max_label) return;
    boxes[4 * l] = boxes[4 * l + 1] = 0x7fffffff;
    boxes[4 * l + 2] = boxes[4 * l + 3] = -1;
}

// a workgroup covers 64 columns of 4 rows: one lane per run of equal labels along a row updates the box of the label
__global__ void __launch_bounds__(256) k_ws_boxes(const int32_t *__restrict__ segm, int H, int W, int max_label, int32_t *__restrict__ boxes,
                                                  int *__restrict__ beyond)
{
    const int lane = threadIdx.x & 63;
    const int x = blockIdx.x * 64 + lane, y = blockIdx.y * 4 + (threadIdx.x >> 6);
    const int l = x < W && y < H ? segm[(size_t)y * W + x] : 0;
    const int before = lane_prev(l, 0), after = lane_next(l, 0);
    if (__ballot(l > max_label) != 0 && lane == 0) atomicOr(beyond, 1);
    if (l < 1 || l > max_label) return;
    if (lane == 0 || before != l) {
        atomicMin(&boxes[4 * l], y);
        atomicMax(&boxes[4 * l + 2], y);
        atomicMin(&boxes[4 * l + 1], x);
    }
    if (lane == 63 || after != l) atomicMax(&boxes[4 * l + 3], x);
}

// the plane of every label: its box padded by `pad` and cut at the image, and its offset in the plane buffers (an exclusive sum of
// the areas by ONE workgroup, lane = label - 1).  Planes that do not fit `capacity` pixels: *overflow raised, no plane at all.
__global__ void __launch_bounds__(WS_MAX_LABELS) k_ws_box_plan(const int32_t *__restrict__ boxes, int H, int W, int max_label, int pad,
                                                               unsigned long long capacity, int32_t *__restrict__ table,
                                                               int *__restrict__ overflow)
{
    const int l = threadIdx.x + 1;
    int r0 = 0, c0 = 0, bh = 0, bw = 0;
    if (l <= max_label) {
        const int a = boxes[4 * l], b = boxes[4 * l + 1], c = boxes[4 * l + 2], d = boxes[4 * l + 3];
        if (a >= 0 && b >= 0 && a <= c && b <= d && c < H && d < W) {
            r0 = max(a - pad, 0), c0 = max(b - pad, 0);
            bh = min(c + pad, H - 1) - r0 + 1, bw = min(d + pad, W - 1) - c0 + 1;
        }
    }
    unsigned long long total = 0;
    const unsigned long long offset = block_exclusive_scan<WS_MAX_LABELS / 64, unsigned long long>((unsigned long long)bh * bw, &total);
    if (total > capacity) {
        bh = bw = 0;
        if (threadIdx.x == 0) *overflow = 1;
    }
    if (l <= max_label) {
        int32_t *row = table + (size_t)l * MORPH_BOX_WORDS;
        row[0] = r0, row[1] = c0, row[2] = bh, row[3] = bw, row[4] = total > capacity ? 0 : (int32_t)offset;
    }
}

// The stages below run for all labels in one launch: label = blockIdx.z + 1, a workgroup covers 256 pixels of row blockIdx.y of the
// label's plane (the grid covers the largest plane; a workgroup outside its plane leaves at once, all its lanes together).
struct WsPlane {
    int r0, c0, bh, bw, label;
    size_t offset;
    bool inside;
};
__device__ __forceinline__ WsPlane ws_plane(const int32_t *__restrict__ table)
{
    const int32_t *row = table + (size_t)(blockIdx.z + 1) * MORPH_BOX_WORDS;
    WsPlane p;
    p.r0 = row[0], p.c0 = row[1], p.bh = row[2], p.bw = row[3], p.offset = (size_t)row[4], p.label = blockIdx.z + 1;
    p.inside = (int)blockIdx.y < p.bh && (int)blockIdx.x * 256 < p.bw;
    return p;
}
__device__ __forceinline__ bool ws_clear(uint8_t v) { return v == 0; }

__global__ void __launch_bounds__(256) k_ws_extract(const int32_t *__restrict__ segm, int W, const int32_t *__restrict__ table,
                                                    uint8_t *__restrict__ planes)
{
    const WsPlane p = ws_plane(table);
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (p.inside && x < p.bw) planes[p.offset + (size_t)y * p.bw + x] = segm[(size_t)(p.r0 + y) * W + p.c0 + x] == p.label;
}

// hole filling inside the plane: the labelling of its clear pixels by the run rule of unionfind.h (indices inside the plane), a
// flag on the roots that a pixel of the plane's border reaches, and the fill of the clear pixels without one
__global__ void __launch_bounds__(256) k_ws_holes_init(const uint8_t *__restrict__ planes, const int32_t *__restrict__ table,
                                                       int32_t *__restrict__ parent, uint8_t *__restrict__ touches)
{
    const WsPlane p = ws_plane(table);
    if (!p.inside) return;
    const int x = blockIdx.x * 256 + threadIdx.x;
    run_label_init(planes + p.offset, parent + p.offset, blockIdx.y, x, p.bw, ws_clear);
    if (x < p.bw) touches[p.offset + (size_t)blockIdx.y * p.bw + x] = 0;
}

__global__ void __launch_bounds__(256) k_ws_holes_merge(const uint8_t *__restrict__ planes, const int32_t *__restrict__ table,
                                                        int32_t *parent)
{
    const WsPlane p = ws_plane(table);
    if (!p.inside) return;
    run_label_merge(planes + p.offset, parent + p.offset, blockIdx.y, blockIdx.x * 256 + threadIdx.x, p.bw, ws_clear);
}

// the border pixels of the plane, one lane each: top row, bottom row, left column, right column (blockIdx.y is not used)
__global__ void __launch_bounds__(256) k_ws_holes_touch(const uint8_t *__restrict__ planes, const int32_t *__restrict__ table,
                                                        const int32_t *__restrict__ parent, uint8_t *touches)
{
    const WsPlane p = ws_plane(table);
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (p.bh < 1 || p.bw < 1 || t >= 2 * p.bw + 2 * p.bh) return;
    int y, x;
    if (t < p.bw) {
        y = 0, x = t;
    } else if (t < 2 * p.bw) {
        y = p.bh - 1, x = t - p.bw;
    } else if (t < 2 * p.bw + p.bh) {
        y = t - 2 * p.bw, x = 0;
    } else {
        y = t - 2 * p.bw - p.bh, x = p.bw - 1;
    }
    const int i = y * p.bw + x;
    if (planes[p.offset + i] == 0) touches[p.offset + uf_find(parent + p.offset, i)] = 1;
}

__global__ void __launch_bounds__(256) k_ws_holes_fill(uint8_t *planes, const int32_t *__restrict__ table,
                                                       const int32_t *__restrict__ parent, const uint8_t *__restrict__ touches)
{
    const WsPlane p = ws_plane(table);
    const int x = blockIdx.x * 256 + threadIdx.x;
    if (!p.inside || x >= p.bw) return;
    const int i = blockIdx.y * p.bw + x;
    if (planes[p.offset + i] == 0 && !touches[p.offset + uf_find(parent + p.offset, i)]) planes[p.offset + i] = 1;
}

// clean[pixel] = the largest label whose plane is set there: what painting in ascending label order leaves (clean is zeroed before)
__global__ void __launch_bounds__(256) k_ws_paint(const uint8_t *__restrict__ planes, int W, const int32_t *__restrict__ table,
                                                  int32_t *__restrict__ clean)
{
    const WsPlane p = ws_plane(table);
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (p.inside && x < p.bw && planes[p.offset + (size_t)y * p.bw + x]) atomicMax(&clean[(size_t)(p.r0 + y) * W + p.c0 + x], p.label);
}

__global__ void __launch_bounds__(256) k_ws_widen(const uint8_t *__restrict__ plane, size_t n, int32_t *__restrict__ wide)
{
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (p < n) wide[p] = plane[p] != 0;
}

__global__ void __launch_bounds__(256) k_ws_invert(const uint8_t *__restrict__ background, size_t n, uint8_t *__restrict__ plane)
{
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (p < n) plane[p] = background[p] == 0;
}

inline unsigned flat_grid(size_t n) { return (unsigned)((n + 255) / 256); }

}  // namespace

int launch_ws_mask(const uint8_t *background, size_t n, uint8_t *mask, int *any_background, hipStream_t st)
{
    HIP_TRY(hipMemsetAsync(any_background, 0, sizeof(int), st));
    hipLaunchKernelGGL(k_ws_mask, flat_grid(n), 256, 0, st, background, n, mask, any_background);
    HIP_TRY(hipGetLastError());
    return 0;
}

int launch_ws_negate(uint32_t *d2, size_t n, hipStream_t st)
{
    hipLaunchKernelGGL(k_ws_negate, flat_grid(n), 256, 0, st, d2, n);
    HIP_TRY(hipGetLastError());
    return 0;
}

int launch_ws_flood(const int32_t *comp, const uint32_t *n_comp, const int32_t *keys, int H, int W, const int32_t *seed_pixels,
                    const int32_t *seed_labels, int n_seeds, int32_t *state, uint32_t *count, uint32_t *base, uint32_t *fill,
                    uint32_t *arena, uint32_t *top, int32_t *out, hipStream_t st)
{
    const size_t n = (size_t)H * W;
    HIP_TRY(hipMemsetAsync(count, 0, (n + 1) * 4, st));
    HIP_TRY(hipMemsetAsync(top, 0, 4, st));
    hipLaunchKernelGGL(k_ws_count, flat_grid(n), 256, 0, st, comp, n, state, count);
    hipLaunchKernelGGL(k_ws_alloc, flat_grid(n / 2 + 2), 256, 0, st, n_comp, count, n, base, fill, top);
    if (n_seeds > 0) {
        hipLaunchKernelGGL(k_ws_seed, flat_grid((size_t)n_seeds), 256, 0, st, comp, n, seed_pixels, seed_labels, n_seeds, n_comp, count, base,
                           fill, arena, state);
        hipLaunchKernelGGL(k_ws_flood, WS_BLOCKS, WS_THREADS, 0, st, n_comp, keys, H, W, count, base, fill, arena, state);
    }
    hipLaunchKernelGGL(k_ws_finish, flat_grid(n), 256, 0, st, state, n, out);
    HIP_TRY(hipGetLastError());
    return 0;
}

int launch_ws_boxes(const int32_t *segm, int H, int W, int max_label, int32_t *boxes, int *beyond, hipStream_t st)
{
    HIP_TRY(hipMemsetAsync(beyond, 0, sizeof(int), st));
    hipLaunchKernelGGL(k_ws_boxes_init, cdiv(max_label + 1, 256), 256, 0, st, boxes, max_label);
    hipLaunchKernelGGL(k_ws_boxes, dim3(cdiv(W, 64), cdiv(H, 4)), 256, 0, st, segm, H, W, max_label, boxes, beyond);
    HIP_TRY(hipGetLastError());
    return 0;
}

int launch_ws_widen(const uint8_t *plane, size_t n, int32_t *wide, hipStream_t st)
{
    hipLaunchKernelGGL(k_ws_widen, flat_grid(n), 256, 0, st, plane, n, wide);
    HIP_TRY(hipGetLastError());
    return 0;
}

int launch_ws_invert(const uint8_t *background, size_t n, uint8_t *plane, hipStream_t st)
{
    hipLaunchKernelGGL(k_ws_invert, flat_grid(n), 256, 0, st, background, n, plane);
    HIP_TRY(hipGetLastError());
    return 0;
}

int launch_ws_box_plan(const int32_t *boxes, int H, int W, int max_label, int pad, size_t capacity, int32_t *table, int *overflow,
                       hipStream_t st)
{
    HIP_TRY(hipMemsetAsync(overflow, 0, sizeof(int), st));
    hipLaunchKernelGGL(k_ws_box_plan, 1, WS_MAX_LABELS, 0, st, boxes, H, W, max_label, pad, (unsigned long long)capacity, table, overflow);
    HIP_TRY(hipGetLastError());
    return 0;
}

int launch_ws_extract(const int32_t *segm, int H, int W, const int32_t *table, int max_label, uint8_t *planes, hipStream_t st)
{
    hipLaunchKernelGGL(k_ws_extract, dim3(cdiv(W, 256), H, max_label), 256, 0, st, segm, W, table, planes);
    HIP_TRY(hipGetLastError());
    return 0;
}

int launch_ws_fill_holes(uint8_t *planes, int H, int W, const int32_t *table, int max_label, int32_t *parent, uint8_t *touches,
                         hipStream_t st)
{
    const dim3 rows(cdiv(W, 256), H, max_label);
    hipLaunchKernelGGL(k_ws_holes_init, rows, 256, 0, st, planes, table, parent, touches);
    hipLaunchKernelGGL(k_ws_holes_merge, rows, 256, 0, st, planes, table, parent);
    hipLaunchKernelGGL(k_ws_holes_touch, dim3(cdiv(2L * W + 2L * H, 256), 1, max_label), 256, 0, st, planes, table, parent, touches);
    hipLaunchKernelGGL(k_ws_holes_fill, rows, 256, 0, st, planes, table, parent, touches);
    HIP_TRY(hipGetLastError());
    return 0;
}

int launch_ws_paint(const uint8_t *planes, int H, int W, const int32_t *table, int max_label, int32_t *clean, hipStream_t st)
{
    hipLaunchKernelGGL(k_ws_paint, dim3(cdiv(W, 256), H, max_label), 256, 0, st, planes, W, table, clean);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // namespace imsegm
