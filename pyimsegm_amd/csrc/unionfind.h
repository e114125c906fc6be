// unionfind.h -- the union-find forest in global memory that the labelling passes share (connectivity.hip, label_cc.hip): a set's
// root is its SMALLEST index (atomicMin on the parent of the larger root), so the result does not depend on the order of the unions.
// (The 2-D tile path of connectivity.hip keeps a forest of its own in volatile LDS -- lds_find / lds_union -- with other memory
// semantics; it is not this one.)  Also here: the 2-D labelling by row segments that morphology.hip and object_shapes.hip share
// (run_start_lane, run_label_init, run_label_merge), and load4_i32, the 16-byte load of four consecutive words with a tail that these passes
// and their neighbours (k_kept_scan, k_small_bbox) read parents with.
#pragma once
#include "common.h"

namespace imsegm {

__device__ __forceinline__ int uf_find(const int32_t *parent, int a)
{
    int p = parent[a];
    while (p != a) {
        a = p;
        p = parent[a];
    }
    return a;
}

__device__ __forceinline__ void uf_union(int32_t *parent, int a, int b)
{
    while (true) {
        a = uf_find(parent, a);
        b = uf_find(parent, b);
        if (a == b) return;
        if (a < b) {
            int t = a;
            a = b;
            b = t;
        }
        // a > b: hang the larger root below the smaller one
        int old = atomicMin(&parent[a], b);
        if (old == a) return;
        a = old;
    }
}

// union with the two finds walked together (both loads of a step in flight at once: half the dependent trips of uf_union)
__device__ __forceinline__ void uf_union_pair(int32_t *parent, int a, int b)
{
    while (true) {
        while (true) {
            const int pa = parent[a], pb = parent[b];
            if (pa == a && pb == b) break;
            a = pa;
            b = pb;
        }
        if (a == b) return;
        if (a < b) {
            const int t = a;
            a = b;
            b = t;
        }
        const int old = atomicMin(&parent[a], b);
        if (old == a) return;
        a = old;
    }
}

// the lane at which the run of `lane` starts: the highest bit of `starts` (one bit per lane that begins a run) at or below it
__device__ __forceinline__ int run_start_lane(unsigned long long starts, int lane)
{
    const unsigned long long below = starts & ((2ULL << lane) - 1ULL);
    return 63 - __clzll((long long)below);
}

// ---- 4-connected labelling of the pixels of a 2-D map that a predicate on their value selects, by row segments -----------------
// (k_holes_* of morphology.hip on the pixels <= 0, k_os_cc_* of object_shapes.hip on the pixels != 0, k_ca_cc_* of
// center_annotation.hip on the set bytes of a mask.)  A wave covers 64
// consecutive pixels of row y, lane = x & 63, and every lane of the wave calls.  run_label_init: every selected pixel starts out
// pointing at the first pixel of its run INSIDE its segment, every other pixel at itself, so the unions that are left lie where a
// run crosses a segment and where a run meets the row above for the first time.
template <typename Map, typename Selected>
__device__ __forceinline__ void run_label_init(const Map *__restrict__ segm, int32_t *__restrict__ parent, int y, int x, int W,
                                               Selected selected)
{
    const int lane = threadIdx.x & 63;
    const size_t row = (size_t)y * W;
    const bool inx = x < W;
    const bool sel = inx && selected(segm[row + x]);
    const unsigned long long z = __ballot(sel);
    if (!inx) return;
    const int start = sel ? run_start_lane(z & ~(z << 1), lane) : lane;
    parent[row + x] = (int)(row + x) - (lane - start);
}

// run_label_merge: p and the pixel above it are tied when p starts a run of its segment or the pixel above p - 1 is not selected:
// otherwise p - 1 is tied to the pixel above it, which shares a run (and a segment) with the pixel above p
template <typename Map, typename Selected>
__device__ __forceinline__ void run_label_merge(const Map *__restrict__ segm, int32_t *parent, int y, int x, int W, Selected selected)
{
    const int lane = threadIdx.x & 63;
    const size_t row = (size_t)y * W;
    const bool inx = x < W;
    const bool sel = inx && selected(segm[row + x]);
    const bool up_any = inx && y > 0 && selected(segm[row - W + x]);
    const bool up = sel && up_any;
    const unsigned long long z = __ballot(sel), zu = __ballot(up_any);
    if (!sel) return;
    const int p = (int)(row + x);
    const bool first = lane == 0 || !((z >> (lane - 1)) & 1ULL);
    if (lane == 0 && x > 0 && selected(segm[p - 1])) uf_union_pair(parent, p, p - 1);
    if (up && (first || !((zu >> (lane - 1)) & 1ULL))) uf_union_pair(parent, p, p - W);
}

// Union-find with the smaller index as the root (atomicMin on the parent of the larger root), TWO unions of a lane side by side:
// (a0, b0) and, where a1 >= 0, (a1, b1).  The four walks to the roots advance together -- four loads in flight per step instead
// of the one of a find after the other -- and a union whose atomicMin lost a race goes on from what it saw.  Unions of one lane
// may touch the same sets: atomicMin keeps every interleaving a forest whose roots are the smallest indices.
__device__ __forceinline__ void union2_min_root(int32_t *parent, int a0, int b0, int a1, int b1)
{
    bool on0 = a0 >= 0, on1 = a1 >= 0;
    while (on0 || on1) {
        const int pa0 = on0 ? parent[a0] : 0, pb0 = on0 ? parent[b0] : 0;
        const int pa1 = on1 ? parent[a1] : 0, pb1 = on1 ? parent[b1] : 0;
        if (on0) {
            if (pa0 == a0 && pb0 == b0) {
                const int hi = max(a0, b0), lo = min(a0, b0);
                const int old = hi == lo ? hi : atomicMin(&parent[hi], lo);
                on0 = old != hi;
                a0 = old;
                b0 = lo;
            } else {
                a0 = pa0;
                b0 = pb0;
            }
        }
        if (on1) {
            if (pa1 == a1 && pb1 == b1) {
                const int hi = max(a1, b1), lo = min(a1, b1);
                const int old = hi == lo ? hi : atomicMin(&parent[hi], lo);
                on1 = old != hi;
                a1 = old;
                b1 = lo;
            } else {
                a1 = pa1;
                b1 = pb1;
            }
        }
    }
}

// four consecutive words of an int32 array (one 16-byte load where all four exist, `fill` behind the end)
__device__ __forceinline__ void load4_i32(const int32_t *a, int p, int n, int fill, int (&v)[4])
{
    if (p + 4 <= n) {
        const int4 q = *reinterpret_cast<const int4 *>(a + p);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
#pragma unroll
        for (int c = 0; c < 4; ++c) v[c] = p + c < n ? a[p + c] : fill;
    }
}

// Four walks to the roots side by side: a step moves each r[c] to its parent -- four loads in flight -- and tells whether any of
// them moved.  (A kernel with more than four walks per lane steps them all inside ONE loop, so that their loads stay in flight
// together: k_ccl_flatten_sizes_rows.)
__device__ __forceinline__ bool walk4_step(const int32_t *parent, int (&r)[4])
{
    int q[4];
    bool moved = false;
#pragma unroll
    for (int c = 0; c < 4; ++c) q[c] = parent[r[c]];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        moved |= q[c] != r[c];
        r[c] = q[c];
    }
    return moved;
}
__device__ __forceinline__ void walk4_to_roots(const int32_t *parent, int (&r)[4])
{
    while (walk4_step(parent, r)) {}
}

}  // namespace imsegm
