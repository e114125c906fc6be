// unionfind.h -- the union-find forest in global memory that the labelling passes share (connectivity.hip, label_cc.hip): a set's
// root is its SMALLEST index (atomicMin on the parent of the larger root), so the result does not depend on the order of the unions.
// (The 2-D tile path of connectivity.hip keeps a forest of its own in volatile LDS -- lds_find / lds_union -- with other memory
// semantics; it is not this one.)  Also here: load4_i32, the 16-byte load of four consecutive words with a tail that these passes
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
