// label_cc.hip -- skimage.measure.label of a label volume (imsegm/superpixels.py:111 of the reference: full connectivity, value 0 =
// background) by union-find over row segments; the session entry is imsegm_volume_label_cc (api_volume.hip).
#include "scan.h"
#include "slic.h"
#include "unionfind.h"

namespace imsegm {

// ---- skimage.measure.label: full (26-/8-) connectivity, value 0 = background ------------------------------
__global__ void __launch_bounds__(256) k_cc_init(int32_t *parent, int n)
{
    int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p < n) parent[p] = p;
}

__global__ void __launch_bounds__(256)
k_cc_merge_full(const int32_t *__restrict__ labels, int32_t *parent, int D, int H, int W)
{
    int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= D * H * W) return;
    const int l = labels[p];
    if (l == 0) return;                              // background is never joined
    const int x = p % W, y = (p / W) % H, z = p / (W * H);
    // the 13 "earlier" neighbours of the full 3 x 3 x 3 neighbourhood
    for (int dz = -1; dz <= 0; ++dz)
        for (int dy = -1; dy <= 1; ++dy)
            for (int dx = -1; dx <= 1; ++dx) {
                if (dz == 0 && (dy > 0 || (dy == 0 && dx >= 0))) continue;
                int zz = z + dz, yy = y + dy, xx = x + dx;
                if (zz < 0 || yy < 0 || yy >= H || xx < 0 || xx >= W) continue;
                int q = (zz * H + yy) * W + xx;
                if (labels[q] == l) uf_union(parent, p, q);
            }
}

// Round 5 (k_cc_merge_runs, 28.9 ms at 2^30 voxels; replaced by k_cc_merge_rows below, which keeps its rule): the same components
// with a handful of unions per RUN instead of thirteen per voxel.  Every voxel ties itself to its left neighbour when the labels
// agree, so the voxels of a run (equal labels side by side in one row) are one set.  For each of the four earlier rows that touch
// p -- (z, y-1), (z-1, y-1), (z-1, y), (z-1, y+1) -- with a, b, c its voxels at x-1, x, x+1:
//   * p has no equal left neighbour (a run starts): b equal -> union with b (a and c, if equal, hang on b's run); else union with a
//     and with c, whichever is equal;
//   * p continues a run: its left neighbour is tied to its own equal neighbours of that row, which include a and b, so only c can
//     be news, and only when b is not equal (otherwise c hangs on b's run).
// By induction along the run every voxel ends up in one set with every equal voxel of its 26-neighbourhood, i.e. the components are
// those of k_cc_merge_full; the root of a set is its smallest index either way (uf_union), so numbering and result are identical.
// Unions happen where runs start or the row above changes -- on the surface of the segments, not in their volume.

// Round 6: the same merge rule with the five rows it looks at -- (z, y) and the four earlier rows -- loaded ONCE per wave and the
// x - 1 / x + 1 neighbours taken from the neighbouring lanes (one DPP move each) instead of up to thirteen loads per voxel, no
// division for the coordinates (grid = row segments, y, z), and the forest initialised by runs: a wave covers MR_SPAN = 62 voxels of
// a row with lane 0 and lane 63 carrying the voxels left and right of them; k_cc_init_rows points every voxel of a run at the
// run's first voxel INSIDE its segment, so the merge kernel ties a voxel to its left neighbour only where a run crosses into the
// segment.  Same sets, same roots (the smallest index of a set) as k_cc_merge_runs / k_cc_merge_full.
constexpr int MR_SPAN = 62;

__global__ void __launch_bounds__(256)
k_cc_init_rows(const int32_t *__restrict__ labels, int32_t *__restrict__ parent, int H, int W)
{
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int x = (blockIdx.x * 4 + wave) * MR_SPAN + lane - 1;
    const size_t row = ((size_t)blockIdx.z * H + blockIdx.y) * W;
    const bool inx = x >= 0 && x < W;
    const int l = inx ? labels[row + x] : -1;
    const bool mine = inx && lane >= 1 && lane <= MR_SPAN;
    const bool cont = lane_prev(l, -1) == l && lane > 1 && l != 0;          // continues a run that began inside this segment
    const unsigned long long starts = __ballot(mine && !cont);
    if (!mine) return;
    const int start_lane = run_start_lane(starts, lane);                   // (lane <= 62)
    parent[row + x] = (int)(row + x) - (lane - start_lane);
}

// MR_ROWS rows of the slice per wave: the MR_ROWS + 1 rows of the slice and the MR_ROWS + 2 rows of the slice behind that they touch
// are loaded once, and the unions of a lane over its rows -- a bit each in `todo`: 13 r + 3 e + (dx + 1) for the voxel at x + dx of
// earlier row e, 13 r + 12 for the left neighbour -- are done two at a time (union2_min_root), every lane that still has some side by
// side.  (One row per wave, one union per lane and round: 16.4 ms at 2^30 voxels.)
constexpr int MR_ROWS = 4;

__global__ void __launch_bounds__(256)
k_cc_merge_rows(const int32_t *__restrict__ labels, int32_t *parent, int D, int H, int W)
{
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int x = (blockIdx.x * 4 + wave) * MR_SPAN + lane - 1;
    const int y0 = blockIdx.y * MR_ROWS, z = blockIdx.z;
    const bool inx = x >= 0 && x < W;
    const int plane = H * W;
    const size_t row0 = (size_t)z * plane + (size_t)y0 * W;
    // cz[i]: row y0 - 1 + i of this slice, pz[i]: row y0 - 1 + i of the slice behind; -1 where there is none (labels are >= 0)
    int cz[MR_ROWS + 1], pz[MR_ROWS + 2];
#pragma unroll
    for (int i = 0; i <= MR_ROWS; ++i) {
        const int y = y0 - 1 + i;
        cz[i] = (inx && y >= 0 && y < H) ? labels[row0 + (size_t)(i - 1) * W + x] : -1;
    }
#pragma unroll
    for (int i = 0; i <= MR_ROWS + 1; ++i) {
        const int y = y0 - 1 + i;
        pz[i] = (inx && z > 0 && y >= 0 && y < H) ? labels[row0 - plane + (size_t)(i - 1) * W + x] : -1;
    }
    int czp[MR_ROWS + 1], czn[MR_ROWS + 1], pzp[MR_ROWS + 2], pzn[MR_ROWS + 2];
#pragma unroll
    for (int i = 0; i <= MR_ROWS; ++i) {
        czp[i] = lane_prev(cz[i], -1);
        czn[i] = lane_next(cz[i], -1);
    }
#pragma unroll
    for (int i = 0; i <= MR_ROWS + 1; ++i) {
        pzp[i] = lane_prev(pz[i], -1);
        pzn[i] = lane_next(pz[i], -1);
    }
    const bool seg = inx && lane >= 1 && lane <= MR_SPAN;
    unsigned long long todo = 0;
#pragma unroll
    for (int r = 0; r < MR_ROWS; ++r) {
        const int l = cz[1 + r];
        const bool mine = seg && y0 + r < H && l != 0;                      // background is never joined
        const bool left = czp[1 + r] == l;
        if (mine && left && lane == 1) todo |= 1ULL << (13 * r + 12);        // a run that crosses into the segment
        // the four earlier rows that touch row y0 + r: (z, y-1), (z-1, y-1), (z-1, y), (z-1, y+1)
        const int el[4] = { cz[r], pz[r], pz[r + 1], pz[r + 2] };
        const int ep[4] = { czp[r], pzp[r], pzp[r + 1], pzp[r + 2] };
        const int en[4] = { czn[r], pzn[r], pzn[r + 1], pzn[r + 2] };
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const bool a = ep[e] == l, b = el[e] == l, c = en[e] == l;
            if (!mine) continue;
            if (left) {
                if (c && !b) todo |= 1ULL << (13 * r + 3 * e + 2);
            } else if (b) {
                todo |= 1ULL << (13 * r + 3 * e + 1);
            } else {
                if (a) todo |= 1ULL << (13 * r + 3 * e);
                if (c) todo |= 1ULL << (13 * r + 3 * e + 2);
            }
        }
    }
    const int p0 = (int)(row0 + x);
    while (__any(todo != 0)) {
        int ua[2] = { -1, -1 }, ub[2] = { -1, -1 };
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            if (!todo) continue;
            const int bit = __ffsll((long long)todo) - 1;
            todo &= todo - 1;
            const int r = bit / 13, k = bit - 13 * r;
            const int p = p0 + r * W;
            ua[j] = p;
            if (k == 12) {
                ub[j] = p - 1;
            } else {
                const int e = k / 3, dx = k - 3 * e - 1;
                ub[j] = p + dx + (e == 0 ? -W : e == 1 ? -plane - W : e == 2 ? -plane : -plane + W);
            }
        }
        union2_min_root(parent, ua[0], ub[0], ua[1], ub[1]);
    }
}

// roots of non-background components are numbered 1, 2, ... in raster order (block scan in three steps).  A workgroup takes
// CC_BLOCK voxels as CC_TILES tiles of 1 024 -- four consecutive voxels per lane, one 16-byte load, a wave reads 1 KB contiguous
// (16 consecutive voxels per lane, as before round 6, made every load instruction touch 64 cache lines: 2.3 ms a pass at 2^30
// voxels).  Only ROOTS are looked at -- parent[p] == p, which the merge pass leaves final -- so the forest is not flattened first:
// k_cc_write walks from every voxel to its root itself.
constexpr int CC_TILES = 4;
constexpr int CC_BLOCK = CC_TILES * 1024;

template <bool ASSIGN>
__global__ void __launch_bounds__(256)
k_cc_number(const int32_t *__restrict__ labels, const int32_t *__restrict__ parent, int n, int32_t *blocksum,
            int32_t *newlabel)
{
    const int base = blockIdx.x * CC_BLOCK + threadIdx.x * 4;
    unsigned fg = 0, roots = 0;                     // bit 4 * tile + c: voxel is the root of a foreground / of any component
    int cnt[CC_TILES];
#pragma unroll
    for (int i = 0; i < CC_TILES; ++i) {
        const int p = base + i * 1024;
        int v[4];
        load4_i32(parent, p, n, -1, v);
        cnt[i] = 0;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            if (v[c] != p + c) continue;
            roots |= 1u << (4 * i + c);
            if (labels[p + c] != 0) {
                fg |= 1u << (4 * i + c);
                cnt[i]++;
            }
        }
    }
    if (!ASSIGN) {
        int total;
        block_exclusive_scan<4>(cnt[0] + cnt[1] + cnt[2] + cnt[3], &total);
        if (threadIdx.x == 0) blocksum[blockIdx.x] = total;
    } else {
        int rank0 = blocksum[blockIdx.x];
#pragma unroll
        for (int i = 0; i < CC_TILES; ++i) {
            int total;
            int rank = rank0 + block_exclusive_scan<4>(cnt[i], &total);
            rank0 += total;
#pragma unroll
            for (int c = 0; c < 4; ++c)
                if (roots >> (4 * i + c) & 1u) newlabel[base + i * 1024 + c] = (fg >> (4 * i + c) & 1u) ? 1 + rank++ : 0;
        }
    }
}

// out[p] = number of p's root: four voxels per lane, their walks to the root side by side (four loads in flight per step; the
// forest is what the merge pass left -- a run's voxels point at its first voxel, that one at an earlier run -- two or three steps)
__global__ void __launch_bounds__(256)
k_cc_write(const int32_t *__restrict__ parent, const int32_t *__restrict__ newlabel, int n, int32_t *out)
{
    const int p = (blockIdx.x * 256 + threadIdx.x) * 4;
    if (p >= n) return;
    int r[4];
    load4_i32(parent, p, n, 0, r);
    walk4_to_roots(parent, r);
    int o[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) o[c] = newlabel[r[c]];
    if (p + 4 <= n) {
        *reinterpret_cast<int4 *>(out + p) = make_int4(o[0], o[1], o[2], o[3]);
    } else {
        for (int c = 0; p + c < n; ++c) out[p + c] = o[c];
    }
}

int launch_label_cc(int32_t *labels_inout, int D, int H, int W, int32_t *parent, int32_t *newlabel, int32_t *blocksum,
                    int32_t *total_dev, hipStream_t st)
{
    const int n = D * H * W, grid = cdiv(n, 256), nb = cdiv(n, CC_BLOCK);
    if (knobs().cc_merge_full || H > 65535 || D > 65535) {
        hipLaunchKernelGGL(k_cc_init, grid, 256, 0, st, parent, n);
        hipLaunchKernelGGL(k_cc_merge_full, grid, 256, 0, st, labels_inout, parent, D, H, W);
    } else {
        const dim3 rows(cdiv(W, 4 * MR_SPAN), H, D), row_groups(cdiv(W, 4 * MR_SPAN), cdiv(H, MR_ROWS), D);
        hipLaunchKernelGGL(k_cc_init_rows, rows, 256, 0, st, labels_inout, parent, H, W);
        hipLaunchKernelGGL(k_cc_merge_rows, row_groups, 256, 0, st, labels_inout, parent, D, H, W);
    }
    hipLaunchKernelGGL(k_cc_number<false>, nb, 256, 0, st, labels_inout, parent, n, blocksum, newlabel);
    launch_exclusive_scan(blocksum, nb, total_dev, st);
    hipLaunchKernelGGL(k_cc_number<true>, nb, 256, 0, st, labels_inout, parent, n, blocksum, newlabel);
    hipLaunchKernelGGL(k_cc_write, cdiv(cdiv(n, 4), 256), 256, 0, st, parent, newlabel, n, labels_inout);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // namespace imsegm
