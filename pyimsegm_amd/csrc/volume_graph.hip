// volume_graph.hip -- the 6-connected region adjacency of a label volume and the centres of its supervoxels
// (make_graph_segm_connect_grid3d_conn6 / superpixel_centers of the reference, 3-D branch), as a K x K bitmap or as a neighbour table.
#include "slic.h"

namespace imsegm {

// ---- 6-connected adjacency bitmap + centre sums of a label volume -----------------------------------------
// (table: instead of bit (row b, column a) of a K x K bitmap, every label goes into the row of each of its neighbours in a K x cap
// table of neighbour slots -- open addressing inside the row, -1 = free; a row that is full raises *overflow and the caller comes
// back with wider rows.  The bitmap is 11 GB for the 3 * 10^5 supervoxels of BASELINE configs[4] and caps K; the table is
// K * cap * 4 bytes.  Round 6: the table is SYMMETRIC (rounds 4 / 5 kept the smaller neighbours only), so that the fused call can
// build its arcs from it -- terms.hip k_tab_sort_rows / k_tab_emit -- as it does from the mirrored bitmap.)
__device__ __forceinline__ void neighbour_insert(int32_t *table, int cap, int b, int a, int *overflow)
{
    int32_t *row = table + (size_t)b * cap;
    unsigned slot = ((unsigned)a * 2654435761u) >> 7;
    for (int probe = 0; probe < cap; ++probe, ++slot) {
        int32_t *cell = row + (slot & (unsigned)(cap - 1));
        int seen = __hip_atomic_load(cell, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (seen == a) return;
        if (seen == -1) {
            seen = atomicCAS(cell, -1, a);
            if (seen == -1 || seen == a) return;
        }
    }
    *overflow = 1;
}

// Round 6: by rows and runs, like the 2-D kernel (graph.hip).  A wave owns 64 x VA_ROWS voxels of one slice -- VA_ROWS + 1 rows of it
// and VA_ROWS rows of the next slice in registers, the left / right neighbour through one DPP move each.
//   * neighbour pairs: across x a pair exists exactly where a run ends; across y and z the pair (label, label below / behind) of a
//     voxel is the pair of its left neighbour along the whole contact of two segments, so only the lane where EITHER label changes
//     reports it -- a handful of inserts per run instead of one per surface voxel;
//   * centre sums: the first lane of a run knows its length from the vote of the run starts, hence n, sum y, sum x of the run in
//     closed form (z is the workgroup's); they meet in an LDS hash table of the workgroup (a 64 x 16 cross-section sees a dozen
//     labels), flushed with one set of int64 global atomics per label and workgroup.
// Rounds 2 - 5 went voxel by voxel: two 32-bit divisions per voxel for its coordinates, a serial loop over the distinct labels of
// a wave with eight int64 wave reductions and four global atomics each (19.8 ms for the 2^30 voxels of BASELINE configs[4]).
// MODE 0: bit (row b, column a), a < b, of the K x K bitmap; MODE 1: a into row b AND b into row a of the neighbour table.
constexpr int VA_ROWS = 4;
constexpr int VA_SLOTS = 64;
constexpr int VA_DEPTH = 8;           // slices a workgroup walks (sums of a table slot stay far below 2^31: 8 192 voxels x 65 535)

// The (up to) three neighbour pairs a voxel reports, both directions each: the six table cells a pair's labels hash to are looked at
// TOGETHER -- one trip to memory -- and nearly always hold the label already (a pair of neighbouring supervoxels is reported by every
// voxel along their common face); what is not found there goes through neighbour_insert.  (One pair after the other, each with
// its own look: twenty-four dependent trips per wave of four rows, 4.6 ms for the 2^30 voxels of config 5.)
__device__ __forceinline__ void neighbour_insert3(int32_t *table, int cap, int l, const int (&nb)[3], int *overflow)
{
    int seen[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        const int row = i < 3 ? l : nb[i - 3], val = i < 3 ? nb[i] : l;
        seen[i] = val;                                             // (no pair: nothing to do)
        if (nb[i % 3] >= 0)
            seen[i] = __hip_atomic_load(table + (size_t)row * cap + ((((unsigned)val * 2654435761u) >> 7) & (unsigned)(cap - 1)),
                                        __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        const int row = i < 3 ? l : nb[i - 3], val = i < 3 ? nb[i] : l;
        if (nb[i % 3] >= 0 && seen[i] != val) neighbour_insert(table, cap, row, val, overflow);
    }
}

template <int MODE>
__device__ __forceinline__ void adjacency_report(int l, int nb, int words, uint32_t *bitmap, int32_t *table, int cap, int *overflow)
{
    if (MODE == 1) {
        neighbour_insert(table, cap, l, nb, overflow);
        neighbour_insert(table, cap, nb, l, overflow);
    } else {
        const int a = min(l, nb), b = max(l, nb);
        uint32_t *wp = bitmap + (size_t)b * words + (a >> 5);
        const uint32_t bit = 1u << (a & 31);
        if (!(*wp & bit)) atomicOr(wp, bit);
    }
}

template <int MODE>
__global__ void __launch_bounds__(256)
k_vol_adjacency_runs(const int32_t *__restrict__ labels, int D, int H, int W, int words, uint32_t *bitmap,
                     long long *__restrict__ cacc, int32_t *table, int cap, int *overflow)
{
    // (round 6, later: a workgroup walks VA_DEPTH slices -- the rows of the slice behind are the next turn's own rows, so a voxel is
    // loaded once instead of twice, and the centre sums of all the slices meet in one LDS table: 4.85 -> see profiles/README_r06.md)
    __shared__ int h_key[VA_SLOTS], h_n[VA_SLOTS], h_sz[VA_SLOTS], h_sy[VA_SLOTS], h_sx[VA_SLOTS];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (threadIdx.x < VA_SLOTS) {
        h_key[threadIdx.x] = -1;
        h_n[threadIdx.x] = 0;
        h_sz[threadIdx.x] = 0;
        h_sy[threadIdx.x] = 0;
        h_sx[threadIdx.x] = 0;
    }
    __syncthreads();
    const int z_first = blockIdx.z * VA_DEPTH, z_end = min(z_first + VA_DEPTH, D);
    const int y0 = (blockIdx.y * 4 + wave) * VA_ROWS;
    const int x = blockIdx.x * 64 + lane;
    const bool xin = x < W;
    const size_t plane = (size_t)H * W;
    const unsigned long long le = (lane == 63) ? ~0ULL : ((2ULL << lane) - 1ULL);
    // (edge: the voxel right of the wave's last lane, fetched by that lane WITH the rows -- asked for row by row where it is used, it
    // was a trip to memory per row and slice for the sake of one lane)
    int lab[VA_ROWS + 1], behind[VA_ROWS + 1], edge[VA_ROWS], edge_behind[VA_ROWS];
    const bool last = lane == 63 && x + 1 < W;
    {
        const int32_t *__restrict__ first = labels + ((size_t)z_first * H + y0) * W;
#pragma unroll
        for (int r = 0; r <= VA_ROWS; ++r) lab[r] = (xin && y0 + r < H) ? first[(size_t)r * W + x] : -1;
#pragma unroll
        for (int r = 0; r < VA_ROWS; ++r) edge[r] = (last && y0 + r < H) ? first[(size_t)r * W + x + 1] : -1;
#pragma unroll
        for (int r = 0; r <= VA_ROWS; ++r) behind[r] = (xin && y0 + r < H && z_first + 1 < D) ? first[plane + (size_t)r * W + x] : -1;
#pragma unroll
        for (int r = 0; r < VA_ROWS; ++r) edge_behind[r] = (last && y0 + r < H && z_first + 1 < D) ? first[plane + (size_t)r * W + x + 1] : -1;
    }
    for (int z = z_first; z < z_end; ++z) {
        // (the rows of slice z + 2 are requested HERE and used in the next turn: a turn does not wait for its own loads)
        const int32_t *__restrict__ base = labels + ((size_t)z * H + y0) * W;          // (wave uniform)
        const bool more = z + 1 < z_end && z + 2 < D;
        int ahead[VA_ROWS + 1], edge_ahead[VA_ROWS];
#pragma unroll
        for (int r = 0; r <= VA_ROWS; ++r) ahead[r] = (more && xin && y0 + r < H) ? base[2 * plane + (size_t)r * W + x] : -1;
#pragma unroll
        for (int r = 0; r < VA_ROWS; ++r) edge_ahead[r] = (more && last && y0 + r < H) ? base[2 * plane + (size_t)r * W + x + 1] : -1;
#pragma unroll
        for (int r = 0; r < VA_ROWS; ++r) {
            const int y = y0 + r;
            const int l = lab[r];
            const bool act = l >= 0;                                   // (the active lanes of a row are lanes 0 .. nact - 1)
            int right = lane_next(l, -1);
            if (lane == 63) right = edge[r];
            const int left = lane_prev(l, -2);
            const int below = lab[r + 1], back = behind[r];
            const int below_left = lane_prev(below, -2), back_left = lane_prev(back, -2);
            const bool rep_right = act && right >= 0 && right != l;
            const bool rep_below = act && below >= 0 && below != l && !(left == l && below_left == below);
            const bool rep_back = act && back >= 0 && back != l && !(left == l && back_left == back);
            if (MODE == 1) {
                if (rep_right || rep_below || rep_back) {
                    const int nb[3] = { rep_right ? right : -1, rep_below ? below : -1, rep_back ? back : -1 };
                    neighbour_insert3(table, cap, l, nb, overflow);
                }
            } else {
                if (rep_right) adjacency_report<MODE>(l, right, words, bitmap, table, cap, overflow);
                if (rep_below) adjacency_report<MODE>(l, below, words, bitmap, table, cap, overflow);
                if (rep_back) adjacency_report<MODE>(l, back, words, bitmap, table, cap, overflow);
            }
            const bool start = act && left != l;                       // (lane 0: left = -2)
            const unsigned long long starts = __ballot(start);
            const int nact = __popcll(__ballot(act));
            if (start) {
                const unsigned long long above = starts & ~le;
                const int len = (above ? __ffsll((long long)above) - 1 : nact) - lane;
                const int sy = len * y, sx = len * x + (len * (len - 1)) / 2;
                int slot = (int)(((unsigned int)l * 2654435761u) >> 26);          // 6 bits
                bool placed = false;
                for (int probe = 0; probe < VA_SLOTS; ++probe) {
                    const int old = atomicCAS(&h_key[slot], -1, l);
                    if (old == -1 || old == l) {
                        placed = true;
                        break;
                    }
                    slot = (slot + 1) & (VA_SLOTS - 1);
                }
                if (placed) {
                    atomicAdd(&h_n[slot], len);
                    atomicAdd(&h_sz[slot], len * z);
                    atomicAdd(&h_sy[slot], sy);
                    atomicAdd(&h_sx[slot], sx);
                } else {                                               // (more than VA_SLOTS labels in the slices of a 64 x 16 cross-section)
                    atomic_add_i64(cacc + (size_t)l * 4 + 0, len);
                    atomic_add_i64(cacc + (size_t)l * 4 + 1, (long long)len * z);
                    atomic_add_i64(cacc + (size_t)l * 4 + 2, (long long)sy);
                    atomic_add_i64(cacc + (size_t)l * 4 + 3, (long long)sx);
                }
            }
        }
#pragma unroll
        for (int r = 0; r <= VA_ROWS; ++r) {
            lab[r] = behind[r];
            behind[r] = ahead[r];
        }
#pragma unroll
        for (int r = 0; r < VA_ROWS; ++r) {
            edge[r] = edge_behind[r];
            edge_behind[r] = edge_ahead[r];
        }
    }
    __syncthreads();
    if (threadIdx.x < VA_SLOTS && h_key[threadIdx.x] >= 0) {
        const int k = h_key[threadIdx.x], n = h_n[threadIdx.x];
        atomic_add_i64(cacc + (size_t)k * 4 + 0, n);
        atomic_add_i64(cacc + (size_t)k * 4 + 1, h_sz[threadIdx.x]);
        atomic_add_i64(cacc + (size_t)k * 4 + 2, h_sy[threadIdx.x]);
        atomic_add_i64(cacc + (size_t)k * 4 + 3, h_sx[threadIdx.x]);
    }
}

__global__ void k_vol_centres_finalize(const long long *__restrict__ cacc, int K, double *centres, uint8_t *present)
{
    int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= K) return;
    long long n = cacc[(size_t)k * 4];
    present[k] = n > 0;
    for (int c = 0; c < 3; ++c)
        centres[3 * k + c] = n > 0 ? i64_to_double(cacc[(size_t)k * 4 + 1 + c]) / (double)n : -1.0;
}

static inline dim3 vol_adjacency_grid(int D, int H, int W) { return dim3(cdiv(W, 64), cdiv(H, 4 * VA_ROWS), cdiv(D, VA_DEPTH)); }

int launch_vol_adjacency(const int32_t *labels, int D, int H, int W, int K, int words, uint32_t *bitmap, long long *cacc,
                         double *centres, uint8_t *present, hipStream_t st)
{
    if (D > 65535 || cdiv(H, 4 * VA_ROWS) > 65535) {
        set_error("adjacency: more than 65 535 slices or 1 048 560 rows");
        return -1;
    }
    HIP_TRY(hipMemsetAsync(bitmap, 0, (size_t)K * words * sizeof(uint32_t), st));
    HIP_TRY(hipMemsetAsync(cacc, 0, (size_t)K * 4 * sizeof(long long), st));
    hipLaunchKernelGGL(k_vol_adjacency_runs<0>, vol_adjacency_grid(D, H, W), 256, 0, st, labels, D, H, W, words, bitmap, cacc, nullptr, 0, nullptr);
    hipLaunchKernelGGL(k_vol_centres_finalize, cdiv(K, 256), 256, 0, st, cacc, K, centres, present);
    HIP_TRY(hipGetLastError());
    return 0;
}

// the same with the neighbour table (K x cap slots, cap a power of two) instead of the bitmap; *overflow (device) is raised when a
// row was too narrow
int launch_vol_adjacency_table(const int32_t *labels, int D, int H, int W, int K, int32_t *table, int cap, int *overflow, long long *cacc,
                               double *centres, uint8_t *present, hipStream_t st)
{
    if (D > 65535 || cdiv(H, 4 * VA_ROWS) > 65535) {
        set_error("adjacency: more than 65 535 slices or 1 048 560 rows");
        return -1;
    }
    HIP_TRY(hipMemsetAsync(table, 0xff, (size_t)K * cap * sizeof(int32_t), st));
    HIP_TRY(hipMemsetAsync(overflow, 0, sizeof(int), st));
    HIP_TRY(hipMemsetAsync(cacc, 0, (size_t)K * 4 * sizeof(long long), st));
    hipLaunchKernelGGL(k_vol_adjacency_runs<1>, vol_adjacency_grid(D, H, W), 256, 0, st, labels, D, H, W, 0, nullptr, cacc, table, cap, overflow);
    hipLaunchKernelGGL(k_vol_centres_finalize, cdiv(K, 256), 256, 0, st, cacc, K, centres, present);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // namespace imsegm
