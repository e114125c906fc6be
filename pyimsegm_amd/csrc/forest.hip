// forest.hip -- predict_proba of a random forest / extra trees / one decision tree on the device, bit for bit with scikit-learn
// (include/imsegm_hip.h "random-forest class models").  Three kernels on one stream:
//   k_forest_scale  z[f][k] = float32((x - mean) / scale): fp64 subtract, IEEE divide, one rounding to float32 (nearest even)
//   k_forest_walk   leaf[t][k]: a workgroup owns one tree -- staged in LDS when it has at most FOREST_LDS_NODES nodes, read from
//                   global memory by the same walk otherwise -- and blocks of FOREST_ROWS rows, one row per lane
//   k_forest_sum    proba[k][c] = (0 + value[leaf[0][k]][c] + value[leaf[1][k]][c] + ...) / T: one lane per (row, class) adds the
//                   trees in their order in fp64 and divides once.  No atomics, no reduction across trees: the order is the result.
// The table is transposed for the walk: the lanes of a wave are consecutive rows, so a node they share is one coalesced read.
#include "forest.h"

namespace imsegm {

__global__ void __launch_bounds__(256) k_forest_scale(ForestArgs a)
{
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (size_t)a.n_rows * a.F) return;
    const size_t k = idx / a.F;
    const int f = (int)(idx - k * a.F);
    const double x = a.table[idx];
    double s = x;
    if (a.mean) s = s - a.mean[f];
    if (a.scale) s = s / a.scale[f];
    const float v = (float)s;
    if (!isfinite(x) || !isfinite(v)) *a.flag = 1;             // (every lane that finds one stores the same word)
    a.z[(size_t)f * a.stride + k] = v;
}

// from node 0 to a leaf: at most `count` steps (a path visits a node once), every index checked against the tree
template <typename Nodes>
__device__ __forceinline__ int forest_leaf(Nodes tree, int count, int F, const float *zk, size_t stride)
{
    int i = 0;
    for (int step = 0; step < count; ++step) {
        const imsegm_forest_node nd = tree[i];
        if (nd.word < 0) return ~nd.word;
        const int f = nd.word & 0xff;
        if (f >= F) return -1;
        const float v = zk[(size_t)f * stride];
        i = v <= nd.threshold ? i + 1 : nd.word >> 8;
        if ((unsigned)i >= (unsigned)count) return -1;
    }
    return -1;
}

__global__ void __launch_bounds__(FOREST_ROWS) k_forest_walk(ForestArgs a, int n_blocks, int n_leaves)
{
    __shared__ imsegm_forest_node staged[FOREST_LDS_NODES];
    const int t = blockIdx.y;
    const int first = a.tree_start[t], count = a.tree_start[t + 1] - first;
    const imsegm_forest_node *tree = a.nodes + first;
    const bool in_lds = count <= FOREST_LDS_NODES;
    if (in_lds) {
        for (int i = threadIdx.x; i < count; i += FOREST_ROWS) staged[i] = tree[i];
        __syncthreads();
    }
    for (int block = blockIdx.x; block < n_blocks; block += gridDim.x) {
        const int k = block * FOREST_ROWS + (int)threadIdx.x;
        if (k >= a.n_rows) continue;
        const float *zk = a.z + k;
        int row = in_lds ? forest_leaf(staged, count, a.F, zk, a.stride) : forest_leaf(tree, count, a.F, zk, a.stride);
        if ((unsigned)row >= (unsigned)n_leaves) {
            *a.flag = 2;
            row = 0;
        }
        a.leaf[(size_t)t * a.stride + k] = row;
    }
}

__global__ void __launch_bounds__(256) k_forest_sum(ForestArgs a)
{
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (size_t)a.n_rows * a.C) return;
    const size_t k = idx / a.C;
    const int c = (int)(idx - k * a.C);
    double sum = 0.0;
    for (int t = 0; t < a.T; ++t) sum += a.leaf_values[(size_t)a.leaf[(size_t)t * a.stride + k] * a.C + c];
    a.proba[idx] = sum / (double)a.T;
}

int launch_forest_proba(const ForestArgs &a, int n_leaves, hipStream_t st)
{
    if (a.n_rows < 1 || a.T < 1) return 0;
    const int n_blocks = (int)(a.stride / FOREST_ROWS);
    // a tree is staged once per workgroup: up to 64 workgroups per tree share the blocks of rows between them
    const dim3 walk_grid((unsigned)std::min(n_blocks, 64), (unsigned)a.T);
    hipLaunchKernelGGL(k_forest_scale, cdiv((long)a.n_rows * a.F, 256), 256, 0, st, a);
    hipLaunchKernelGGL(k_forest_walk, walk_grid, FOREST_ROWS, 0, st, a, n_blocks, n_leaves);
    hipLaunchKernelGGL(k_forest_sum, cdiv((long)a.n_rows * a.C, 256), 256, 0, st, a);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // namespace imsegm
