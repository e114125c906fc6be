// cluster.hip -- DBSCAN of many small sets of 2-D points: ONE workgroup per set, the set's coordinates and its forest in LDS
// (cluster.h).  The result is the closed form of scikit-learn's scan ("Centre detection"): core points by
// count, clusters = connected components of the core points numbered by their smallest index, a border point takes the smallest
// number among the core points near it, centres are sums in index order.  Nothing here depends on the order the atomics land in.
#include <climits>

#include "cluster.h"
#include "scan.h"
#include "unionfind.h"

namespace imsegm {

namespace {

// dx * dx + dy * dy <= eps2 with two rounded products and one rounded sum, spelled with the _rn intrinsics and not left to the
// build's -ffp-contract=off: a fused dx * dx + (dy * dy) keeps one product exact, and a pair that lies at eps exactly on the host
// (3-4-5 triangles, points on a grid) would fall on the other side of the comparison here.
__device__ __forceinline__ bool db_near(double ax, double ay, double bx, double by, double eps2)
{
    const double dx = ax - bx, dy = ay - by;
    return __dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)) <= eps2;
}

__global__ __launch_bounds__(DBSCAN_THREADS) void k_dbscan_sets(const double *__restrict__ points, const int32_t *__restrict__ offsets,
                                                                int n_max, double eps2, int min_samples, int32_t *__restrict__ labels,
                                                                int32_t *__restrict__ counts, double *__restrict__ centres)
{
    extern __shared__ __align__(16) unsigned char db_lds[];
    double *px = reinterpret_cast<double *>(db_lds), *py = px + n_max;
    int32_t *parent = reinterpret_cast<int32_t *>(py + n_max);      // -1: not a core point; else the forest of the core points
    int32_t *num = parent + n_max;                                   // at a root: the number of its cluster
    int32_t *lab = num + n_max;                                      // the labels, for the centres
    const int tid = threadIdx.x, set = blockIdx.x;
    const int first = offsets[set], n = offsets[set + 1] - first;
    const double *pts = points + (size_t)first * 2;

    for (int i = tid; i < n; i += DBSCAN_THREADS) {
        px[i] = pts[2 * i];
        py[i] = pts[2 * i + 1];
    }
    __syncthreads();
    // pass 1: the points near every point (itself among them) -> core or not
    for (int i = tid; i < n; i += DBSCAN_THREADS) {
        const double x = px[i], y = py[i];
        int near = 0;
        for (int j = 0; j < n; ++j) near += db_near(x, y, px[j], py[j], eps2);       // (every lane reads the same j: a broadcast)
        parent[i] = near >= min_samples ? i : -1;
    }
    __syncthreads();
    // pass 2: the near core pairs, the larger root below the smaller (a core point's parent never goes below 0)
    for (int i = tid; i < n; i += DBSCAN_THREADS) {
        if (parent[i] < 0) continue;
        const double x = px[i], y = py[i];
        for (int j = 0; j < i; ++j)
            if (parent[j] >= 0 && db_near(x, y, px[j], py[j], eps2)) uf_union_pair(parent, i, j);
    }
    __syncthreads();
    // every core point to its root (a walk that meets a flattened entry meets the root itself)
    for (int i = tid; i < n; i += DBSCAN_THREADS)
        if (parent[i] >= 0) parent[i] = uf_find(parent, i);
    __syncthreads();
    // the roots in index order are the clusters in the order of their smallest core points
    int n_clusters = 0;
    for (int base = 0; base < n; base += DBSCAN_THREADS) {
        const int i = base + tid;
        const int is_root = i < n && parent[i] == i;
        int total;
        const int before = block_exclusive_scan<DBSCAN_THREADS / 64, int>(is_root, &total);
        if (is_root) num[i] = n_clusters + before;
        n_clusters += total;
    }
    __syncthreads();
    // pass 3: a core point has the number of its root, any other point the smallest number among the core points near it
    for (int i = tid; i < n; i += DBSCAN_THREADS) {
        int label = INT_MAX;
        if (parent[i] >= 0) {
            label = num[parent[i]];
        } else {
            const double x = px[i], y = py[i];
            for (int j = 0; j < n; ++j) {
                const int root = parent[j];
                if (root >= 0 && db_near(x, y, px[j], py[j], eps2)) label = min(label, num[root]);
            }
        }
        if (label == INT_MAX) label = -1;
        lab[i] = label;
        labels[first + i] = label;
    }
    __syncthreads();
    // the centre of cluster c in slot c of the set: np.mean(points[labels == c], axis=0) adds the rows one after the other
    for (int c = tid; c < n; c += DBSCAN_THREADS) {
        double sx = 0.0, sy = 0.0;
        int members = 0;
        if (c < n_clusters)
            for (int j = 0; j < n; ++j)
                if (lab[j] == c) {
                    sx = members ? __dadd_rn(sx, px[j]) : px[j];
                    sy = members ? __dadd_rn(sy, py[j]) : py[j];
                    ++members;
                }
        double *out = centres + (size_t)(first + c) * 2;
        out[0] = members ? sx / (double)members : 0.0;
        out[1] = members ? sy / (double)members : 0.0;
    }
    if (tid == 0) counts[set] = n_clusters;
}

}  // namespace

int launch_dbscan_points(const double *points, const int32_t *offsets, int nb_sets, int n_max, double eps2, int min_samples,
                         int32_t *labels, int32_t *counts, double *centres, hipStream_t st)
{
    if (nb_sets < 1) return 0;
    if (n_max < 1 || n_max > DBSCAN_MAX_POINTS) {
        set_error("dbscan: a set of 1 .. DBSCAN_MAX_POINTS points at the most");
        return -1;
    }
    // the opt-in above 48 KB is per device and always for the cap: remembered per device (benign race: the same value)
    static bool lds_set[IMSEGM_MAX_DEVICES];
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    if (dev < 0 || dev >= IMSEGM_MAX_DEVICES || !lds_set[dev]) {
        HIP_TRY(hipFuncSetAttribute((const void *)k_dbscan_sets, hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)dbscan_lds_bytes(DBSCAN_MAX_POINTS)));
        if (dev >= 0 && dev < IMSEGM_MAX_DEVICES) lds_set[dev] = true;
    }
    hipLaunchKernelGGL(k_dbscan_sets, dim3(nb_sets), dim3(DBSCAN_THREADS), dbscan_lds_bytes(n_max), st, points, offsets, n_max, eps2,
                       min_samples, labels, counts, centres);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // namespace imsegm
