// api_cluster.hip -- C ABI of the clustering of centre candidates (experiments_ovary_centres/run_center_clustering.py of the
// reference: cluster_center_candidates).  A stateless call on a context and host arrays; arguments and caps are checked before the
// device is touched; the kernel is in cluster.hip.  Points and offsets go up as one block of the page-locked staging memory, labels,
// counts and centres come down as one.
#include <cmath>

#include "cluster.h"
#include "session.h"

static_assert(DBSCAN_MAX_POINTS == IMSEGM_DBSCAN_MAX_POINTS, "the LDS layout of cluster.hip");

namespace imsegm {

namespace {

// where the pieces of one call live inside the context's scratch buffer and, at the same offsets, inside the staging block: what
// goes up (points | offsets) in front, what comes down (labels | counts | centres) behind it; every piece on a 256-byte boundary
struct ClusterPlan {
    size_t o_points, o_offsets, up_bytes, o_labels, o_counts, o_centres, bytes;
};

ClusterPlan cluster_plan(size_t total, size_t nb_sets)
{
    ClusterPlan p;
    size_t at = 0;
    auto take = [&](size_t bytes) { size_t o = at; at += (bytes + 255) & ~(size_t)255; return o; };
    p.o_points = take(total * 16);
    p.o_offsets = take((nb_sets + 1) * 4);
    p.up_bytes = at;
    p.o_labels = take(total * 4);
    p.o_counts = take(nb_sets * 4);
    p.o_centres = take(total * 16);
    p.bytes = at;
    return p;
}

}  // namespace

}  // namespace imsegm

extern "C" {

int imsegm_dbscan_points(imsegm_ctx *ctx, const double *points, const int32_t *offsets, int nb_sets, double eps, int min_samples,
                         int32_t *labels_out, int32_t *counts_out, double *centres_out)
{
    if (!offsets || nb_sets < 0 || (nb_sets > 0 && !counts_out)) {
        set_error("dbscan_points: null argument or a negative number of sets");
        return -1;
    }
    if (nb_sets > IMSEGM_DBSCAN_MAX_SETS) return IMSEGM_E_OBJECT_CAPS;
    int n_max = 0;
    for (int s = 0; s < nb_sets; ++s) {
        if (offsets[s] < 0 || offsets[s + 1] < offsets[s]) {
            set_error("dbscan_points: the offsets must start at 0 or above and must not descend");
            return -1;
        }
        n_max = std::max(n_max, offsets[s + 1] - offsets[s]);
    }
    if (n_max > IMSEGM_DBSCAN_MAX_POINTS) return IMSEGM_E_OBJECT_CAPS;
    const size_t first = nb_sets ? (size_t)offsets[0] : 0, total = nb_sets ? (size_t)offsets[nb_sets] : 0;
    if (total > IMSEGM_DBSCAN_MAX_TOTAL) return IMSEGM_E_OBJECT_CAPS;
    if (total > first && (!points || !labels_out || !centres_out)) {
        set_error("dbscan_points: null argument");
        return -1;
    }
    // what scikit-learn answers with a ValueError
    if (!(eps > 0.0) || !std::isfinite(eps) || min_samples < 1) {
        set_error("dbscan_points: eps must be positive and finite, min_samples at least 1");
        return IMSEGM_E_CLUSTER_INPUT;
    }
    for (size_t i = 2 * first; i < 2 * total; ++i)
        if (!std::isfinite(points[i])) {
            set_error("dbscan_points: a coordinate is not finite");
            return IMSEGM_E_CLUSTER_INPUT;
        }
    if (nb_sets == 0) return 0;
    if (total == first) {
        memset(counts_out, 0, (size_t)nb_sets * 4);
        return 0;
    }
    if (bind(ctx)) return -1;
    hipStream_t st = ctx->stream;
    const ClusterPlan p = cluster_plan(total, (size_t)nb_sets);
    if (ctx->gc_buf.ensure(p.bytes)) return -1;
    unsigned char *dev = ctx->gc_buf.as<unsigned char>();
    unsigned char *host = static_cast<unsigned char *>(ctx->stage(p.bytes));
    if (!host) {
        set_error("cannot allocate pinned staging memory");
        return -1;
    }
    // (the rows in front of offsets[0] belong to nobody: they go up as they are and nothing reads them)
    memcpy(host + p.o_points, points, total * 16);
    memcpy(host + p.o_offsets, offsets, ((size_t)nb_sets + 1) * 4);
    HIP_TRY(hipMemcpyAsync(dev, host, p.up_bytes, hipMemcpyHostToDevice, st));
    if (launch_dbscan_points(reinterpret_cast<const double *>(dev + p.o_points), reinterpret_cast<const int32_t *>(dev + p.o_offsets),
                             nb_sets, n_max, eps * eps, min_samples, reinterpret_cast<int32_t *>(dev + p.o_labels),
                             reinterpret_cast<int32_t *>(dev + p.o_counts), reinterpret_cast<double *>(dev + p.o_centres), st))
        return -1;
    HIP_TRY(hipMemcpyAsync(host + p.o_labels, dev + p.o_labels, p.bytes - p.o_labels, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    memcpy(labels_out + first, host + p.o_labels + first * 4, (total - first) * 4);
    memcpy(counts_out, host + p.o_counts, (size_t)nb_sets * 4);
    memcpy(centres_out + 2 * first, host + p.o_centres + first * 16, (total - first) * 16);
    return 0;
}

}  // extern "C"
