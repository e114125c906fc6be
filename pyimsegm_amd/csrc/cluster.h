// cluster.h -- what api_cluster.hip launches from cluster.hip: DBSCAN of many small sets of 2-D points, one workgroup per set
// (experiments_ovary_centres/run_center_clustering.py of the reference: cluster_center_candidates :61-83 -- scikit-learn's
// DBSCAN(eps, min_samples).fit(points).labels_ and np.mean(points[labels == i], axis=0) per cluster)
#pragma once
#include "common.h"

namespace imsegm {

// a set holds at most DBSCAN_MAX_POINTS points (IMSEGM_DBSCAN_MAX_POINTS of include/imsegm_hip.h): 16 bytes of coordinates and three
// words per point in LDS, 112 KB of the 160 KB of a CDNA4 compute unit at the cap
constexpr int DBSCAN_MAX_POINTS = 4096, DBSCAN_THREADS = 1024;

// LDS bytes of the workgroup of a set of up to n_max points
inline size_t dbscan_lds_bytes(int n_max) { return (size_t)n_max * (16 + 3 * 4); }

// points [total][2] (row, col), offsets [nb_sets + 1] into them, eps2 = eps * eps rounded once -> labels [total] (cluster number
// inside the set, -1 noise), counts [nb_sets] (clusters of the set), centres [total][2]: slot offsets[s] + c holds the mean of
// cluster c of set s, the other slots of the set are zeroed.  n_max: the largest set, 1 .. DBSCAN_MAX_POINTS.
int launch_dbscan_points(const double *points, const int32_t *offsets, int nb_sets, int n_max, double eps2, int min_samples,
                         int32_t *labels, int32_t *counts, double *centres, hipStream_t st);

}  // namespace imsegm
