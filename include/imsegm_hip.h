/*
 * imsegm_hip.h -- C ABI of libimsegm_hip.so: the MI355X (gfx950) implementation of pyImSegm's
 * SLIC -> per-superpixel descriptors -> alpha-expansion GraphCut hot path.
 *
 * Conventions: every function returns 0 on success and a negative value on error; the message is
 * available from imsegm_last_error() (thread local).  All host arrays are C-contiguous and owned
 * by the caller; the library never keeps a host pointer past the return of a call.  The HIP
 * runtime is initialised lazily by the first call that needs it (never at load time), so the
 * library is safe to load before a fork() (reference: imsegm/utilities/experiments.py:392-403).
 *
 * Each entry point names the interface of the reference (Borda/pyImSegm @ /root/reference) or of
 * its third-party native dependency that it replaces.
 */
#ifndef IMSEGM_HIP_H
#define IMSEGM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IMSEGM_API __attribute__((visibility("default")))

#define IMSEGM_U8 0
#define IMSEGM_F64 1
#define IMSEGM_F32 2

/* status of imsegm_image2d_segment / imsegm_image2d_graph_prepare when the FUSED form of the back half does not apply to this
 * label map on this device (its adjacency store does not fit the free memory, a label has more neighbours than a row of the
 * neighbour table): nothing is wrong with the session -- the caller builds the graph with imsegm_volume_graph /
 * imsegm_image2d_graph and cuts it with imsegm_cut_general_graph, the staged calls of imsegm/graph_cuts.py:660-747 */
#define IMSEGM_E_FUSED_PATH (-3)

/* status of imsegm_kmeans_lloyd / imsegm_mixture_em for a problem outside the caps of the device fit (more than 16 features, 8
 * components, 16 restarts, 2^31 - 1 rows), and of imsegm_kmeans_lloyd_wide / imsegm_mixture_em_wide outside theirs (fewer than
 * 17 or more than 256 features, 8 components, 16 restarts, 2^31 - 1 rows): nothing is wrong with the context -- the caller
 * fits on the host */
#define IMSEGM_E_FIT_CAPS (-4)

/* status of imsegm_object_shapes for a map it does not take -- more objects than the caller's capacity, or more than two label
 * values that span IMSEGM_OBJECT_SHAPES_MAX_SPAN or more: nothing is wrong with the context and no error message is set -- the
 * caller evaluates the map on the host.  imsegm_cut_objects and the imsegm_center_* / imsegm_correct_segm calls return it in the
 * same sense for a request outside their caps */
#define IMSEGM_E_OBJECT_CAPS (-5)

/* status of imsegm_forest_proba / imsegm_image2d_forest_proba (and of the imsegm_image2d_segment that takes the probabilities of
 * the latter) for a forest or a table they refuse -- a non-finite value in the table (or one that leaves float32's range), more
 * than IMSEGM_FOREST_MAX_CLASSES classes, IMSEGM_FOREST_MAX_FEATURES columns or IMSEGM_FOREST_MAX_TREES trees, a node whose
 * child, feature or leaf row is out of range: nothing is written to the outputs, nothing is wrong with the context -- the
 * caller evaluates the model on the host */
#define IMSEGM_E_FOREST_INPUT (-6)

/* status of imsegm_dbscan_points for the input scikit-learn's DBSCAN answers with a ValueError -- a coordinate that is not finite,
 * eps that is not a positive finite number, min_samples below 1: nothing is written to the outputs, nothing is wrong with the
 * context */
#define IMSEGM_E_CLUSTER_INPUT (-7)

typedef struct imsegm_ctx imsegm_ctx;           /* one device + one stream */
typedef struct imsegm_image2d imsegm_image2d;   /* device-resident state of one H x W image */

IMSEGM_API const char *imsegm_last_error(void);
IMSEGM_API int imsegm_version(void);
IMSEGM_API int imsegm_device_count(int *count_out);
/* PCI address of a device ("0000:c1:00.0", hipDeviceGetPCIBusId): with one process per GPU the host side of a rank belongs on the
 * NUMA node its GPU hangs off -- /sys/bus/pci/devices/<id>/numa_node (pyimsegm_amd.distributed.bind_to_device_numa_node).  The
 * reference's pool workers are not placed (imsegm/utilities/experiments.py:392-403); eight ranks each moving tens of GB/s over
 * the host link are. */
IMSEGM_API int imsegm_device_pci_bus_id(int device, char *id_out, int capacity);
/* free and total bytes of a device's memory right now (hipMemGetInfo): a gray-volume session keeps ~75 bytes per voxel resident
 * (imsegm_volume_*), so how many volumes of BASELINE configs[4] a device holds in flight is asked, not assumed */
IMSEGM_API int imsegm_device_mem_info(int device, size_t *free_bytes_out, size_t *total_bytes_out);
/* Optional, once per process and BEFORE the first call that touches a device: the number of hardware queues the HIP runtime maps
 * the streams of this process onto (the runtime's GPU_MAX_HW_QUEUES, default 4; with one stream per image in flight a fifth
 * stream shares a queue with another one and its kernels wait behind that image's -- bench.py asks for 8).  The runtime reads
 * the setting when it starts: returns 0 when the request was recorded, 1 when it can have no effect any more (this library has
 * already started the runtime) or the user has set GPU_MAX_HW_QUEUES himself (his value wins); nothing is changed then.
 * No reference counterpart (the reference's parallelism is a process pool, imsegm/utilities/experiments.py:392-403). */
IMSEGM_API int imsegm_init(int hardware_queues);
/* Debug / experiment switches (IMSEGM_* environment variables) are read once, at first use; this call reads them again
 * (tests flip them at run time).  No reference counterpart. */
IMSEGM_API void imsegm_debug_reload_env(void);

/* page-locked host memory: images / results living in it travel by DMA, asynchronously to the host (the Python layer
 * hands out numpy arrays backed by it: pyimsegm_amd._hip.pinned_empty) */
IMSEGM_API int imsegm_host_alloc(size_t bytes, void **ptr_out);
IMSEGM_API void imsegm_host_free(void *ptr);

/* plain device buffers and copies for the multi-GPU layer (pyimsegm_amd/distributed.py hands these pointers and the
 * context's stream to RCCL): hipMalloc / hipFree, hipSetDevice for the calling thread, hipMemcpyAsync (any direction)
 * on the context's stream */
IMSEGM_API int imsegm_device_alloc(int device, size_t bytes, void **ptr_out);
IMSEGM_API void imsegm_device_free(void *ptr);
IMSEGM_API int imsegm_set_device(int device);

IMSEGM_API int imsegm_ctx_create(int device, imsegm_ctx **ctx_out);
IMSEGM_API void imsegm_ctx_destroy(imsegm_ctx *ctx);
IMSEGM_API int imsegm_ctx_synchronize(imsegm_ctx *ctx);
IMSEGM_API int imsegm_ctx_stream(imsegm_ctx *ctx, void **hip_stream_out);
IMSEGM_API int imsegm_ctx_copy(imsegm_ctx *ctx, void *dst, const void *src, size_t bytes, int synchronize);

/* HIP-event timing of the kernels launched on the context's stream (bench.py roofline leg).
 * group: 0 = SLIC assignment(+accumulate) kernel, 1 = whole SLIC stage, 2 = connectivity,
 *        3 = colour statistics, 4 = adjacency + centres, 5 = alpha expansion, 6 = gathers,
 *        7 = SLIC pre-processing, 8 = class model + graph-cut terms, 9 = Leung-Malik filter batteries.  Returns accumulated milliseconds and launch
 *        count since reset. */
IMSEGM_API int imsegm_ctx_profile_enable(imsegm_ctx *ctx, int enable);
IMSEGM_API int imsegm_ctx_profile_reset(imsegm_ctx *ctx);
IMSEGM_API int imsegm_ctx_profile_get(imsegm_ctx *ctx, int group, double *total_ms_out, int *count_out);

/* ---------------------------------------------------------------------------------------------
 * device-resident pipeline object (keeps image, Lab planes, label map, ... in HBM between stages)
 * ------------------------------------------------------------------------------------------- */
IMSEGM_API int imsegm_image2d_create(imsegm_ctx *ctx, int height, int width, imsegm_image2d **img_out);
IMSEGM_API void imsegm_image2d_destroy(imsegm_image2d *img);

/* H2D copy of an H x W x 3 interleaved colour image (dtype IMSEGM_U8 / IMSEGM_F32 / IMSEGM_F64).  A page-locked source
 * (imsegm_host_alloc) is copied asynchronously: keep it unchanged until the next synchronising call (imsegm_image2d_slic). */
IMSEGM_API int imsegm_image2d_upload(imsegm_image2d *img, const void *host_pixels, int dtype);

/* Replaces skimage.segmentation.slic(image, n_segments, compactness, sigma, enforce_connectivity=True)
 * as called at imsegm/superpixels.py:61-63, with the min-max scaling of superpixels.py:53-54 folded
 * in (minmax_normalize: 1 = always, 0 = never, 2 = as the reference: unless min == 0 and max == 1).
 * taps_*: half kernels (taps[0] = centre, radius taps follow) of scipy.ndimage.gaussian_filter1d for
 * sigma / spacing per axis; radius < 0 disables the axis, radius > 16 (sigma / spacing > 4) is refused.  max_candidates: 0 = default (debug knob
 * that forces the kernel's global-memory fallback when small).  slic_zero: skimage's slic_zero=True
 * (SLICO, superpixels.py:63 `slic_zero=slico`).  Labels stay on the device. */
IMSEGM_API int imsegm_image2d_slic(imsegm_image2d *img, int minmax_normalize, int n_segments, double compactness,
                        const double *taps_z, int radius_z, const double *taps_y, int radius_y,
                        const double *taps_x, int radius_x, int max_iter, int enforce_connectivity,
                        double min_size_factor, double max_size_factor, int start_label,
                        int max_candidates, int slic_zero, int *n_labels_out);

/* copy the current label map to the host as int64 (dtype leaked by skimage, superpixels.py:69) */
IMSEGM_API int imsegm_image2d_get_labels(imsegm_image2d *img, int64_t *labels_out);
/* install an arbitrary label map (int32, values in [0, n_labels)) -- stage-level entry for the
 * descriptor / graph functions that take a user segmentation.  The range is not checked here (the kernels index per-label
 * tables with the labels): callers check it (pyimsegm_amd._hip.Image2D.set_labels raises ValueError) */
IMSEGM_API int imsegm_image2d_set_labels(imsegm_image2d *img, const int32_t *labels, int n_labels);
/* Diagnostic (no reference counterpart): how many 2-D connectivity passes of this process could not be finished by the
 * tile path of csrc/connectivity.hip and were redone by the general one (results are identical; tests use it to make sure
 * ordinary inputs stay on the fast path). */
IMSEGM_API long imsegm_debug_conn_general_runs(void);
/* Diagnostic (no reference counterpart): which kernels finished the last single-map connectivity pass of this process -- the
 * counters the host reads at the synchronisations it makes anyway (no kernel, copy or synchronisation of its own).  28 ints:
 *   [0]      1 when the 2-D tile path was attempted, [1] 1 when the general path ran, [2] rounds of the general path that
 *            truncated an oversize component (0: none reached max_size), [3] unused
 *   [4..19]  the 16 counters of the tile attempt (csrc/connectivity.hip CNT_*: 0 oversize, 1 small, 3 kept, 4 wave-BFS rejects,
 *            9 a tile beyond its slots, 10 / 11 components handed to the 128 K tile / to the LDS-frontier kernel)
 *   [20..27] the counters of the general path's last tail (0 oversize, 1 small, 3 kept, 4 components the thread BFS took from
 *            the wave kernel, 5 / 6 big / little bounding boxes)
 * The batch entry does not record. */
IMSEGM_API int imsegm_debug_conn_last(int32_t *out28);
/* Diagnostic (no reference counterpart): 2-D SLIC runs of this process whose sweeps 2..max_iter ran in the ONE persistent launch
 * of csrc/slic.hip (k_slic_sweeps), and how many of those gave the image back to the per-sweep launches (results are identical;
 * tests use it to make sure ordinary images stay on the persistent path, bench.py to know how many sweeps one launch covers). */
IMSEGM_API int imsegm_debug_slic_sweep_runs(long *persistent_runs_out, long *fallback_runs_out);
/* Diagnostic (no reference counterpart): graph cuts of this process that the grid-wide kernel (csrc/graphcut.hip
 * k_alpha_expansion_grid) gave up -- a workgroup of its grid was not resident within the bounded wait of its barrier, e.g. on a GPU
 * shared with another process -- and the single workgroup cut again from scratch (results are identical). */
IMSEGM_API long imsegm_debug_gc_grid_fallbacks(void);
/* Diagnostic (no reference counterpart): the one-workgroup exclusive prefix sum that the labelling, graph and compaction stages share
 * (csrc/scan.hip), on n host values: host_out[i] = host_in[0] + ... + host_in[i - 1], *total = the sum of all n (tests). */
IMSEGM_API int imsegm_debug_exclusive_scan(const int32_t *host_in, int n, int32_t *host_out, int32_t *total);
/* Diagnostics (no reference counterpart) for the tests of reused scratch: fill every device allocation the context / the session
 * owns with the 32-bit `word`, over its whole capacity, and put the host-side bookkeeping of the object back to that of a new one
 * (no table of a mixture fit; no image, label map, converted image, filter bank, feature table or prepared graph).  After the call
 * the object differs from a new one only in that its buffers keep their capacity and hold `word`.  *bytes_out = bytes filled.
 * The page-locked staging memory is left alone; batch and region-growing handles own their device memory themselves. */
IMSEGM_API int imsegm_debug_poison_context(imsegm_ctx *ctx, uint32_t word, size_t *bytes_out);
IMSEGM_API int imsegm_debug_image2d_poison(imsegm_image2d *img, uint32_t word, size_t *bytes_out);
/* Replaces skimage.segmentation._slic._enforce_label_connectivity_cython(segments, min_size, max_size, start_label)
 * (scikit-image 0.18; the connectivity pass of skimage.segmentation.slic, reached from imsegm/superpixels.py:61-63 and
 * :104-106 with enforce_connectivity=True) on a label map given by the caller: labels = host int32, one value per
 * pixel (voxel) of the session, raster order, all values >= start_label (skimage's mask label start_label - 1 does not
 * occur in the reference's calls and is not interpreted).  The result becomes the session's label map (imsegm_image2d_get_labels). */
IMSEGM_API int imsegm_image2d_enforce_connectivity(imsegm_image2d *img, const int32_t *labels, long min_size, long max_size,
                                                   int start_label, int *n_labels_out);
/* Replaces the per-pixel Python loop of imsegm/labeling.py:208-247 histogram_regions_labels_counts(slic, segm)
 * (called through histogram_regions_labels_norm at imsegm/pipelines.py:284 to label superpixels from an
 * annotation): hist_out[k * nb_annot + a] = number of pixels with resident label k and annotation a.
 * annot: host int32, one value per pixel (voxel) of the session; values outside [0, nb_annot) are not counted.
 * hist_out: host int64 [n_labels * nb_annot].  Works on image and volume sessions. */
IMSEGM_API int imsegm_image2d_label_hist(imsegm_image2d *img, const int32_t *annot, int nb_annot, int64_t *hist_out);
/* inspection for the parity tests: pre-processed Lab planes [3][H][W] and raw k-means assignment */
IMSEGM_API int imsegm_image2d_get_lab(imsegm_image2d *img, double *lab_out);
IMSEGM_API int imsegm_image2d_get_nearest(imsegm_image2d *img, int32_t *nearest_out);
/* out[3] = { min, max of the uploaded image as the last imsegm_image2d_slic reduced them on the device, max |value| of its
 * pre-processed planes (what fixes the fixed-point format of the centroid sums) } */
IMSEGM_API int imsegm_image2d_get_pre_scalars(imsegm_image2d *img, double out[3]);
/* inspection: the centroid table of the last imsegm_image2d_slic as its last centroid update left it (no update follows the last
 * sweep: after max_iter sweeps this is the table that went INTO sweep max_iter).  centroids_out: *n_centroids_out rows of
 * (cy, cx, cL, ca, cb) float64; windows_out: as many integer search windows (y0, y1, x0, x1), empty (all zero) for a centroid that
 * lost its last pixel, whose row keeps the values it last had.  Both NULL: only the count.  Reads the table, launches nothing. */
IMSEGM_API int imsegm_image2d_get_centroids(imsegm_image2d *img, double *centroids_out, int32_t *windows_out, int *n_centroids_out);

/* Replaces imsegm.features_cython.computeColorImage2dMean / Energy / Variance + normColorFeatures
 * (imsegm/features_cython.pyx:59-141) on the uploaded image and the current label map.
 * Outputs are n_labels x 3 float64 (NULL = not wanted); variance uses the float32-rounded means as
 * descriptors.py:293 does. */
IMSEGM_API int imsegm_image2d_color_stats(imsegm_image2d *img, double *mean_out, double *energy_out, double *var_out);

/* Replaces make_graph_segm_connect_grid2d_conn4 (imsegm/superpixels.py:157-177) and
 * superpixel_centers (superpixels.py:205-242) on the current label map.
 * edges_out: capacity x 2 int32, pairs [a, b] with a < b ordered by (b, a); *n_edges_out receives the
 * real count (may exceed capacity: call again).  centres_out: n_labels x 2 (row, col), -1 for labels
 * without pixels; present_out: n_labels flags (the `vertices` of the reference). */
IMSEGM_API int imsegm_image2d_graph(imsegm_image2d *img, int32_t *edges_out, int edge_capacity, int *n_edges_out,
                         double *centres_out, uint8_t *present_out);

/* Replaces the LUT gathers graph_labels[slic] and proba[slic] (imsegm/pipelines.py:104,109).
 * Either output may be NULL. segm_out: H x W int32; soft_out: H x W x n_classes float64. */
IMSEGM_API int imsegm_image2d_gather(imsegm_image2d *img, const int32_t *graph_labels, const double *proba,
                          int n_classes, int32_t *segm_out, double *soft_out);

/* The whole Leung-Malik statistics of /root/reference/imsegm/descriptors.py:1041-1106 (compute_texture_desc_lm_img2d_clr: per
 * battery the filter responses, the maximum over the orientations, the clip, `response * (log(1 + norm) / 0.03) / norm` with
 * norm = the L2 norm over the three channels, then mean / std / energy per superpixel) in ONE call: the norm of a battery stays on
 * the device, the K x (3 * flags * n_batteries) table comes back once.  weights: the batteries one after the other, each
 * [kx][ky][kernel] with n_kernels[b] in {1, 2, 4, 8} kernels (flipped for a true convolution, last kernel repeated as padding:
 * what imsegm_image2d_lm_battery takes); feature_mask: 1 mean | 2 std | 4 energy, columns per battery in that order, three
 * channels each -- the column order of descriptors.py:1098-1103.  Needs imsegm_image2d_lm_prepare and a label map. */
IMSEGM_API int imsegm_image2d_lm_features(imsegm_image2d *img, const double *weights, const int *n_kernels, int n_batteries, int radius,
                                          double clip, int feature_mask, double *features_out);

/* The same with the separable kernels of the bank taken out of the dense sums: 28 of the 76 Leung-Malik kernels (the Gaussians, both
 * Laplacians of a Gaussian, the edge / bar filters at 0 and 90 degrees; descriptors.py:903-948) are matrices of rank 1 or 2, i.e.
 * sums of one or two products of a column and a row filter.  Battery b: n_kernels[b] dense kernels (0, 1, 2, 4, 6 or 8; laid out
 * as above) plus sep_groups[b] (0..2) separable kernels of sep_rank[b] (1..4) components each; sep_taps holds, battery after
 * battery, kernel after kernel, component after component, the 2 radius + 1 taps along x and then along y of the FLIPPED kernel
 * (the singular value folded into the y taps: K_flipped = sum_i y_i x_i^T).  The response of a battery is the maximum over all its
 * kernels, as before; the factorisation is the caller's (pyimsegm_amd._hip: numpy SVD, components above 1e-13 of the largest).
 * dense_parity[b] (or NULL): +1 / -1 when EVERY dense kernel of battery b is even / odd under the point reflection, K[-p] ==
 * +/- K[p] bit for bit (all bar / edge filters of the bank are) -- the sums are then formed over half the kernel, one addition
 * per pair of pixels serving all kernels of the battery; 0: no symmetry is assumed.  +2 / -2: the n_kernels[b] (2, 4, 6, 8) even /
 * odd kernels of side 33 are, in addition, mirror images of each other in pairs, Kb(dy, dx) = m Ka(dy, -dx) -- the orientations
 * theta and pi - theta of descriptors.py:924-928 -- and the weights block of the battery (still 33 * 33 * n_kernels[b] doubles)
 * holds, from its start, the table [x = 0..16][t = 0..16][WS of the pairs | WD of the pairs] with WS / WD = (Ka[t][16 + x] +/-
 * Ka[t][16 - x]) / 2 of the flipped kernel Ka, row t = 16 halved once more, followed by the signs m of the pairs: two additions and
 * two multiply-adds per four pixels and pair of kernels (csrc/texture.hip k_conv_battery_quad). */
IMSEGM_API int imsegm_image2d_lm_features_sep(imsegm_image2d *img, const double *weights, const int *n_kernels, const int *dense_parity,
                                              const double *sep_taps, const int *sep_groups, const int *sep_rank, int n_batteries,
                                              int radius, double clip, int feature_mask, double *features_out);
/* (features_out NULL, here only: the table stays on the device for imsegm_image2d_segment / imsegm_image2d_get_features and the call
 * returns without waiting for the kernels) */

/* Leung-Malik texture responses (imsegm/descriptors.py:951-1106, scipy.ndimage in the reference).
 * lm_prepare: planes = image - gaussian_filter(image, sigma) with `taps` = half kernel of
 *   scipy.ndimage.gaussian_filter1d(sigma) (taps[0] centre) for the two image axes and `channel_mix`
 *   the 3 x 3 matrix the same filter amounts to along the 3-element channel axis (descriptors.py:1078).
 * lm_battery: one filter battery = n_kernels (1, 2, 4, 8) square kernels of side 2*radius+1; `weights` is
 *   laid out [kx][ky][kernel] and already FLIPPED, i.e. response = max_k correlate(plane, weights[..k]) ==
 *   max_k ndimage.convolve(plane, kernel_k, mode='reflect') (descriptors.py:960-963), clipped at `clip`
 *   (:1088); returns the sum of squares over the three channels (for the norm of :1090).
 * response_stats: per-superpixel mean / energy / variance of (response * mul) / div (:1094-1096),
 *   float32 staging as imsegm_image2d_color_stats. */
IMSEGM_API int imsegm_image2d_lm_prepare(imsegm_image2d *img, const double *taps, int radius, const double *channel_mix);
IMSEGM_API int imsegm_image2d_lm_battery(imsegm_image2d *img, const double *weights, int n_kernels, int radius,
                                         double clip, double *sum_squares_out);
IMSEGM_API int imsegm_image2d_response_stats(imsegm_image2d *img, double mul, double div, double *mean_out,
                                             double *energy_out, double *var_out);
/* response_median / response_mean_gradient: per superpixel (K x 3; a volume: K) the median of (response * mul) / div (NaN for
 *   a label without pixels) and the mean of np.sum(np.gradient(plane), axis=0) of that normalised response per channel plane
 *   (a volume: per slice), float32 staging as the other means -- the 'median' / 'meanGrad' columns of :1096 on the device.
 *   mul >= 0, div > 0; the gradient needs H, W >= 2.  Neither changes the prepared planes, the response, the uploaded image,
 *   the resident feature table or a prepared graph: the next lm_battery runs without another lm_prepare.
 *   response_mean_gradient: div must be at least the largest magnitude of the response (the L2 norm that lm_battery returns
 *   is) -- the fixed-point scale of the mean is taken from mul (|gradient sum| <= 4 mul), not from a min / max pass. */
IMSEGM_API int imsegm_image2d_response_median(imsegm_image2d *img, double mul, double div, double *median_out);
IMSEGM_API int imsegm_image2d_response_mean_gradient(imsegm_image2d *img, double mul, double div, double *mean_out);
/* inspection for the parity tests: the current filter response as [3][H][W] planes */
IMSEGM_API int imsegm_image2d_get_response(imsegm_image2d *img, double *planes_out);

/* ---------------------------------------------------------------------------------------------
 * gray volumes D x H x W (the session type is shared; get_labels / set_labels / gather work on it)
 * ------------------------------------------------------------------------------------------- */
IMSEGM_API int imsegm_volume_create(imsegm_ctx *ctx, int depth, int height, int width, imsegm_image2d **vol_out);
/* The descriptors read the voxels as uploaded (float32 staging of features_cython.pyx); SLIC reads
 * (v + slic_offset) * slic_scale, the affine form of skimage.util.img_as_float for the source dtype
 * (uint8: 0, 1/255; floats: 0, 1). */
IMSEGM_API int imsegm_volume_upload(imsegm_image2d *vol, const void *host_voxels, int dtype, double slic_offset,
                                    double slic_scale);
/* Replaces skimage.segmentation.slic(im, n_segments, compactness, multichannel=False, spacing=space,
 * sigma=1) as called at imsegm/superpixels.py:104-106: gray supervoxels, anisotropic spacing[3] (z, y, x);
 * taps_* are the half kernels for sigma / spacing per axis. */
IMSEGM_API int imsegm_volume_slic(imsegm_image2d *vol, int n_segments, double compactness, const double *taps_z,
                                  int radius_z, const double *taps_y, int radius_y, const double *taps_x, int radius_x,
                                  const double *spacing, int max_iter, int enforce_connectivity, double min_size_factor,
                                  double max_size_factor, int start_label, int *n_labels_out);
/* inspection for the parity tests: the state of the last imsegm_volume_slic (an error before the first one).
 * get_pre: the pre-processed plane [D][H][W] in the type the SLIC kernels read it -- *dtype_out = IMSEGM_F32 for a float32 volume,
 *   IMSEGM_F64 for every other -- and, for the latter, *premax_out = max |value| of the plane as the device reduced it (what fixes the
 *   fixed-point format of the centroid sums; 0 for a float32 volume, which has none).  plane_out NULL: only the type is reported.
 * get_centroids: the centroid table, *n_centroids_out rows of (z, y, x, value) in the same type.  centroids_out NULL: only type and
 *   count.  The table is what the last centroid UPDATE left: max_iter sweeps are followed by max_iter - 1 updates. */
IMSEGM_API int imsegm_volume_get_pre(imsegm_image2d *vol, void *plane_out, int *dtype_out, double *premax_out);
IMSEGM_API int imsegm_volume_get_centroids(imsegm_image2d *vol, void *centroids_out, int *dtype_out, int *n_centroids_out);
/* Replaces skimage.measure.label(segments) (imsegm/superpixels.py:111): components of equal non-zero
 * value under full connectivity, numbered 1.. in raster order of their first voxel; 0 stays background.
 * (On the map imsegm_volume_slic has just written with enforce_connectivity -- every value > 0 one connected set -- this is a
 * renumbering by first voxels and is computed as one; any other map goes through the union-find.  Same result either way.) */
IMSEGM_API int imsegm_volume_label_cc(imsegm_image2d *vol, int *n_labels_out);
/* Replaces imsegm.features_cython.computeGrayImage3dMean / Energy / Variance (features_cython.pyx:144-219);
 * outputs n_labels float64 each (NULL = not wanted). */
IMSEGM_API int imsegm_volume_gray_stats(imsegm_image2d *vol, double *mean_out, double *energy_out, double *var_out);
/* Replaces make_graph_segm_connect_grid3d_conn6 and the 3-D branch of superpixel_centers
 * (imsegm/superpixels.py:180-242); centres_out is n_labels x 3 (z, y, x). */
IMSEGM_API int imsegm_volume_graph(imsegm_image2d *vol, int32_t *edges_out, int edge_capacity, int *n_edges_out,
                                   double *centres_out, uint8_t *present_out);

/* ---------------------------------------------------------------------------------------------
 * fused back half of the pipeline (no host round trip between the stages)
 * ------------------------------------------------------------------------------------------- */
/* Per-superpixel feature table of compute_image2d_color_statistic / compute_image3d_gray_statistic
 * (imsegm/descriptors.py:705-863) for the flags mean (1) | std (2) | energy (4): columns ordered mean, std, energy,
 * three columns each (colour channels; a gray volume repeats its single channel), NaN -> 0, -0 -> +0.  The table
 * stays resident for imsegm_image2d_segment; features_out (n_labels x 3*nflags float64) may be NULL. */
IMSEGM_API int imsegm_image2d_features_color(imsegm_image2d *img, int feature_mask, double *features_out);

/* The feature table of SEVERAL descriptor groups side by side, as compute_selected_features_color2d concatenates them
 * (imsegm/descriptors.py:1207-1270: the 'color' statistics, then the 'tLM' ones): the NEXT call of
 * imsegm_image2d_features_color / imsegm_image2d_lm_features_sep (with features_out NULL) writes its columns at `column` of a
 * resident table `total_columns` wide instead of a table of its own.  imsegm_image2d_segment evaluates the class model on that
 * table (F <= 256); the host reads it with imsegm_image2d_get_features (capacity_columns = its width, as a check). */
IMSEGM_API int imsegm_image2d_features_place(imsegm_image2d *img, int total_columns, int column);
IMSEGM_API int imsegm_image2d_get_features(imsegm_image2d *img, double *features_out, int capacity_columns);

/* class model evaluated on the device: sklearn Pipeline([StandardScaler,] [PCA,] mixture) as
 * imsegm.graph_cuts.estim_class_model builds it (imsegm/graph_cuts.py:73-163), the mixture a GaussianMixture or a
 * BayesianGaussianMixture with covariance_type='full'.  The host passes what scikit-learn itself precomputes per model (not
 * per sample); the per-component constants of the Bayesian mixture are folded into log_det and log_weights.
 * n_features (F) is the dimension the mixture works in.  Without a PCA (n_inputs 0) it is also the width of the feature table.
 * With one (version >= 101) the table is n_inputs (I) columns wide, 1 <= F <= I <= 256, the scaler vectors are [I] long, and a
 * row x becomes (x @ pca_components_t - pca_shift) / pca_scale before the mixture sees it.  A zero-initialised tail behind
 * const_term is the model without a PCA. */
typedef struct {
    int n_features, n_classes;
    const double *scaler_mean;    /* [F] ([I] with a PCA) StandardScaler.mean_ or NULL */
    const double *scaler_scale;   /* [F] ([I] with a PCA) StandardScaler.scale_ or NULL */
    const double *prec_chol;      /* [C][F][F] precisions_cholesky_ */
    const double *mu_proj;        /* [C][F]   means_[c] @ precisions_cholesky_[c] */
    const double *log_det;        /* [C]      _compute_log_det_cholesky (+ the Bayesian mixture's constants) */
    const double *log_weights;    /* [C]      log(weights_) (Bayesian mixture: _estimate_log_weights) */
    double const_term;            /* n_features * log(2 pi) */
    int n_inputs;                 /* columns of the feature table the model reads; 0: n_features, no projection */
    const double *pca_components_t;   /* [I][F] PCA.components_.T, contiguous */
    const double *pca_shift;      /* [F] PCA.mean_ @ components_.T */
    const double *pca_scale;      /* [F] sqrt(explained_variance_) clipped at eps (whiten=True) or NULL */
} imsegm_gmm;

/* edge types of imsegm.graph_cuts.compute_edge_weights (imsegm/graph_cuts.py:574-657); `| IMSEGM_EDGE_SPATIAL_NORM`
 * divides the weights by the relative distance of the superpixel centres (:647-650: 'model', 'features', 'spatial') */
#define IMSEGM_EDGE_CONST 0
#define IMSEGM_EDGE_SPATIAL 1
#define IMSEGM_EDGE_MODEL_LT 2
#define IMSEGM_EDGE_MODEL_L1 3
#define IMSEGM_EDGE_MODEL_L2 4
#define IMSEGM_EDGE_FEATURES 5
#define IMSEGM_EDGE_SPATIAL_NORM 0x100

/* optional inspection outputs of imsegm_image2d_segment (parity tests, debug_visual): NULL pointers are skipped */
typedef struct {
    int edge_capacity;            /* in: rows of edges / edge_weights / edge_weights_int */
    int n_edges;                  /* out */
    int32_t *edges;               /* E x 2, a < b, ordered by (b, a) */
    double *edge_weights;         /* E, after clipping and edge_cost */
    int32_t *edge_weights_int;    /* E, the pyGCO integers */
    double *unary;                /* K x C */
    int32_t *unary_int;           /* K x C */
    double *centres;              /* K x ndim */
    int64_t *energy;              /* final integer energy of the expansion */
    int keep_soft_on_device;      /* in: compute proba[slic] into the session's buffer even when soft_out is NULL */
    /* in: narrow result formats (NOT the reference's dtypes -- explicit opt-in of the caller, SURVEY section 8f row 3: the
     * 100 MB float64 soft segmentation / the int32 class map dominate the device-to-host time once the kernels are fast) */
    int segm_u8;                  /* segm_out points to uint8 (height x width), classes must be < 256 */
    int soft_f32;                 /* soft_out points to float32 (height x width x n_classes) */
} imsegm_terms_debug;

/* Replaces, on the resident label map (and feature table): model.predict_proba (gmm != NULL; else `proba`, K x C, comes
 * from the host), compute_unary_cost, compute_edge_weights, compute_pairwise_cost's result `pairwise` (C x C, host),
 * gco.cut_general_graph(..., algorithm='expansion', n_iter=-1) (use_graphcut = 0: argmin of the unary cost,
 * graph_cuts.py:729-731), classes_[graph_labels] (classes_lut, may be NULL) and the gathers graph_labels[slic],
 * proba[slic] (imsegm/graph_cuts.py:660-747, imsegm/pipelines.py:96-109,232-240).  One stream, one synchronisation at
 * the end.  Outputs (each may be NULL): segm_out H x W int32, soft_out H x W x C float64, graph_labels_out K int32
 * (before classes_lut), proba_out K x C.  With gmm == NULL and proba == NULL (version >= 102) the probabilities are those the last
 * imsegm_image2d_forest_proba left on the device for this label map and feature table; without them the call fails as before. */
IMSEGM_API int imsegm_image2d_segment(imsegm_image2d *img, const imsegm_gmm *gmm, const double *proba, int n_classes,
                                      const double *pairwise, int edge_type, double edge_cost, int use_graphcut,
                                      const int32_t *classes_lut, int32_t *segm_out, double *soft_out,
                                      int32_t *graph_labels_out, double *proba_out, imsegm_terms_debug *debug_out);

/* The part of imsegm_image2d_segment that depends on the label map alone -- make_graph_segm_connect_grid2d_conn4 / 3d_conn6 and
 * superpixel_centers (imsegm/superpixels.py:115-242) as edges, centres and the arcs the cut walks -- enqueued AHEAD of it and
 * without a synchronisation: the next imsegm_image2d_segment on the same label map finds the graph ready.  The gray-volume
 * pipeline fits its class model on the host between the descriptors and the cut (imsegm/pipelines.py:412-421); the graph is
 * built under that fit.  Any call that changes the label map drops the prepared graph.  May return IMSEGM_E_FUSED_PATH. */
IMSEGM_API int imsegm_image2d_graph_prepare(imsegm_image2d *img);

/* segment_color2d_slic_features_model_graphcut (imsegm/pipelines.py:160-241) for a colour image, colour statistics and a
 * mixture model the device evaluates, in ONE call: imsegm_image2d_upload + imsegm_image2d_slic (isotropic `taps`,
 * connectivity enforced with skimage's 0.5 / 3 size factors) + imsegm_image2d_features_color + imsegm_image2d_segment. */
IMSEGM_API int imsegm_image2d_run_color(imsegm_image2d *img, const void *host_pixels, int dtype, int minmax_normalize,
                                        int n_segments, double compactness, const double *taps, int radius, int max_iter,
                                        int start_label, int slic_zero, int feature_mask, const imsegm_gmm *gmm,
                                        int n_classes, const double *pairwise, int edge_type, double edge_cost,
                                        int use_graphcut, const int32_t *classes_lut, int32_t *segm_out, double *soft_out,
                                        int *n_labels_out);

/* ---------------------------------------------------------------------------------------------
 * several images of ONE size per launch chain
 * ------------------------------------------------------------------------------------------- */
/* Replaces the pool map of the reference's experiment driver over the images of a batch
 * (/root/reference/experiments_segmentation/run_segm_slic_model_graphcut.py:451-473 and :505-514 `segment_image_model` mapped through
 * imsegm/utilities/experiments.py:392-403 WrapExecuteSequence): up to `max_images` images of height x width go through
 * segment_color2d_slic_features_model_graphcut (imsegm/pipelines.py:160-241) TOGETHER -- every kernel of the chain is launched once
 * for the batch (image = blockIdx.z), with two host synchronisations per batch instead of two per image.  Results are those of
 * imsegm_image2d_run_color image by image, bit for bit. */
typedef struct imsegm_batch2d imsegm_batch2d;
IMSEGM_API int imsegm_batch2d_create(imsegm_ctx *ctx, int max_images, int height, int width, imsegm_batch2d **batch_out);
IMSEGM_API void imsegm_batch2d_destroy(imsegm_batch2d *batch);
/* host_pixels[i]: H x W x 3 interleaved image i (all of `dtype`); segm_out[i]: H x W int32 (a null entry, or segm_out == NULL:
 * that map stays on the device, imsegm_batch2d_device_ptr); n_labels_out: n_images superpixel counts or NULL.  Arguments as
 * imsegm_image2d_run_color; SLICO, a blur radius above 8 and host-evaluated class models take the single-image calls (an
 * error here, not a fallback). */
IMSEGM_API int imsegm_batch2d_run_color(imsegm_batch2d *batch, int n_images, const void *const *host_pixels, int dtype,
                                        int minmax_normalize, int n_segments, double compactness, const double *taps, int radius,
                                        int max_iter, int start_label, int feature_mask, const imsegm_gmm *gmm, int n_classes,
                                        const double *pairwise, int edge_type, double edge_cost, int use_graphcut,
                                        const int32_t *classes_lut, int32_t *const *segm_out, int *n_labels_out);
/* device address of a result of image `image` of the last batch: which = 0 label map, 1 segmentation (int32 H x W each),
 * 2 feature table (float64, n_labels_out[image] rows of 3 x (number of feature_mask bits) columns: mean | std | energy),
 * 3 the pre-processed planes SLIC ran on (float64 3 x H x W), 4 {min, max} of the image and the largest |value| of those planes
 * (three float64) */
IMSEGM_API int imsegm_batch2d_device_ptr(imsegm_batch2d *batch, int image, int which, void **ptr_out);

/* The 'median' and 'meanGrad' statistics of compute_image2d_color_statistic / compute_image3d_gray_statistic
 * (imsegm/descriptors.py:420-455, 671-702, 766-770, 841-845) on the resident image (K x 3) or volume (K):
 * median of the pixel values per label and channel (NaN for labels without pixels, as np.median of an empty list);
 * mean over the label of np.sum(np.gradient(slice), axis=0) stored in the image's dtype (float32 staging as the other
 * means).  Both invalidate a prepared Leung-Malik state (they borrow its buffers). */
IMSEGM_API int imsegm_image2d_median(imsegm_image2d *img, double *median_out);
IMSEGM_API int imsegm_image2d_mean_gradient(imsegm_image2d *img, double *mean_out);

/* The uploaded RGB image in another colour space, converted on the device as pyimsegm_amd/utilities/data_io.py states the
 * conversions (skimage.color.rgb2hsv / rgb2luv / rgb2lab / rgb2hed / rgb2xyz of scikit-image 0.18 behind
 * imsegm/utilities/data_io.py:28-58), NaN / inf replaced as np.nan_to_num does: a float64 interleaved H x W x 3 image in a
 * buffer of the session.  space: 1 hsv, 2 luv, 3 lab, 4 hed, 5 xyz; matrix9: the row-major 3 x 3 stain matrix of hed
 * (out = log-ratio @ matrix; NULL for the other spaces).  Enqueued on the session's stream, no synchronisation.
 * From then on imsegm_image2d_color_stats, _features_color, _median and _mean_gradient read the CONVERTED image -- until a
 * call with space 0 (which converts nothing) or the next upload; every other call (slic, lm_prepare, ...) keeps reading the
 * upload.  Refused before the device is touched: no upload, a volume session, an unknown space, hed without a matrix. */
IMSEGM_API int imsegm_image2d_convert_color(imsegm_image2d *img, int space, const double *matrix9);
/* the converted image (H x W x 3 float64) to the host; one synchronisation */
IMSEGM_API int imsegm_image2d_get_converted(imsegm_image2d *img, double *out_hw3);

/* 1 when the uploaded image / volume holds no NaN and no inf (uint8: always).  The pipelines replace non-finite descriptor
 * values by zero (/root/reference/imsegm/pipelines.py:410 `features[np.isnan(features)] = 0`, descriptors.py:818), which the
 * resident statistics cannot reproduce from non-finite pixels: the host mirror asks before it takes the resident path (a
 * float64 sum over 10^9 voxels on the host costs more than the whole supervoxel stage). */
IMSEGM_API int imsegm_image2d_all_finite(imsegm_image2d *img, int *all_finite_out);

/* Device address of a result buffer of the session (valid until the next call that rewrites it):
 * which = 0: label map int32 H x W; 1: gathered segmentation int32 H x W; 2: gathered soft
 * segmentation float64 H x W x C; 3: resident feature table float64 n_labels x F, F as the last descriptor
 * call (or its imsegm_image2d_features_place) laid it out -- an error while no table exists.  A caller may
 * overwrite the n_labels x F values of the table (a class model is then evaluated on the caller's features).
 * For zero-copy hand-over to a collective library (RCCL) running on the same HIP runtime; call
 * imsegm_ctx_synchronize first. */
IMSEGM_API int imsegm_image2d_device_ptr(imsegm_image2d *img, int which, void **ptr_out);

/* ---------------------------------------------------------------------------------------------
 * stand-alone stages
 * ------------------------------------------------------------------------------------------- */
/* Replaces imsegm.labeling.assume_bg_on_boundary(segm, bg_label, boundary_size) for 2-D label images
 * (/root/reference/imsegm/labeling.py:719-753; called by the driver right after the pipeline,
 * experiments_segmentation/run_segm_slic_model_graphcut.py:373,422) including the border statistics of
 * imsegm.utilities.data_io.get_image2d_boundary_color (utilities/data_io.py:1025-1027: np.bincount over the four border
 * strips `image[:size, :], image[:, :size].T, image[-size:, :], image[:, -size:].T`, argmax = lowest label on ties).
 * segm_inout: host int32, height x width, non-negative on the border; strips: the four slices as {row0, row1, col0, col1}
 * (the caller resolves numpy's slice semantics); the label that dominates the border and `bg_label` are exchanged in place.
 * Returns < 0 with "negative label" when np.bincount would raise. */
IMSEGM_API int imsegm_assume_bg_on_boundary(imsegm_ctx *ctx, int32_t *segm_inout, int height, int width, const int32_t strips[16],
                                            int bg_label, int *boundary_label_out);

/* Replaces imsegm.features_cython.computeLabelHistogram2d (imsegm/features_cython.pyx:222-241; called per position through
 * descriptors.py:1411-1495 compute_label_hist_segm / cython_label_hist_seg2d) for a BATCH of windows of one label image:
 * window p = segm[y0 : y0 + h, x0 : x0 + w] against struc_elem[sy0 : sy0 + h, sx0 : sx0 + w], windows[p] = {y0, x0, h, w, sy0,
 * sx0}; hist_out[p][l] = pixels with label l (0 <= l < nb_labels) where the structuring element equals 1. */
IMSEGM_API int imsegm_label_hist2d(imsegm_ctx *ctx, const int16_t *segm, int height, int width, const int32_t *windows,
                                   int n_windows, const int16_t *struc_elem, int se_height, int se_width, int nb_labels,
                                   uint32_t *hist_out);
/* Replaces imsegm.features_cython.computeRayFeaturesBinary2d (features_cython.pyx:244-282; descriptors.py:1630-1660
 * cython_ray_features_seg2d) for a BATCH of positions (row, col): directions[a] = (sin, cos) of angle a divided by the
 * larger of their magnitudes, float32, formed by the caller as the .pyx forms them; edge 1 = 'up', -1 = 'down';
 * ray_dist_out[p][a] = distance to the edge along ray a, -1 if none (0 for every ray when 'up' starts inside). */
IMSEGM_API int imsegm_ray_features_binary2d(imsegm_ctx *ctx, const int8_t *seg_binary, int height, int width,
                                            const int32_t *positions, int n_positions, const float *directions, int n_angles,
                                            int edge, float *ray_dist_out);

/* ---------------------------------------------------------------------------------------------
 * centre-candidate point descriptors: one launch for all positions (row, col) of a map
 * ------------------------------------------------------------------------------------------- */
#define IMSEGM_RING_MAX_BINS 32            /* imsegm_ring_hist2d: n_radii * (nb_labels + 1) counters per lane fit the LDS budget */
#define IMSEGM_RING_PROBA_MAX_DISCS 16     /* imsegm_ring_hist_proba2d: n_radii sums per lane fit the LDS budget */
#define IMSEGM_RAY_MAX_ANGLES 4096
#define IMSEGM_RAY_MAX_BORDER_LABELS 64
/* Replaces the loops over positions and discs of imsegm.descriptors.compute_label_histograms_positions for label maps
 * (imsegm/descriptors.py:1288-1369: per position and disc one compute_label_hist_segm :1413-1459 = adjust_bounding_box_crop
 * :1372-1410 + computeLabelHistogram2d + np.sum(struc_elem)).  Disc d is skimage.morphology.disk(radii[d]), dy^2 + dx^2 <=
 * radii[d]^2, clipped to the map; radii grow strictly, positions lie inside the map, n_radii * (nb_labels + 1) <=
 * IMSEGM_RING_MAX_BINS.  hist_out[p][d][l] = pixels with label l (0 <= l < nb_labels) under disc d around position p;
 * size_out[p][d] = pixels under the clipped disc whatever their label (the reference's sel_size).  Exact integers. */
IMSEGM_API int imsegm_ring_hist2d(imsegm_ctx *ctx, const int16_t *segm, int height, int width, const int32_t *positions,
                                  int n_positions, const int32_t *radii, int n_radii, int nb_labels, uint32_t *hist_out,
                                  uint32_t *size_out);
/* Replaces imsegm.descriptors.compute_label_hist_proba (descriptors.py:1498-1528) under the same loops (:1343-1363) for
 * probability layers proba[height][width][n_layers] (float64): sum_out[p][d][c] = sum of layer c under disc d, float64 in a fixed
 * order (two calls give the same bits), size_out[p][d] as above; n_radii <= IMSEGM_RING_PROBA_MAX_DISCS. */
IMSEGM_API int imsegm_ring_hist_proba2d(imsegm_ctx *ctx, const double *proba, int height, int width, int n_layers,
                                        const int32_t *positions, int n_positions, const int32_t *radii, int n_radii,
                                        double *sum_out, uint32_t *size_out);
/* Replaces the mask and the loop over positions of imsegm.descriptors.compute_ray_features_positions (descriptors.py:1869-1886:
 * seg_binary[segm == lb] = True for every border label, then per position compute_ray_features_segm_2d :1715-1758 =
 * computeRayFeaturesBinary2d + scipy.ndimage.gaussian_filter1d).  segm: host int32; the mask is formed on the device from
 * border_labels; directions and edge as imsegm_ray_features_binary2d.  smooth_taps: NULL (no smoothing) or smooth_radius + 1
 * weights of gaussian_filter1d's kernel from its centre outwards; the row of a position is filtered along the angle with
 * boundary mode 'reflect', float64 sums in scipy's order, and stored as float32. */
IMSEGM_API int imsegm_ray_features_labels2d(imsegm_ctx *ctx, const int32_t *segm, int height, int width, const int32_t *border_labels,
                                            int n_border, const int32_t *positions, int n_positions, const float *directions,
                                            int n_angles, int edge, const double *smooth_taps, int smooth_radius,
                                            float *ray_dist_out);

/* ---------------------------------------------------------------------------------------------
 * scoring label maps (imsegm/labeling.py): boundary masks, exact Euclidean distance maps, boundary distances, label overlaps.
 * Label maps are host int32, height x width, raster order.  Integer arithmetic up to one correctly rounded fp64 square root per
 * value: same bits as scipy.ndimage.distance_transform_edt on the same mask.  Squared distances are held in 32 bits: maps with
 * height^2 + width^2 > 2^32 - 1 (or more than 65535 rows) are refused with an error.
 * ------------------------------------------------------------------------------------------- */
#define IMSEGM_BOUNDARY_THICK 0            /* skimage.segmentation.find_boundaries(mode='thick'): a 4-neighbour inside the image differs */
#define IMSEGM_BOUNDARY_CONTOUR 1          /* labeling.py:59-66: interior pixels that carry `label` with a 4-neighbour that does not */
#define IMSEGM_BOUNDARY_CONTOUR_BORDER 2   /* labeling.py:59-77 include_boundary=True: plus the border pixels that carry `label` */
/* Replaces the per-pixel Python loops of imsegm/labeling.py:34-79 contour_binary_map(seg, label, include_boundary) (modes 1, 2;
 * also the points of contour_coords :82-117 in row-major order) and skimage.segmentation.find_boundaries(seg, mode='thick')
 * as called at labeling.py:708,710 (mode 0, `label` unused).  mask_out: host uint8, 1 on the boundary. */
IMSEGM_API int imsegm_boundary_mask(imsegm_ctx *ctx, const int32_t *labels, int height, int width, int mode, int label,
                                    uint8_t *mask_out);
/* Replaces imsegm/labeling.py:146-169 compute_distance_map(seg, label) (mode 1: contour_coords, binary_image_from_coords and
 * scipy.ndimage.distance_transform_edt of the complement) and, with mode 0, the distance map of labeling.py:710-711.
 * dist_out: host float64, distance of every pixel to the nearest mask pixel.  A map without a mask pixel gives what scipy gives:
 * the distance to (row -1, column 0). */
IMSEGM_API int imsegm_distance_map(imsegm_ctx *ctx, const int32_t *labels, int height, int width, int mode, int label,
                                   double *dist_out);
/* Replaces imsegm/labeling.py:684-716 compute_boundary_distances(segm_ref, segm) (the superpixel measure of
 * experiments_segmentation/run_eval_superpixels.py:108-131): the pixels of the thick boundary of segm_ref in row-major order as
 * points_out[2 i] = row, points_out[2 i + 1] = column, and dist_out[i] = their distance to the thick boundary of segm.  Only the
 * points travel back, never a height x width map.  *n_points_out = number of points (0: segm_ref has no boundary); more points
 * than `capacity` (entries of dist_out, pairs of points_out) is an error that still reports the number. */
IMSEGM_API int imsegm_boundary_distances(imsegm_ctx *ctx, const int32_t *segm_ref, const int32_t *segm, int height, int width,
                                         int32_t *points_out, double *dist_out, int capacity, int *n_points_out);
/* The same against the label map a 2-D session holds (from imsegm_image2d_slic or imsegm_image2d_set_labels) as `segm`: only
 * segm_ref is uploaded. */
IMSEGM_API int imsegm_image2d_boundary_distances(imsegm_image2d *img, const int32_t *segm_ref, int32_t *points_out, double *dist_out,
                                                 int capacity, int *n_points_out);
/* The same on label volumes: host int32, depth x height x width, raster order, thick boundaries only.  Volumes with
 * depth^2 + height^2 + width^2 > 2^32 - 1 or more than 2^30 voxels are refused with an error before anything is launched.
 * Replaces skimage.segmentation.find_boundaries(segm, mode='thick') as imsegm/labeling.py:708,710 calls it on a 3-D map: mask_out
 * is host uint8, 1 where a neighbour along z, y or x inside the volume carries another label. */
IMSEGM_API int imsegm_boundary_mask3d(imsegm_ctx *ctx, const int32_t *labels, int depth, int height, int width, uint8_t *mask_out);
/* Replaces the distance map of imsegm/labeling.py:710-711 (find_boundaries and scipy.ndimage.distance_transform_edt of the
 * complement) on a 3-D map.  dist_out: host float64, distance of every voxel to the nearest mask voxel.  A volume without a mask
 * voxel gives what scipy gives: the distance to (slice -1, row 0, column 0). */
IMSEGM_API int imsegm_distance_map3d(imsegm_ctx *ctx, const int32_t *labels, int depth, int height, int width, double *dist_out);
/* Replaces imsegm/labeling.py:684-716 compute_boundary_distances(segm_ref, segm) on 3-D maps: the voxels of the thick boundary of
 * segm_ref in raster order as points_out[3 i] = slice, [3 i + 1] = row, [3 i + 2] = column, and dist_out[i] = their distance to the
 * thick boundary of segm.  Only the points travel back.  `capacity` and *n_points_out as in imsegm_boundary_distances: more points
 * than `capacity` (entries of dist_out, triples of points_out) is an error that still reports the number. */
IMSEGM_API int imsegm_boundary_distances3d(imsegm_ctx *ctx, const int32_t *segm_ref, const int32_t *segm, int depth, int height,
                                           int width, int32_t *points_out, double *dist_out, int capacity, int *n_points_out);
/* The same against the label map a volume session holds (from imsegm_volume_slic or imsegm_volume_label_cc) as `segm`: only
 * segm_ref is uploaded. */
IMSEGM_API int imsegm_volume_boundary_distances(imsegm_image2d *vol, const int32_t *segm_ref, int32_t *points_out, double *dist_out,
                                                int capacity, int *n_points_out);
/* Replaces the per-pixel Python loop of imsegm/labeling.py:490-523 compute_labels_overlap_matrix(seg1, seg2) (and the matrix
 * relabel_max_overlap_unique :583 and relabel_max_overlap_merge :664 start from): overlap_out[a * n_labels2 + b] = number of
 * positions i < n with seg1[i] == a and seg2[i] == b; pairs with a negative label (or one beyond its extent) are skipped.
 * overlap_out: host int64 [n_labels1 * n_labels2], at most 2^28 entries. */
IMSEGM_API int imsegm_labels_overlap(imsegm_ctx *ctx, const int32_t *seg1, const int32_t *seg2, size_t n, int n_labels1,
                                     int n_labels2, int64_t *overlap_out);

/* Replaces gco.cut_general_graph(edges, edge_weights, unary_cost, pairwise_cost, n_iter,
 * algorithm='expansion') (gco-wrapper >= 3.0.8) as called at imsegm/graph_cuts.py:735-744.
 * edges: E x 2 int32 with edges[:,0] < edges[:,1]; edge_weights: E; unary: K x C; pairwise: C x C
 * symmetric.  Float costs are converted to integer energies exactly as pyGCO does.
 * Limits (an error, not a fallback): C <= 64 labels; n_iter < 0 = until convergence. */
IMSEGM_API int imsegm_cut_general_graph(imsegm_ctx *ctx, const int32_t *edges, int n_edges, const double *edge_weights,
                             const double *unary_cost, int n_sites, int n_labels, const double *pairwise_cost,
                             int n_iter, int32_t *labels_out, int64_t *energy_out);
/* imsegm_cut_general_graph with pyGCO's scaling maximum of |edge_weights| stated by the caller: weight_max >= 0 enters the
 * maximum next to the weights of the edges handed over, weight_max < 0 is imsegm_cut_general_graph itself.  For callers that drop
 * edges joining a site with itself (imsegm/region_growing.py:117-122 sets the edges at a seed to (0, 0)): such an edge adds nothing
 * to any labelling, but pyGCO takes its maximum over all weights before GCO sees an edge. */
IMSEGM_API int imsegm_cut_general_graph_scaled(imsegm_ctx *ctx, const int32_t *edges, int n_edges, const double *edge_weights,
                                               const double *unary_cost, int n_sites, int n_labels, const double *pairwise_cost,
                                               double weight_max, int n_iter, int32_t *labels_out, int64_t *energy_out);
/* (tests) The arcs the grid entries build on the device for a height x width grid: edges E x 2, arc_start height * width + 1,
 * arc_to 2 E, arc_rev 2 E, edge_arc E x 2, E = (height - 1) * width + height * (width - 1); the arrays the host loop of
 * imsegm_cut_general_graph builds for pyGCO's edge list of that grid. */
IMSEGM_API int imsegm_debug_grid_arcs(imsegm_ctx *ctx, int height, int width, int32_t *edges_out, int32_t *arc_start_out,
                                      int32_t *arc_to_out, int32_t *arc_rev_out, int32_t *edge_arc_out);
/* Replaces gco.cut_grid_graph(unary_cost, pairwise_cost, cost_v, cost_h, n_iter, algorithm='expansion') as called at
 * imsegm/region_growing.py:246-248: the 4-connected height x width grid, unary height x width x n_labels, cost_v (height - 1) x
 * width, cost_h height x (width - 1), pairwise n_labels x n_labels symmetric -- gco's own float arguments.  The float costs go up
 * as they are; pyGCO's down-weight factor, its truncation to integers and the arcs of the grid (pyGCO's edge order: all vertical
 * edges row-major, then the horizontal ones) are computed on the device.  Labels and energy are those of imsegm_cut_general_graph
 * on the same graph.  Limits as there, and height * width <= 2^29. */
IMSEGM_API int imsegm_cut_grid_graph(imsegm_ctx *ctx, const double *unary, int height, int width, int n_labels,
                                     const double *pairwise, const double *cost_v, const double *cost_h, int n_iter,
                                     int32_t *labels_out, int64_t *energy_out);
/* Replaces the numpy in front of the cut and the cut of imsegm/region_growing.py:202-249 object_segmentation_graphcut_pixels:
 * the unary cost of class l at integer distance d from centre i is a_fg[l] - coef_shape * b[d] (label i + 1) and a_bg[l] -
 * coef_shape * s_bg[l] (label 0) when coef_shape > 0, a_fg[l] / a_bg[l] otherwise; 0 at the seeds (seed_size > 0: the disc of that
 * radius around the seed where segm > 0, else the seed pixel).  segm: height x width int32 with -n_table_labels <= segm <
 * n_table_labels (a negative class counts from the end, as numpy indexes); centres: n_centres x 4 int32 = row, column the
 * distance is taken from, row, column of the seed; b: n_dist entries, n_dist above every integer distance that occurs.  Edge
 * weights are 1, pairwise = (1 - eye) * gc_regul.  Only segm, the centres and the tables go up, only the labels come down.
 * unary_int_out (height * width * (n_centres + 1) int32) and dwf_out: pyGCO's integers and down-weight factor, or NULL (tests).
 * Limits: n_centres <= 63, tables of (3 n_table_labels + n_dist) * 8 + 16 n_centres <= 61440 bytes, height * width <= 2^29. */
IMSEGM_API int imsegm_object_cut_pixels(imsegm_ctx *ctx, const int32_t *segm, int height, int width, const int32_t *centres,
                                        int n_centres, const double *a_bg, const double *a_fg, const double *s_bg,
                                        int n_table_labels, const double *b, int n_dist, double coef_shape, double gc_regul,
                                        int seed_size, int n_iter, int32_t *labels_out, int64_t *energy_out,
                                        int32_t *unary_int_out, double *dwf_out);

/* ---------------------------------------------------------------------------------------------
 * the class model's fit (imsegm/graph_cuts.py:73-163 estim_class_model: scikit-learn's GaussianMixture.fit on the host in the
 * reference) for all restarts at once on one uploaded table; sums in a fixed order, no atomics: same call, same bits
 * ------------------------------------------------------------------------------------------- */
/* Replaces the Lloyd iterations of sklearn.cluster.KMeans(algorithm='lloyd') (sklearn/cluster/_kmeans.py _kmeans_single_lloyd,
 * the initialisation GaussianMixture(init_params='kmeans') runs per restart) from given centres.  table: n_rows x n_features
 * float64, uploaded once and kept in the context for the imsegm_mixture_em that follows; seeds: n_restarts x n_clusters x
 * n_features.  Nearest centre with ties to the lowest index; a restart stops when no label changes, or when the summed squared
 * centre shift is <= tol (absolute; then one more labelling), or after max_iter iterations.  Per restart (each output may be
 * NULL): labels_out n_restarts x n_rows int32, centres_out, inertia_out, n_iter_out, empty_out (1: an iteration left a cluster
 * without rows -- the restart stopped there, nothing is repaired).  The labels also stay on the device.
 * Returns IMSEGM_E_FIT_CAPS outside n_features <= 16, n_clusters <= 8, n_restarts <= 16, n_rows < 2^31. */
IMSEGM_API int imsegm_kmeans_lloyd(imsegm_ctx *ctx, const double *table, long n_rows, int n_features, const double *seeds,
                                   int n_restarts, int n_clusters, int max_iter, double tol, int32_t *labels_out,
                                   double *centres_out, double *inertia_out, int32_t *n_iter_out, int32_t *empty_out);
/* Replaces the EM loop of sklearn.mixture.GaussianMixture(covariance_type='full') (sklearn/mixture/_base.py fit_predict with
 * _gaussian_mixture.py _estimate_gaussian_parameters -- covariances in their centred form --, _compute_precision_cholesky,
 * _estimate_log_gaussian_prob) on the resident table.  Start per restart: the three *_init arrays (n_restarts x n_components
 * [x n_features [x n_features]]; weights, means, precisions_cholesky_), or else one-hot responsibilities from `labels`
 * (n_restarts x n_rows int32, host), or else (labels NULL) from the labels the last imsegm_kmeans_lloyd left on the device.
 * A restart stops when |lower bound - previous| < tol or after max_iter iterations (tol = 0: exactly max_iter) and is frozen
 * from then on.  Outputs per restart (each may be NULL): weights, means, covariances, precision Cholesky factors, last lower
 * bound, iterations, converged flag, not_pd_out (1: a covariance was not positive definite -- the restart stopped there). */
IMSEGM_API int imsegm_mixture_em(imsegm_ctx *ctx, int n_restarts, int n_components, const int32_t *labels,
                                 const double *weights_init, const double *means_init, const double *prec_chol_init,
                                 double reg_covar, double tol, int max_iter, double *weights_out, double *means_out,
                                 double *covariances_out, double *prec_chol_out, double *lower_bound_out, int32_t *n_iter_out,
                                 int32_t *converged_out, int32_t *not_pd_out);
/* Replaces the variational loop of sklearn.mixture.BayesianGaussianMixture(covariance_type='full') (sklearn/mixture/_base.py
 * fit_predict with _bayesian_mixture.py _initialize, _m_step, _estimate_log_prob, _estimate_log_weights, _compute_lower_bound) on
 * the resident table, from one-hot responsibilities: `labels` (n_restarts x n_rows int32, host) or else (NULL) the labels the last
 * imsegm_kmeans_lloyd left on the device.  prior_type: 0 dirichlet_process, 1 dirichlet_distribution; the priors are the
 * estimator's checked ones (weight_concentration_prior_, mean_precision_prior_, mean_prior_ [n_features],
 * degrees_of_freedom_prior_, covariance_prior_ [n_features x n_features]).  A restart stops when |lower bound - previous| < tol or
 * after max_iter iterations (tol = 0: exactly max_iter) and is frozen from then on.  Outputs per restart (each may be NULL):
 * weight_concentration_out n_restarts x 2 x n_components (rows a, b of the process; row 0 of the distribution, row 1 zero),
 * mean_precision_out, means_out, degrees_of_freedom_out, covariances_out, prec_chol_out, last lower bound, iterations, converged
 * flag, not_pd_out (1: a covariance was not positive definite -- the restart stopped there).  Caps and status: imsegm_mixture_em's. */
IMSEGM_API int imsegm_bayes_mixture_em(imsegm_ctx *ctx, int n_restarts, int n_components, const int32_t *labels, int prior_type,
                                       double weight_concentration_prior, double mean_precision_prior, const double *mean_prior,
                                       double degrees_of_freedom_prior, const double *covariance_prior, double reg_covar,
                                       double tol, int max_iter, double *weight_concentration_out, double *mean_precision_out,
                                       double *means_out, double *degrees_of_freedom_out, double *covariances_out,
                                       double *prec_chol_out, double *lower_bound_out, int32_t *n_iter_out,
                                       int32_t *converged_out, int32_t *not_pd_out);
/* The same two calls for WIDE tables, 17 <= n_features <= 256 (csrc/mixture_fit_wide.hip: fp64 matrix-instruction tiles instead
 * of a table row in registers): argument lists, outputs and status conventions are those of imsegm_kmeans_lloyd and
 * imsegm_mixture_em; the table imsegm_kmeans_lloyd_wide uploaded stays in the context for the imsegm_mixture_em_wide that
 * follows, with the labels.  Both return IMSEGM_E_FIT_CAPS outside 17 <= n_features <= 256, n_clusters <= 8, n_restarts <= 16,
 * n_rows < 2^31 -- ALSO for n_features <= 16, which the narrow pair fits: the caller routes by width
 * (graph_cuts.fit_mixture_device_wide).  Of prec_chol_init imsegm_mixture_em_wide reads the upper triangle (precisions_cholesky_
 * is upper triangular; what lies below its diagonal is taken as zero).  When a covariance is not positive definite, nothing of
 * that iteration is written for the restart: weights, means, covariances, precision factors and the lower bound are those of
 * its last COMPLETED iteration (all zero when the M step of the initialisation failed). */
IMSEGM_API int imsegm_kmeans_lloyd_wide(imsegm_ctx *ctx, const double *table, long n_rows, int n_features, const double *seeds,
                                        int n_restarts, int n_clusters, int max_iter, double tol, int32_t *labels_out,
                                        double *centres_out, double *inertia_out, int32_t *n_iter_out, int32_t *empty_out);
IMSEGM_API int imsegm_mixture_em_wide(imsegm_ctx *ctx, int n_restarts, int n_components, const int32_t *labels,
                                      const double *weights_init, const double *means_init, const double *prec_chol_init,
                                      double reg_covar, double tol, int max_iter, double *weights_out, double *means_out,
                                      double *covariances_out, double *prec_chol_out, double *lower_bound_out,
                                      int32_t *n_iter_out, int32_t *converged_out, int32_t *not_pd_out);

/* ---------------------------------------------------------------------------------------------
 * RANSAC scoring of ellipse trials (imsegm/ellipse_fitting.py ransac_segm :228-254 with EllipseModelSegm.criterion :121-139 and
 * skimage's EllipseModel.residuals), every trial of every egg candidate of an image in one launch chain; csrc/ellipse.hip
 * ------------------------------------------------------------------------------------------- */
/* Egg e owns the boundary points [point_offsets[e], point_offsets[e + 1]) of `points` (float64 x, y pairs; at least 5 per egg) and
 * the trials t with trial_egg[t] == e (trial_egg must not decrease; an egg may have none).  params: n_trials x 5 float64 (xc, yc,
 * a, b, theta), success: one byte per trial (0: the estimate failed, the trial is skipped).  points_all: n_all x 2 float64,
 * point_value[n] = weights[labels[n]] * (q[0][labels[n]] - q[1][labels[n]]) with q = -log(table_prob), prepared by the caller.
 * Per trial: criterion_out[t] = sum of point_value over the centres inside the ellipse (the reference's inside test; a fixed
 * summation tree that depends on n_all alone; NaN for a failed trial).  Per (trial, point of the trial's egg): the distance to the
 * closest point of the ellipse in the basin of the reference's starting parameter; the point is an inlier when |distance| <
 * residual_threshold.  Per egg, by the reference's update rule over its trials in order: best_out[e] = the trial whose criterion
 * was last found below the best so far, kept_out[e] = the trial whose inlier mask was kept, both counted among the egg's own
 * trials, -1 for none; mask_out[point_offsets[e] ...] = the kept mask (zeros for none).  residuals_out (may be NULL): the distances
 * of all pairs, trial after trial, each trial with one entry per point of its egg (NaN for a failed trial).
 * All outputs are host arrays.  Returns -1 (no launch) for n_eggs, n_trials or n_all < 1, offsets that do not start at 0 or are
 * not monotone, an egg with fewer than 5 points, or a trial_egg outside [0, n_eggs). */
IMSEGM_API int imsegm_ellipse_ransac(imsegm_ctx *ctx, int n_eggs, const int32_t *point_offsets, const double *points, int n_trials,
                                     const double *params, const uint8_t *success, const int32_t *trial_egg,
                                     const double *points_all, const double *point_value, int n_all, double residual_threshold,
                                     int32_t *best_out, int32_t *kept_out, uint8_t *mask_out, double *criterion_out,
                                     double *residuals_out);

/* ---------------------------------------------------------------------------------------------
 * Fitted ellipses into a label map with the overlap test (imsegm/ellipse_fitting.py add_overlap_ellipse :282-349, the last call of
 * segment_fit_ellipse / _ransac / _ransac_segm in experiments_ovary_detect/run_ovary_egg-segmentation.py and the inner loop of
 * run_ellipse_annot_match.py and run_ellipse_cut_scale.py); csrc/ellipse_place.hip.  The mask of an ellipse is scikit-image
 * 0.18.3's draw.ellipse(r, c, r_radius, c_radius, shape, rotation) (behind imsegm/utilities/drawing.py ellipse :116-151): the pixels
 * of its clipped bounding box with ((a cos + b sin) / r_radius)^2 + ((a sin - b cos) / c_radius)^2 < 1 for their integer offsets
 * (a, b) from the centre, in fp64 with one rounding per operation.  Integers and that one expression: same call, same bytes.
 * ------------------------------------------------------------------------------------------- */
#define IMSEGM_ELLIPSE_PLACE_LABELS 4096   /* labels 0 .. 4095 own a slot of the two int32 label tables the fold keeps in LDS (32 KiB) */
/* An ellipse is 8 int32 of geom -- centre row, centre column, row radius, column radius (radii >= 1; all four at most 2^30 in
 * absolute value), then first row, first column, last row, last column of its bounding box clipped to the map (inclusive; a last
 * below its first: the ellipse has no pixel) -- and 2 doubles of sincos, the sine and the cosine of its angle taken modulo pi.  The
 * caller computes the boxes and the pair (pyimsegm_amd/ellipse_fitting.py ellipse_geometry): no kernel evaluates a
 * transcendental or a ceil.
 *
 * imsegm_ellipse_place replaces the fold `for e: segm = add_overlap_ellipse(segm, params[e], labels[e], thr_overlap)`: ellipse e is
 * painted with labels[e] (placed[e] = 1) unless its mask is empty or one label lb >= 1 under it has
 * (double)overlap / (double)min(pixels of lb in the map as it stands, pixels of the mask) > thr_overlap -- one IEEE division, a
 * strict comparison.  segm: host int32 height x width, read and written in place (only rows that were painted are written);
 * every value must be below IMSEGM_ELLIPSE_PLACE_LABELS (values <= 0 are never tested, as in the reference), every label too (a
 * label <= 0 may be painted).  Returns -1 with segm untouched for a map of 2^31 pixels or more, a box that is not clipped, a radius
 * below 1, thr_overlap negative or NaN, or a value or label without a slot.  n = 0 is a no-op. */
IMSEGM_API int imsegm_ellipse_place(imsegm_ctx *ctx, int32_t *segm, int height, int width, int n, const int32_t *geom,
                                    const double *sincos, const int32_t *labels, double thr_overlap, uint8_t *placed);
/* For every ellipse on its own: areas[e] = pixels of its mask, counts[e * nb_labels + l] = those of them with segm == l for
 * 0 <= l < nb_labels <= IMSEGM_ELLIPSE_PLACE_LABELS (other values count in the area only) -- what the Jaccard indices of
 * run_ellipse_annot_match.py select_optimal_ellipse need besides one bincount.  One launch, int64 atomics.  Both outputs are host
 * arrays; errors as above. */
IMSEGM_API int imsegm_ellipse_overlaps(imsegm_ctx *ctx, const int32_t *segm, int height, int width, int n, const int32_t *geom,
                                       const double *sincos, int nb_labels, int64_t *counts, int64_t *areas);

/* ---------------------------------------------------------------------------------------------
 * From an egg class map with centre candidates to the rays the boundary points of the RANSAC are made of (imsegm/ellipse_fitting.py
 * split_segm_background_foreground :400-443 and the ray casting of prepare_boundary_points_ray_join / _edge / _mean / _dist
 * :352-597); csrc/morphology.hip.  Integers only up to the ray walk: same call, same bytes.
 * ------------------------------------------------------------------------------------------- */
#define IMSEGM_MORPH_MAX_RADIUS 64         /* the 64 x 64 tile of the disc kernels with its halo fits 48 KiB of LDS */
/* Replaces split_segm_background_foreground(seg, sel_bg, sel_fg) (ellipse_fitting.py:400-443) for integer radii: seg_bg = 1 -
 * scipy.ndimage.binary_fill_holes(segm > 0) and seg_fg = (segm == 1), each opened with skimage.morphology.disk(sel) when sel > 0
 * (opening :438, :442 = grey erosion and dilation with scipy's boundary mode 'reflect', which for a disc equals "pixels outside
 * the image do not count").  segm: host int32, height x width; the outputs host uint8 of the same shape, either may be NULL (a NULL
 * seg_fg_out skips the foreground opening).  Returns -1 (no launch) for a radius above IMSEGM_MORPH_MAX_RADIUS, a non-positive
 * height or width, more than 65535 rows or 2^31 pixels. */
IMSEGM_API int imsegm_split_background_foreground(imsegm_ctx *ctx, const int32_t *segm, int height, int width, int sel_bg, int sel_fg,
                                                  uint8_t *seg_bg_out, uint8_t *seg_fg_out);
/* Replaces the split and the two compute_ray_features_segm_2d calls per centre of prepare_boundary_points_ray_* (:381-390, :476-482,
 * :527-533, :577-581): the masks above stay on the device, the rays of all positions (row, col) on seg_bg with edge 'up' go to
 * rays_bg_out and on seg_fg with edge 'down' to rays_fg_out (n_positions x n_angles float32, -1: no edge met, also for a position
 * outside the map), both from one launch; directions as imsegm_ray_features_binary2d.  Either output may be NULL; a NULL
 * rays_fg_out skips the foreground opening entirely.  Returns -1 (no launch) as imsegm_split_background_foreground does and for
 * n_angles outside [1, IMSEGM_RAY_MAX_ANGLES]. */
IMSEGM_API int imsegm_boundary_rays(imsegm_ctx *ctx, const int32_t *segm, int height, int width, int sel_bg, int sel_fg,
                                    const int32_t *positions, int n_positions, const float *directions, int n_angles,
                                    float *rays_bg_out, float *rays_fg_out);

/* ---------------------------------------------------------------------------------------------
 * Region growing with a ray shape prior on superpixels (imsegm/region_growing.py region_growing_shape_slic_greedy :1155-1388,
 * region_growing_shape_slic_graphcut :1482-1730): a resident state on top of a label session; csrc/region_growing.hip.  The host
 * keeps the iteration, the thresholds, LAPACK's eigenvectors and the mixture weights (pyimsegm_amd/region_growing.py)
 * ------------------------------------------------------------------------------------------- */
typedef struct imsegm_rg imsegm_rg;             /* device-resident state of one growth */
/* Replaces the set-up of both growth functions (:1297-1304, :1622-1629): on the label map of the session (imsegm_image2d_set_labels;
 * it must stay as it is while the state is open) with its n_edges edges (the list imsegm_image2d_graph returned; its length is compared
 * with the map's and every index is range-checked, the pairs themselves are taken as given) the state keeps
 * np.round(superpixel_centers).astype(int) (half to even), np.bincount(slic) with the exact int64 row and column sums of every superpixel, the neighbour lists of get_neighboring_segments in CSR form, two K x (n_objects + 1) float64
 * cost tables and K int32 labels.  Returns -1 for a volume session, no label map, n_objects < 1 or an edge outside the map.
 * The state borrows the session: once the session is destroyed every imsegm_rg_* call on the state is undefined, EXCEPT
 * imsegm_rg_close, which frees the state's own buffers without reading the session (the Python wrapper refuses the others). */
IMSEGM_API int imsegm_rg_open(imsegm_image2d *im, const int32_t *edges, int n_edges, int n_objects, imsegm_rg **rg_out);
IMSEGM_API void imsegm_rg_close(imsegm_rg *rg);
/* what = 0: K x 3 int64 (pixel count = slic_weights :1299, row sum, column sum); 1: K x 2 int32 rounded centres (:1298);
 * 2: the K x (n_objects + 1) float64 shape costs (for debug_history and prepare_graphcut_variables :1391) */
IMSEGM_API int imsegm_rg_get(imsegm_rg *rg, int what, void *out);
/* uploads lut_data_cost (compute_data_costs_points :993-1011) and / or lut_shape_cost with its background column (:1308-1310);
 * either may be NULL */
IMSEGM_API int imsegm_rg_set_costs(imsegm_rg *rg, const double *lut_data, const double *lut_shape);
/* Replaces the inner loop of compute_update_shape_costs_points_table_cdf / _close_mean_cdf (:845-851, :984-989) for the objects
 * that passed the threshold tests: lut_shape[:, objects[j] + 1] = -log(compute_shape_prior_table_cdf(point, table_j, centres[j],
 * shifts[j]) + MIN_SHAPE_PROB) (:591-652, bilinear on the 2 x 2 cell where the reference calls interp2d; +-inf replaced by
 * GC_REPLACE_INF) for every superpixel.  dims: n_selected x 2 (angles, distances) of each object's table, the tables one after the
 * other in `tables`.  proba_out (may be NULL): the n_selected x K priors.  Centres and shifts must be finite. */
IMSEGM_API int imsegm_rg_shape_costs(imsegm_rg *rg, int n_selected, const int32_t *objects, const double *centres, const double *shifts,
                                     const int32_t *dims, const double *tables, double *proba_out);
/* Replaces compute_ray_features_segm_2d(labels[slic] == i + 1, centre_i, edge='down') of compute_segm_object_shape (:259-286,
 * called at :943) for every object at once, the mask read through the label vector: positions n_objects x 2 int32 (the rounded
 * centres of mass, which the caller forms from the int64 sums of imsegm_rg_get), directions n_angles x 2 float32 (the table of
 * imsegm_ray_features_binary2d), rays_out n_objects x n_angles float32 (-1: no edge met).  labels: K int32 in [0, n_objects], or
 * NULL to keep the resident vector (also below). */
IMSEGM_API int imsegm_rg_object_shapes(imsegm_rg *rg, const int32_t *labels, const int32_t *positions, const float *directions,
                                       int n_angles, float *rays_out);
/* Replaces the candidate search and scoring of one greedy iteration (get_neighboring_candidates :1088-1111 per object,
 * :1346-1371): the (object, superpixel) pairs in the reference's order (object-major, superpixels ascending; objects count from
 * 1) and, when changes_out is not NULL, crit - crit_new of each pair in its delta form.  coefs: coef_data, coef_shape,
 * coef_pairwise, -log(prob_label_trans[0]), -log(prob_label_trans[1]) (inf replaced by the caller).  The result arrays hold
 * n_objects x K entries. */
IMSEGM_API int imsegm_rg_greedy_step(imsegm_rg *rg, const int32_t *labels, int allow_obj_swap, const double *coefs, int *n_out,
                                     int32_t *objects_out, int32_t *superpixels_out, double *changes_out);
/* Replaces compute_rg_crit (:1114-1133) on the resident tables: a fixed summation tree, the same labels give the same bytes */
IMSEGM_API int imsegm_rg_criterion(imsegm_rg *rg, const int32_t *labels, const double *coefs, double *criterion_out);

/* ---------------------------------------------------------------------------------------------
 * From annotated egg maps to the rays a shape model is estimated from (imsegm/region_growing.py compute_object_shapes :289-331 with
 * the first half of compute_segm_object_shape :259-280); csrc/object_shapes.hip.  Integers up to the centre of mass, then the ray
 * walk: same map, same bytes.
 * ------------------------------------------------------------------------------------------- */
#define IMSEGM_OBJECT_SHAPES_MAX_SPAN 65536     /* entries of the presence table: max - min of a map of more than two values stays below it */
#define IMSEGM_OBJECT_SHAPES_MAX_OBJECTS 65536  /* the largest capacity a caller may ask for */
/* Replaces, for all objects of one map at once, the loop of :319-329 -- np.unique, scipy.ndimage.label, one `img == label` mask,
 * ndimage.center_of_mass and compute_ray_features_segm_2d(mask, centre, ray_step, 0, edge='down') per object -- by one labelling, one
 * reduction and one ray launch.  segm: host int32, height x width.
 *   * At most two distinct values (np.unique(img) <= 2, :321): the objects are the 4-connected components of the pixels != 0,
 *     numbered from 1 in raster order of their first pixel (scipy.ndimage.label with its default cross), labels_out[k] = k + 1.  As
 *     np.unique(labelled)[1:] drops the first value whatever it is, a map without a 0 has no objects, and neither has a constant map.
 *   * More than two values: the objects are the distinct values in ascending order WITHOUT the smallest (0 or not); an object is not
 *     split into components; labels_out[k] is the value.  max - min must stay below IMSEGM_OBJECT_SHAPES_MAX_SPAN.
 * Per object k < *n_objects_out, in that order: moments_out[3 k ..] = pixel count, sum of rows, sum of columns (int64, exact);
 * centres_out[2 k ..] = int(round(sum / count)) per coordinate, one IEEE fp64 division and round-half-to-even (ndimage.center_of_mass of
 * a boolean mask forms this quotient); rays_out[k * n_angles ..] = the float32 distances from the centre to where the object ends
 * along directions (n_angles x 2 float32, the table of imsegm_ray_features_binary2d), -1 where no such edge is met.  The centre of
 * an object of several pieces may lie outside it; the walk then starts outside, as the reference's does.
 * Returns 0; IMSEGM_E_OBJECT_CAPS with *n_objects_out = the number of objects when that exceeds max_objects, or = -1 when the values
 * span too much -- no per-object output is written and no error message set; -1 with a message for n_angles outside
 * [1, IMSEGM_RAY_MAX_ANGLES], a non-positive height or width, 2^31 pixels or more, or max_objects outside
 * [0, IMSEGM_OBJECT_SHAPES_MAX_OBJECTS] (with 0 the per-object outputs may be NULL: the call counts).  One upload, one chain of
 * launches on the context's stream without a host round trip, one download. */
IMSEGM_API int imsegm_object_shapes(imsegm_ctx *ctx, const int32_t *segm, int height, int width, const float *directions,
                                    int n_angles, int max_objects, int *n_objects_out, int32_t *labels_out, int64_t *moments_out,
                                    int32_t *centres_out, float *rays_out);

/* ---------------------------------------------------------------------------------------------
 * Cutting every labelled object of an image out, centred and turned level (imsegm/utilities/data_io.py cut_object :1060-1128 as
 * experiments_ovary_detect/run_cut_segmented_objects.py :93-101 loops it over the labels of an annotation); csrc/cut_objects.hip.
 * Integers on the device up to the moments, then two composed nearest-neighbour index maps in fp64 without fused operations: same
 * call, same bytes.
 * ------------------------------------------------------------------------------------------- */
#define IMSEGM_CUT_OBJECTS_MAX_LABELS 1024     /* labels of one call: the ascending list lives in LDS */
#define IMSEGM_CUT_OBJECTS_MAX_CHANNELS 4      /* interleaved uint8 channels of the image */
#define IMSEGM_CUT_MOMENT_WORDS 10             /* int64 per label: count, sum r, sum c, sum r^2, sum c^2, sum r c, r min, r max, c min, c max */
#define IMSEGM_CUT_GEOMETRY_DOUBLES 8          /* per label: shift s_r, s_c; matrix m00, m01, m10, m11; offset o_r, o_c */
#define IMSEGM_CUT_FRAME_INTS 6                /* per label: canvas height, width; window r0, r1, c0, c1 (half open) on the canvas */
/* The fp64 step between the moments and the index maps, supplied by the caller so that it is stated once (the package hands in
 * the function its host statement uses: centroid = sum / count, scikit-image 0.18.3's orientation, scipy.ndimage.rotate's matrix,
 * offset and canvas shape).  moments: n_labels x IMSEGM_CUT_MOMENT_WORDS (a label without a pixel has count 0, minima
 * 0x7f7f7f7f, maxima -1); to fill: geometry_out n_labels x IMSEGM_CUT_GEOMETRY_DOUBLES and frames_out n_labels x
 * IMSEGM_CUT_FRAME_INTS.  Canvas pixel (i, j) reads the shifted frame at x = ((0 + i m_0) + j m_1) + o per axis, which reads the
 * source at k + s per axis; at either step a coordinate below 0 or above n - 1 is outside, else the index is floor(x + 0.5).
 * Outside the window the turned mask must be False.  A return value other than 0 ends the call with -1. */
typedef int (*imsegm_cut_geometry_fn)(void *user, int n_labels, int allow_rotate, int height, int width, const int64_t *moments,
                                      double *geometry_out, int32_t *frames_out);
/* Replaces [cut_object(img, segm == l, padding, use_mask, bg_color, allow_rotate) for l in labels] for a uint8 image (host,
 * height x width x channels interleaved), an int32 label map (host, height x width) and n_labels strictly ascending labels: the
 * moments and boxes of all labels in one pass, `geometry` on the host, the exact box of every turned mask inside its window, the
 * crops (box widened by add_padding :1039-1057 against the canvas) written by one launch and brought down by one copy.  A pixel
 * from outside the source is 0; with use_mask a crop pixel whose turned mask is False gets bg_color (channels bytes).  The image
 * and the map are uploaded once each.  Results: moments_out (may be NULL) as handed to the hook; boxes_out[4 k ..] = r0, c0, r1,
 * c1 of crop k on its canvas; offsets_out[k] (n_labels + 1 entries) = where its (r1 - r0) x (c1 - c0) x channels bytes start in
 * *packed_out, page-locked memory of the context that stays valid until the next call on it.  *first_empty_out = -1, or the
 * first label whose turned mask has no pixel (regionprops(...)[0] of the reference raises): then nothing else is written.
 * Returns 0; IMSEGM_E_OBJECT_CAPS -- no message, the caller evaluates on the host -- for more than
 * IMSEGM_CUT_OBJECTS_MAX_LABELS labels, more than IMSEGM_CUT_OBJECTS_MAX_CHANNELS channels, 2^31 pixels or more, a padding above
 * 2^20 (all before anything is launched) and more than 2^30 bytes of crops; -1 with a message for null arguments, sizes below 1, a
 * negative padding, labels that do not ascend and what the hook refuses. */
IMSEGM_API int imsegm_cut_objects(imsegm_ctx *ctx, const uint8_t *image, const int32_t *segm, int height, int width, int channels,
                                  const int32_t *labels, int n_labels, int padding, int use_mask, const uint8_t *bg_color,
                                  int allow_rotate, imsegm_cut_geometry_fn geometry, void *user, int64_t *moments_out,
                                  int32_t *boxes_out, int64_t *offsets_out, const uint8_t **packed_out, int *first_empty_out);

/* ---------------------------------------------------------------------------------------------
 * Centre-level annotations from maps of annotated eggs (experiments_ovary_centres/run_create_annotation.py of the reference:
 * load_correct_segm :68-83, segm_set_center_levels :100-132, compute_eggs_center :52-65); csrc/center_annotation.hip and the
 * label-aware disc kernels of csrc/morphology.hip.  Integers up to the fp64 operations numpy takes: same call, same bytes.  All
 * arrays are host arrays.  Every entry returns IMSEGM_E_OBJECT_CAPS -- no message, the caller evaluates on the host -- for what it
 * does not take: more than 65535 rows, 2^31 pixels or more, height^2 + width^2 > 2^32 - 1, more than
 * IMSEGM_CENTER_ANNOT_MAX_LABELS labels, an opening radius of a level above IMSEGM_MORPH_MAX_RADIUS; -1 with a message for null
 * arguments, sizes below 1, radii outside [0, IMSEGM_MORPH_MAX_RADIUS], more than IMSEGM_CENTER_ANNOT_MAX_LEVELS levels and
 * levels that descend.
 * ------------------------------------------------------------------------------------------- */
#define IMSEGM_CENTER_ANNOT_MAX_LABELS 1024    /* label values 1 .. 1024 own a slot of the per-label tables */
#define IMSEGM_CENTER_ANNOT_MAX_LEVELS 8       /* one bit per level in a byte per pixel */
/* load_correct_segm after the read: img > 0 (img_is_i32: int32 pixels, otherwise uint8), opening with disk(sel_radius) (0: none),
 * 4-connected components with fewer than min_size pixels removed -> seg_out (uint8 0 / 1, may be NULL); its 8-connected components
 * numbered from 1 in raster order of their first pixels -> labels_out (int32, may be NULL), their number -> *n_labels_out. */
IMSEGM_API int imsegm_correct_segm(imsegm_ctx *ctx, const void *img, int img_is_i32, int height, int width, int sel_radius,
                                   int min_size, uint8_t *seg_out, int32_t *labels_out, int *n_labels_out);
/* segm_set_center_levels without the save and compute_eggs_center, for the labels 1 .. max_label of `labels` (int32; other values
 * are background).  levels: n_levels ascending doubles; n_levels = 0 computes the centres only.  levels_out (uint8, may be NULL
 * then): 0, or i + 1 for the highest level i whose opened mask holds the pixel.  counts_out (int64 [max_label + 1]): the pixels
 * of every label, 0 for an absent one; centres_out (double [2 (max_label + 1)]): column mean, row mean -- the quotient of two
 * exact integer sums.  The fp64 radius, disc and opening radius of every (label, level) are computed on the host side of the
 * call between two launches (one small download, one small upload). */
IMSEGM_API int imsegm_center_levels(imsegm_ctx *ctx, const int32_t *labels, int height, int width, int max_label, const double *levels,
                                    int n_levels, uint8_t *levels_out, int64_t *counts_out, double *centres_out);
/* Diagnostic (no reference counterpart; tests): what imsegm_center_levels holds in front of its code pass, by the function that
 * entry calls, stopped there.  d2_out (uint32 [height * width]): the squared distance of every pixel of a label 1 .. max_label to
 * the nearest pixel of another value, 0 for other pixels; a map of one value has no such pixel and gets (y + 1)^2 + x^2.
 * max2_out (uint32 [max_label + 1]): the largest d2 of every label; sums_out (int64 [3 (max_label + 1)]): pixel count, row sum,
 * column sum.  Slot 0 stays 0.  Caps and errors as imsegm_center_levels. */
IMSEGM_API int imsegm_debug_center_distances(imsegm_ctx *ctx, const int32_t *labels, int height, int width, int max_label,
                                             uint32_t *d2_out, uint32_t *max2_out, int64_t *sums_out);
/* create_annot_centers without the files: the two calls above with the label map staying on the device.  counts_out and
 * centres_out hold IMSEGM_CENTER_ANNOT_MAX_LABELS + 1 rows; *n_labels_out = the number of labels (rows 1 .. n are filled). */
IMSEGM_API int imsegm_create_annot_centers(imsegm_ctx *ctx, const void *img, int img_is_i32, int height, int width, int sel_radius,
                                           int min_size, const double *levels, int n_levels, uint8_t *levels_out, int *n_labels_out,
                                           int64_t *counts_out, double *centres_out);

/* ---------------------------------------------------------------------------------------------
 * Egg segmentation by marker watershed (experiments_ovary_detect/run_ovary_egg-segmentation.py of the reference: segment_watershed
 * :239-275, method 'watershed_morph'); csrc/watershed.hip with the hole filling and disc kernels of csrc/morphology.hip, the
 * distance transform of csrc/boundary.hip and the labelling of csrc/center_annotation.hip.  Integers only: same call, same bytes
 * as the statements of pyimsegm_amd/egg_segmentation.py.  The flood is defined by rounds (DESIGN.md section 4 "Watershed"), not by
 * scikit-image's queue.  All arrays are host arrays.  Every entry returns IMSEGM_E_OBJECT_CAPS -- no message, the caller evaluates
 * on the host -- for what it does not take: more than 65535 rows, 2^31 pixels or more, height^2 + width^2 >= 2^31 (the keys are
 * int32), labels above IMSEGM_WATERSHED_MAX_LABELS, a radius above IMSEGM_MORPH_MAX_RADIUS; -1 with a message for null arguments,
 * sizes below 1, negative radii and seeds outside the map.
 * ------------------------------------------------------------------------------------------- */
#define IMSEGM_WATERSHED_MAX_LABELS 1024       /* labels 1 .. 1024: a label and the claim bit share a word of the flood's state */
/* morphology.watershed(keys, markers, mask=mask) (:259) as the round flood, 4-connected: mask (uint8, non-zero: inside), keys (int32
 * per pixel in [-2^31 + 1, 2^31 - 2]; NULL: minus the exact squared distance to the nearest zero of mask, :253 squared), the
 * non-zero markers inside the mask as n_seeds (pixel index, label) pairs with distinct pixels.  segm_out (int32): the label that
 * arrives, 0 outside the mask and where none does.  One workgroup floods one component of the mask. */
IMSEGM_API int imsegm_watershed_markers(imsegm_ctx *ctx, const uint8_t *mask, int height, int width, const int32_t *keys,
                                        const int32_t *seed_pixels, const int32_t *seed_labels, int n_seeds, int32_t *segm_out);
/* The clean-up loop :265-274: for every label 1 .. max_label in ascending order segm == label closed with disk(radius_close)
 * (binary_closing: dilation with clear pixels outside the image, erosion with set ones), its holes filled (binary_fill_holes), opened
 * with disk(radius_open) (binary_opening: erosion, dilation) and painted over the earlier labels into clean_out (int32).  A radius of
 * 0 leaves its step out.  Every stage is one launch over all labels, each inside the plane of its bounding box padded by
 * radius_close + 1; planes that together exceed the scratch of the call (boxes that overlap heavily) give IMSEGM_E_OBJECT_CAPS. */
IMSEGM_API int imsegm_watershed_post_morph(imsegm_ctx *ctx, const int32_t *segm, int height, int width, int max_label, int radius_close,
                                           int radius_open, int32_t *clean_out);
/* segment_watershed :249-275 in one call: seg (uint8, the bytes of seg > 0), binary_fill_holes (:250), the squared
 * distance_transform_edt (:253), markers[row, col] = i + 1 for centre i of centres (int32 [2 n_centres], rows and columns inside the
 * map; a later centre replaces an earlier one on the same pixel, :255-256), the flood (:259) and, with post_morph, the clean-up with
 * radii[0], radii[1] (NULL: 5 and 15, the reference's).  One upload, one chain of launches, one download. */
IMSEGM_API int imsegm_watershed(imsegm_ctx *ctx, const uint8_t *seg, int height, int width, const int32_t *centres, int n_centres,
                                int post_morph, const int32_t *radii, int32_t *segm_out);

/* ---------------------------------------------------------------------------------------------
 * Orientation of egg cut-outs (experiments_ovary_detect/run_egg_swap_orientation.py of the reference: compute_mean_image :92-98,
 * condition_swap_correl :77-80, condition_swap_density :65-74, perform_orientation_swap :39-62, main :101-128);
 * csrc/egg_orientation.hip.  Integers only: same call, same bytes as the statements of pyimsegm_amd/egg_orientation.py
 * (stack_median2_host, orientation_sums_host; DESIGN.md section 4 "Egg orientation").  A stack is n_images uint8 images
 * [height, width, channels], C-contiguous, already cropped to one size; `channel` is the one both tests read (the reference's
 * IMAGE_CHANNEL = 0).  All arrays are host arrays.  Both entries return IMSEGM_E_OBJECT_CAPS -- no message, the caller evaluates on
 * the host -- for more than IMSEGM_ORIENT_MAX_IMAGES images (the counters of the median are 16 bits wide), more than 4 channels,
 * more than 2^30 pixels per image or a stack above 2^31 - 1 bytes; -1 with a message for null arguments, sizes below 1, a channel
 * outside the image, an unknown mode and a given template above 510.
 * ------------------------------------------------------------------------------------------- */
#define IMSEGM_ORIENT_MAX_IMAGES 65535
#define IMSEGM_ORIENT_SUM_WORDS 9              /* A = sum a, min a, max a, P, Pf, cnt, S, L, R */
/* template2_out (uint16 [height, width]) = s[(n - 1) / 2] + s[n / 2] of the n channel values of every pixel sorted: exactly
 * 2 * np.median(stack[..., channel], axis=0) (:97).  One lane per pixel, radix selection in two passes of 16 bins. */
IMSEGM_API int imsegm_stack_median_u8(imsegm_ctx *ctx, const uint8_t *stack, int n_images, int height, int width, int channels,
                                      int channel, uint16_t *template2_out);
/* main :114-128 in one call.  template2_in: twice the template as uint16 in 0 .. 510, or NULL for the median of the stack; it is
 * written to template2_out either way.  sums_out (int64 [n_images, 9]), with a the channel of an image, t the template2 and m = min a:
 * A = sum a, min a, max a, P = sum a t, Pf = sum a[h - 1 - r, w - 1 - c] t[r, c], cnt = #{a > m}, S = sum of the a > m, and with
 * g = [a cnt > S] and part = width / 3: L = sum g[:, :part], R = sum g[:, width - part:] (part = 0: the sum of all of g, as the
 * reference's img[:, -0:]).  flags_out (uint8 [n_images]): mode 0 (correlation) = min a != max a and min t != max t and P < Pf;
 * mode 1 (density) = L > R.  turned_out (the size of stack; may be stack itself): every image, as img[::-1, ::-1, :] where its
 * flag is set.  The stack goes up once; the template, the sums, the flags and only the turned images come down. */
IMSEGM_API int imsegm_orient_stack(imsegm_ctx *ctx, const uint8_t *stack, int n_images, int height, int width, int channels, int channel,
                                   int mode, const uint16_t *template2_in, uint16_t *template2_out, uint8_t *flags_out,
                                   int64_t *sums_out, uint8_t *turned_out);

/* ---------------------------------------------------------------------------------------------
 * Cut-outs of ellipse-annotated eggs scaled to the normal size of their stage (experiments_ovary_detect/run_ellipse_cut_scale.py
 * of the reference: extract_ellipse_object :46-72, whose output run_egg_swap_orientation.py reads); csrc/resize.hip, the ellipse
 * masks of csrc/cut_objects.hip and the inside test of csrc/ellipse_place.h.  Same call, same bytes as the statements of
 * pyimsegm_amd/ellipse_cut_scale.py (resize_image_host, export_image_array, extract_ellipse_objects_host; DESIGN.md section 4 "Cut
 * and scale").  All arrays are host arrays.  Both entries return IMSEGM_E_OBJECT_CAPS -- no message, the caller evaluates on the
 * host -- for more than IMSEGM_RESIZE_MAX_CROPS crops, more than IMSEGM_CUT_OBJECTS_MAX_CHANNELS channels, a blur radius above
 * IMSEGM_RESIZE_MAX_RADIUS, a side of a crop or of the output above 32768, more than 2^30 bytes of crops or more than 2^28 output
 * values; -1 with a message for null arguments, sizes below 1, negative radii and what a hook refuses.
 * ------------------------------------------------------------------------------------------- */
#define IMSEGM_RESIZE_MAX_RADIUS 64            /* a 16 x 64 pixel tile of 4 channels with a halo of 64 rows on both sides: 36 KiB of LDS */
#define IMSEGM_RESIZE_MAX_CROPS 1024           /* crops of one call (IMSEGM_CUT_OBJECTS_MAX_LABELS: the chain cuts what it resizes) */
/* skimage.transform.resize(crop, (out_h, out_w)) of scikit-image 0.18.3 (run_ellipse_cut_scale.py :69; order 1, mode 'reflect',
 * anti-aliasing, clip) for n uint8 crops of unequal sizes, and the array half of export_image (imsegm/utilities/data_io.py :459-462,
 * called at :72).  Crop k is sizes[2 k] x sizes[2 k + 1] x channels bytes at packed + offsets[k] (offsets: n + 1 running sums).
 * The blur is scipy.ndimage.gaussian_filter on the uint8 crop, down the rows and then along them with a uint8 intermediate, each
 * byte (uint8)tmp with tmp = x[0] w[0], then tmp += (x[-j] + x[+j]) w[j] for j = radius .. 1 in fp64, mirrored edges.  radii[2 k + a]
 * and weights[(2 k + a) * (IMSEGM_RESIZE_MAX_RADIUS + 1) + j] (the weight at distance j) for axis a of crop k are COMPUTED BY THE
 * CALLER exactly as scipy does -- exp(-0.5 / sigma^2 * x^2) over arange(-r, r + 1) divided by its sum, r = int(4 sigma + 0.5),
 * sigma = max(0, (in / out - 1) / 2); an axis that is not shrunk has radius 0 and weight 1 -- so that no kernel evaluates exp.
 * Then byte * (1. / 255), the bilinear lookup at r = (H / h)(y + 0.5) - 0.5, c = (W / w)(x + 0.5) - 0.5 (a 1 x 1 output: the centre)
 * with mirrored neighbours, clipped to the range of the blurred crop -> out (float64 [n, out_h, out_w, channels]; may be NULL when
 * out_u8 is given).  out_u8 (may be NULL): (uint8)(v / max * 255) with the maximum of every image, (uint8)v for an image of
 * zeros. */
IMSEGM_API int imsegm_resize_crops(imsegm_ctx *ctx, const uint8_t *packed, const int64_t *offsets, const int32_t *sizes, int n,
                                   int channels, int out_h, int out_w, const int32_t *radii, const double *weights, double *out,
                                   uint8_t *out_u8);
/* The weights of the blur for n crops of sizes[2 k] x sizes[2 k + 1] and the output size, as above, supplied by the caller of
 * imsegm_ellipse_cut_scale because the crop sizes only exist in the middle of that call: to fill radii_out (n x 2) and weights_out
 * (n x 2 x (IMSEGM_RESIZE_MAX_RADIUS + 1), zeroed).  A radius above the cap in radii_out ends the call with IMSEGM_E_OBJECT_CAPS, a
 * return value other than 0 with -1. */
typedef int (*imsegm_blur_taps_fn)(void *user, int n, const int32_t *sizes, int out_h, int out_w, int32_t *radii_out,
                                   double *weights_out);
/* The loop of extract_ellipse_object :62-72 over the n ellipses of one image (uint8, height x width x channels interleaved, uploaded
 * once), the ellipses in the geom / sincos form of imsegm_ellipse_place.  Per ellipse: the mask of add_overlap_ellipse(zeros, ell, 1)
 * (:63) -- never rasterised: its moments come from the ellipse expression inside the clipped box, so ellipses may overlap --, the
 * `geometry` hook of imsegm_cut_objects, cut_object(img, mask, 0, use_mask=True) (:66; the mask is an int64 map, so a canvas pixel
 * from outside the turned frame keeps its 0 instead of bg_color), the resize (:69) with the weights of `taps`, and the export (:72).
 * The crops stay on the device between the cut and the resize; the stack comes down by one copy.  out / out_u8 as in
 * imsegm_resize_crops.  *first_empty_out = -1, or the first ellipse whose turned mask has no pixel: then nothing else is written.
 * An ellipse without a pixel at all is the hook's to refuse (count 0).  Ellipses are checked as in imsegm_ellipse_place. */
IMSEGM_API int imsegm_ellipse_cut_scale(imsegm_ctx *ctx, const uint8_t *image, int height, int width, int channels, int n,
                                        const int32_t *geom, const double *sincos, const uint8_t *bg_color, int out_h, int out_w,
                                        imsegm_cut_geometry_fn geometry, imsegm_blur_taps_fn taps, void *user, double *out,
                                        uint8_t *out_u8, int *first_empty_out);

/* ---------------------------------------------------------------------------------------------
 * Annotation colours: RGB annotation images <-> integer label maps, colour counts and the quantisation of a painted image to the
 * nearest exactly-coloured pixel (imsegm/annotation.py, the module behind handling_annotations/run_image_color_quantization.py,
 * run_image_convert_label_color.py, run_overlap_images_segms.py and run_segm_annot_inpaint.py); csrc/annotation.hip.  Integers
 * only: same call, same bytes.  Images are interleaved uint8 (height x width x 3), label maps int32, colour tables n_colors x 3
 * uint8 with 1 <= n_colors <= IMSEGM_ANNOT_MAX_COLORS.  All arrays are host arrays.
 * ------------------------------------------------------------------------------------------- */
#define IMSEGM_ANNOT_MAX_COLORS 256        /* entries of a colour table: it lives in LDS as one packed word per colour */
#define IMSEGM_ANNOT_MATCH_EXACT 0         /* out: int32 per pixel, labels[k] of the colour the pixel equals, -1 for none */
#define IMSEGM_ANNOT_MATCH_NEAREST 1       /* out: int32 per pixel, the index of the nearest colour */
#define IMSEGM_ANNOT_MATCH_NEAREST_COLOR 2 /* out: uint8 x 3 per pixel, the nearest colour itself */
/* One pass over n_pixels pixels against the table.  EXACT replaces the loop of convert_img_colors_to_labels_reverted
 * (annotation.py:113-121) and the labelling loop of quantize_image_nearest_pixel (:311-316): when several entries hold the pixel's
 * colour the LAST one's label is taken (later colours overwrite); labels (none negative) may be NULL for labels[k] = k;
 * *unmatched_out (may be NULL) = the number of pixels without an entry (:122 compares it against the pixel count).  NEAREST replaces image_color_2_labels
 * (:245-248) and NEAREST_COLOR quantize_image_nearest_color (:271-275): the first entry with the smallest
 * |r - r_k| + |g - g_k| + |b - b_k| (np.argmin over the colours in table order).  Returns -1 (no launch) for n_pixels < 1, a table
 * size outside [1, IMSEGM_ANNOT_MAX_COLORS] or an unknown mode. */
IMSEGM_API int imsegm_annot_match(imsegm_ctx *ctx, const uint8_t *image, size_t n_pixels, const uint8_t *colors, const int32_t *labels,
                                  int n_colors, int mode, void *out, int64_t *unmatched_out);
/* Replaces convert_img_labels_to_colors (:146-160): image_out[i] = table[labels[i] - min_label] for a table of n_table colours with
 * one `present` byte per entry (0: the label has no colour).  A pixel whose label lies outside the table or has no colour makes the
 * call return -1 with image_out untouched (:146-147 raises). */
IMSEGM_API int imsegm_annot_paint(imsegm_ctx *ctx, const int32_t *labels, size_t n_pixels, int min_label, int n_table,
                                  const uint8_t *table, const uint8_t *present, uint8_t *image_out);
/* Replaces PIL's Image.getcolors behind unique_image_colors (:61-67) and image_frequent_colors (:184-185): the distinct colours of
 * the image as packed keys r << 16 | g << 8 | b in ascending order with their pixel counts.  *n_colors_out = their number; keys_out
 * and counts_out (capacity entries each; NULL with capacity 0 to count only) are written only when that number fits. */
IMSEGM_API int imsegm_annot_color_hist(imsegm_ctx *ctx, const uint8_t *image, size_t n_pixels, int capacity, int *n_colors_out,
                                       uint32_t *keys_out, uint32_t *counts_out);
/* Replaces image_inpaint_pixels (:279-286, scipy's NearestNDInterpolator over all valid pixels) on a label map: a pixel equal to -1
 * is invalid and gets the label of the valid pixel at the smallest squared Euclidean distance (exact, uint32); among several at
 * that distance the one with the smallest row-major index.  Every other value is a label and stays.  Returns -1 with labels_out
 * untouched for a map without a valid pixel, height^2 + width^2 > 2^32 - 1 or more than 65535 rows.  labels_out may be labels. */
IMSEGM_API int imsegm_annot_nearest_valid(imsegm_ctx *ctx, const int32_t *labels, int height, int width, int32_t *labels_out);
/* Replaces quantize_image_nearest_pixel (:308-321): EXACT match with labels[k] = k, imsegm_annot_nearest_valid and the gather of
 * colors[label] per pixel with ONE upload of the image and ONE download.  Errors as the two calls; image_out may be image. */
IMSEGM_API int imsegm_annot_quantize_nearest_pixel(imsegm_ctx *ctx, const uint8_t *image, int height, int width, const uint8_t *colors,
                                                   int n_colors, uint8_t *image_out);

/* ---------------------------------------------------------------------------------------------
 * Scoring label maps against annotations (imsegm/classification.py compute_classif_metrics :305-371,
 * compute_classif_stat_segm_annot :374-421, compute_stat_per_image :424-471): everything those report is a function of the
 * contingency table of the two maps over the labels present; csrc/scoring.hip counts it, the host does the rest on a U x U matrix.
 * Integers only: same call, same bytes.  All arrays are host arrays.
 * ------------------------------------------------------------------------------------------- */
#define IMSEGM_SCORE_I32 0                 /* element type of the maps: int32 */
#define IMSEGM_SCORE_U8 1                  /* uint8, uploaded at one byte per pixel and widened on load */
#define IMSEGM_SCORE_MAX_LABELS 64         /* distinct labels of a pair the device counts */
#define IMSEGM_SCORE_MAX_DROP 64           /* entries of the drop list */
#define IMSEGM_SCORE_OK 0                  /* status of a pair: counted */
#define IMSEGM_SCORE_TOO_MANY_LABELS 1     /* more than IMSEGM_SCORE_MAX_LABELS labels: nothing else of the pair is written */
/* geometry of the two pixel kernels (the tests take their sizes from here) */
#define IMSEGM_SCORE_THREADS 256           /* lanes of a workgroup: four waves of 64 */
#define IMSEGM_SCORE_RUN 8                 /* consecutive pixels a lane loads per step */
#define IMSEGM_SCORE_CHUNK_STEPS 4         /* steps of a workgroup: it owns THREADS * RUN * CHUNK_STEPS consecutive pixels of one pair */
#define IMSEGM_SCORE_WAVE_TABLE_LABELS 32  /* up to here every wave counts into an LDS table of its own, above into one per workgroup */
/* Pair i is annots[i] and segms[i], sizes[i] elements each (0 is legal, 2^40 at the most) of the type `dtype`; a pixel is dropped
 * when either map carries one of the n_drop drop_labels there (:404-410).  Per pair: status_out[i]; n_labels_out[i] = U, the number
 * of distinct values of both maps over the pixels that stay; labels_out[i * MAX_LABELS ..] those values ascending;
 * tables_out[i * MAX_LABELS^2 + a * U + b] = #{annot == labels[a] and segm == labels[b]} (row stride U).  A pair with more than
 * MAX_LABELS labels gets IMSEGM_SCORE_TOO_MANY_LABELS and nothing else; the other pairs are not affected.  One upload per array,
 * one chain of launches over all pairs, one download.  Returns -1 (nothing launched) for a null array, a negative count, more than
 * 2^20 pairs, an unknown dtype, a size that is negative or above 2^40 and more than MAX_DROP drop labels. */
IMSEGM_API int imsegm_score_pairs(imsegm_ctx *ctx, int n_pairs, const void *const *annots, const void *const *segms, const int64_t *sizes,
                                  int dtype, const int32_t *drop_labels, int n_drop, int32_t *status_out, int32_t *n_labels_out,
                                  int32_t *labels_out, int64_t *tables_out);

/* ---------------------------------------------------------------------------------------------
 * random-forest class models (version >= 102): predict_proba of sklearn Pipeline([StandardScaler,] clf), clf a
 * RandomForestClassifier, ExtraTreesClassifier or DecisionTreeClassifier with one output, bit for bit (n_jobs = 1):
 *   z = float32((x - mean) / scale)     two fp64 operations, then round to nearest even (scikit-learn's input validation)
 *   per tree, in estimators_ order: from node 0, left while z[feature] <= threshold, until a leaf
 *   proba = (0 + row(leaf of tree 0) + row(leaf of tree 1) + ...) / n_trees   in fp64, in that order, one division
 * A tree is stored in preorder: the left child of node i is node i + 1, only the right child is kept.
 * ------------------------------------------------------------------------------------------- */
#define IMSEGM_FOREST_MAX_CLASSES 16       /* the cut's own limit */
#define IMSEGM_FOREST_MAX_FEATURES 256
#define IMSEGM_FOREST_MAX_TREES 1024
#define IMSEGM_FOREST_MAX_TREE_NODES (1 << 23)   /* the right child has 23 bits */
#define IMSEGM_FOREST_ROWS 256             /* rows of the table a workgroup walks at a time: one per lane */
#define IMSEGM_FOREST_LDS_NODES 4096       /* a tree of up to this many nodes (32 KB) is walked in LDS, a larger one in global memory */
typedef struct {
    float threshold;              /* the largest float32 <= the float64 threshold of scikit-learn (0 in a leaf) */
    int32_t word;                 /* >= 0: feature | right child << 8 (index inside the tree); < 0: a leaf, ~word its row of leaf_values */
} imsegm_forest_node;
/* zero-initialised by callers, as imsegm_gmm */
typedef struct {
    int n_features, n_classes, n_trees;
    int n_nodes, n_leaves;                 /* of all trees together */
    const double *scaler_mean;             /* [F] StandardScaler.mean_ or NULL */
    const double *scaler_scale;            /* [F] StandardScaler.scale_ or NULL */
    const imsegm_forest_node *nodes;       /* [n_nodes], tree after tree */
    const int32_t *tree_start;             /* [n_trees + 1] first node of every tree, n_nodes last */
    const double *leaf_values;             /* [n_leaves][C] what the tree's predict_proba returns in that leaf */
} imsegm_forest;
/* proba_out [n_rows][C] of the host table [n_rows][n_columns] (float64, n_columns == forest->n_features).  The forest is checked
 * on the host before it goes up (sizes, every child, feature and leaf row in range, children behind their parent: every path ends
 * in a leaf); returns IMSEGM_E_FOREST_INPUT with proba_out untouched for what it refuses. */
IMSEGM_API int imsegm_forest_proba(imsegm_ctx *ctx, const imsegm_forest *forest, const double *table, int n_rows, int n_columns,
                                   double *proba_out);
/* the same on the resident feature table of a 2-D or volume session (imsegm_image2d_features_color, ...): K x C probabilities
 * stay resident, and the next imsegm_image2d_segment with gmm == NULL and proba == NULL takes them.  proba_out may be NULL: the
 * call then does not wait, and a table the forest refuses shows as IMSEGM_E_FOREST_INPUT of that segment call.  Any call that
 * changes the label map or the feature table drops the probabilities, as it drops the prepared graph. */
IMSEGM_API int imsegm_image2d_forest_proba(imsegm_image2d *img, const imsegm_forest *forest, double *proba_out);

/* ---------------------------------------------------------------------------------------------
 * clustering of centre candidates (version >= 103): experiments_ovary_centres/run_center_clustering.py::cluster_center_candidates
 * :61-83 of the reference -- scikit-learn's DBSCAN(eps, min_samples).fit(points).labels_ and np.mean(points[labels == i], axis=0)
 * per cluster -- for many sets of 2-D points in one call, one workgroup per set.  The closed form of scikit-learn's scan:
 *   near(a, b):  dx * dx + dy * dy <= eps * eps in fp64, two rounded products and one rounded sum (no fused multiply-add);
 *                every point is near itself
 *   core:        at least min_samples points of the set are near
 *   clusters:    the connected components of the core points under near, numbered 0, 1, ... by their smallest core index
 *   border:      a point that is not core takes the smallest cluster number among the core points near it; -1 (noise) without one
 *   centre:      the sum of the cluster's points in index order, in fp64, over their count
 * ------------------------------------------------------------------------------------------- */
#define IMSEGM_DBSCAN_MAX_POINTS 4096      /* points of one set: its coordinates and forest live in the LDS of one compute unit */
#define IMSEGM_DBSCAN_MAX_SETS 4096        /* sets of one call */
#define IMSEGM_DBSCAN_MAX_TOTAL (1 << 20)  /* points of one call (the page-locked staging block holds 36 bytes per point) */
/* points [offsets[nb_sets]][2] as (row, col), offsets [nb_sets + 1] (not descending; set s is the rows offsets[s] .. offsets[s + 1]
 * - 1, empty sets allowed) -> labels_out [offsets[nb_sets]], counts_out [nb_sets] (clusters per set), centres_out
 * [offsets[nb_sets]][2]: row offsets[s] + c is the centre of cluster c of set s, the other rows of the set are 0.  Equal bytes from
 * every call on equal input.  Returns IMSEGM_E_OBJECT_CAPS -- no message, the caller clusters on the host -- outside the three caps
 * above, and IMSEGM_E_CLUSTER_INPUT with the outputs untouched for what scikit-learn raises a ValueError. */
IMSEGM_API int imsegm_dbscan_points(imsegm_ctx *ctx, const double *points, const int32_t *offsets, int nb_sets, double eps,
                                    int min_samples, int32_t *labels_out, int32_t *counts_out, double *centres_out);

#ifdef __cplusplus
}
#endif
#endif /* IMSEGM_HIP_H */
