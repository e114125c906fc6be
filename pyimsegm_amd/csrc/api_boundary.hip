// api_boundary.hip -- C ABI of the label-map scoring calls: boundary masks, distance maps, boundary distances, label overlaps
// (imsegm/labeling.py contour_binary_map, compute_distance_map, compute_boundary_distances, compute_labels_overlap_matrix).
// Stateless calls on a context and host arrays, plus the boundary distances against the label map a 2-D session or a volume session
// holds.  Arguments are checked before the device is touched; the kernels are in boundary.hip, boundary3d.hip and stats.hip
// (k_label_hist).
#include "session.h"

namespace imsegm {

BoundaryPlan boundary_plan(int H, int W, int kind)
{
    BoundaryPlan p;
    const size_t n = (size_t)H * (size_t)W;
    size_t at = 0;
    auto take = [&at](size_t bytes) {
        const size_t here = at;
        at += (bytes + 255) & ~(size_t)255;
        return here;
    };
    p.o_ref = take(n * 4);                                     // the uploaded label map (the reference map of the distances)
    if (kind == BP_DISTANCES) p.o_seg = take(n * 4);           // the second map (a session brings its own)
    if (kind != BP_MASK) p.o_g = take(n * 4);
    if (kind == BP_DISTANCES || kind == BP_DISTANCES_SESSION) p.o_d2 = take(n * 4);
    if (kind == BP_DISTANCE_MAP) p.o_dist = take(n * 8);
    p.o_mask_a = take(n);
    if (kind == BP_DISTANCES || kind == BP_DISTANCES_SESSION) {
        p.o_mask_b = take(n);
        p.o_counts = take(compact_count_words(n) * 4);
    }
    p.o_flags = take(2 * sizeof(int));
    p.bytes = at;
    return p;
}

static int check_map(const char *what, const void *a, const void *out, int H, int W)
{
    if (!a || !out) {
        set_error(std::string(what) + ": null array");
        return -1;
    }
    if (H < 1 || W < 1) {
        set_error(std::string(what) + ": height and width must be positive");
        return -1;
    }
    return 0;
}

// the distances of the thick boundary of d_ref to the thick boundary of d_seg (both on the device), points in row-major order
static int boundary_distances_run(imsegm_ctx *ctx, const int32_t *d_ref, const int32_t *d_seg, int H, int W, unsigned char *dev,
                                  const BoundaryPlan &p, int32_t *points_out, double *dist_out, int capacity, int *n_out)
{
    hipStream_t st = ctx->stream;
    const size_t n = (size_t)H * W;
    uint8_t *mask_seg = dev + p.o_mask_a, *mask_ref = dev + p.o_mask_b;
    uint32_t *g = reinterpret_cast<uint32_t *>(dev + p.o_g), *d2 = reinterpret_cast<uint32_t *>(dev + p.o_d2);
    uint32_t *counts = reinterpret_cast<uint32_t *>(dev + p.o_counts);
    int *flags = reinterpret_cast<int *>(dev + p.o_flags);
    if (launch_boundary_mask(d_seg, H, W, 0, 0, mask_seg, flags, st)) return -1;
    if (launch_edt(mask_seg, flags, H, W, g, d2, nullptr, st)) return -1;
    if (launch_boundary_mask(d_ref, H, W, 0, 0, mask_ref, flags + 1, st)) return -1;
    if (launch_compact_count(mask_ref, n, counts, st)) return -1;
    const size_t words = compact_count_words(n);
    uint32_t total = 0;
    HIP_TRY(hipMemcpyAsync(&total, counts + (words - 1), 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    *n_out = (int)total;
    if (total == 0) return 0;
    if ((size_t)total > (size_t)capacity) {
        set_error("boundary_distances: " + std::to_string(total) + " boundary points, the output arrays hold " + std::to_string(capacity));
        return -1;
    }
    const size_t b_pts = ((size_t)total * 8 + 255) & ~(size_t)255;
    if (ctx->aux_buf.ensure(b_pts + (size_t)total * 8)) return -1;
    int32_t *d_pts = ctx->aux_buf.as<int32_t>();
    double *d_dist = reinterpret_cast<double *>(ctx->aux_buf.as<unsigned char>() + b_pts);
    if (launch_compact_gather(mask_ref, d2, n, W, counts, d_pts, d_dist, st)) return -1;
    HIP_TRY(hipMemcpyAsync(points_out, d_pts, (size_t)total * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(dist_out, d_dist, (size_t)total * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

// ---------------------------------------------------------------------------------------------------
// volumes: the same calls on D x H x W label maps (thick boundaries only)
// ---------------------------------------------------------------------------------------------------
static BoundaryPlan boundary_plan3d(int D, int H, int W, int kind)
{
    BoundaryPlan p;
    const size_t n = (size_t)D * (size_t)H * (size_t)W;
    size_t at = 0;
    auto take = [&at](size_t bytes) {
        const size_t here = at;
        at += (bytes + 255) & ~(size_t)255;
        return here;
    };
    p.o_ref = take(n * 4);
    if (kind == BP_DISTANCES) p.o_seg = take(n * 4);
    if (kind != BP_MASK) {
        p.o_g = take(n * 4);
        p.o_d2 = take(n * 4);
    }
    if (kind == BP_DISTANCE_MAP) p.o_dist = take(n * 8);
    p.o_mask_a = take(n);
    if (kind == BP_DISTANCES || kind == BP_DISTANCES_SESSION) {
        p.o_mask_b = take(n);
        p.o_counts = take(compact_count_words(n) * 4);
    }
    p.o_flags = take(2 * ((size_t)D + 1) * sizeof(int));       // volume flag + one per slice, for either mask
    p.bytes = at;
    return p;
}

static int check_volume(const char *what, const void *a, const void *out, int D, int H, int W)
{
    if (!a || !out) {
        set_error(std::string(what) + ": null array");
        return -1;
    }
    return edt3d_size_ok(D, H, W) ? 0 : -1;
}

// the distances of the thick boundary of d_ref to the thick boundary of d_seg (both on the device), points in raster order
static int boundary_distances3d_run(imsegm_ctx *ctx, const int32_t *d_ref, const int32_t *d_seg, int D, int H, int W, unsigned char *dev,
                                    const BoundaryPlan &p, int32_t *points_out, double *dist_out, int capacity, int *n_out)
{
    hipStream_t st = ctx->stream;
    const size_t n = (size_t)D * H * W;
    uint8_t *mask_seg = dev + p.o_mask_a, *mask_ref = dev + p.o_mask_b;
    uint32_t *g = reinterpret_cast<uint32_t *>(dev + p.o_g), *d2 = reinterpret_cast<uint32_t *>(dev + p.o_d2);
    uint32_t *counts = reinterpret_cast<uint32_t *>(dev + p.o_counts);
    int *flags_seg = reinterpret_cast<int *>(dev + p.o_flags), *flags_ref = flags_seg + D + 1;
    if (launch_boundary_mask3d(d_seg, D, H, W, mask_seg, flags_seg, st)) return -1;
    if (launch_edt3d(mask_seg, flags_seg, D, H, W, g, d2, nullptr, st)) return -1;
    if (launch_boundary_mask3d(d_ref, D, H, W, mask_ref, flags_ref, st)) return -1;
    if (launch_compact_count(mask_ref, n, counts, st)) return -1;
    const size_t words = compact_count_words(n);
    uint32_t total = 0;
    HIP_TRY(hipMemcpyAsync(&total, counts + (words - 1), 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    *n_out = (int)total;
    if (total == 0) return 0;
    if ((size_t)total > (size_t)capacity) {
        set_error("boundary_distances3d: " + std::to_string(total) + " boundary points, the output arrays hold " + std::to_string(capacity));
        return -1;
    }
    const size_t b_pts = ((size_t)total * 12 + 255) & ~(size_t)255;
    if (ctx->aux_buf.ensure(b_pts + (size_t)total * 8)) return -1;
    int32_t *d_pts = ctx->aux_buf.as<int32_t>();
    double *d_dist = reinterpret_cast<double *>(ctx->aux_buf.as<unsigned char>() + b_pts);
    if (launch_compact_gather3d(mask_ref, d2, n, H, W, counts, d_pts, d_dist, st)) return -1;
    HIP_TRY(hipMemcpyAsync(points_out, d_pts, (size_t)total * 12, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(dist_out, d_dist, (size_t)total * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

}  // namespace imsegm

extern "C" {

int imsegm_boundary_mask(imsegm_ctx *ctx, const int32_t *labels, int height, int width, int mode, int label, uint8_t *mask_out)
{
    if (check_map("boundary_mask", labels, mask_out, height, width)) return -1;
    if (mode < IMSEGM_BOUNDARY_THICK || mode > IMSEGM_BOUNDARY_CONTOUR_BORDER) {
        set_error("boundary_mask: unknown mode");
        return -1;
    }
    if (bind(ctx)) return -1;
    hipStream_t st = ctx->stream;
    const size_t n = (size_t)height * width;
    const BoundaryPlan p = boundary_plan(height, width, BP_MASK);
    if (ctx->gc_buf.ensure(p.bytes)) return -1;
    unsigned char *dev = ctx->gc_buf.as<unsigned char>();
    HIP_TRY(hipMemcpyAsync(dev + p.o_ref, labels, n * 4, hipMemcpyHostToDevice, st));
    if (launch_boundary_mask(reinterpret_cast<int32_t *>(dev + p.o_ref), height, width, mode, label, dev + p.o_mask_a,
                             reinterpret_cast<int *>(dev + p.o_flags), st))
        return -1;
    HIP_TRY(hipMemcpyAsync(mask_out, dev + p.o_mask_a, n, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

int imsegm_distance_map(imsegm_ctx *ctx, const int32_t *labels, int height, int width, int mode, int label, double *dist_out)
{
    if (check_map("distance_map", labels, dist_out, height, width)) return -1;
    if (mode < IMSEGM_BOUNDARY_THICK || mode > IMSEGM_BOUNDARY_CONTOUR_BORDER) {
        set_error("distance_map: unknown mode");
        return -1;
    }
    if (!edt_size_ok(height, width)) return -1;
    if (bind(ctx)) return -1;
    hipStream_t st = ctx->stream;
    const size_t n = (size_t)height * width;
    const BoundaryPlan p = boundary_plan(height, width, BP_DISTANCE_MAP);
    if (ctx->gc_buf.ensure(p.bytes)) return -1;
    unsigned char *dev = ctx->gc_buf.as<unsigned char>();
    int *flags = reinterpret_cast<int *>(dev + p.o_flags);
    HIP_TRY(hipMemcpyAsync(dev + p.o_ref, labels, n * 4, hipMemcpyHostToDevice, st));
    if (launch_boundary_mask(reinterpret_cast<int32_t *>(dev + p.o_ref), height, width, mode, label, dev + p.o_mask_a, flags, st)) return -1;
    if (launch_edt(dev + p.o_mask_a, flags, height, width, reinterpret_cast<uint32_t *>(dev + p.o_g), nullptr,
                   reinterpret_cast<double *>(dev + p.o_dist), st))
        return -1;
    HIP_TRY(hipMemcpyAsync(dist_out, dev + p.o_dist, n * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

int imsegm_boundary_distances(imsegm_ctx *ctx, const int32_t *segm_ref, const int32_t *segm, int height, int width,
                              int32_t *points_out, double *dist_out, int capacity, int *n_points_out)
{
    if (check_map("boundary_distances", segm_ref, segm, height, width)) return -1;
    if (!n_points_out || capacity < 0 || (capacity > 0 && (!points_out || !dist_out))) {
        set_error("boundary_distances: output arrays and the point count are required");
        return -1;
    }
    if (!edt_size_ok(height, width)) return -1;
    if (bind(ctx)) return -1;
    hipStream_t st = ctx->stream;
    const size_t n = (size_t)height * width;
    const BoundaryPlan p = boundary_plan(height, width, BP_DISTANCES);
    if (ctx->gc_buf.ensure(p.bytes)) return -1;
    unsigned char *dev = ctx->gc_buf.as<unsigned char>();
    HIP_TRY(hipMemcpyAsync(dev + p.o_ref, segm_ref, n * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(dev + p.o_seg, segm, n * 4, hipMemcpyHostToDevice, st));
    return boundary_distances_run(ctx, reinterpret_cast<int32_t *>(dev + p.o_ref), reinterpret_cast<int32_t *>(dev + p.o_seg), height,
                                  width, dev, p, points_out, dist_out, capacity, n_points_out);
}

int imsegm_image2d_boundary_distances(imsegm_image2d *im, const int32_t *segm_ref, int32_t *points_out, double *dist_out, int capacity,
                                      int *n_points_out)
{
    if (!im) {
        set_error("null session");
        return -1;
    }
    if (wrong_kind(im, false)) return -1;
    if (!im->have_labels) {
        set_error("boundary_distances needs a label map (run slic or set_labels first)");
        return -1;
    }
    if (!segm_ref || !n_points_out || capacity < 0 || (capacity > 0 && (!points_out || !dist_out))) {
        set_error("boundary_distances: the reference map, output arrays and the point count are required");
        return -1;
    }
    if (!edt_size_ok(im->H, im->W)) return -1;
    imsegm_ctx *ctx = im->ctx;
    if (bind(ctx)) return -1;
    hipStream_t st = ctx->stream;
    const BoundaryPlan p = boundary_plan(im->H, im->W, BP_DISTANCES_SESSION);
    if (ctx->gc_buf.ensure(p.bytes)) return -1;
    unsigned char *dev = ctx->gc_buf.as<unsigned char>();
    HIP_TRY(hipMemcpyAsync(dev + p.o_ref, segm_ref, im->n * 4, hipMemcpyHostToDevice, st));
    return boundary_distances_run(ctx, reinterpret_cast<int32_t *>(dev + p.o_ref), im->labels.as<int32_t>(), im->H, im->W, dev, p,
                                  points_out, dist_out, capacity, n_points_out);
}

int imsegm_boundary_mask3d(imsegm_ctx *ctx, const int32_t *labels, int depth, int height, int width, uint8_t *mask_out)
{
    if (check_volume("boundary_mask3d", labels, mask_out, depth, height, width)) return -1;
    if (bind(ctx)) return -1;
    hipStream_t st = ctx->stream;
    const size_t n = (size_t)depth * height * width;
    const BoundaryPlan p = boundary_plan3d(depth, height, width, BP_MASK);
    if (ctx->gc_buf.ensure(p.bytes)) return -1;
    unsigned char *dev = ctx->gc_buf.as<unsigned char>();
    HIP_TRY(hipMemcpyAsync(dev + p.o_ref, labels, n * 4, hipMemcpyHostToDevice, st));
    if (launch_boundary_mask3d(reinterpret_cast<int32_t *>(dev + p.o_ref), depth, height, width, dev + p.o_mask_a,
                               reinterpret_cast<int *>(dev + p.o_flags), st))
        return -1;
    HIP_TRY(hipMemcpyAsync(mask_out, dev + p.o_mask_a, n, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

int imsegm_distance_map3d(imsegm_ctx *ctx, const int32_t *labels, int depth, int height, int width, double *dist_out)
{
    if (check_volume("distance_map3d", labels, dist_out, depth, height, width)) return -1;
    if (bind(ctx)) return -1;
    hipStream_t st = ctx->stream;
    const size_t n = (size_t)depth * height * width;
    const BoundaryPlan p = boundary_plan3d(depth, height, width, BP_DISTANCE_MAP);
    if (ctx->gc_buf.ensure(p.bytes)) return -1;
    unsigned char *dev = ctx->gc_buf.as<unsigned char>();
    int *flags = reinterpret_cast<int *>(dev + p.o_flags);
    HIP_TRY(hipMemcpyAsync(dev + p.o_ref, labels, n * 4, hipMemcpyHostToDevice, st));
    if (launch_boundary_mask3d(reinterpret_cast<int32_t *>(dev + p.o_ref), depth, height, width, dev + p.o_mask_a, flags, st)) return -1;
    if (launch_edt3d(dev + p.o_mask_a, flags, depth, height, width, reinterpret_cast<uint32_t *>(dev + p.o_g),
                     reinterpret_cast<uint32_t *>(dev + p.o_d2), reinterpret_cast<double *>(dev + p.o_dist), st))
        return -1;
    HIP_TRY(hipMemcpyAsync(dist_out, dev + p.o_dist, n * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

int imsegm_boundary_distances3d(imsegm_ctx *ctx, const int32_t *segm_ref, const int32_t *segm, int depth, int height, int width,
                                int32_t *points_out, double *dist_out, int capacity, int *n_points_out)
{
    if (check_volume("boundary_distances3d", segm_ref, segm, depth, height, width)) return -1;
    if (!n_points_out || capacity < 0 || (capacity > 0 && (!points_out || !dist_out))) {
        set_error("boundary_distances3d: output arrays and the point count are required");
        return -1;
    }
    if (bind(ctx)) return -1;
    hipStream_t st = ctx->stream;
    const size_t n = (size_t)depth * height * width;
    const BoundaryPlan p = boundary_plan3d(depth, height, width, BP_DISTANCES);
    if (ctx->gc_buf.ensure(p.bytes)) return -1;
    unsigned char *dev = ctx->gc_buf.as<unsigned char>();
    HIP_TRY(hipMemcpyAsync(dev + p.o_ref, segm_ref, n * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(dev + p.o_seg, segm, n * 4, hipMemcpyHostToDevice, st));
    return boundary_distances3d_run(ctx, reinterpret_cast<int32_t *>(dev + p.o_ref), reinterpret_cast<int32_t *>(dev + p.o_seg), depth,
                                    height, width, dev, p, points_out, dist_out, capacity, n_points_out);
}

int imsegm_volume_boundary_distances(imsegm_image2d *vol, const int32_t *segm_ref, int32_t *points_out, double *dist_out, int capacity,
                                     int *n_points_out)
{
    if (!vol) {
        set_error("null session");
        return -1;
    }
    if (wrong_kind(vol, true)) return -1;
    if (!vol->have_labels) {
        set_error("boundary_distances needs a label map (run slic or label_cc first)");
        return -1;
    }
    if (!segm_ref || !n_points_out || capacity < 0 || (capacity > 0 && (!points_out || !dist_out))) {
        set_error("boundary_distances: the reference map, output arrays and the point count are required");
        return -1;
    }
    if (!edt3d_size_ok(vol->D, vol->H, vol->W)) return -1;
    imsegm_ctx *ctx = vol->ctx;
    if (bind(ctx)) return -1;
    hipStream_t st = ctx->stream;
    const BoundaryPlan p = boundary_plan3d(vol->D, vol->H, vol->W, BP_DISTANCES_SESSION);
    if (ctx->gc_buf.ensure(p.bytes)) return -1;
    unsigned char *dev = ctx->gc_buf.as<unsigned char>();
    HIP_TRY(hipMemcpyAsync(dev + p.o_ref, segm_ref, vol->n * 4, hipMemcpyHostToDevice, st));
    return boundary_distances3d_run(ctx, reinterpret_cast<int32_t *>(dev + p.o_ref), vol->labels.as<int32_t>(), vol->D, vol->H, vol->W, dev,
                                    p, points_out, dist_out, capacity, n_points_out);
}

int imsegm_labels_overlap(imsegm_ctx *ctx, const int32_t *seg1, const int32_t *seg2, size_t n, int n_labels1, int n_labels2,
                          int64_t *overlap_out)
{
    if (!seg1 || !seg2 || !overlap_out || n_labels1 < 1 || n_labels2 < 1) {
        set_error("labels_overlap: two label arrays, an output and positive extents are required");
        return -1;
    }
    const size_t bins = (size_t)n_labels1 * (size_t)n_labels2;
    if (bins > ((size_t)1 << 28)) {                            // (2 GB of counts)
        set_error("labels_overlap: matrix of more than 2^28 entries");
        return -1;
    }
    if (n > ((size_t)1 << 40)) {
        set_error("labels_overlap: more than 2^40 pixels");
        return -1;
    }
    if (bind(ctx)) return -1;
    hipStream_t st = ctx->stream;
    auto al = [](size_t v) { return (v + 255) & ~(size_t)255; };
    const size_t b_seg = al(n * 4 + 32);
    if (ctx->gc_buf.ensure(2 * b_seg + bins * 8)) return -1;
    unsigned char *dev = ctx->gc_buf.as<unsigned char>();
    if (n) {
        HIP_TRY(hipMemcpyAsync(dev, seg1, n * 4, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(dev + b_seg, seg2, n * 4, hipMemcpyHostToDevice, st));
    }
    unsigned long long *hist = reinterpret_cast<unsigned long long *>(dev + 2 * b_seg);
    // k_label_hist of stats.hip as it is: pairs with a label outside [0, extent) -- the negative ones -- are not counted
    if (launch_label_hist(reinterpret_cast<int32_t *>(dev), reinterpret_cast<int32_t *>(dev + b_seg), n, n_labels1, n_labels2, hist, st))
        return -1;
    HIP_TRY(hipMemcpyAsync(overlap_out, hist, bins * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

}  // extern "C"
