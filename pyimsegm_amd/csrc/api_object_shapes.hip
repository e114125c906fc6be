// api_object_shapes.hip -- C ABI of the step between annotated egg maps and a ray shape model (imsegm/region_growing.py
// compute_object_shapes :289-331 down to the raw rays of compute_segm_object_shape :259-280).  A stateless call on a context and host
// arrays; arguments are checked before the device is touched; the kernels are in object_shapes.hip.
#include "object_shapes.h"
#include "session.h"

static_assert(OS_MAX_SPAN == IMSEGM_OBJECT_SHAPES_MAX_SPAN, "presence table of object_shapes.hip");

namespace imsegm {

// where the pieces of one call live inside the context's scratch buffer (every piece starts on a 256-byte boundary); the results
// lie side by side behind o_out, so that they come down in one copy
struct OsPlan {
    size_t o_segm = 0, o_parent = 0, o_key = 0, o_table = 0, o_partial = 0, o_blocksum = 0, o_dir = 0, o_obj_key = 0, o_out = 0;
    size_t r_hdr = 0, r_labels = 0, r_moments = 0, r_centres = 0, r_rays = 0, out_bytes = 0;      // relative to o_out
    size_t bytes = 0;
    int table_len = 0;
};

static OsPlan os_plan(int H, int W, int A, int max_objects)
{
    OsPlan p;
    const size_t n = (size_t)H * (size_t)W, m = (size_t)max_objects;
    p.table_len = (int)(n > (size_t)OS_MAX_SPAN ? n : (size_t)OS_MAX_SPAN);
    size_t at = 0;
    auto take = [&at](size_t bytes) {
        const size_t here = at;
        at += (bytes + 255) & ~(size_t)255;
        return here;
    };
    p.o_segm = take(n * 4);
    p.o_parent = take(n * 4);
    p.o_key = take(n * 4);
    p.o_table = take((size_t)p.table_len * 4);
    p.o_partial = take((size_t)OS_RANGE_BLOCKS * 3 * 4);
    p.o_blocksum = take(((size_t)cdiv(p.table_len, 1024) + 1) * 4);
    p.o_dir = take((size_t)A * 8);
    p.o_obj_key = take(m * 4 + 8);
    p.o_out = at;
    at = 0;
    p.r_hdr = take((size_t)OS_HDR_INTS * 4);
    p.r_labels = take(m * 4 + 8);
    p.r_moments = take(m * 24 + 8);
    p.r_centres = take(m * 8 + 8);
    p.r_rays = take(m * A * 4 + 8);
    p.out_bytes = at;
    p.bytes = p.o_out + p.out_bytes;
    return p;
}

}  // namespace imsegm

extern "C" {

int imsegm_object_shapes(imsegm_ctx *ctx, const int32_t *segm, int height, int width, const float *directions, int n_angles,
                         int max_objects, int *n_objects_out, int32_t *labels_out, int64_t *moments_out, int32_t *centres_out,
                         float *rays_out)
{
    if (height < 1 || width < 1) {
        set_error("object_shapes: height and width must be positive");
        return -1;
    }
    if ((size_t)height * (size_t)width >= ((size_t)1 << 31)) {
        set_error("object_shapes: a map of 2^31 pixels or more");
        return -1;
    }
    if (n_angles < 1 || n_angles > IMSEGM_RAY_MAX_ANGLES) {
        set_error("object_shapes: between 1 and IMSEGM_RAY_MAX_ANGLES (" + std::to_string(IMSEGM_RAY_MAX_ANGLES) + ") angles are required");
        return -1;
    }
    if (max_objects < 0 || max_objects > IMSEGM_OBJECT_SHAPES_MAX_OBJECTS) {
        set_error("object_shapes: the capacity must lie in [0, IMSEGM_OBJECT_SHAPES_MAX_OBJECTS]");
        return -1;
    }
    if (!segm || !directions || !n_objects_out || (max_objects > 0 && (!labels_out || !moments_out || !centres_out || !rays_out))) {
        set_error("object_shapes: null argument");
        return -1;
    }
    if (bind(ctx)) return -1;
    hipStream_t st = ctx->stream;
    const size_t n = (size_t)height * width, m = (size_t)max_objects;
    const OsPlan p = os_plan(height, width, n_angles, max_objects);
    if (ctx->gc_buf.ensure(p.bytes)) return -1;
    unsigned char *dev = ctx->gc_buf.as<unsigned char>(), *out = dev + p.o_out;
    unsigned char *host = static_cast<unsigned char *>(ctx->stage(p.out_bytes));
    if (!host) {
        set_error("object_shapes: no page-locked memory for the results");
        return -1;
    }
    OsView v;
    v.H = height, v.W = width, v.A = n_angles, v.max_objects = max_objects, v.table_len = p.table_len;
    v.segm = reinterpret_cast<int32_t *>(dev + p.o_segm);
    v.parent = reinterpret_cast<int32_t *>(dev + p.o_parent);
    v.key = reinterpret_cast<int32_t *>(dev + p.o_key);
    v.table = reinterpret_cast<int32_t *>(dev + p.o_table);
    v.partial = reinterpret_cast<int32_t *>(dev + p.o_partial);
    v.blocksum = reinterpret_cast<int32_t *>(dev + p.o_blocksum);
    v.directions = reinterpret_cast<float *>(dev + p.o_dir);
    v.obj_key = reinterpret_cast<int32_t *>(dev + p.o_obj_key);
    v.hdr = reinterpret_cast<int32_t *>(out + p.r_hdr);
    v.labels = reinterpret_cast<int32_t *>(out + p.r_labels);
    v.moments = reinterpret_cast<long long *>(out + p.r_moments);
    v.centres = reinterpret_cast<int32_t *>(out + p.r_centres);
    v.rays = reinterpret_cast<float *>(out + p.r_rays);
    // one upload (the map, with its direction table), one chain of launches, one download
    HIP_TRY(hipMemcpyAsync(dev + p.o_segm, segm, n * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(dev + p.o_dir, directions, (size_t)n_angles * 8, hipMemcpyHostToDevice, st));
    if (launch_object_shapes(v, st)) return -1;
    HIP_TRY(hipMemcpyAsync(host, out, p.out_bytes, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    const int32_t *hdr = reinterpret_cast<const int32_t *>(host + p.r_hdr);
    if (hdr[OS_MODE] == OS_SPAN) {
        *n_objects_out = -1;
        return IMSEGM_E_OBJECT_CAPS;
    }
    const int count = hdr[OS_COUNT];
    *n_objects_out = count;
    if (count > max_objects) return IMSEGM_E_OBJECT_CAPS;
    const size_t c = (size_t)count;
    if (c > 0 && m > 0) {
        memcpy(labels_out, host + p.r_labels, c * 4);
        memcpy(moments_out, host + p.r_moments, c * 24);
        memcpy(centres_out, host + p.r_centres, c * 8);
        memcpy(rays_out, host + p.r_rays, c * (size_t)n_angles * 4);
    }
    return 0;
}

}  // extern "C"
