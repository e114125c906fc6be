// api_morphology.hip -- C ABI of the step between an egg class map with centre candidates and the ellipse RANSAC
// (imsegm/ellipse_fitting.py split_segm_background_foreground :400-443 and the ray casting of prepare_boundary_points_ray_* :352-597).
// Stateless calls on a context and host arrays; arguments are checked before the device is touched; the kernels are in morphology.hip.
#include "morphology.h"
#include "session.h"

static_assert(MORPH_MAX_RADIUS == IMSEGM_MORPH_MAX_RADIUS, "LDS budget of morphology.hip");

namespace imsegm {

// where the pieces of one call live inside the context's scratch buffer (every piece starts on a 256-byte boundary)
struct MorphPlan {
    size_t o_segm = 0, o_parent = 0, o_touch = 0, o_bg = 0, o_fg = 0, o_tmp = 0, o_pos = 0, o_dir = 0, o_rays_bg = 0, o_rays_fg = 0, bytes = 0;
};

static MorphPlan morph_plan(int H, int W, int P, int A)
{
    MorphPlan p;
    const size_t n = (size_t)H * (size_t)W;
    size_t at = 0;
    auto take = [&at](size_t bytes) {
        const size_t here = at;
        at += (bytes + 255) & ~(size_t)255;
        return here;
    };
    p.o_segm = take(n * 4);
    p.o_parent = take(n * 4);
    p.o_touch = take(n);
    p.o_bg = take(n);
    p.o_fg = take(n);
    p.o_tmp = take(n);                                          // the eroded mask between the two halves of an opening
    p.o_pos = take((size_t)P * 8 + 8);
    p.o_dir = take((size_t)A * 8 + 8);
    p.o_rays_bg = take((size_t)P * A * 4 + 8);
    p.o_rays_fg = take((size_t)P * A * 4 + 8);
    p.bytes = at;
    return p;
}

static int check_split(const char *who, const int32_t *segm, int H, int W, int sel_bg, int sel_fg)
{
    if (H < 1 || W < 1) {
        set_error(std::string(who) + ": height and width must be positive");
        return -1;
    }
    if (!segm) {
        set_error(std::string(who) + ": null class map");
        return -1;
    }
    if (sel_bg > IMSEGM_MORPH_MAX_RADIUS || sel_fg > IMSEGM_MORPH_MAX_RADIUS) {
        set_error(std::string(who) + ": a disc radius above IMSEGM_MORPH_MAX_RADIUS (" + std::to_string(IMSEGM_MORPH_MAX_RADIUS) + ")");
        return -1;
    }
    return morph_size_ok(H, W) ? 0 : -1;
}

// upload the class map, fill the holes, open both masks: seg_bg and (with_fg) seg_fg of the plan are final afterwards
static int split_run(imsegm_ctx *ctx, const int32_t *segm, int H, int W, int sel_bg, int sel_fg, bool with_fg, unsigned char *dev,
                     const MorphPlan &p)
{
    hipStream_t st = ctx->stream;
    const size_t n = (size_t)H * W;
    uint8_t *bg = dev + p.o_bg, *fg = dev + p.o_fg, *tmp = dev + p.o_tmp;
    HIP_TRY(hipMemcpyAsync(dev + p.o_segm, segm, n * 4, hipMemcpyHostToDevice, st));
    if (launch_fill_holes_split(reinterpret_cast<int32_t *>(dev + p.o_segm), H, W, reinterpret_cast<int32_t *>(dev + p.o_parent),
                                dev + p.o_touch, bg, fg, st))
        return -1;
    if (sel_bg > 0) {
        if (launch_disc_morph(bg, H, W, sel_bg, 0, tmp, st)) return -1;
        if (launch_disc_morph(tmp, H, W, sel_bg, 1, bg, st)) return -1;
    }
    if (with_fg && sel_fg > 0) {
        if (launch_disc_morph(fg, H, W, sel_fg, 0, tmp, st)) return -1;
        if (launch_disc_morph(tmp, H, W, sel_fg, 1, fg, st)) return -1;
    }
    return 0;
}

}  // namespace imsegm

extern "C" {

int imsegm_split_background_foreground(imsegm_ctx *ctx, const int32_t *segm, int height, int width, int sel_bg, int sel_fg,
                                       uint8_t *seg_bg_out, uint8_t *seg_fg_out)
{
    if (check_split("split_background_foreground", segm, height, width, sel_bg, sel_fg)) return -1;
    if (!seg_bg_out && !seg_fg_out) {
        set_error("split_background_foreground: no output array");
        return -1;
    }
    if (bind(ctx)) return -1;
    hipStream_t st = ctx->stream;
    const size_t n = (size_t)height * width;
    const MorphPlan p = morph_plan(height, width, 0, 0);
    if (ctx->gc_buf.ensure(p.bytes)) return -1;
    unsigned char *dev = ctx->gc_buf.as<unsigned char>();
    if (split_run(ctx, segm, height, width, sel_bg, sel_fg, seg_fg_out != nullptr, dev, p)) return -1;
    if (seg_bg_out) HIP_TRY(hipMemcpyAsync(seg_bg_out, dev + p.o_bg, n, hipMemcpyDeviceToHost, st));
    if (seg_fg_out) HIP_TRY(hipMemcpyAsync(seg_fg_out, dev + p.o_fg, n, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

int imsegm_boundary_rays(imsegm_ctx *ctx, const int32_t *segm, int height, int width, int sel_bg, int sel_fg, const int32_t *positions,
                         int n_positions, const float *directions, int n_angles, float *rays_bg_out, float *rays_fg_out)
{
    if (check_split("boundary_rays", segm, height, width, sel_bg, sel_fg)) return -1;
    if (n_positions < 0 || (n_positions && !positions) || !directions || n_angles < 1 || n_angles > IMSEGM_RAY_MAX_ANGLES) {
        set_error("boundary_rays: bad arguments (positions, directions and between 1 and IMSEGM_RAY_MAX_ANGLES angles are required)");
        return -1;
    }
    if (!rays_bg_out && !rays_fg_out) {
        set_error("boundary_rays: no output array");
        return -1;
    }
    if (n_positions == 0) return 0;
    if (bind(ctx)) return -1;
    hipStream_t st = ctx->stream;
    const size_t rays = (size_t)n_positions * n_angles;
    const MorphPlan p = morph_plan(height, width, n_positions, n_angles);
    if (ctx->gc_buf.ensure(p.bytes)) return -1;
    unsigned char *dev = ctx->gc_buf.as<unsigned char>();
    HIP_TRY(hipMemcpyAsync(dev + p.o_pos, positions, (size_t)n_positions * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(dev + p.o_dir, directions, (size_t)n_angles * 8, hipMemcpyHostToDevice, st));
    // a NULL rays_fg_out: seg_fg is not opened at all (prepare_boundary_points_ray_dist never reads it)
    if (split_run(ctx, segm, height, width, sel_bg, sel_fg, rays_fg_out != nullptr, dev, p)) return -1;
    float *d_bg = rays_bg_out ? reinterpret_cast<float *>(dev + p.o_rays_bg) : nullptr;
    float *d_fg = rays_fg_out ? reinterpret_cast<float *>(dev + p.o_rays_fg) : nullptr;
    if (launch_boundary_rays(dev + p.o_bg, dev + p.o_fg, height, width, reinterpret_cast<int32_t *>(dev + p.o_pos), n_positions,
                             reinterpret_cast<float *>(dev + p.o_dir), n_angles, d_bg, d_fg, st))
        return -1;
    if (rays_bg_out) HIP_TRY(hipMemcpyAsync(rays_bg_out, d_bg, rays * 4, hipMemcpyDeviceToHost, st));
    if (rays_fg_out) HIP_TRY(hipMemcpyAsync(rays_fg_out, d_fg, rays * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

}  // extern "C"
