// api_resize.hip -- C ABI of the cut-and-scale step of the egg chain (experiments_ovary_detect/run_ellipse_cut_scale.py of the
// reference: extract_ellipse_object :46-72): imsegm_resize_crops, the anti-aliased resize of a batch of crops with the export, and
// imsegm_ellipse_cut_scale, the whole loop over the ellipses of one image with the crops staying on the device between the cut and
// the resize.  Stateless calls on a context and host arrays; arguments and caps are checked before the device is touched.  The
// kernels are in resize.hip, cut_objects.hip (the masks of ellipses) and ellipse_place.h (the inside test).  The two fp64 steps
// that numpy and scipy define belong to the caller, as hooks: the geometry of an object from its moments (as imsegm_cut_objects)
// and the weights of the blur.
#include <algorithm>
#include <vector>

#include "cut_objects.h"
#include "ellipse_place.h"
#include "resize.h"
#include "session.h"

static_assert(RESIZE_MAX_RADIUS == IMSEGM_RESIZE_MAX_RADIUS, "LDS budget of resize.hip");
static_assert(CUT_MAX_LABELS == IMSEGM_RESIZE_MAX_CROPS, "the chain cuts what it resizes");

namespace imsegm {

namespace {

constexpr int RESIZE_MAX_SIDE = 32768;                 // rows or columns of a crop and of the output
constexpr size_t RESIZE_MAX_PACKED = (size_t)1 << 30;  // bytes of all crops of one call
constexpr size_t RESIZE_MAX_VALUES = (size_t)1 << 28;  // n h w C of one call (2 GiB of doubles)

struct Carve {
    size_t at = 0;
    size_t take(size_t bytes)
    {
        const size_t here = at;
        at += (bytes + 255) & ~(size_t)255;
        return here;
    }
};

// sizes and caps of the output: 0, -1 with a message, or IMSEGM_E_OBJECT_CAPS
int check_output(const char *who, int n, int channels, int out_h, int out_w)
{
    if (n < 1 || channels < 1 || out_h < 1 || out_w < 1) {
        set_error(std::string(who) + ": the numbers of crops and channels and the output size must be positive");
        return -1;
    }
    if (n > IMSEGM_RESIZE_MAX_CROPS || channels > IMSEGM_CUT_OBJECTS_MAX_CHANNELS || out_h > RESIZE_MAX_SIDE || out_w > RESIZE_MAX_SIDE ||
        (size_t)n * (size_t)out_h * (size_t)out_w * (size_t)channels > RESIZE_MAX_VALUES)
        return IMSEGM_E_OBJECT_CAPS;
    return 0;
}

// the table of the crops from their sizes and radii: 0, -1 with a message, or IMSEGM_E_OBJECT_CAPS
int crop_table(const char *who, int n, int channels, const int32_t *sizes, const int32_t *radii, std::vector<ResizeCrop> &crops,
               size_t *total)
{
    crops.resize((size_t)n);
    size_t at = 0;
    for (int k = 0; k < n; ++k) {
        const int h = sizes[2 * k], w = sizes[2 * k + 1], r0 = radii[2 * k], r1 = radii[2 * k + 1];
        if (h < 1 || w < 1 || r0 < 0 || r1 < 0) {
            set_error(std::string(who) + ": crop " + std::to_string(k) + " has a side below 1 or a negative blur radius");
            return -1;
        }
        if (h > RESIZE_MAX_SIDE || w > RESIZE_MAX_SIDE || r0 > RESIZE_MAX_RADIUS || r1 > RESIZE_MAX_RADIUS) return IMSEGM_E_OBJECT_CAPS;
        crops[k].offset = (long long)at;
        crops[k].h = h, crops[k].w = w, crops[k].radius[0] = r0, crops[k].radius[1] = r1;
        at += (size_t)h * w * channels;
        if (at > RESIZE_MAX_PACKED) return IMSEGM_E_OBJECT_CAPS;
    }
    *total = at;
    return 0;
}

// the crops `d_packed` (device, as `crops` lays them out) -> out / out_u8 (host; either may be NULL), through ctx->resize_buf
int resize_run(imsegm_ctx *ctx, const uint8_t *d_packed, const std::vector<ResizeCrop> &crops, size_t total, int C, int h, int w,
               const double *weights, double *out, uint8_t *out_u8)
{
    hipStream_t st = ctx->stream;
    const size_t n = crops.size(), values = n * h * w * C;
    std::vector<int> prefix(n + 1, 0);
    int max_radius[2] = { 0, 0 };
    for (size_t k = 0; k < n; ++k) {
        prefix[k + 1] = prefix[k] + cdiv(crops[k].h, RESIZE_TILE_H) * cdiv(crops[k].w, RESIZE_TILE_W);
        max_radius[0] = std::max(max_radius[0], crops[k].radius[0]);
        max_radius[1] = std::max(max_radius[1], crops[k].radius[1]);
    }
    Carve c;
    const size_t o_crops = c.take(n * sizeof(ResizeCrop)), o_prefix = c.take((n + 1) * 4), o_weights = c.take(n * 2 * RESIZE_TAPS * 8);
    const size_t o_range = c.take(n * 8), o_max = c.take(n * 8), o_tmp = c.take(total), o_blur = c.take(total), o_out = c.take(values * 8);
    const size_t o_u8 = out_u8 ? c.take(values) : 0;
    if (ctx->resize_buf.ensure(c.at)) return -1;
    unsigned char *dev = ctx->resize_buf.as<unsigned char>();
    const ResizeCrop *d_crops = reinterpret_cast<ResizeCrop *>(dev + o_crops);
    const int *d_prefix = reinterpret_cast<int *>(dev + o_prefix);
    const double *d_weights = reinterpret_cast<double *>(dev + o_weights);
    unsigned *d_range = reinterpret_cast<unsigned *>(dev + o_range);
    unsigned long long *d_max = reinterpret_cast<unsigned long long *>(dev + o_max);
    double *d_out = reinterpret_cast<double *>(dev + o_out);
    // (pageable sources: each copy has left its source when the call returns)
    HIP_TRY(hipMemcpyAsync(dev + o_crops, crops.data(), n * sizeof(ResizeCrop), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(dev + o_prefix, prefix.data(), (n + 1) * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(dev + o_weights, weights, n * 2 * RESIZE_TAPS * 8, hipMemcpyHostToDevice, st));
    {
        std::vector<unsigned> range(2 * n);
        for (size_t k = 0; k < n; ++k) range[2 * k] = 0xffffffffu, range[2 * k + 1] = 0u;
        HIP_TRY(hipMemcpyAsync(d_range, range.data(), n * 8, hipMemcpyHostToDevice, st));
        HIP_TRY(hipStreamSynchronize(st));             // (`range` and `prefix` leave scope)
    }
    HIP_TRY(hipMemsetAsync(d_max, 0, n * 8, st));
    if (launch_resize_blur(d_packed, dev + o_tmp, d_crops, d_prefix, prefix[n], (int)n, C, d_weights, 0, max_radius[0], nullptr, st)) return -1;
    if (launch_resize_blur(dev + o_tmp, dev + o_blur, d_crops, d_prefix, prefix[n], (int)n, C, d_weights, 1, max_radius[1], d_range, st))
        return -1;
    if (launch_resize_gather(dev + o_blur, d_crops, (int)n, C, h, w, d_range, d_out, d_max, st)) return -1;
    if (out_u8) {
        if (launch_resize_export(d_out, (int)n, (size_t)h * w * C, d_max, dev + o_u8, st)) return -1;
        HIP_TRY(hipMemcpyAsync(out_u8, dev + o_u8, values, hipMemcpyDeviceToHost, st));
    }
    if (out) HIP_TRY(hipMemcpyAsync(out, d_out, values * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

}  // namespace

}  // namespace imsegm

extern "C" {

int imsegm_resize_crops(imsegm_ctx *ctx, const uint8_t *packed, const int64_t *offsets, const int32_t *sizes, int n, int channels,
                        int out_h, int out_w, const int32_t *radii, const double *weights, double *out, uint8_t *out_u8)
{
    if (!packed || !offsets || !sizes || !radii || !weights || (!out && !out_u8)) {
        set_error("resize_crops: null argument");
        return -1;
    }
    if (const int status = check_output("resize_crops", n, channels, out_h, out_w)) return status;
    std::vector<ResizeCrop> crops;
    size_t total = 0;
    if (const int status = crop_table("resize_crops", n, channels, sizes, radii, crops, &total)) return status;
    for (int k = 0; k <= n; ++k)
        if (offsets[k] != (k < n ? (int64_t)crops[k].offset : (int64_t)total)) {
            set_error("resize_crops: the offsets are not the running sums of the crop sizes");
            return -1;
        }
    if (bind(ctx)) return -1;
    if (ctx->aux_buf.ensure(total)) return -1;
    HIP_TRY(hipMemcpyAsync(ctx->aux_buf.p, packed, total, hipMemcpyHostToDevice, ctx->stream));
    return resize_run(ctx, ctx->aux_buf.as<uint8_t>(), crops, total, channels, out_h, out_w, weights, out, out_u8);
}

int imsegm_ellipse_cut_scale(imsegm_ctx *ctx, const uint8_t *image, int height, int width, int channels, int n, const int32_t *geom,
                             const double *sincos, const uint8_t *bg_color, int out_h, int out_w, imsegm_cut_geometry_fn geometry,
                             imsegm_blur_taps_fn taps, void *user, double *out, uint8_t *out_u8, int *first_empty_out)
{
    if (!image || !geom || !sincos || !bg_color || !geometry || !taps || !first_empty_out || (!out && !out_u8)) {
        set_error("ellipse_cut_scale: null argument");
        return -1;
    }
    if (const int status = check_output("ellipse_cut_scale", n, channels, out_h, out_w)) return status;
    int max_box_rows = 0;
    if (check_ellipses("ellipse_cut_scale", image, height, width, n, geom, sincos, &max_box_rows)) return -1;
    if (bind(ctx)) return -1;
    hipStream_t st = ctx->stream;
    const size_t pixels = (size_t)height * width, m = (size_t)n;
    Carve c;
    const size_t o_img = c.take(pixels * channels), o_ell = c.take(m * ELLIPSE_GEOM_INTS * 4), o_sincos = c.take(m * 16),
                 o_geom = c.take(m * sizeof(CutGeom)), o_frames = c.take(m * sizeof(CutFrame)), o_crops = c.take(m * sizeof(CutCrop));
    const size_t o_mom = c.take(m * CUT_MOMENT_WORDS * 8), o_smin = c.take(m * 8), o_smax = c.take(m * 8);
    const size_t o_cmin = c.take(m * 8), o_cmax = c.take(m * 8);
    if (ctx->gc_buf.ensure(c.at)) return -1;
    unsigned char *dev = ctx->gc_buf.as<unsigned char>();
    const int32_t *d_ell = reinterpret_cast<int32_t *>(dev + o_ell);
    const double *d_sincos = reinterpret_cast<double *>(dev + o_sincos);
    const CutGeom *d_geom = reinterpret_cast<CutGeom *>(dev + o_geom);
    // one upload of the image; no mask goes up
    HIP_TRY(hipMemcpyAsync(dev + o_img, image, pixels * channels, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(dev + o_ell, geom, m * ELLIPSE_GEOM_INTS * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(dev + o_sincos, sincos, m * 16, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(dev + o_mom, 0, m * CUT_MOMENT_WORDS * 8, st));
    HIP_TRY(hipMemsetAsync(dev + o_smin, 0x7f, m * 8, st));
    HIP_TRY(hipMemsetAsync(dev + o_smax, 0xff, m * 8, st));
    HIP_TRY(hipMemsetAsync(dev + o_cmin, 0x7f, m * 8, st));
    HIP_TRY(hipMemsetAsync(dev + o_cmax, 0xff, m * 8, st));
    if (launch_cut_ellipse_moments(d_ell, d_sincos, n, max_box_rows, reinterpret_cast<unsigned long long *>(dev + o_mom),
                                   reinterpret_cast<int *>(dev + o_smin), reinterpret_cast<int *>(dev + o_smax), st))
        return -1;
    const size_t first_bytes = o_cmin - o_mom;
    unsigned char *host = static_cast<unsigned char *>(ctx->stage(first_bytes));
    if (!host) {
        set_error("ellipse_cut_scale: no page-locked memory for the moments");
        return -1;
    }
    HIP_TRY(hipMemcpyAsync(host, dev + o_mom, first_bytes, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    std::vector<int64_t> words(m * IMSEGM_CUT_MOMENT_WORDS);
    {
        const int64_t *mom = reinterpret_cast<const int64_t *>(host);
        const int32_t *smin = reinterpret_cast<const int32_t *>(host + (o_smin - o_mom)), *smax = reinterpret_cast<const int32_t *>(host + (o_smax - o_mom));
        for (size_t k = 0; k < m; ++k) {
            int64_t *w = words.data() + k * IMSEGM_CUT_MOMENT_WORDS;
            for (int i = 0; i < CUT_MOMENT_WORDS; ++i) w[i] = mom[k * CUT_MOMENT_WORDS + i];
            w[6] = smin[2 * k], w[7] = smax[2 * k], w[8] = smin[2 * k + 1], w[9] = smax[2 * k + 1];
        }
    }
    std::vector<CutGeom> cut_geom(m);
    std::vector<CutFrame> frames(m);
    if (geometry(user, n, 1, height, width, words.data(), reinterpret_cast<double *>(cut_geom.data()),
                 reinterpret_cast<int32_t *>(frames.data()))) {
        set_error("ellipse_cut_scale: the geometry hook refused the objects");
        return -1;
    }
    int win_h = 1, win_w = 1;
    for (size_t k = 0; k < m; ++k) {
        const CutFrame &f = frames[k];
        if (f.canvas_h < 1 || f.canvas_w < 1 || f.canvas_h > height + width + 2 || f.canvas_w > height + width + 2 || f.r0 < 0 ||
            f.c0 < 0 || f.r1 > f.canvas_h || f.c1 > f.canvas_w || f.r0 > f.r1 || f.c0 > f.c1) {
            set_error("ellipse_cut_scale: the geometry hook returned a window outside its canvas");
            return -1;
        }
        win_h = std::max(win_h, f.r1 - f.r0);
        win_w = std::max(win_w, f.c1 - f.c0);
    }
    HIP_TRY(hipMemcpyAsync(dev + o_geom, cut_geom.data(), m * sizeof(CutGeom), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(dev + o_frames, frames.data(), m * sizeof(CutFrame), hipMemcpyHostToDevice, st));
    if (launch_cut_canvas_boxes_ellipses(d_ell, d_sincos, height, width, d_geom, reinterpret_cast<CutFrame *>(dev + o_frames), n, win_h, win_w,
                                         reinterpret_cast<int *>(dev + o_cmin), reinterpret_cast<int *>(dev + o_cmax), st))
        return -1;
    std::vector<int32_t> cbox(m * 4);
    HIP_TRY(hipMemcpyAsync(cbox.data(), dev + o_cmin, m * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(cbox.data() + m * 2, dev + o_cmax, m * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    // the crops: the box of every turned mask, no padding (cut_object(img, mask, 0, ...) of the script)
    std::vector<CutCrop> cut_crops(m);
    std::vector<int32_t> sizes(m * 2);
    size_t total = 0;
    int crop_h = 1, crop_w = 1;
    *first_empty_out = -1;
    for (size_t k = 0; k < m; ++k) {
        const int lo_r = cbox[2 * k], lo_c = cbox[2 * k + 1], hi_r = cbox[2 * m + 2 * k], hi_c = cbox[2 * m + 2 * k + 1];
        if (hi_r < 0) {                                // regionprops(...)[0] of the reference fails on the turned mask
            *first_empty_out = (int)k;
            return 0;
        }
        CutCrop &crop = cut_crops[k];
        crop.r0 = lo_r, crop.c0 = lo_c, crop.h = hi_r + 1 - lo_r, crop.w = hi_c + 1 - lo_c;
        crop.offset = (long long)total;
        sizes[2 * k] = crop.h, sizes[2 * k + 1] = crop.w;
        total += (size_t)crop.h * crop.w * channels;
        crop_h = std::max(crop_h, crop.h);
        crop_w = std::max(crop_w, crop.w);
        if (total > RESIZE_MAX_PACKED) return IMSEGM_E_OBJECT_CAPS;
    }
    // the weights of the blur for these sizes, as scipy makes them: the caller's
    std::vector<int32_t> radii(m * 2, 0);
    std::vector<double> weights(m * 2 * RESIZE_TAPS, 0.0);
    if (taps(user, n, sizes.data(), out_h, out_w, radii.data(), weights.data())) {
        set_error("ellipse_cut_scale: the hook of the blur weights failed");
        return -1;
    }
    std::vector<ResizeCrop> crops;
    size_t packed = 0;
    if (const int status = crop_table("ellipse_cut_scale", n, channels, sizes.data(), radii.data(), crops, &packed)) return status;
    // the crops stay on the device: the cut writes them into the second scratch, the resize reads them there
    if (ctx->aux_buf.ensure(total)) return -1;
    uint32_t bg = 0;
    for (int ch = 0; ch < channels; ++ch) bg |= (uint32_t)bg_color[ch] << (8 * ch);
    HIP_TRY(hipMemcpyAsync(dev + o_crops, cut_crops.data(), m * sizeof(CutCrop), hipMemcpyHostToDevice, st));
    if (launch_cut_write_ellipses(dev + o_img, d_ell, d_sincos, height, width, channels, d_geom, reinterpret_cast<CutCrop *>(dev + o_crops), n,
                                  crop_h, crop_w, bg, ctx->aux_buf.as<uint8_t>(), st))
        return -1;
    HIP_TRY(hipStreamSynchronize(st));                  // (`cut_crops` is pageable and leaves scope before the stream is drained)
    return resize_run(ctx, ctx->aux_buf.as<uint8_t>(), crops, total, channels, out_h, out_w, weights.data(), out, out_u8);
}

}  // extern "C"
