// api_annotation.hip -- C ABI of the annotation calls (imsegm/annotation.py): colour matching, label painting, colour counts, the
// nearest-valid-pixel transform and their composition quantize_image_nearest_pixel.  Stateless calls on a context and host arrays.
// Arguments are checked before the device is touched; the kernels are in annotation.hip.
#include "annotation.h"
#include "session.h"

namespace imsegm {

namespace {

// carves 256-byte aligned pieces out of one scratch allocation
struct Carve {
    size_t at = 0;
    size_t take(size_t bytes)
    {
        const size_t here = at;
        at += (bytes + 255) & ~(size_t)255;
        return here;
    }
};

constexpr size_t ANNOT_MAX_PIXELS = 0xffffffffull;     // counts are uint32

int check_pixels(const char *what, size_t n)
{
    if (n < 1 || n > ANNOT_MAX_PIXELS) {
        set_error(std::string(what) + ": 1 to 2^32 - 1 pixels");
        return -1;
    }
    return 0;
}

int check_table(const char *what, const uint8_t *colors, int n_colors)
{
    if (!colors || n_colors < 1 || n_colors > ANNOT_MAX_COLORS) {
        set_error(std::string(what) + ": a colour table holds 1 to " + std::to_string(ANNOT_MAX_COLORS) + " colours");
        return -1;
    }
    return 0;
}

void pack_keys(const uint8_t *colors, int n, uint32_t *keys)
{
    for (int k = 0; k < n; ++k) keys[k] = ((uint32_t)colors[3 * k] << 16) | ((uint32_t)colors[3 * k + 1] << 8) | (uint32_t)colors[3 * k + 2];
}

int check_nearest_size(int H, int W)
{
    if (!edt_size_ok(H, W)) return -1;
    if (H > 65535) {                                   // (gridDim.y of the row pass)
        set_error("annot_nearest_valid: more than 65535 rows");
        return -1;
    }
    return 0;
}

}  // namespace

}  // namespace imsegm

extern "C" {

int imsegm_annot_match(imsegm_ctx *ctx, const uint8_t *image, size_t n_pixels, const uint8_t *colors, const int32_t *labels, int n_colors,
                       int mode, void *out, int64_t *unmatched_out)
{
    if (!image || !out) {
        set_error("annot_match: null array");
        return -1;
    }
    if (check_pixels("annot_match", n_pixels) || check_table("annot_match", colors, n_colors)) return -1;
    if (mode < IMSEGM_ANNOT_MATCH_EXACT || mode > IMSEGM_ANNOT_MATCH_NEAREST_COLOR) {
        set_error("annot_match: unknown mode");
        return -1;
    }
    uint32_t keys[ANNOT_MAX_COLORS];
    int32_t labs[ANNOT_MAX_COLORS];
    pack_keys(colors, n_colors, keys);
    for (int k = 0; k < n_colors; ++k) {
        labs[k] = (mode == IMSEGM_ANNOT_MATCH_EXACT && labels) ? labels[k] : k;
        if (labs[k] < 0) {
            set_error("annot_match: labels must not be negative (-1 marks a pixel without an entry)");
            return -1;
        }
    }
    if (bind(ctx)) return -1;
    hipStream_t st = ctx->stream;
    Carve c;
    const size_t out_bytes = mode == IMSEGM_ANNOT_MATCH_NEAREST_COLOR ? n_pixels * 3 : n_pixels * 4;
    const size_t o_img = c.take(n_pixels * 3), o_out = c.take(out_bytes), o_keys = c.take(sizeof(keys)), o_labs = c.take(sizeof(labs)),
                 o_cnt = c.take(8);
    if (ctx->gc_buf.ensure(c.at)) return -1;
    unsigned char *dev = ctx->gc_buf.as<unsigned char>();
    unsigned long long *d_cnt = reinterpret_cast<unsigned long long *>(dev + o_cnt);
    HIP_TRY(hipMemcpyAsync(dev + o_img, image, n_pixels * 3, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(dev + o_keys, keys, (size_t)n_colors * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(dev + o_labs, labs, (size_t)n_colors * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(d_cnt, 0, 8, st));
    if (launch_annot_match(dev + o_img, n_pixels, reinterpret_cast<uint32_t *>(dev + o_keys), reinterpret_cast<int32_t *>(dev + o_labs),
                           n_colors, mode, dev + o_out, d_cnt, st))
        return -1;
    unsigned long long missed = 0;
    HIP_TRY(hipMemcpyAsync(out, dev + o_out, out_bytes, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(&missed, d_cnt, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (unmatched_out) *unmatched_out = (int64_t)missed;
    return 0;
}

int imsegm_annot_paint(imsegm_ctx *ctx, const int32_t *labels, size_t n_pixels, int min_label, int n_table, const uint8_t *table,
                       const uint8_t *present, uint8_t *image_out)
{
    if (!labels || !image_out || !present) {
        set_error("annot_paint: null array");
        return -1;
    }
    if (check_pixels("annot_paint", n_pixels) || check_table("annot_paint", table, n_table)) return -1;
    uint32_t keys[ANNOT_MAX_COLORS];
    pack_keys(table, n_table, keys);
    if (bind(ctx)) return -1;
    hipStream_t st = ctx->stream;
    Carve c;
    const size_t o_lab = c.take(n_pixels * 4), o_img = c.take(n_pixels * 3), o_keys = c.take(sizeof(keys)), o_present = c.take(ANNOT_MAX_COLORS),
                 o_flag = c.take(sizeof(int));
    if (ctx->gc_buf.ensure(c.at)) return -1;
    unsigned char *dev = ctx->gc_buf.as<unsigned char>();
    int *d_flag = reinterpret_cast<int *>(dev + o_flag);
    HIP_TRY(hipMemcpyAsync(dev + o_lab, labels, n_pixels * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(dev + o_keys, keys, (size_t)n_table * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(dev + o_present, present, (size_t)n_table, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(d_flag, 0, sizeof(int), st));
    if (launch_annot_paint(reinterpret_cast<int32_t *>(dev + o_lab), n_pixels, min_label, n_table, reinterpret_cast<uint32_t *>(dev + o_keys),
                           dev + o_present, dev + o_img, d_flag, st))
        return -1;
    int missing = 0;
    HIP_TRY(hipMemcpyAsync(&missing, d_flag, sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (missing) {
        set_error("annot_paint: a label of the map has no colour in the table");
        return -1;
    }
    HIP_TRY(hipMemcpyAsync(image_out, dev + o_img, n_pixels * 3, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

int imsegm_annot_color_hist(imsegm_ctx *ctx, const uint8_t *image, size_t n_pixels, int capacity, int *n_colors_out, uint32_t *keys_out,
                            uint32_t *counts_out)
{
    if (!image || !n_colors_out || capacity < 0 || (capacity > 0 && (!keys_out || !counts_out))) {
        set_error("annot_color_hist: the image, the colour count and output arrays of `capacity` entries are required");
        return -1;
    }
    if (check_pixels("annot_color_hist", n_pixels)) return -1;
    if (bind(ctx)) return -1;
    hipStream_t st = ctx->stream;
    const size_t most = n_pixels < ANNOT_HIST_BINS ? n_pixels : ANNOT_HIST_BINS;      // distinct colours an image of this size can hold
    Carve c;
    const size_t o_bins = c.take(ANNOT_HIST_BINS * 4), o_chunks = c.take(((size_t)ANNOT_HIST_CHUNKS + 1) * 4), o_img = c.take(n_pixels * 3),
                 o_keys = c.take(most * 4), o_counts = c.take(most * 4);
    if (ctx->gc_buf.ensure(c.at)) return -1;
    unsigned char *dev = ctx->gc_buf.as<unsigned char>();
    uint32_t *bins = reinterpret_cast<uint32_t *>(dev + o_bins), *chunks = reinterpret_cast<uint32_t *>(dev + o_chunks);
    uint32_t *d_keys = reinterpret_cast<uint32_t *>(dev + o_keys), *d_counts = reinterpret_cast<uint32_t *>(dev + o_counts);
    HIP_TRY(hipMemsetAsync(bins, 0, ANNOT_HIST_BINS * 4, st));
    HIP_TRY(hipMemcpyAsync(dev + o_img, image, n_pixels * 3, hipMemcpyHostToDevice, st));
    if (launch_annot_hist(dev + o_img, n_pixels, bins, st)) return -1;
    if (launch_annot_hist_count(bins, chunks, st)) return -1;
    uint32_t total = 0;
    HIP_TRY(hipMemcpyAsync(&total, chunks + ANNOT_HIST_CHUNKS, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    *n_colors_out = (int)total;
    if ((size_t)total > (size_t)capacity || total == 0) return 0;
    if (launch_annot_hist_gather(bins, chunks, d_keys, d_counts, st)) return -1;
    HIP_TRY(hipMemcpyAsync(keys_out, d_keys, (size_t)total * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(counts_out, d_counts, (size_t)total * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

int imsegm_annot_nearest_valid(imsegm_ctx *ctx, const int32_t *labels, int height, int width, int32_t *labels_out)
{
    if (!labels || !labels_out) {
        set_error("annot_nearest_valid: null array");
        return -1;
    }
    if (check_nearest_size(height, width)) return -1;
    if (bind(ctx)) return -1;
    hipStream_t st = ctx->stream;
    const size_t n = (size_t)height * width;
    Carve c;
    const size_t o_lab = c.take(n * 4), o_src = c.take(n * 4), o_out = c.take(n * 4), o_flag = c.take(sizeof(int));
    if (ctx->gc_buf.ensure(c.at)) return -1;
    unsigned char *dev = ctx->gc_buf.as<unsigned char>();
    int *d_flag = reinterpret_cast<int *>(dev + o_flag);
    HIP_TRY(hipMemcpyAsync(dev + o_lab, labels, n * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(d_flag, 0, sizeof(int), st));
    if (launch_annot_nearest_valid(reinterpret_cast<int32_t *>(dev + o_lab), height, width, reinterpret_cast<int32_t *>(dev + o_src),
                                   reinterpret_cast<int32_t *>(dev + o_out), d_flag, st))
        return -1;
    int any_valid = 0;
    HIP_TRY(hipMemcpyAsync(&any_valid, d_flag, sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (!any_valid) {
        set_error("annot_nearest_valid: the map has no valid pixel");
        return -1;
    }
    HIP_TRY(hipMemcpyAsync(labels_out, dev + o_out, n * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

int imsegm_annot_quantize_nearest_pixel(imsegm_ctx *ctx, const uint8_t *image, int height, int width, const uint8_t *colors, int n_colors,
                                        uint8_t *image_out)
{
    if (!image || !image_out) {
        set_error("annot_quantize_nearest_pixel: null array");
        return -1;
    }
    if (check_nearest_size(height, width) || check_table("annot_quantize_nearest_pixel", colors, n_colors)) return -1;
    uint32_t keys[ANNOT_MAX_COLORS];
    int32_t labs[ANNOT_MAX_COLORS];
    uint8_t present[ANNOT_MAX_COLORS];
    pack_keys(colors, n_colors, keys);
    for (int k = 0; k < n_colors; ++k) {
        labs[k] = k;
        present[k] = 1;
    }
    if (bind(ctx)) return -1;
    hipStream_t st = ctx->stream;
    const size_t n = (size_t)height * width;
    Carve c;
    const size_t o_img = c.take(n * 3), o_lab = c.take(n * 4), o_src = c.take(n * 4), o_out = c.take(n * 4), o_keys = c.take(sizeof(keys)),
                 o_labs = c.take(sizeof(labs)), o_present = c.take(sizeof(present)), o_flags = c.take(2 * sizeof(int));
    if (ctx->gc_buf.ensure(c.at)) return -1;
    unsigned char *dev = ctx->gc_buf.as<unsigned char>();
    int32_t *d_lab = reinterpret_cast<int32_t *>(dev + o_lab), *d_src = reinterpret_cast<int32_t *>(dev + o_src);
    int32_t *d_out = reinterpret_cast<int32_t *>(dev + o_out);
    uint32_t *d_keys = reinterpret_cast<uint32_t *>(dev + o_keys);
    int *d_flags = reinterpret_cast<int *>(dev + o_flags);                 // [0]: the map has a valid pixel, [1]: paint met a missing label
    HIP_TRY(hipMemcpyAsync(dev + o_img, image, n * 3, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_keys, keys, (size_t)n_colors * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(dev + o_labs, labs, (size_t)n_colors * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(dev + o_present, present, (size_t)n_colors, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(d_flags, 0, 2 * sizeof(int), st));
    if (launch_annot_match(dev + o_img, n, d_keys, reinterpret_cast<int32_t *>(dev + o_labs), n_colors, IMSEGM_ANNOT_MATCH_EXACT, d_lab,
                           nullptr, st))
        return -1;
    if (launch_annot_nearest_valid(d_lab, height, width, d_src, d_out, d_flags, st)) return -1;
    // (the image buffer is free again: the exact match was its only reader)
    if (launch_annot_paint(d_out, n, 0, n_colors, d_keys, dev + o_present, dev + o_img, d_flags + 1, st)) return -1;
    int flags[2] = { 0, 0 };
    HIP_TRY(hipMemcpyAsync(flags, d_flags, sizeof(flags), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (!flags[0]) {
        set_error("annot_quantize_nearest_pixel: no pixel of the image has one of the colours");
        return -1;
    }
    if (flags[1]) {
        set_error("annot_quantize_nearest_pixel: internal error, a pixel was left without a label");
        return -1;
    }
    HIP_TRY(hipMemcpyAsync(image_out, dev + o_img, n * 3, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

}  // extern "C"
