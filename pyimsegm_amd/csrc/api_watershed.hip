// api_watershed.hip -- C ABI of the egg segmentation by marker watershed (experiments_ovary_detect/run_ovary_egg-segmentation.py
// segment_watershed :239-275 of the reference).  Stateless calls on a context and host arrays; arguments and caps are checked before
// the device is touched.  The flood is watershed.hip; hole filling and disc erosion / dilation are morphology.hip, the squared
// distances boundary.hip, the component labels center_annotation.hip -- the kernels the other entries run, no second copies.
// The clean-up works on all labels at once, every stage one launch over the planes of the labels' padded bounding boxes; the boxes
// stay on the device.  Each call is one upload, one chain of launches and one download.
#include <algorithm>
#include <vector>

#include "center_annotation.h"
#include "morphology.h"
#include "session.h"
#include "slic.h"
#include "watershed.h"

static_assert(WS_MAX_LABELS == IMSEGM_WATERSHED_MAX_LABELS && WS_MAX_LABELS < WS_CLAIM, "state words of watershed.hip");

namespace imsegm {

namespace {

struct Carve {
    size_t at = 0;
    size_t take(size_t bytes)
    {
        const size_t here = at;
        at += (bytes + 255) & ~(size_t)255;
        return here;
    }
};

// where the pieces of one call live inside the context's scratch buffer
struct WsPlan {
    size_t o_wide, o_parent, o_touch, o_bg, o_fg, o_mask, o_kept, o_g, o_keys, o_comp, o_size, o_roots, o_chunks, o_state, o_count, o_base,
        o_fill, o_arena, o_seedp, o_seedl, o_boxes, o_table, o_pa, o_pb, o_ptouch, o_pparent, o_words, capacity, bytes;
};

// capacity: the pixels of all planes of the clean-up together (0: no clean-up)
WsPlan ws_plan(int H, int W, size_t seeds, size_t capacity = 0)
{
    WsPlan p;
    Carve c;
    const size_t n = (size_t)H * W;
    p.o_wide = c.take(n * 4);                           // the mask as int32 for the hole filling
    p.o_parent = c.take(n * 4);                         // the forests of the hole filling and of the labelling
    p.o_touch = c.take(n);
    p.o_bg = c.take(n);                                 // 1 - filled mask
    p.o_fg = c.take(n);                                 // (the second output of launch_fill_holes_split, not read)
    p.o_mask = c.take(n);                               // the filled mask
    p.o_kept = c.take(n);                               // the mask once more (launch_ca_label)
    p.o_g = c.take(n * 4);
    p.o_keys = c.take(n * 4);                           // d2, then the keys, then the cleaned map
    p.o_comp = c.take(n * 4);
    p.o_size = c.take(n * 4);
    p.o_roots = c.take(n);
    p.o_chunks = c.take(compact_count_words(n) * 4);    // its last word: the number of components
    p.o_state = c.take(n * 4);                          // the flood's state, then its map
    p.o_count = c.take((n + 1) * 4);
    p.o_base = c.take((n + 1) * 4);
    p.o_fill = c.take((n + 1) * 4);
    p.o_arena = c.take(2 * n * 4);
    p.o_seedp = c.take(std::max<size_t>(seeds, 1) * 4);
    p.o_seedl = c.take(std::max<size_t>(seeds, 1) * 4);
    p.o_boxes = c.take((size_t)(WS_MAX_LABELS + 1) * 4 * 4);
    p.o_table = c.take((size_t)(WS_MAX_LABELS + 1) * MORPH_BOX_WORDS * 4);
    p.capacity = capacity;
    p.o_pa = c.take(capacity);                          // the planes of all labels, and a second set for the disc passes
    p.o_pb = c.take(capacity);
    p.o_ptouch = c.take(capacity);
    p.o_pparent = c.take(capacity * 4);
    p.o_words = c.take(16);                             // any background | arena top | label beyond the cap | planes beyond the capacity
    p.bytes = c.at;
    return p;
}

int check_size(const char *who, int H, int W)
{
    if (H < 1 || W < 1) {
        set_error(std::string(who) + ": height and width must be positive");
        return -1;
    }
    const unsigned long long h = (unsigned long long)H, w = (unsigned long long)W;
    // (the keys -d2 are int32: the squared diagonal stays below 2^31)
    if (H > 65535 || h * w >= (1ull << 31) || h * h + w * w >= (1ull << 31)) return IMSEGM_E_OBJECT_CAPS;
    return 0;
}

int check_seeds(const char *who, const int32_t *pixels, const int32_t *labels, int n_seeds, size_t n)
{
    if (n_seeds < 0 || (n_seeds && (!pixels || !labels))) {
        set_error(std::string(who) + ": null seeds");
        return -1;
    }
    for (int i = 0; i < n_seeds; ++i) {
        if (pixels[i] < 0 || (size_t)pixels[i] >= n) {
            set_error(std::string(who) + ": a seed lies outside the map");
            return -1;
        }
        if (labels[i] < 1 || labels[i] > WS_MAX_LABELS) return IMSEGM_E_OBJECT_CAPS;
    }
    return 0;
}

// the mask (0 / 1 bytes at o_mask, its complement at o_bg, the flag of launch_ws_mask raised) and the keys at o_keys (d2_keys: the
// squared distances to the background are computed and negated there) -> the flooded map at o_state
int flood_run(imsegm_ctx *ctx, unsigned char *dev, const WsPlan &p, int H, int W, bool d2_keys, int n_seeds)
{
    hipStream_t st = ctx->stream;
    const size_t n = (size_t)H * W;
    uint8_t *mask = dev + p.o_mask;
    int32_t *keys = reinterpret_cast<int32_t *>(dev + p.o_keys), *comp = reinterpret_cast<int32_t *>(dev + p.o_comp);
    int32_t *state = reinterpret_cast<int32_t *>(dev + p.o_state);
    uint32_t *chunks = reinterpret_cast<uint32_t *>(dev + p.o_chunks), *words = reinterpret_cast<uint32_t *>(dev + p.o_words);
    if (d2_keys) {
        if (launch_edt(dev + p.o_bg, reinterpret_cast<int *>(words), H, W, reinterpret_cast<uint32_t *>(dev + p.o_g),
                       reinterpret_cast<uint32_t *>(keys), nullptr, st))
            return -1;
        if (launch_ws_negate(reinterpret_cast<uint32_t *>(keys), n, st)) return -1;
    }
    // (8-connected components: unions of the 4-connected ones the flood stays inside)
    if (launch_ca_label(mask, H, W, 0, reinterpret_cast<int32_t *>(dev + p.o_parent), reinterpret_cast<int32_t *>(dev + p.o_size),
                        dev + p.o_roots, chunks, dev + p.o_kept, comp, st))
        return -1;
    return launch_ws_flood(comp, chunks + (compact_count_words(n) - 1), keys, H, W, reinterpret_cast<int32_t *>(dev + p.o_seedp),
                           reinterpret_cast<int32_t *>(dev + p.o_seedl), n_seeds, state, reinterpret_cast<uint32_t *>(dev + p.o_count),
                           reinterpret_cast<uint32_t *>(dev + p.o_base), reinterpret_cast<uint32_t *>(dev + p.o_fill),
                           reinterpret_cast<uint32_t *>(dev + p.o_arena), words + 1, state, st);
}

// what the planes of the clean-up may take together: every label's box padded by radius_close + 1 on all sides.  Labels of a
// flood tile the mask, so their boxes overlap little; IMSEGM_E_OBJECT_CAPS (the host statement) where they take more, or 2^31
size_t cleanup_capacity(int H, int W, int max_label, int radius_close)
{
    if (max_label < 1) return 0;
    const size_t side = 2 * ((size_t)radius_close + 1);
    return 8 * (size_t)H * W + (size_t)max_label * side * (side + 2);
}

// the label map at o_state -> the cleaned map at o_keys; *(o_words + 2), + 3 raised for a label above max_label and for planes beyond
// the capacity (the caller reads them behind its download).  Every label has a plane: its bounding box padded by radius_close + 1
// and cut at the image.  The closing stays inside the box with a ring of clear pixels along every side that is not the image's, so
// erosions see the clear pixel the whole image would show them, a side of the image is a side of the plane (set outside for
// erosions, clear for dilations: k_disc_morph), and a zero component that reaches the ring is no hole.  One launch per stage for
// all labels: boxes, planes, extraction, dilation, erosion, hole filling, erosion, dilation, paint.
int cleanup_run(imsegm_ctx *ctx, unsigned char *dev, const WsPlan &p, int H, int W, int max_label, int radius_close, int radius_open)
{
    hipStream_t st = ctx->stream;
    const size_t n = (size_t)H * W;
    const int32_t *segm = reinterpret_cast<int32_t *>(dev + p.o_state);
    int32_t *clean = reinterpret_cast<int32_t *>(dev + p.o_keys), *boxes = reinterpret_cast<int32_t *>(dev + p.o_boxes);
    int32_t *table = reinterpret_cast<int32_t *>(dev + p.o_table);
    int *flags = reinterpret_cast<int *>(dev + p.o_words) + 2;
    uint8_t *a = dev + p.o_pa, *b = dev + p.o_pb;
    HIP_TRY(hipMemsetAsync(clean, 0, n * 4, st));
    HIP_TRY(hipMemsetAsync(flags, 0, 2 * sizeof(int), st));
    if (max_label < 1) return 0;
    if (launch_ws_boxes(segm, H, W, max_label, boxes, flags, st)) return -1;
    if (launch_ws_box_plan(boxes, H, W, max_label, radius_close + 1, p.capacity, table, flags + 1, st)) return -1;
    if (launch_ws_extract(segm, H, W, table, max_label, a, st)) return -1;
    if (radius_close > 0) {
        if (launch_disc_morph_boxed(a, H, W, radius_close, 1, b, table, max_label, st)) return -1;
        if (launch_disc_morph_boxed(b, H, W, radius_close, 0, a, table, max_label, st)) return -1;
    }
    if (launch_ws_fill_holes(a, H, W, table, max_label, reinterpret_cast<int32_t *>(dev + p.o_pparent), dev + p.o_ptouch, st)) return -1;
    if (radius_open > 0) {
        if (launch_disc_morph_boxed(a, H, W, radius_open, 0, b, table, max_label, st)) return -1;
        if (launch_disc_morph_boxed(b, H, W, radius_open, 1, a, table, max_label, st)) return -1;
    }
    return launch_ws_paint(a, H, W, table, max_label, clean, st);
}

// the result at o_result and the two flags of cleanup_run come to the host: IMSEGM_E_OBJECT_CAPS when one is raised
int cleanup_download(imsegm_ctx *ctx, unsigned char *dev, const WsPlan &p, size_t o_result, size_t n, int32_t *out)
{
    int flags[2] = { 0, 0 };
    HIP_TRY(hipMemcpyAsync(out, dev + o_result, n * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipMemcpyAsync(flags, dev + p.o_words + 8, sizeof(flags), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return flags[0] || flags[1] ? IMSEGM_E_OBJECT_CAPS : 0;
}

int check_radii(const char *who, int radius_close, int radius_open)
{
    if (radius_close < 0 || radius_open < 0) {
        set_error(std::string(who) + ": a radius must not be negative");
        return -1;
    }
    if (radius_close > IMSEGM_MORPH_MAX_RADIUS || radius_open > IMSEGM_MORPH_MAX_RADIUS) return IMSEGM_E_OBJECT_CAPS;
    return 0;
}

}  // namespace

}  // namespace imsegm

extern "C" {

int imsegm_watershed_markers(imsegm_ctx *ctx, const uint8_t *mask, int height, int width, const int32_t *keys, const int32_t *seed_pixels,
                             const int32_t *seed_labels, int n_seeds, int32_t *segm_out)
{
    if (const int status = check_size("watershed_markers", height, width)) return status;
    if (!mask || !segm_out) {
        set_error("watershed_markers: null argument");
        return -1;
    }
    const size_t n = (size_t)height * width;
    if (const int status = check_seeds("watershed_markers", seed_pixels, seed_labels, n_seeds, n)) return status;
    if (bind(ctx)) return -1;
    hipStream_t st = ctx->stream;
    const WsPlan p = ws_plan(height, width, (size_t)n_seeds);
    if (ctx->gc_buf.ensure(p.bytes)) return -1;
    unsigned char *dev = ctx->gc_buf.as<unsigned char>();
    HIP_TRY(hipMemcpyAsync(dev + p.o_kept, mask, n, hipMemcpyHostToDevice, st));
    if (keys) HIP_TRY(hipMemcpyAsync(dev + p.o_keys, keys, n * 4, hipMemcpyHostToDevice, st));
    if (n_seeds) {
        HIP_TRY(hipMemcpyAsync(dev + p.o_seedp, seed_pixels, (size_t)n_seeds * 4, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(dev + p.o_seedl, seed_labels, (size_t)n_seeds * 4, hipMemcpyHostToDevice, st));
    }
    // any byte but 0 is inside: the complement, then the mask as 0 / 1 bytes with the flag of the distance transform
    if (launch_ws_invert(dev + p.o_kept, n, dev + p.o_bg, st)) return -1;
    if (launch_ws_mask(dev + p.o_bg, n, dev + p.o_mask, reinterpret_cast<int *>(dev + p.o_words), st)) return -1;
    if (flood_run(ctx, dev, p, height, width, keys == nullptr, n_seeds)) return -1;
    HIP_TRY(hipMemcpyAsync(segm_out, dev + p.o_state, n * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

int imsegm_watershed_post_morph(imsegm_ctx *ctx, const int32_t *segm, int height, int width, int max_label, int radius_close,
                                int radius_open, int32_t *clean_out)
{
    if (const int status = check_size("watershed_post_morph", height, width)) return status;
    if (!segm || !clean_out) {
        set_error("watershed_post_morph: null argument");
        return -1;
    }
    if (const int status = check_radii("watershed_post_morph", radius_close, radius_open)) return status;
    if (max_label > WS_MAX_LABELS) return IMSEGM_E_OBJECT_CAPS;
    if (bind(ctx)) return -1;
    hipStream_t st = ctx->stream;
    const size_t n = (size_t)height * width;
    const size_t capacity = cleanup_capacity(height, width, max_label, radius_close);
    if (capacity >= ((size_t)1 << 31)) return IMSEGM_E_OBJECT_CAPS;
    const WsPlan p = ws_plan(height, width, 0, capacity);
    if (ctx->gc_buf.ensure(p.bytes)) return -1;
    unsigned char *dev = ctx->gc_buf.as<unsigned char>();
    HIP_TRY(hipMemcpyAsync(dev + p.o_state, segm, n * 4, hipMemcpyHostToDevice, st));
    if (const int status = cleanup_run(ctx, dev, p, height, width, max_label, radius_close, radius_open)) return status;
    return cleanup_download(ctx, dev, p, p.o_keys, n, clean_out);
}

int imsegm_watershed(imsegm_ctx *ctx, const uint8_t *seg, int height, int width, const int32_t *centres, int n_centres, int post_morph,
                     const int32_t *radii, int32_t *segm_out)
{
    if (const int status = check_size("watershed", height, width)) return status;
    if (!seg || !segm_out || n_centres < 0 || (n_centres && !centres)) {
        set_error("watershed: null argument");
        return -1;
    }
    if (n_centres > WS_MAX_LABELS) return IMSEGM_E_OBJECT_CAPS;
    const int radius_close = radii ? radii[0] : 5, radius_open = radii ? radii[1] : 15;
    if (post_morph)
        if (const int status = check_radii("watershed", radius_close, radius_open)) return status;
    const size_t n = (size_t)height * width;
    // markers[row, col] = i + 1 in the order of the centres: the last centre of a pixel stays
    std::vector<int32_t> pixels, labels;
    for (int i = n_centres - 1; i >= 0; --i) {
        const int row = centres[2 * i], col = centres[2 * i + 1];
        if (row < 0 || row >= height || col < 0 || col >= width) {
            set_error("watershed: a centre lies outside the map");
            return -1;
        }
        const int32_t pixel = (int32_t)((size_t)row * width + col);
        if (std::find(pixels.begin(), pixels.end(), pixel) != pixels.end()) continue;
        pixels.push_back(pixel);
        labels.push_back(i + 1);
    }
    const int n_seeds = (int)pixels.size();
    if (bind(ctx)) return -1;
    hipStream_t st = ctx->stream;
    const size_t capacity = post_morph ? cleanup_capacity(height, width, n_centres, radius_close) : 0;
    if (capacity >= ((size_t)1 << 31)) return IMSEGM_E_OBJECT_CAPS;
    const WsPlan p = ws_plan(height, width, (size_t)n_seeds, capacity);
    if (ctx->gc_buf.ensure(p.bytes)) return -1;
    unsigned char *dev = ctx->gc_buf.as<unsigned char>();
    HIP_TRY(hipMemcpyAsync(dev + p.o_kept, seg, n, hipMemcpyHostToDevice, st));
    if (n_seeds) {
        HIP_TRY(hipMemcpyAsync(dev + p.o_seedp, pixels.data(), (size_t)n_seeds * 4, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(dev + p.o_seedl, labels.data(), (size_t)n_seeds * 4, hipMemcpyHostToDevice, st));
    }
    // seg_binary = binary_fill_holes(seg > 0); distance_transform_edt(seg_binary); watershed(-distance, markers, mask=seg_binary)
    if (launch_ws_widen(dev + p.o_kept, n, reinterpret_cast<int32_t *>(dev + p.o_wide), st)) return -1;
    if (launch_fill_holes_split(reinterpret_cast<int32_t *>(dev + p.o_wide), height, width, reinterpret_cast<int32_t *>(dev + p.o_parent),
                                dev + p.o_touch, dev + p.o_bg, dev + p.o_fg, st))
        return -1;
    if (launch_ws_mask(dev + p.o_bg, n, dev + p.o_mask, reinterpret_cast<int *>(dev + p.o_words), st)) return -1;
    if (flood_run(ctx, dev, p, height, width, true, n_seeds)) return -1;
    if (post_morph) {
        if (const int status = cleanup_run(ctx, dev, p, height, width, n_centres, radius_close, radius_open)) return status;
        // (the synchronisation inside also covers the uploads of the pageable seed vectors)
        return cleanup_download(ctx, dev, p, p.o_keys, n, segm_out);
    }
    HIP_TRY(hipMemcpyAsync(segm_out, dev + p.o_state, n * 4, hipMemcpyDeviceToHost, st));
    // (the seed vectors are pageable: their uploads have to be over before they go)
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

}  // extern "C"
