// api_cut_objects.hip -- C ABI of the object cut-outs (imsegm/utilities/data_io.py cut_object :1060-1128 for every label of a map at
// once).  A stateless call on a context and host arrays; arguments and caps are checked before the device is touched; the kernels
// are in cut_objects.hip.  The fp64 step between the integer moments and the index maps (centroid, orientation, cosine and sine)
// belongs to the caller: it is the hook `geometry`, so that the package's host statement and this entry share ONE definition.
#include "cut_objects.h"
#include "session.h"

static_assert(CUT_MAX_LABELS == IMSEGM_CUT_OBJECTS_MAX_LABELS, "label list of cut_objects.hip");
static_assert(sizeof(CutGeom) == IMSEGM_CUT_GEOMETRY_DOUBLES * sizeof(double), "geometry row of the hook");
static_assert(sizeof(CutFrame) == IMSEGM_CUT_FRAME_INTS * sizeof(int32_t), "frame row of the hook");

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

constexpr size_t CUT_MAX_PACKED = (size_t)1 << 30;     // bytes of all crops of one call

}  // namespace

}  // namespace imsegm

extern "C" {

int imsegm_cut_objects(imsegm_ctx *ctx, const uint8_t *image, const int32_t *segm, int height, int width, int channels,
                       const int32_t *labels, int n_labels, int padding, int use_mask, const uint8_t *bg_color, int allow_rotate,
                       imsegm_cut_geometry_fn geometry, void *user, int64_t *moments_out, int32_t *boxes_out, int64_t *offsets_out,
                       const uint8_t **packed_out, int *first_empty_out)
{
    if (!image || !segm || !labels || !bg_color || !geometry || !boxes_out || !offsets_out || !packed_out || !first_empty_out) {
        set_error("cut_objects: null argument");
        return -1;
    }
    if (height < 1 || width < 1 || channels < 1 || n_labels < 1 || padding < 0) {
        set_error("cut_objects: height, width, channels and the number of labels must be positive, the padding not negative");
        return -1;
    }
    for (int k = 1; k < n_labels; ++k)
        if (labels[k - 1] >= labels[k]) {
            set_error("cut_objects: the labels must be strictly ascending");
            return -1;
        }
    // outside the caps: a status, no message, nothing launched
    if (n_labels > IMSEGM_CUT_OBJECTS_MAX_LABELS || channels > IMSEGM_CUT_OBJECTS_MAX_CHANNELS ||
        (size_t)height * (size_t)width >= ((size_t)1 << 31) || padding > (1 << 20))
        return IMSEGM_E_OBJECT_CAPS;
    if (bind(ctx)) return -1;
    hipStream_t st = ctx->stream;
    const size_t n = (size_t)height * width, m = (size_t)n_labels;
    Carve c;
    const size_t o_img = c.take(n * channels), o_segm = c.take(n * 4), o_labels = c.take(m * 4), o_geom = c.take(m * sizeof(CutGeom)),
                 o_frames = c.take(m * sizeof(CutFrame)), o_crops = c.take(m * sizeof(CutCrop));
    // the words that come down side by side: moments | source box min | source box max, and canvas box min | max
    const size_t o_mom = c.take(m * CUT_MOMENT_WORDS * 8), o_smin = c.take(m * 8), o_smax = c.take(m * 8);
    const size_t o_cmin = c.take(m * 8), o_cmax = c.take(m * 8);
    if (ctx->gc_buf.ensure(c.at)) return -1;
    unsigned char *dev = ctx->gc_buf.as<unsigned char>();
    const int32_t *d_segm = reinterpret_cast<int32_t *>(dev + o_segm), *d_labels = reinterpret_cast<int32_t *>(dev + o_labels);
    const CutGeom *d_geom = reinterpret_cast<CutGeom *>(dev + o_geom);
    // one upload of the image and of the map, whatever the number of labels
    HIP_TRY(hipMemcpyAsync(dev + o_img, image, n * channels, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(dev + o_segm, segm, n * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(dev + o_labels, labels, m * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(dev + o_mom, 0, m * CUT_MOMENT_WORDS * 8, st));
    HIP_TRY(hipMemsetAsync(dev + o_smin, 0x7f, m * 8, st));
    HIP_TRY(hipMemsetAsync(dev + o_smax, 0xff, m * 8, st));
    HIP_TRY(hipMemsetAsync(dev + o_cmin, 0x7f, m * 8, st));
    HIP_TRY(hipMemsetAsync(dev + o_cmax, 0xff, m * 8, st));
    if (launch_cut_moments(d_segm, height, width, d_labels, n_labels, reinterpret_cast<unsigned long long *>(dev + o_mom),
                           reinterpret_cast<int *>(dev + o_smin), reinterpret_cast<int *>(dev + o_smax), st))
        return -1;
    // (a) -> (b): the ten words per label come to the host
    const size_t first_bytes = o_cmin - o_mom;
    unsigned char *host = static_cast<unsigned char *>(ctx->stage(first_bytes));
    if (!host) {
        set_error("cut_objects: no page-locked memory for the moments");
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
    if (moments_out) memcpy(moments_out, words.data(), words.size() * 8);
    std::vector<CutGeom> geom(m);
    std::vector<CutFrame> frames(m);
    if (geometry(user, n_labels, allow_rotate, height, width, words.data(), reinterpret_cast<double *>(geom.data()),
                 reinterpret_cast<int32_t *>(frames.data()))) {
        set_error("cut_objects: the geometry hook refused the objects");
        return -1;
    }
    int win_h = 1, win_w = 1;
    for (size_t k = 0; k < m; ++k) {
        const CutFrame &f = frames[k];
        // (a canvas is never larger than the diagonal of the map in either direction)
        if (f.canvas_h < 1 || f.canvas_w < 1 || f.canvas_h > height + width + 2 || f.canvas_w > height + width + 2 || f.r0 < 0 ||
            f.c0 < 0 || f.r1 > f.canvas_h || f.c1 > f.canvas_w || f.r0 > f.r1 || f.c0 > f.c1) {
            set_error("cut_objects: the geometry hook returned a window outside its canvas");
            return -1;
        }
        win_h = std::max(win_h, f.r1 - f.r0);
        win_w = std::max(win_w, f.c1 - f.c0);
    }
    HIP_TRY(hipMemcpyAsync(dev + o_geom, geom.data(), m * sizeof(CutGeom), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(dev + o_frames, frames.data(), m * sizeof(CutFrame), hipMemcpyHostToDevice, st));
    // (c): the exact box of every turned mask, then (d) the one small download in the middle of the chain
    if (launch_cut_canvas_boxes(d_segm, height, width, d_labels, d_geom, reinterpret_cast<CutFrame *>(dev + o_frames), n_labels, win_h, win_w,
                                reinterpret_cast<int *>(dev + o_cmin), reinterpret_cast<int *>(dev + o_cmax), st))
        return -1;
    std::vector<int32_t> cbox(m * 4);
    HIP_TRY(hipMemcpyAsync(cbox.data(), dev + o_cmin, m * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(cbox.data() + m * 2, dev + o_cmax, m * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    std::vector<CutCrop> crops(m);
    size_t total = 0;
    int crop_h = 1, crop_w = 1;
    *first_empty_out = -1;
    for (size_t k = 0; k < m; ++k) {
        const int lo_r = cbox[2 * k], lo_c = cbox[2 * k + 1], hi_r = cbox[2 * m + 2 * k], hi_c = cbox[2 * m + 2 * k + 1];
        if (hi_r < 0) {                                // no canvas pixel of the window saw the object: regionprops(...)[0] of the reference fails
            *first_empty_out = (int)k;
            return 0;
        }
        // add_padding (:1039-1057) of the half-open box against the canvas
        CutCrop &crop = crops[k];
        crop.r0 = std::max(0, lo_r - padding);
        crop.c0 = std::max(0, lo_c - padding);
        crop.h = std::min(frames[k].canvas_h, hi_r + 1 + padding) - crop.r0;
        crop.w = std::min(frames[k].canvas_w, hi_c + 1 + padding) - crop.c0;
        crop.offset = (long long)total;
        offsets_out[k] = (int64_t)total;
        boxes_out[4 * k] = crop.r0, boxes_out[4 * k + 1] = crop.c0, boxes_out[4 * k + 2] = crop.r0 + crop.h, boxes_out[4 * k + 3] = crop.c0 + crop.w;
        total += (size_t)crop.h * crop.w * channels;
        crop_h = std::max(crop_h, crop.h);
        crop_w = std::max(crop_w, crop.w);
        if (total > CUT_MAX_PACKED) return IMSEGM_E_OBJECT_CAPS;
    }
    offsets_out[m] = (int64_t)total;
    // (e), (f): all crops by one launch into the context's second scratch, one download
    if (ctx->aux_buf.ensure(total)) return -1;
    uint32_t bg = 0;
    for (int ch = 0; ch < channels; ++ch) bg |= (uint32_t)bg_color[ch] << (8 * ch);
    HIP_TRY(hipMemcpyAsync(dev + o_crops, crops.data(), m * sizeof(CutCrop), hipMemcpyHostToDevice, st));
    if (launch_cut_write(dev + o_img, d_segm, height, width, channels, d_labels, d_geom, reinterpret_cast<CutCrop *>(dev + o_crops), n_labels,
                         crop_h, crop_w, use_mask != 0, bg, ctx->aux_buf.as<uint8_t>(), st))
        return -1;
    unsigned char *packed = static_cast<unsigned char *>(ctx->stage(total));
    if (!packed) {
        set_error("cut_objects: no page-locked memory for the crops");
        return -1;
    }
    HIP_TRY(hipMemcpyAsync(packed, ctx->aux_buf.p, total, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    *packed_out = packed;
    return 0;
}

}  // extern "C"
