// api_center_annotation.hip -- C ABI of the centre-level annotations (experiments_ovary_centres/run_create_annotation.py of the
// reference).  Stateless calls on a context and host arrays; arguments and caps are checked before the device is touched; the
// kernels are in center_annotation.hip and morphology.hip.  The fp64 step between the per-label counts and the discs -- centre,
// radius, draw.disk's box and offsets, the radius of the opening -- is done here, once per (label, level), with the IEEE operations
// numpy takes (this file is built with -ffp-contract=off like all others): one small download and one small upload in the chain.
#include <cmath>

#include "center_annotation.h"
#include "session.h"
#include "slic.h"

static_assert(CA_MAX_LABELS == IMSEGM_CENTER_ANNOT_MAX_LABELS && CA_MAX_LEVELS == IMSEGM_CENTER_ANNOT_MAX_LEVELS, "tables of center_annotation.hip");

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
struct CaPlan {
    size_t o_img, o_labels, o_a, o_b, o_m0, o_m1, o_m2, o_counts, o_levels, o_discs, o_radius, o_tables, o_max2, o_lcount, o_sums, o_foreign,
        tables_bytes, bytes;
};

CaPlan ca_plan(int H, int W)
{
    CaPlan p;
    Carve c;
    const size_t n = (size_t)H * W;
    p.o_img = c.take(n * 4);
    p.o_labels = c.take(n * 4);
    p.o_a = c.take(n * 4);                              // the forest, then g
    p.o_b = c.take(n * 4);                              // the component sizes and numbers, then d2
    p.o_m0 = c.take(n);                                 // the mask, then the code bytes
    p.o_m1 = c.take(n);                                 // the eroded mask of an opening
    p.o_m2 = c.take(n);                                 // the kept mask, then the level map
    p.o_counts = c.take(compact_count_words(n) * 4 + n);    // the chunk counts, behind them the root bytes
    p.o_levels = c.take(CA_MAX_LEVELS * 8);
    p.o_discs = c.take((size_t)CA_SLOTS * CA_MAX_LEVELS * sizeof(CaDisc));
    p.o_radius = c.take((size_t)CA_SLOTS * CA_MAX_LEVELS * 4);
    // the words that are zeroed together and come down side by side: max2 | level counts | sums | foreign
    p.o_tables = p.o_max2 = c.take((size_t)CA_SLOTS * 4);
    p.o_lcount = c.take((size_t)CA_SLOTS * CA_MAX_LEVELS * 4);
    p.o_sums = c.take((size_t)CA_SLOTS * 3 * 8);
    p.o_foreign = c.take(4);
    p.tables_bytes = c.at - p.o_tables;
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
    if (H > 65535 || h * w >= (1ull << 31) || h * h + w * w > 0xffffffffull) return IMSEGM_E_OBJECT_CAPS;
    return 0;
}

int check_correct(const char *who, const void *img, int sel_radius)
{
    if (!img) {
        set_error(std::string(who) + ": null map");
        return -1;
    }
    if (sel_radius < 0 || sel_radius > IMSEGM_MORPH_MAX_RADIUS) {
        set_error(std::string(who) + ": the radius of the opening must lie in [0, IMSEGM_MORPH_MAX_RADIUS]");
        return -1;
    }
    return 0;
}

int check_levels(const char *who, const double *levels, int n_levels)
{
    if (n_levels < 0 || n_levels > CA_MAX_LEVELS || (n_levels && !levels)) {
        set_error(std::string(who) + ": 0 to IMSEGM_CENTER_ANNOT_MAX_LEVELS levels");
        return -1;
    }
    for (int i = 0; i < n_levels; ++i)
        if (!(levels[i] == levels[i]) || (i && levels[i] < levels[i - 1])) {
            set_error(std::string(who) + ": the levels must be numbers that do not descend");
            return -1;
        }
    return 0;
}

// the map on the device at o_img -> the kept mask at o_m2, the labels at o_labels, *n_labels on the host (one synchronisation)
int correct_run(imsegm_ctx *ctx, unsigned char *dev, const CaPlan &p, int is_i32, int H, int W, int sel_radius, int min_size, int *n_labels)
{
    hipStream_t st = ctx->stream;
    const size_t n = (size_t)H * W;
    uint8_t *mask = dev + p.o_m0, *tmp = dev + p.o_m1, *kept = dev + p.o_m2;
    uint32_t *counts = reinterpret_cast<uint32_t *>(dev + p.o_counts);
    const size_t words = compact_count_words(n);
    if (launch_ca_threshold(dev + p.o_img, is_i32, n, mask, st)) return -1;
    if (sel_radius > 0) {
        if (launch_disc_morph(mask, H, W, sel_radius, 0, tmp, st)) return -1;
        if (launch_disc_morph(tmp, H, W, sel_radius, 1, mask, st)) return -1;
    }
    if (launch_ca_label(mask, H, W, min_size, reinterpret_cast<int32_t *>(dev + p.o_a), reinterpret_cast<int32_t *>(dev + p.o_b),
                        dev + p.o_counts + words * 4, counts, kept, reinterpret_cast<int32_t *>(dev + p.o_labels), st))
        return -1;
    uint32_t total = 0;
    HIP_TRY(hipMemcpyAsync(&total, counts + (words - 1), 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    *n_labels = (int)total;
    return 0;
}

// the labels on the device at o_labels -> d2 at o_b (with_distances), max2, pixel counts and sums of the labels in the zeroed tables:
// what the level chain runs in front of its code pass (imsegm_debug_center_distances stops here)
int levels_front(imsegm_ctx *ctx, unsigned char *dev, const CaPlan &p, int H, int W, int max_label, bool with_distances)
{
    hipStream_t st = ctx->stream;
    const int32_t *labels = reinterpret_cast<int32_t *>(dev + p.o_labels);
    uint32_t *d2 = with_distances ? reinterpret_cast<uint32_t *>(dev + p.o_b) : nullptr;
    HIP_TRY(hipMemsetAsync(dev + p.o_tables, 0, p.tables_bytes, st));
    if (with_distances &&
        launch_ca_distances(labels, H, W, max_label, reinterpret_cast<uint32_t *>(dev + p.o_a), reinterpret_cast<int *>(dev + p.o_foreign), d2,
                            st))
        return -1;
    return launch_ca_reduce(labels, d2, H, W, max_label, reinterpret_cast<uint32_t *>(dev + p.o_max2),
                            reinterpret_cast<unsigned long long *>(dev + p.o_sums), st);
}

// the labels on the device at o_labels -> the level map at o_m2 (n_levels > 0), counts and centres of the labels 0 .. max_label on
// the host.  Returns IMSEGM_E_OBJECT_CAPS when a level asks for an opening above IMSEGM_MORPH_MAX_RADIUS.
int levels_run(imsegm_ctx *ctx, unsigned char *dev, const CaPlan &p, int H, int W, int max_label, const double *levels, int n_levels,
               int64_t *counts_out, double *centres_out)
{
    hipStream_t st = ctx->stream;
    const int32_t *labels = reinterpret_cast<int32_t *>(dev + p.o_labels);
    uint32_t *d2 = n_levels ? reinterpret_cast<uint32_t *>(dev + p.o_b) : nullptr;
    uint32_t *max2 = reinterpret_cast<uint32_t *>(dev + p.o_max2), *lcount = reinterpret_cast<uint32_t *>(dev + p.o_lcount);
    uint8_t *code = dev + p.o_m0, *tmp = dev + p.o_m1, *out = dev + p.o_m2;
    if (n_levels) HIP_TRY(hipMemcpyAsync(dev + p.o_levels, levels, (size_t)n_levels * 8, hipMemcpyHostToDevice, st));
    if (levels_front(ctx, dev, p, H, W, max_label, n_levels > 0)) return -1;
    if (n_levels &&
        launch_ca_code(labels, d2, H, W, max_label, max2, reinterpret_cast<double *>(dev + p.o_levels), n_levels, code, lcount, st))
        return -1;
    // the level counts and the sums of the labels 0 .. max_label come to the host
    const size_t slots = (size_t)max_label + 1;
    std::vector<uint32_t> h_count(slots * CA_MAX_LEVELS);
    std::vector<int64_t> h_sums(slots * 3);
    HIP_TRY(hipMemcpyAsync(h_count.data(), lcount, h_count.size() * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(h_sums.data(), dev + p.o_sums, h_sums.size() * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    std::vector<CaDisc> discs(slots * CA_MAX_LEVELS);
    std::vector<int32_t> radius(slots * CA_MAX_LEVELS, 0);
    int halo[CA_MAX_LEVELS] = { 0 };
    for (size_t v = 0; v < slots; ++v) {
        const int64_t count = h_sums[3 * v];
        counts_out[v] = v ? count : 0;
        centres_out[2 * v] = centres_out[2 * v + 1] = 0.0;
        if (!v || count < 1) continue;
        // ndimage.center_of_mass: the quotients of exact sums
        const double cr = (double)h_sums[3 * v + 1] / (double)count, cc = (double)h_sums[3 * v + 2] / (double)count;
        centres_out[2 * v] = cc;
        centres_out[2 * v + 1] = cr;
        for (int i = 1; i < n_levels; ++i) {
            // radius = int(np.sqrt(np.sum(mask) / np.pi)); draw.disk -> draw.ellipse with equal radii; disk(int(radius * 0.15))
            const int rad = (int)std::sqrt((double)h_count[v * CA_MAX_LEVELS + i] / 3.141592653589793);
            const double dr = (double)rad;
            CaDisc &d = discs[v * CA_MAX_LEVELS + i];
            d.r0 = (int32_t)std::max(std::ceil(cr - dr), 0.0);
            d.c0 = (int32_t)std::max(std::ceil(cc - dr), 0.0);
            d.r1 = (int32_t)std::min(std::floor(cr + dr), (double)(H - 1));
            d.c1 = (int32_t)std::min(std::floor(cc + dr), (double)(W - 1));
            d.r_org = cr - (double)d.r0;
            d.c_org = cc - (double)d.c0;
            d.radius = dr;
            d.pad[0] = d.pad[1] = 0;
            const int open = (int)(dr * 0.15);
            if (open > IMSEGM_MORPH_MAX_RADIUS) return IMSEGM_E_OBJECT_CAPS;
            radius[v * CA_MAX_LEVELS + i] = open;
            halo[i] = std::max(halo[i], open);
        }
    }
    if (!n_levels) return 0;
    HIP_TRY(hipMemcpyAsync(dev + p.o_discs, discs.data(), discs.size() * sizeof(CaDisc), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(dev + p.o_radius, radius.data(), radius.size() * 4, hipMemcpyHostToDevice, st));
    if (launch_ca_discs(labels, H, W, max_label, reinterpret_cast<CaDisc *>(dev + p.o_discs), n_levels, code, out, st)) return -1;
    MorphLabels ml;
    ml.labels = labels;
    ml.radius = reinterpret_cast<int32_t *>(dev + p.o_radius);
    ml.max_label = max_label;
    for (int i = 1; i < n_levels; ++i) {
        ml.level = i;
        if (launch_disc_morph_labelled(code, H, W, halo[i], 0, tmp, ml, st)) return -1;
        if (launch_disc_morph_labelled(tmp, H, W, halo[i], 1, out, ml, st)) return -1;
    }
    // (the vectors above are pageable: their uploads have to be over before they go)
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

}  // namespace

int ca_debug_distances(imsegm_ctx *ctx, const int32_t *labels, int H, int W, int max_label, uint32_t *d2_out, uint32_t *max2_out,
                       int64_t *sums_out)
{
    if (const int status = check_size("debug_center_distances", H, W)) return status;
    if (bind(ctx)) return -1;
    hipStream_t st = ctx->stream;
    const size_t n = (size_t)H * W, slots = (size_t)max_label + 1;
    const CaPlan p = ca_plan(H, W);
    if (ctx->gc_buf.ensure(p.bytes)) return -1;
    unsigned char *dev = ctx->gc_buf.as<unsigned char>();
    HIP_TRY(hipMemcpyAsync(dev + p.o_labels, labels, n * 4, hipMemcpyHostToDevice, st));
    if (levels_front(ctx, dev, p, H, W, max_label, true)) return -1;
    HIP_TRY(hipMemcpyAsync(d2_out, dev + p.o_b, n * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(max2_out, dev + p.o_max2, slots * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(sums_out, dev + p.o_sums, slots * 3 * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

}  // namespace imsegm

extern "C" {

int imsegm_correct_segm(imsegm_ctx *ctx, const void *img, int img_is_i32, int height, int width, int sel_radius, int min_size,
                        uint8_t *seg_out, int32_t *labels_out, int *n_labels_out)
{
    if (const int status = check_size("correct_segm", height, width)) return status;
    if (check_correct("correct_segm", img, sel_radius)) return -1;
    if (bind(ctx)) return -1;
    hipStream_t st = ctx->stream;
    const size_t n = (size_t)height * width;
    const CaPlan p = ca_plan(height, width);
    if (ctx->gc_buf.ensure(p.bytes)) return -1;
    unsigned char *dev = ctx->gc_buf.as<unsigned char>();
    HIP_TRY(hipMemcpyAsync(dev + p.o_img, img, n * (img_is_i32 ? 4 : 1), hipMemcpyHostToDevice, st));
    int n_labels = 0;
    if (correct_run(ctx, dev, p, img_is_i32, height, width, sel_radius, min_size, &n_labels)) return -1;
    if (seg_out) HIP_TRY(hipMemcpyAsync(seg_out, dev + p.o_m2, n, hipMemcpyDeviceToHost, st));
    if (labels_out) HIP_TRY(hipMemcpyAsync(labels_out, dev + p.o_labels, n * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (n_labels_out) *n_labels_out = n_labels;
    return 0;
}

int imsegm_center_levels(imsegm_ctx *ctx, const int32_t *labels, int height, int width, int max_label, const double *levels, int n_levels,
                         uint8_t *levels_out, int64_t *counts_out, double *centres_out)
{
    if (const int status = check_size("center_levels", height, width)) return status;
    if (!labels || !counts_out || !centres_out || (n_levels > 0 && !levels_out)) {
        set_error("center_levels: null argument");
        return -1;
    }
    if (max_label < 1) {
        set_error("center_levels: the largest label must be positive");
        return -1;
    }
    if (check_levels("center_levels", levels, n_levels)) return -1;
    if (max_label > IMSEGM_CENTER_ANNOT_MAX_LABELS) return IMSEGM_E_OBJECT_CAPS;
    if (bind(ctx)) return -1;
    hipStream_t st = ctx->stream;
    const size_t n = (size_t)height * width;
    const CaPlan p = ca_plan(height, width);
    if (ctx->gc_buf.ensure(p.bytes)) return -1;
    unsigned char *dev = ctx->gc_buf.as<unsigned char>();
    HIP_TRY(hipMemcpyAsync(dev + p.o_labels, labels, n * 4, hipMemcpyHostToDevice, st));
    if (const int status = levels_run(ctx, dev, p, height, width, max_label, levels, n_levels, counts_out, centres_out)) return status;
    if (n_levels) HIP_TRY(hipMemcpyAsync(levels_out, dev + p.o_m2, n, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

int imsegm_create_annot_centers(imsegm_ctx *ctx, const void *img, int img_is_i32, int height, int width, int sel_radius, int min_size,
                                const double *levels, int n_levels, uint8_t *levels_out, int *n_labels_out, int64_t *counts_out,
                                double *centres_out)
{
    if (const int status = check_size("create_annot_centers", height, width)) return status;
    if (check_correct("create_annot_centers", img, sel_radius)) return -1;
    if (!levels_out || !n_labels_out || !counts_out || !centres_out || n_levels < 1) {
        set_error("create_annot_centers: null argument or no level");
        return -1;
    }
    if (check_levels("create_annot_centers", levels, n_levels)) return -1;
    if (bind(ctx)) return -1;
    hipStream_t st = ctx->stream;
    const size_t n = (size_t)height * width;
    const CaPlan p = ca_plan(height, width);
    if (ctx->gc_buf.ensure(p.bytes)) return -1;
    unsigned char *dev = ctx->gc_buf.as<unsigned char>();
    HIP_TRY(hipMemcpyAsync(dev + p.o_img, img, n * (img_is_i32 ? 4 : 1), hipMemcpyHostToDevice, st));
    int n_labels = 0;
    if (correct_run(ctx, dev, p, img_is_i32, height, width, sel_radius, min_size, &n_labels)) return -1;
    if (n_labels > IMSEGM_CENTER_ANNOT_MAX_LABELS) return IMSEGM_E_OBJECT_CAPS;
    *n_labels_out = n_labels;
    if (n_labels == 0) {
        memset(levels_out, 0, n);
        return 0;
    }
    if (const int status = levels_run(ctx, dev, p, height, width, n_labels, levels, n_levels, counts_out, centres_out)) return status;
    HIP_TRY(hipMemcpyAsync(levels_out, dev + p.o_m2, n, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

}  // extern "C"
