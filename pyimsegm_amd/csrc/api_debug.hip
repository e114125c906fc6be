// api_debug.hip -- diagnostics for the tests of reused scratch (tests/test_gpu_stale_scratch.py): fill everything a context or a
// session owns on the device with one word, and put the host-side bookkeeping back to that of a new object.  After the call the
// object is a new one in all but two respects: its buffers keep their capacity, and they hold the word instead of whatever
// hipMalloc would have returned.  And what imsegm_center_levels holds on the device in front of its code pass
// (tests/test_gpu_center_annotation_edges.py).
#include "center_annotation.h"
#include "session.h"

namespace {

// the whole capacity of a buffer, not only the part the last call used (a capacity is bytes + bytes / 8 + 256 of a request:
// whatever is left behind the last whole word is filled byte by byte with the word's low byte)
int fill(DevBuf &b, uint32_t word, hipStream_t st, size_t &total)
{
    if (!b.p || !b.cap) return 0;
    const size_t words = b.cap / 4, tail = b.cap % 4;
    if (words) HIP_TRY(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(b.p), (int)word, words, st));
    if (tail) HIP_TRY(hipMemsetAsync(static_cast<unsigned char *>(b.p) + words * 4, (int)(word & 0xff), tail, st));
    total += b.cap;
    return 0;
}

}  // namespace

extern "C" {

int imsegm_debug_poison_context(imsegm_ctx *ctx, uint32_t word, size_t *bytes_out)
{
    if (bind(ctx)) return -1;
    hipStream_t st = ctx->stream;
    HIP_TRY(hipStreamSynchronize(st));                     // (an upload out of the staging block nobody has waited for)
    ctx->pinned_busy = false;
    size_t total = 0;
    // every DevBuf of imsegm_ctx.  The batch (batch.hip: `arena`) and region-growing (api_region_growing.hip: `state`, `job`)
    // handles own their device memory themselves: it is not reachable from the context and is not filled here; what those
    // handles carve out of the context's scratch is.  The page-locked staging block is host memory and stays as it is.
    DevBuf *all[] = { &ctx->gc_buf, &ctx->aux_buf, &ctx->fit_table, &ctx->fit_work };
    for (auto b : all)
        if (fill(*b, word, st, total)) return -1;
    HIP_TRY(hipStreamSynchronize(st));
    // a new context has no table of a mixture fit and no labels of its restarts
    ctx->fit_n = 0;
    ctx->fit_F = 0;
    ctx->fit_label_restarts = 0;
    ctx->fit_label_classes = 0;
    if (bytes_out) *bytes_out = total;
    return 0;
}

int imsegm_debug_image2d_poison(imsegm_image2d *im, uint32_t word, size_t *bytes_out)
{
    if (!im || bind(im->ctx)) return -1;
    hipStream_t st = im->ctx->stream;
    HIP_TRY(hipStreamSynchronize(st));
    size_t total = 0;
    // every DevBuf of imsegm_image2d (the list of imsegm_image2d_destroy); the context's scratch a session call borrows
    // (gc_buf for the cut and the boundary distances) belongs to the context: imsegm_debug_poison_context fills it
    DevBuf *all[] = { &im->img, &im->labA, &im->labB, &im->nearest, &im->labels, &im->conn_i32, &im->conn_u8, &im->small,
                      &im->cent, &im->tiles, &im->feat, &im->graph, &im->gather_lut, &im->gather_out_i, &im->gather_out_f,
                      &im->tex_planes, &im->tex_resp, &im->tex_small, &im->tex_aux, &im->vol_cent, &im->annot, &im->hist, &im->featK, &im->seg,
                      &im->gseg, &im->narrow, &im->conv, &im->forest };
    for (auto b : all)
        if (fill(*b, word, st, total)) return -1;
    HIP_TRY(hipStreamSynchronize(st));
    // the bookkeeping of a session imsegm_image2d_create / imsegm_volume_create has just returned (sizes and kind stay)
    im->dtype = -1;                                        // no image uploaded
    im->n_labels = 0;
    im->have_labels = false;
    im->labels_connected = false;
    im->tex_ready = false;                                 // no filter bank, no response planes
    im->vol_off = 0.0;
    im->vol_scale = 1.0;
    im->vol_pre_dtype = -1;
    im->vol_K = 0;
    im->conv_source = false;                               // no converted image
    im->gplan = GraphPlan();
    im->graph_ready = false;
    im->forest_ready = false;
    im->feat_mask = 0;                                     // no resident feature table, no placement pending
    im->feat_F = 0;
    im->place_F = 0;
    im->place_col = 0;
    im->slic_K = 0;
    im->slic_ran = false;                                  // nothing for get_lab / get_nearest / get_pre_scalars to report
    im->small_zeroed = false;                              // the page of reduction words is cleared again where it is next needed
    if (im->slic_exec) {
        (void)hipGraphExecDestroy(im->slic_exec);
        im->slic_exec = nullptr;
    }
    im->slic_key.clear();
    if (bytes_out) *bytes_out = total;
    return 0;
}

int imsegm_debug_center_distances(imsegm_ctx *ctx, const int32_t *labels, int height, int width, int max_label, uint32_t *d2_out,
                                  uint32_t *max2_out, int64_t *sums_out)
{
    if (!labels || !d2_out || !max2_out || !sums_out) {
        set_error("debug_center_distances: null argument");
        return -1;
    }
    if (max_label < 1) {
        set_error("debug_center_distances: the largest label must be positive");
        return -1;
    }
    if (max_label > IMSEGM_CENTER_ANNOT_MAX_LABELS) return IMSEGM_E_OBJECT_CAPS;
    return imsegm::ca_debug_distances(ctx, labels, height, width, max_label, d2_out, max2_out, sums_out);
}

}  // extern "C"
