// api_scoring.hip -- C ABI of the scoring call (imsegm/classification.py :305-471): the labels present and the contingency table of
// every (annotation, segmentation) pair of a batch.  A stateless call on a context and host arrays.  Arguments are checked before
// the device is touched; the kernels are in scoring.hip.
#include "scoring.h"
#include "session.h"

#include <string>
#include <vector>

namespace imsegm {

namespace {

constexpr int64_t SCORE_MAX_ELEMENTS = (int64_t)1 << 40;
constexpr int SCORE_MAX_PAIRS = 1 << 20;

size_t aligned(size_t bytes) { return (bytes + 255) & ~(size_t)255; }

}  // namespace

}  // namespace imsegm

extern "C" {

int imsegm_score_pairs(imsegm_ctx *ctx, int n_pairs, const void *const *annots, const void *const *segms, const int64_t *sizes, int dtype,
                       const int32_t *drop_labels, int n_drop, int32_t *status_out, int32_t *n_labels_out, int32_t *labels_out,
                       int64_t *tables_out)
{
    if (n_pairs < 0 || n_pairs > SCORE_MAX_PAIRS) {
        set_error("score_pairs: 0 to 2^20 pairs");
        return -1;
    }
    if (n_drop < 0 || n_drop > SCORE_MAX_DROP || (n_drop > 0 && !drop_labels)) {
        set_error("score_pairs: a drop list holds 0 to " + std::to_string(SCORE_MAX_DROP) + " labels");
        return -1;
    }
    if (dtype != IMSEGM_SCORE_I32 && dtype != IMSEGM_SCORE_U8) {
        set_error("score_pairs: unknown dtype (int32 and uint8 maps are taken)");
        return -1;
    }
    if (n_pairs > 0 && (!annots || !segms || !sizes || !status_out || !n_labels_out || !labels_out || !tables_out)) {
        set_error("score_pairs: null array");
        return -1;
    }
    const size_t elem = dtype == IMSEGM_SCORE_U8 ? 1 : 4;
    std::vector<ScorePair> pairs((size_t)n_pairs);
    std::vector<unsigned int> chunk_first((size_t)n_pairs + 1);
    size_t at = 0;                                       // bytes of the maps so far, every one 256-byte aligned
    unsigned long long chunks = 0;
    for (int i = 0; i < n_pairs; ++i) {
        if (sizes[i] < 0) {
            set_error("score_pairs: negative size");
            return -1;
        }
        if (sizes[i] > SCORE_MAX_ELEMENTS) {
            set_error("score_pairs: more than 2^40 elements in a pair");
            return -1;
        }
        if (sizes[i] > 0 && (!annots[i] || !segms[i])) {
            set_error("score_pairs: null array");
            return -1;
        }
        const size_t n = (size_t)sizes[i];
        pairs[i].n = n;
        pairs[i].off_annot = at;
        pairs[i].off_segm = at + aligned(n * elem);
        at += 2 * aligned(n * elem);
        chunk_first[i] = (unsigned int)chunks;
        chunks += (n + SCORE_CHUNK_PIXELS - 1) / SCORE_CHUNK_PIXELS;
        if (chunks > 0x7fffffffull) {                    // (one workgroup per chunk: the grid's limit)
            set_error("score_pairs: more than 2^31 - 1 chunks of " + std::to_string(SCORE_CHUNK_PIXELS) + " pixels in a call");
            return -1;
        }
    }
    if (n_pairs == 0) return 0;
    chunk_first[n_pairs] = (unsigned int)chunks;
    if (bind(ctx)) return -1;
    hipStream_t st = ctx->stream;

    // scratch: [maps][pair table][chunk table][drop list][state: sets, set sizes, | results: tables, labels, status, counts]
    const size_t P = (size_t)n_pairs;
    const size_t o_pairs = at, o_chunks = o_pairs + aligned(P * sizeof(ScorePair)), o_drop = o_chunks + aligned((P + 1) * 4);
    const size_t o_state = o_drop + aligned((size_t)SCORE_MAX_DROP * 4);
    const size_t b_sets = P * SCORE_SET_SLOTS * 8, b_set_state = P * 2 * 4;                      // (both multiples of 8)
    const size_t b_tables = P * SCORE_TABLE_BINS * 8, b_labels = P * SCORE_MAX_LABELS * 4, b_flags = P * 4;
    const size_t o_results = o_state + b_sets + b_set_state, result_bytes = b_tables + b_labels + 2 * b_flags;
    if (ctx->gc_buf.ensure(o_results + result_bytes)) return -1;
    unsigned char *dev = ctx->gc_buf.as<unsigned char>();
    ScoreState state;
    state.sets = reinterpret_cast<unsigned long long *>(dev + o_state);
    state.set_state = reinterpret_cast<unsigned int *>(dev + o_state + b_sets);
    state.tables = reinterpret_cast<unsigned long long *>(dev + o_results);
    state.labels = reinterpret_cast<int32_t *>(dev + o_results + b_tables);
    state.status = reinterpret_cast<int32_t *>(dev + o_results + b_tables + b_labels);
    state.n_labels = reinterpret_cast<int32_t *>(dev + o_results + b_tables + b_labels + b_flags);

    for (int i = 0; i < n_pairs; ++i) {
        if (!pairs[i].n) continue;
        HIP_TRY(hipMemcpyAsync(dev + pairs[i].off_annot, annots[i], (size_t)pairs[i].n * elem, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(dev + pairs[i].off_segm, segms[i], (size_t)pairs[i].n * elem, hipMemcpyHostToDevice, st));
    }
    HIP_TRY(hipMemcpyAsync(dev + o_pairs, pairs.data(), P * sizeof(ScorePair), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(dev + o_chunks, chunk_first.data(), (P + 1) * 4, hipMemcpyHostToDevice, st));
    if (n_drop) HIP_TRY(hipMemcpyAsync(dev + o_drop, drop_labels, (size_t)n_drop * 4, hipMemcpyHostToDevice, st));
    // the scratch is shared with other calls and holds what they left: the sets, their sizes and every result word are cleared here
    if (launch_score_pairs(dev, reinterpret_cast<ScorePair *>(dev + o_pairs), reinterpret_cast<unsigned int *>(dev + o_chunks), n_pairs,
                           (unsigned int)chunks, dtype, reinterpret_cast<int32_t *>(dev + o_drop), n_drop, state, dev + o_state,
                           b_sets + b_set_state + result_bytes, st))
        return -1;
    std::vector<unsigned char> host(result_bytes);
    HIP_TRY(hipMemcpyAsync(host.data(), dev + o_results, result_bytes, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    const int64_t *tables = reinterpret_cast<const int64_t *>(host.data());
    const int32_t *labels = reinterpret_cast<const int32_t *>(host.data() + b_tables);
    const int32_t *status = reinterpret_cast<const int32_t *>(host.data() + b_tables + b_labels);
    const int32_t *counts = reinterpret_cast<const int32_t *>(host.data() + b_tables + b_labels + b_flags);
    for (size_t i = 0; i < P; ++i) {
        status_out[i] = status[i];
        if (status[i] != IMSEGM_SCORE_OK) continue;      // too many labels: nothing else of the pair is written
        const size_t U = (size_t)counts[i];
        n_labels_out[i] = counts[i];
        std::memcpy(labels_out + i * SCORE_MAX_LABELS, labels + i * SCORE_MAX_LABELS, U * 4);
        std::memcpy(tables_out + i * SCORE_TABLE_BINS, tables + i * SCORE_TABLE_BINS, U * U * 8);
    }
    return 0;
}

}  // extern "C"
