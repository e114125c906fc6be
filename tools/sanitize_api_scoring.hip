// Stand-alone host check of csrc/api_scoring.hip under AddressSanitizer / UBSan: argument validation of imsegm_score_pairs.
// Needs no GPU (every valid call ends at "no device"), runs nothing on one, and is not loaded into Python.
//
//   cd pyimsegm_amd/csrc && hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//       -Xarch_host -fno-sanitize-recover=undefined ../../tools/sanitize_api_scoring.hip api_scoring.hip scoring.hip \
//       -o /tmp/sanitize_api_scoring && /tmp/sanitize_api_scoring
//
// The two helpers the API takes from api.hip (error text, HIP status check) are defined here so that the rest of the library stays out.
#include "../pyimsegm_amd/csrc/scoring.h"
#include "../pyimsegm_amd/csrc/session.h"

#include <cstdio>
#include <string>
#include <vector>

static std::string g_error;
namespace imsegm {
void set_error(const std::string &msg) { g_error = msg; }
bool hip_ok(hipError_t e, const char *what, const char *, int)
{
    if (e == hipSuccess) return true;
    g_error = std::string(what) + ": " + hipGetErrorString(e);
    return false;
}
}  // namespace imsegm

static int failures = 0;
#define EXPECT(cond)                                                        \
    do {                                                                    \
        if (!(cond)) {                                                      \
            std::printf("FAILED line %d: %s (last error: %s)\n", __LINE__, #cond, g_error.c_str()); \
            ++failures;                                                     \
        }                                                                   \
    } while (0)

static bool refused_with(int rc, const char *part) { return rc == -1 && g_error.find(part) != std::string::npos; }

int main()
{
    std::vector<int32_t> annot(42, 0), segm(42, 1), drop(IMSEGM_SCORE_MAX_DROP + 1, 5);
    const void *annots[2] = { annot.data(), annot.data() }, *segms[2] = { segm.data(), segm.data() };
    const void *holes[2] = { annot.data(), nullptr };
    int64_t sizes[2] = { 42, 7 };
    std::vector<int32_t> status(2, -5), counts(2, -5), labels(2 * IMSEGM_SCORE_MAX_LABELS, -5);
    std::vector<int64_t> tables((size_t)2 * IMSEGM_SCORE_MAX_LABELS * IMSEGM_SCORE_MAX_LABELS, -5);
    imsegm_ctx ctx;                                     // a context nobody created on a device: valid calls stop at the device

    auto call = [&](imsegm_ctx *c, int n, const void *const *a, const void *const *s, const int64_t *sz, int dtype, const int32_t *d, int nd) {
        return imsegm_score_pairs(c, n, a, s, sz, dtype, d, nd, status.data(), counts.data(), labels.data(), tables.data());
    };
    EXPECT(refused_with(call(&ctx, -1, annots, segms, sizes, IMSEGM_SCORE_I32, nullptr, 0), "2^20 pairs"));
    EXPECT(refused_with(call(&ctx, (1 << 20) + 1, annots, segms, sizes, IMSEGM_SCORE_I32, nullptr, 0), "2^20 pairs"));
    EXPECT(refused_with(call(&ctx, 2, nullptr, segms, sizes, IMSEGM_SCORE_I32, nullptr, 0), "null array"));
    EXPECT(refused_with(call(&ctx, 2, annots, nullptr, sizes, IMSEGM_SCORE_I32, nullptr, 0), "null array"));
    EXPECT(refused_with(call(&ctx, 2, annots, segms, nullptr, IMSEGM_SCORE_I32, nullptr, 0), "null array"));
    EXPECT(refused_with(call(&ctx, 2, holes, segms, sizes, IMSEGM_SCORE_I32, nullptr, 0), "null array"));
    EXPECT(refused_with(call(&ctx, 2, annots, holes, sizes, IMSEGM_SCORE_U8, nullptr, 0), "null array"));
    EXPECT(refused_with(imsegm_score_pairs(&ctx, 2, annots, segms, sizes, IMSEGM_SCORE_I32, nullptr, 0, nullptr, counts.data(), labels.data(),
                                           tables.data()), "null array"));
    EXPECT(refused_with(imsegm_score_pairs(&ctx, 2, annots, segms, sizes, IMSEGM_SCORE_I32, nullptr, 0, status.data(), counts.data(), labels.data(),
                                           nullptr), "null array"));
    EXPECT(refused_with(call(&ctx, 2, annots, segms, sizes, 2, nullptr, 0), "unknown dtype"));
    EXPECT(refused_with(call(&ctx, 2, annots, segms, sizes, -1, nullptr, 0), "unknown dtype"));
    EXPECT(refused_with(call(&ctx, 2, annots, segms, sizes, IMSEGM_SCORE_I32, drop.data(), -1), "drop list"));
    EXPECT(refused_with(call(&ctx, 2, annots, segms, sizes, IMSEGM_SCORE_I32, drop.data(), IMSEGM_SCORE_MAX_DROP + 1), "drop list"));
    EXPECT(refused_with(call(&ctx, 2, annots, segms, sizes, IMSEGM_SCORE_I32, nullptr, 1), "drop list"));
    int64_t negative[2] = { 42, -1 }, huge[2] = { ((int64_t)1 << 40) + 1, 7 };
    EXPECT(refused_with(call(&ctx, 2, annots, segms, negative, IMSEGM_SCORE_I32, nullptr, 0), "negative size"));
    EXPECT(refused_with(call(&ctx, 2, annots, segms, huge, IMSEGM_SCORE_I32, nullptr, 0), "2^40"));
    // sizes that pass one by one but need more workgroups than a grid has: refused from the sizes alone
    std::vector<int64_t> many(20, (int64_t)1 << 40);
    std::vector<const void *> same(20, annot.data());
    EXPECT(refused_with(imsegm_score_pairs(&ctx, 20, same.data(), same.data(), many.data(), IMSEGM_SCORE_U8, nullptr, 0, status.data(), counts.data(),
                                           labels.data(), tables.data()), "chunks"));
    // a zero-length pair needs no arrays; no pairs at all is legal and touches nothing
    int64_t none[2] = { 42, 0 };
    EXPECT(imsegm_score_pairs(nullptr, 0, nullptr, nullptr, nullptr, IMSEGM_SCORE_I32, nullptr, 0, nullptr, nullptr, nullptr, nullptr) == 0);
    EXPECT(refused_with(call(nullptr, 2, annots, holes, none, IMSEGM_SCORE_I32, nullptr, 0), "null context"));

    // valid arguments: on a machine without a GPU the call stops at the device, with an error status and untouched outputs
    int n_devices = 0;
    if (hipGetDeviceCount(&n_devices) != hipSuccess || n_devices == 0) {
        EXPECT(call(&ctx, 2, annots, segms, sizes, IMSEGM_SCORE_I32, drop.data(), 3) == -1);
        EXPECT(call(&ctx, 2, annots, holes, none, IMSEGM_SCORE_U8, nullptr, 0) == -1);
    }
    for (int32_t v : status) EXPECT(v == -5);
    for (int32_t v : counts) EXPECT(v == -5);
    for (int32_t v : labels) EXPECT(v == -5);
    EXPECT(tables.front() == -5 && tables.back() == -5);
    static_assert(imsegm::SCORE_CHUNK_PIXELS == 8192, "the sizes above assume 2^40 / 8192 = 2^27 chunks per pair");
    if (failures) std::printf("%d check(s) failed\n", failures);
    else std::printf("api_scoring host checks passed\n");
    return failures ? 1 : 0;
}
