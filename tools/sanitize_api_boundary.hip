// Stand-alone host check of csrc/api_boundary.hip under AddressSanitizer / UBSan: argument validation and buffer sizing.
// Needs no GPU (every valid call ends at "no device"), runs nothing on one, and is not loaded into Python.
//
//   cd pyimsegm_amd/csrc && hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//       -Xarch_host -fno-sanitize-recover=undefined ../../tools/sanitize_api_boundary.hip api_boundary.hip boundary.hip scan.hip stats.hip \
//       -o /tmp/sanitize_api_boundary && /tmp/sanitize_api_boundary
//
// The two helpers the API takes from api.hip (error text, HIP status check) are defined here so that the rest of the library stays out.
#include "../pyimsegm_amd/csrc/session.h"

#include <algorithm>
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

// the pieces of a plan are 256-byte aligned, disjoint and inside `bytes`
static void check_plan(int H, int W, int kind)
{
    const imsegm::BoundaryPlan p = imsegm::boundary_plan(H, W, kind);
    const size_t n = (size_t)H * W;
    std::vector<std::pair<size_t, size_t>> parts;       // (offset, size)
    parts.push_back({ p.o_ref, n * 4 });
    if (kind == 2) parts.push_back({ p.o_seg, n * 4 });
    if (kind != 0) parts.push_back({ p.o_g, n * 4 });
    if (kind >= 2) parts.push_back({ p.o_d2, n * 4 });
    if (kind == 1) parts.push_back({ p.o_dist, n * 8 });
    parts.push_back({ p.o_mask_a, n });
    if (kind >= 2) {
        parts.push_back({ p.o_mask_b, n });
        parts.push_back({ p.o_counts, imsegm::compact_count_words(n) * 4 });
    }
    parts.push_back({ p.o_flags, 2 * sizeof(int) });
    std::sort(parts.begin(), parts.end());
    for (size_t i = 0; i < parts.size(); ++i) {
        EXPECT(parts[i].first % 256 == 0);
        EXPECT(parts[i].first + parts[i].second <= (i + 1 < parts.size() ? parts[i + 1].first : p.bytes));
    }
    EXPECT(imsegm::compact_count_words(n) == (n + 2047) / 2048 + 1);
}

int main()
{
    std::vector<int32_t> labels(6 * 7, 0);
    std::vector<uint8_t> mask(6 * 7);
    std::vector<double> dist(6 * 7);
    std::vector<int32_t> points(2 * 6 * 7);
    std::vector<int64_t> overlap(4);
    int count = -5;
    imsegm_ctx ctx;                                     // a context nobody created on a device: valid calls stop at the device

    EXPECT(refused_with(imsegm_boundary_mask(&ctx, nullptr, 6, 7, 0, 0, mask.data()), "null array"));
    EXPECT(refused_with(imsegm_boundary_mask(&ctx, labels.data(), 6, 7, 0, 0, nullptr), "null array"));
    EXPECT(refused_with(imsegm_boundary_mask(&ctx, labels.data(), 0, 7, 0, 0, mask.data()), "positive"));
    EXPECT(refused_with(imsegm_boundary_mask(&ctx, labels.data(), 6, -1, 0, 0, mask.data()), "positive"));
    EXPECT(refused_with(imsegm_boundary_mask(&ctx, labels.data(), 6, 7, 3, 0, mask.data()), "unknown mode"));
    EXPECT(refused_with(imsegm_boundary_mask(nullptr, labels.data(), 6, 7, 0, 0, mask.data()), "null context"));
    EXPECT(refused_with(imsegm_distance_map(&ctx, labels.data(), 6, 7, -1, 0, dist.data()), "unknown mode"));
    EXPECT(refused_with(imsegm_distance_map(&ctx, labels.data(), 6, 7, 1, 0, nullptr), "null array"));
    // squared distances beyond 32 bits: refused from the sizes alone, before any array is read
    EXPECT(refused_with(imsegm_distance_map(&ctx, labels.data(), 1, 65536, 0, 0, dist.data()), "32 bits"));
    EXPECT(refused_with(imsegm_distance_map(&ctx, labels.data(), 46341, 46341, 0, 0, dist.data()), "32 bits"));
    EXPECT(refused_with(imsegm_distance_map(&ctx, labels.data(), 2147483647, 2147483647, 0, 0, dist.data()), "32 bits"));
    EXPECT(refused_with(imsegm_boundary_distances(&ctx, labels.data(), labels.data(), 65535, 4097, points.data(), dist.data(), 42, &count), "32 bits"));
    EXPECT(imsegm::edt_size_ok(46340, 46340) == 1 && imsegm::edt_size_ok(65535, 361) == 1 && imsegm::edt_size_ok(65535, 363) == 0);
    EXPECT(refused_with(imsegm_boundary_distances(&ctx, labels.data(), nullptr, 6, 7, points.data(), dist.data(), 42, &count), "null array"));
    EXPECT(refused_with(imsegm_boundary_distances(&ctx, labels.data(), labels.data(), 6, 7, points.data(), dist.data(), 42, nullptr), "required"));
    EXPECT(refused_with(imsegm_boundary_distances(&ctx, labels.data(), labels.data(), 6, 7, nullptr, dist.data(), 42, &count), "required"));
    EXPECT(refused_with(imsegm_boundary_distances(&ctx, labels.data(), labels.data(), 6, 7, points.data(), dist.data(), -1, &count), "required"));
    EXPECT(refused_with(imsegm_image2d_boundary_distances(nullptr, labels.data(), points.data(), dist.data(), 42, &count), "null session"));
    imsegm_image2d session;
    session.ctx = &ctx;
    session.H = 6, session.W = 7, session.n = 42;
    EXPECT(refused_with(imsegm_image2d_boundary_distances(&session, labels.data(), points.data(), dist.data(), 42, &count), "needs a label map"));
    session.have_labels = true;
    EXPECT(refused_with(imsegm_image2d_boundary_distances(&session, nullptr, points.data(), dist.data(), 42, &count), "required"));
    session.is_volume = true;
    EXPECT(refused_with(imsegm_image2d_boundary_distances(&session, labels.data(), points.data(), dist.data(), 42, &count), "2-D"));
    EXPECT(count == -5);                                // no refused call wrote the count
    EXPECT(refused_with(imsegm_labels_overlap(&ctx, labels.data(), labels.data(), 42, 0, 2, overlap.data()), "required"));
    EXPECT(refused_with(imsegm_labels_overlap(&ctx, labels.data(), nullptr, 42, 2, 2, overlap.data()), "required"));
    EXPECT(refused_with(imsegm_labels_overlap(&ctx, labels.data(), labels.data(), 42, 1 << 20, 1 << 20, overlap.data()), "2^28"));
    EXPECT(refused_with(imsegm_labels_overlap(&ctx, labels.data(), labels.data(), 42, 2147483647, 2147483647, overlap.data()), "2^28"));
    EXPECT(refused_with(imsegm_labels_overlap(&ctx, labels.data(), labels.data(), (size_t)1 << 41, 2, 2, overlap.data()), "2^40"));

    const int sides[] = { 1, 2, 7, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 46340 };
    for (int H : sides)
        for (int W : sides)
            for (int kind = 0; kind < 4; ++kind) check_plan(H, W, kind);

    // valid arguments: on a machine without a GPU the call stops at the device, with an error status and untouched outputs
    int n_devices = 0;
    if (hipGetDeviceCount(&n_devices) != hipSuccess || n_devices == 0) {
        EXPECT(imsegm_boundary_mask(&ctx, labels.data(), 6, 7, 0, 0, mask.data()) == -1);
        EXPECT(imsegm_distance_map(&ctx, labels.data(), 6, 7, 1, 1, dist.data()) == -1);
        EXPECT(imsegm_boundary_distances(&ctx, labels.data(), labels.data(), 6, 7, points.data(), dist.data(), 42, &count) == -1);
        EXPECT(imsegm_labels_overlap(&ctx, labels.data(), labels.data(), 42, 2, 2, overlap.data()) == -1);
        EXPECT(count == -5);
    }
    if (failures) std::printf("%d check(s) failed\n", failures);
    else std::printf("api_boundary host checks passed\n");
    return failures ? 1 : 0;
}
