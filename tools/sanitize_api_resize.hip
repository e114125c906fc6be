// Stand-alone host check of csrc/api_resize.hip under AddressSanitizer / UBSan: the argument checks and the caps of
// imsegm_resize_crops and imsegm_ellipse_cut_scale, the paths that return before any launch.  Needs no GPU (every valid call ends at
// "no device"), runs nothing on one, and is not loaded into Python.
//
//   cd pyimsegm_amd/csrc && hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//       -Xarch_host -fno-sanitize-recover=undefined ../../tools/sanitize_api_resize.hip api_resize.hip api_ellipse.hip resize.hip \
//       cut_objects.hip ellipse_place.hip ellipse.hip -o /tmp/sanitize_api_resize && /tmp/sanitize_api_resize
//
// The two helpers the API takes from api.hip (error text, HIP status check) are defined here so that the rest of the library stays out.
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

static int hooks_called = 0;
static int geometry_hook(void *, int, int, int, int, const int64_t *, double *, int32_t *)
{
    ++hooks_called;
    return 1;
}
static int taps_hook(void *, int, const int32_t *, int, int, int32_t *, double *)
{
    ++hooks_called;
    return 1;
}

int main()
{
    const int taps = IMSEGM_RESIZE_MAX_RADIUS + 1;
    // two crops of 3 x 4 and 2 x 5 pixels, 3 channels
    std::vector<uint8_t> packed(3 * 4 * 3 + 2 * 5 * 3, 7);
    std::vector<int64_t> offsets = { 0, 36, 66 };
    std::vector<int32_t> sizes = { 3, 4, 2, 5 }, radii = { 1, 0, 0, 2 };
    std::vector<double> weights(2 * 2 * taps, 0.0), out(2 * 2 * 2 * 3, -1.0);
    std::vector<uint8_t> out_u8(2 * 2 * 2 * 3, 9);
    imsegm_ctx ctx;                                     // a context nobody created on a device: valid calls stop at the device
    auto resize = [&](const uint8_t *p, const int64_t *o, const int32_t *s, int n, int c, int h, int w, const int32_t *r, const double *wt,
                      double *f, uint8_t *u) { return imsegm_resize_crops(&ctx, p, o, s, n, c, h, w, r, wt, f, u); };

    EXPECT(refused_with(resize(nullptr, offsets.data(), sizes.data(), 2, 3, 2, 2, radii.data(), weights.data(), out.data(), nullptr), "null"));
    EXPECT(refused_with(resize(packed.data(), nullptr, sizes.data(), 2, 3, 2, 2, radii.data(), weights.data(), out.data(), nullptr), "null"));
    EXPECT(refused_with(resize(packed.data(), offsets.data(), sizes.data(), 2, 3, 2, 2, radii.data(), nullptr, out.data(), nullptr), "null"));
    EXPECT(refused_with(resize(packed.data(), offsets.data(), sizes.data(), 2, 3, 2, 2, radii.data(), weights.data(), nullptr, nullptr), "null"));
    EXPECT(refused_with(resize(packed.data(), offsets.data(), sizes.data(), 0, 3, 2, 2, radii.data(), weights.data(), out.data(), nullptr), "positive"));
    EXPECT(refused_with(resize(packed.data(), offsets.data(), sizes.data(), 2, 0, 2, 2, radii.data(), weights.data(), out.data(), nullptr), "positive"));
    EXPECT(refused_with(resize(packed.data(), offsets.data(), sizes.data(), 2, 3, 0, 2, radii.data(), weights.data(), out.data(), nullptr), "positive"));
    EXPECT(refused_with(resize(packed.data(), offsets.data(), sizes.data(), 2, 3, 2, -1, radii.data(), weights.data(), out.data(), nullptr), "positive"));
    // the caps: a status without a message, before the tables are read beyond what the status needs
    EXPECT(resize(packed.data(), offsets.data(), sizes.data(), IMSEGM_RESIZE_MAX_CROPS + 1, 3, 2, 2, radii.data(), weights.data(), out.data(), nullptr) ==
           IMSEGM_E_OBJECT_CAPS);
    EXPECT(resize(packed.data(), offsets.data(), sizes.data(), 2, IMSEGM_CUT_OBJECTS_MAX_CHANNELS + 1, 2, 2, radii.data(), weights.data(), out.data(),
                  nullptr) == IMSEGM_E_OBJECT_CAPS);
    EXPECT(resize(packed.data(), offsets.data(), sizes.data(), 2, 3, 32769, 2, radii.data(), weights.data(), out.data(), nullptr) == IMSEGM_E_OBJECT_CAPS);
    EXPECT(resize(packed.data(), offsets.data(), sizes.data(), 2, 3, 32768, 32768, radii.data(), weights.data(), out.data(), nullptr) ==
           IMSEGM_E_OBJECT_CAPS);
    {
        std::vector<int32_t> bad = radii;
        bad[3] = IMSEGM_RESIZE_MAX_RADIUS + 1;
        EXPECT(resize(packed.data(), offsets.data(), sizes.data(), 2, 3, 2, 2, bad.data(), weights.data(), out.data(), nullptr) == IMSEGM_E_OBJECT_CAPS);
        bad[3] = -1;
        EXPECT(refused_with(resize(packed.data(), offsets.data(), sizes.data(), 2, 3, 2, 2, bad.data(), weights.data(), out.data(), nullptr), "negative"));
        std::vector<int32_t> flat = sizes;
        flat[2] = 0;
        EXPECT(refused_with(resize(packed.data(), offsets.data(), flat.data(), 2, 3, 2, 2, radii.data(), weights.data(), out.data(), nullptr), "below 1"));
        flat[2] = 32769;
        EXPECT(resize(packed.data(), offsets.data(), flat.data(), 2, 3, 2, 2, radii.data(), weights.data(), out.data(), nullptr) == IMSEGM_E_OBJECT_CAPS);
        flat[2] = 32768, flat[3] = 32768;              // 3 GiB of one crop: beyond the packed cap
        EXPECT(resize(packed.data(), offsets.data(), flat.data(), 2, 3, 2, 2, radii.data(), weights.data(), out.data(), nullptr) == IMSEGM_E_OBJECT_CAPS);
        std::vector<int64_t> gap = offsets;
        gap[1] = 40;
        EXPECT(refused_with(resize(packed.data(), gap.data(), sizes.data(), 2, 3, 2, 2, radii.data(), weights.data(), out.data(), nullptr), "running sums"));
        gap = offsets, gap[2] = 67;
        EXPECT(refused_with(resize(packed.data(), gap.data(), sizes.data(), 2, 3, 2, 2, radii.data(), weights.data(), out.data(), nullptr), "running sums"));
    }
    EXPECT(refused_with(imsegm_resize_crops(nullptr, packed.data(), offsets.data(), sizes.data(), 2, 3, 2, 2, radii.data(), weights.data(), out.data(),
                                            out_u8.data()), "null context"));

    // the chain: a 6 x 7 image of 3 channels and two ellipses
    std::vector<uint8_t> image(6 * 7 * 3, 50), bg = { 1, 2, 3 };
    std::vector<int32_t> geom = { 3, 3, 2, 2, 2, 2, 4, 4, 2, 4, 1, 2, 2, 3, 2, 5 };
    std::vector<double> sincos = { 0.0, 1.0, 0.6, 0.8 };
    int first_empty = -7;
    auto chain = [&](const uint8_t *img, int H, int W, int c, int n, const int32_t *g, const double *sc, const uint8_t *b, int h, int w,
                     imsegm_cut_geometry_fn gf, imsegm_blur_taps_fn tf, double *f, uint8_t *u, int *fe) {
        return imsegm_ellipse_cut_scale(&ctx, img, H, W, c, n, g, sc, b, h, w, gf, tf, nullptr, f, u, fe);
    };
    EXPECT(refused_with(chain(nullptr, 6, 7, 3, 2, geom.data(), sincos.data(), bg.data(), 2, 2, geometry_hook, taps_hook, nullptr, out_u8.data(), &first_empty), "null"));
    EXPECT(refused_with(chain(image.data(), 6, 7, 3, 2, nullptr, sincos.data(), bg.data(), 2, 2, geometry_hook, taps_hook, nullptr, out_u8.data(), &first_empty), "null"));
    EXPECT(refused_with(chain(image.data(), 6, 7, 3, 2, geom.data(), sincos.data(), nullptr, 2, 2, geometry_hook, taps_hook, nullptr, out_u8.data(), &first_empty), "null"));
    EXPECT(refused_with(chain(image.data(), 6, 7, 3, 2, geom.data(), sincos.data(), bg.data(), 2, 2, nullptr, taps_hook, nullptr, out_u8.data(), &first_empty), "null"));
    EXPECT(refused_with(chain(image.data(), 6, 7, 3, 2, geom.data(), sincos.data(), bg.data(), 2, 2, geometry_hook, nullptr, nullptr, out_u8.data(), &first_empty), "null"));
    EXPECT(refused_with(chain(image.data(), 6, 7, 3, 2, geom.data(), sincos.data(), bg.data(), 2, 2, geometry_hook, taps_hook, nullptr, nullptr, &first_empty), "null"));
    EXPECT(refused_with(chain(image.data(), 6, 7, 3, 2, geom.data(), sincos.data(), bg.data(), 2, 2, geometry_hook, taps_hook, nullptr, out_u8.data(), nullptr), "null"));
    EXPECT(refused_with(chain(image.data(), 6, 7, 3, 0, geom.data(), sincos.data(), bg.data(), 2, 2, geometry_hook, taps_hook, nullptr, out_u8.data(), &first_empty), "positive"));
    EXPECT(refused_with(chain(image.data(), 6, 7, 3, 2, geom.data(), sincos.data(), bg.data(), 0, 2, geometry_hook, taps_hook, nullptr, out_u8.data(), &first_empty), "positive"));
    EXPECT(refused_with(chain(image.data(), 0, 7, 3, 2, geom.data(), sincos.data(), bg.data(), 2, 2, geometry_hook, taps_hook, nullptr, out_u8.data(), &first_empty), "height and width"));
    EXPECT(refused_with(chain(image.data(), 46341, 46341, 3, 2, geom.data(), sincos.data(), bg.data(), 2, 2, geometry_hook, taps_hook, nullptr, out_u8.data(), &first_empty),
                        "2^31"));
    EXPECT(chain(image.data(), 6, 7, 5, 2, geom.data(), sincos.data(), bg.data(), 2, 2, geometry_hook, taps_hook, nullptr, out_u8.data(), &first_empty) ==
           IMSEGM_E_OBJECT_CAPS);
    EXPECT(chain(image.data(), 6, 7, 3, IMSEGM_RESIZE_MAX_CROPS + 1, geom.data(), sincos.data(), bg.data(), 2, 2, geometry_hook, taps_hook, nullptr, out_u8.data(),
                 &first_empty) == IMSEGM_E_OBJECT_CAPS);
    {
        std::vector<int32_t> bad = geom;
        bad[14] = 6;                                    // last row of the second box beyond the image
        EXPECT(refused_with(chain(image.data(), 6, 7, 3, 2, bad.data(), sincos.data(), bg.data(), 2, 2, geometry_hook, taps_hook, nullptr, out_u8.data(), &first_empty),
                            "not clipped"));
        bad = geom, bad[2] = 0;
        EXPECT(refused_with(chain(image.data(), 6, 7, 3, 2, bad.data(), sincos.data(), bg.data(), 2, 2, geometry_hook, taps_hook, nullptr, out_u8.data(), &first_empty),
                            "radius below 1"));
    }
    EXPECT(first_empty == -7 && hooks_called == 0);     // no refused call wrote a result or reached a hook
    for (uint8_t v : out_u8) EXPECT(v == 9);
    for (double v : out) EXPECT(v == -1.0);

    // valid arguments: on a machine without a GPU the call stops at the device, with an error status and untouched outputs
    int n_devices = 0;
    if (hipGetDeviceCount(&n_devices) != hipSuccess || n_devices == 0) {
        EXPECT(resize(packed.data(), offsets.data(), sizes.data(), 2, 3, 2, 2, radii.data(), weights.data(), out.data(), out_u8.data()) == -1);
        EXPECT(chain(image.data(), 6, 7, 3, 2, geom.data(), sincos.data(), bg.data(), 2, 2, geometry_hook, taps_hook, out.data(), out_u8.data(), &first_empty) == -1);
        EXPECT(first_empty == -7 && hooks_called == 0);
    }
    if (failures) std::printf("%d check(s) failed\n", failures);
    else std::printf("api_resize host checks passed\n");
    return failures ? 1 : 0;
}
