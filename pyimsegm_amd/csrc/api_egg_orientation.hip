// api_egg_orientation.hip -- C ABI of the orientation step of the egg cut-outs (experiments_ovary_detect/run_egg_swap_orientation.py
// of the reference: main :101-128).  Stateless calls on a context and host arrays; arguments and caps are checked before the device
// is touched.  The stack goes up once and stays in the context's scratch between the kernels of egg_orientation.hip; the template,
// the sums and the flags come down, and of the stack only the images that were turned.
#include <cstring>

#include "egg_orientation.h"
#include "session.h"

static_assert(EO_SUM_WORDS == IMSEGM_ORIENT_SUM_WORDS && EO_MAX_IMAGES == IMSEGM_ORIENT_MAX_IMAGES, "include/imsegm_hip.h");

namespace imsegm {

namespace {

// where the pieces of one call live inside the context's scratch buffer (every piece starts on a 256-byte boundary)
struct EoPlan {
    size_t o_stack, o_planes, o_template, o_sums, o_flags, o_range, bytes;
};

EoPlan eo_plan(size_t N, size_t hw, size_t C)
{
    EoPlan p;
    size_t at = 0;
    auto take = [&at](size_t bytes) {
        const size_t here = at;
        at += (bytes + 255) & ~(size_t)255;
        return here;
    };
    p.o_stack = take(N * hw * C);
    p.o_planes = C > 1 ? take(N * hw) : p.o_stack;          // one channel: the stack is its own plane set
    p.o_template = take(hw * 2);
    p.o_sums = take(N * EO_SUM_WORDS * 8);
    p.o_flags = take(N);
    p.o_range = take(8);
    p.bytes = at;
    return p;
}

int check_stack(const char *who, const void *stack, int N, int h, int w, int C, int channel)
{
    if (!stack) {
        set_error(std::string(who) + ": null argument");
        return -1;
    }
    if (N < 1 || h < 1 || w < 1 || C < 1 || channel < 0 || channel >= C) {
        set_error(std::string(who) + ": the number of images, height, width and channels must be positive and the channel one of them");
        return -1;
    }
    const unsigned long long hw = (unsigned long long)h * (unsigned long long)w;
    if (N > EO_MAX_IMAGES || C > EO_MAX_CHANNELS || hw > EO_MAX_PIXELS || hw * (unsigned long long)N * (unsigned long long)C > EO_MAX_BYTES)
        return IMSEGM_E_OBJECT_CAPS;
    return 0;
}

// the stack at o_stack -> the channel planes at o_planes and, without a given template, template2 at o_template
int template_run(imsegm_ctx *ctx, unsigned char *dev, const EoPlan &p, int N, size_t hw, int C, int channel, bool median)
{
    if (C > 1 && launch_eo_extract(dev + p.o_stack, N, hw, C, channel, dev + p.o_planes, ctx->stream)) return -1;
    if (!median) return 0;
    const int span = ctx->begin(PG_STATS);
    const int status = launch_eo_median(dev + p.o_planes, N, hw, reinterpret_cast<uint16_t *>(dev + p.o_template), ctx->stream);
    ctx->end(span);
    return status;
}

}  // namespace

}  // namespace imsegm

extern "C" {

int imsegm_stack_median_u8(imsegm_ctx *ctx, const uint8_t *stack, int n_images, int height, int width, int channels, int channel,
                           uint16_t *template2_out)
{
    if (const int status = check_stack("stack_median_u8", stack, n_images, height, width, channels, channel)) return status;
    if (!template2_out) {
        set_error("stack_median_u8: null argument");
        return -1;
    }
    if (bind(ctx)) return -1;
    hipStream_t st = ctx->stream;
    const size_t hw = (size_t)height * width;
    const EoPlan p = eo_plan((size_t)n_images, hw, (size_t)channels);
    if (ctx->gc_buf.ensure(p.bytes)) return -1;
    unsigned char *dev = ctx->gc_buf.as<unsigned char>();
    HIP_TRY(hipMemcpyAsync(dev + p.o_stack, stack, (size_t)n_images * hw * channels, hipMemcpyHostToDevice, st));
    if (template_run(ctx, dev, p, n_images, hw, channels, channel, true)) return -1;
    HIP_TRY(hipMemcpyAsync(template2_out, dev + p.o_template, hw * 2, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

int imsegm_orient_stack(imsegm_ctx *ctx, const uint8_t *stack, int n_images, int height, int width, int channels, int channel, int mode,
                        const uint16_t *template2_in, uint16_t *template2_out, uint8_t *flags_out, int64_t *sums_out, uint8_t *turned_out)
{
    if (const int status = check_stack("orient_stack", stack, n_images, height, width, channels, channel)) return status;
    if (!template2_out || !flags_out || !sums_out || !turned_out) {
        set_error("orient_stack: null argument");
        return -1;
    }
    if (mode != EO_MODE_CC && mode != EO_MODE_DENSITY) {
        set_error("orient_stack: the mode is 0 (correlation) or 1 (density)");
        return -1;
    }
    const size_t hw = (size_t)height * width, N = (size_t)n_images, image_bytes = hw * channels;
    if (template2_in)
        for (size_t i = 0; i < hw; ++i)
            if (template2_in[i] > 510) {
                set_error("orient_stack: a given template2 lies in 0 .. 510");
                return -1;
            }
    if (bind(ctx)) return -1;
    hipStream_t st = ctx->stream;
    const EoPlan p = eo_plan(N, hw, (size_t)channels);
    if (ctx->gc_buf.ensure(p.bytes)) return -1;
    unsigned char *dev = ctx->gc_buf.as<unsigned char>();
    uint16_t *tmpl = reinterpret_cast<uint16_t *>(dev + p.o_template);
    uint32_t *range = reinterpret_cast<uint32_t *>(dev + p.o_range);
    HIP_TRY(hipMemcpyAsync(dev + p.o_stack, stack, N * image_bytes, hipMemcpyHostToDevice, st));
    if (template2_in) HIP_TRY(hipMemcpyAsync(tmpl, template2_in, hw * 2, hipMemcpyHostToDevice, st));
    if (template_run(ctx, dev, p, n_images, hw, channels, channel, template2_in == nullptr)) return -1;
    if (launch_eo_template_range(tmpl, hw, range, st)) return -1;
    if (launch_eo_sums(dev + p.o_planes, n_images, height, width, tmpl, range, mode, reinterpret_cast<long long *>(dev + p.o_sums),
                       dev + p.o_flags, st))
        return -1;
    if (launch_eo_turn(dev + p.o_stack, n_images, hw, channels, dev + p.o_flags, st)) return -1;
    HIP_TRY(hipMemcpyAsync(template2_out, tmpl, hw * 2, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(sums_out, dev + p.o_sums, N * EO_SUM_WORDS * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(flags_out, dev + p.o_flags, N, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    // only the turned images come down, one copy per run of them; the others are the caller's own bytes
    for (size_t i = 0; i < N;) {
        size_t j = i + 1;
        while (j < N && (flags_out[j] != 0) == (flags_out[i] != 0)) ++j;
        if (flags_out[i])
            HIP_TRY(hipMemcpyAsync(turned_out + i * image_bytes, dev + p.o_stack + i * image_bytes, (j - i) * image_bytes,
                                   hipMemcpyDeviceToHost, st));
        else if (turned_out != stack)
            memcpy(turned_out + i * image_bytes, stack + i * image_bytes, (j - i) * image_bytes);
        i = j;
    }
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

}  // extern "C"
