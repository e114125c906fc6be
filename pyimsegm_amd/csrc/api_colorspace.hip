// api_colorspace.hip -- C ABI of the colour-space conversion of the resident image (kernels: colorspace.hip)
#include "session.h"

extern "C" {

int imsegm_image2d_convert_color(imsegm_image2d *im, int space, const double *matrix9)
{
    if (!im) {
        set_error("null session");
        return -1;
    }
    // every refusal comes before the first device call
    if (wrong_kind(im, false)) return -1;
    if (im->dtype < 0 || !im->img.p) {
        set_error("convert_color needs an uploaded image");
        return -1;
    }
    if (space != 0 && space != CS_HSV && space != CS_LUV && space != CS_LAB && space != CS_HED && space != CS_XYZ) {
        set_error("convert_color: the colour space is 0 (back to the upload), 1 hsv, 2 luv, 3 lab, 4 hed or 5 xyz");
        return -1;
    }
    if (space == CS_HED && !matrix9) {
        set_error("convert_color: hed needs the 3 x 3 stain matrix");
        return -1;
    }
    if (space == 0) {
        im->conv_source = false;
        return 0;
    }
    if (bind(im->ctx)) return -1;
    ColorMatrix mat;
    for (int i = 0; i < 9; ++i) mat.m[i] = matrix9 ? matrix9[i] : 0.0;
    im->conv_source = false;
    if (im->conv.ensure(im->n * 3 * sizeof(double) + 16)) return -1;
    const int sp = im->ctx->begin(PG_STATS);          // (profiled with the descriptor statistics it feeds)
    if (launch_convert_color(im->img.p, im->dtype, im->n, space, mat, im->conv.as<double>(), im->ctx->stream)) return -1;
    im->ctx->end(sp);
    im->conv_source = true;
    return 0;
}

int imsegm_image2d_get_converted(imsegm_image2d *im, double *out_hw3)
{
    if (!im) {
        set_error("null session");
        return -1;
    }
    if (wrong_kind(im, false)) return -1;
    if (!im->conv_source || !out_hw3) {
        set_error("get_converted needs a conversion (imsegm_image2d_convert_color) and an output");
        return -1;
    }
    if (bind(im->ctx)) return -1;
    hipStream_t st = im->ctx->stream;
    HIP_TRY(hipMemcpyAsync(out_hw3, im->conv.p, im->n * 3 * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

}  // extern "C"
