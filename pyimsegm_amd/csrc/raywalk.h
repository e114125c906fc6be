// raywalk.h -- the ray walk of computeRayFeaturesBinary2d (imsegm/features_cython.pyx:244-282), stated once for every kernel that
// casts rays: k_ray_features_binary2d (natives.hip), k_ray_features_labels2d (points.hip), k_boundary_rays (morphology.hip),
// k_rg_object_rays (region_growing.hip), k_os_rays (object_shapes.hip).  They differ only in what "this pixel is on the mask" means,
// which each hands over as a predicate, and in whether the edge 'up' exists.
//
// The precision chain is a bit-exactness contract with the compiled reference, and this is its one statement: the position is a
// float32 pair advanced by the float32 step (g0, g1) -- sin / cos of the float32 angle divided by its larger component, formed on the
// host with the numpy calls the reference makes; the pixel under it is round() of the position in fp64 (half away from zero); the
// ray leaves the image where a float32 coordinate is negative or a rounded one reaches H or W; the distance is the fp64 root of the
// float32 sum of the float32 squares of the offset, stored as float32.  The host statement of the same walk is ray_walk_host
// (descriptors.py).
#pragma once
#include "common.h"

namespace imsegm {

// One ray from (py, px) in unit steps of the larger direction component, at most `diag` of them, until it meets the searched edge
// (edge 1, 'up': the first pixel on the mask; edge -1, 'down': the first pixel off the mask after one on it).  `inside`: the
// position lies in the image; `start`: it lies on the mask (false outside the image).  on_mask(y, x) is asked for pixels inside the
// image only.  Returns 0 for 'up' from a position on the mask, the distance to the edge, or -1 where the ray meets none.
template <typename OnMask>
__device__ __forceinline__ float ray_walk(int py, int px, bool inside, bool start, float g0, float g1, int H, int W, int diag, int edge,
                                          OnMask on_mask)
{
    if (start && edge == 1) return 0.f;
    if (!inside) return -1.f;
    float pos0 = (float)py, pos1 = (float)px;
    bool last = start;
    for (int it = 0; it < diag; ++it) {
        pos0 += g0;
        pos1 += g1;
        const double r0 = round((double)pos0), r1 = round((double)pos1);
        if (pos0 < 0 || r0 >= H || pos1 < 0 || r1 >= W) break;
        const bool actual = on_mask((int)r0, (int)r1);
        if ((edge == 1 && actual) || (edge == -1 && last && !actual)) {
            const float dx = pos0 - (float)py, dy = pos1 - (float)px;
            return (float)sqrt((double)((dx * dx) + (dy * dy)));
        }
        last = actual;
    }
    return -1.f;
}

// the step limit of every walk: the diagonal of the image, truncated
__device__ __forceinline__ int ray_walk_limit(int H, int W) { return (int)sqrt((double)W * W + (double)H * H); }

}  // namespace imsegm
