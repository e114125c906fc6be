// natives.hip -- the two remaining natives of the reference's Cython module, for BATCHES of positions (one launch):
//   computeLabelHistogram2d      /root/reference/imsegm/features_cython.pyx:222-241   (descriptors.py:1411-1495)
//   computeRayFeaturesBinary2d   features_cython.pyx:244-282                          (descriptors.py:1630-1660)
// The reference calls them once per position from Python loops (compute_label_hist_proba, compute_ray_features_positions,
// the region-growing and centre-detection tools); here one wave serves one position.
#include "raywalk.h"
#include "slic.h"

namespace imsegm {

// hist[p][l] = number of pixels of window p (segm[y0 : y0 + h, x0 : x0 + w]) with label l >= 0 where the structuring
// element (rows from sy0, columns from sx0) equals 1.  Integer atomics: exact, order independent.
__global__ void __launch_bounds__(256)
k_label_hist2d(const int16_t *__restrict__ segm, int H, int W, const int32_t *__restrict__ windows, int P,
               const int16_t *__restrict__ selem, int SH, int SW, int nb_labels, unsigned int *__restrict__ hist)
{
    const int p = blockIdx.x;
    if (p >= P) return;
    const int y0 = windows[6 * p + 0], x0 = windows[6 * p + 1], h = windows[6 * p + 2], w = windows[6 * p + 3];
    const int sy0 = windows[6 * p + 4], sx0 = windows[6 * p + 5];
    const int n = h * w;
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const int r = i / w, c = i - r * w;
        const int y = y0 + r, x = x0 + c, sy = sy0 + r, sx = sx0 + c;
        if (y < 0 || y >= H || x < 0 || x >= W || sy < 0 || sy >= SH || sx < 0 || sx >= SW) continue;
        const int l = segm[(size_t)y * W + x];
        if (l >= 0 && l < nb_labels && selem[(size_t)sy * SW + sx] == 1) atomicAdd(&hist[(size_t)p * nb_labels + l], 1u);
    }
}

// Ray features: from every position a ray per angle walks the binary segmentation until it meets the searched edge ('up' = 1:
// first foreground pixel, 'down' = -1: first background pixel after foreground); the walk and its precision are ray_walk's
// (raywalk.h), the per-angle direction table comes from the host.  One wave per position, one lane per angle.
__global__ void __launch_bounds__(64)
k_ray_features_binary2d(const int8_t *__restrict__ seg, int H, int W, const int32_t *__restrict__ positions, int P,
                        const float *__restrict__ grad, int A, int edge, float *__restrict__ out)
{
    const int p = blockIdx.x;
    if (p >= P) return;
    const int py = positions[2 * p], px = positions[2 * p + 1];
    const bool inside = py >= 0 && py < H && px >= 0 && px < W;
    auto on_mask = [&](int y, int x) -> bool { return seg[(size_t)y * W + x] != 0; };
    const bool start = inside ? on_mask(py, px) : false;
    const int diag = ray_walk_limit(H, W);
    for (int a = threadIdx.x; a < A; a += blockDim.x)
        out[(size_t)p * A + a] = ray_walk(py, px, inside, start, grad[2 * a], grad[2 * a + 1], H, W, diag, edge, on_mask);
}

int launch_label_hist2d(const int16_t *segm, int H, int W, const int32_t *windows, int P, const int16_t *selem, int SH, int SW,
                        int nb_labels, unsigned int *hist, hipStream_t st)
{
    HIP_TRY(hipMemsetAsync(hist, 0, (size_t)P * nb_labels * sizeof(unsigned int), st));
    if (P > 0) hipLaunchKernelGGL(k_label_hist2d, P, 256, 0, st, segm, H, W, windows, P, selem, SH, SW, nb_labels, hist);
    HIP_TRY(hipGetLastError());
    return 0;
}

int launch_ray_features_binary2d(const int8_t *seg, int H, int W, const int32_t *positions, int P, const float *grad, int A, int edge,
                                 float *out, hipStream_t st)
{
    if (P > 0) hipLaunchKernelGGL(k_ray_features_binary2d, P, 64, 0, st, seg, H, W, positions, P, grad, A, edge, out);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // namespace imsegm
