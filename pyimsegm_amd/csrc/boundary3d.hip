// boundary3d.hip -- the third axis of boundary.hip: the thick boundary mask of a D x H x W label volume and the depth pass of the
// exact Euclidean distance transform, the device side of imsegm/labeling.py compute_boundary_distances (:684-716) on volumes
// (find_boundaries and distance_transform_edt work in n dimensions there).
//
//   mask      uint8 per voxel, 1 where a 6-neighbour inside the volume carries another label; one flag for the volume, one per slice
//   slices    boundary.hip's column and row pass in every slice that has a set voxel (launch_edt_slices):
//             s(z, y, x) = min over (y', x') of (y - y')^2 + (x - x')^2 to the set voxels of slice z, NONE all over an empty slice
//   depth     d2(z, y, x) = min over z' of (z - z')^2 + s(z', y, x)                       (uint32, outward search, lanes along x)
//   value     sqrt((double)d2), the one fp64 operation (see boundary.hip on why it is scipy's bit for bit)
//
// Squared distances are uint32: the caller refuses volumes with D^2 + H^2 + W^2 > 2^32 - 1 (edt3d_size_ok), nothing wraps; NONE is
// compared with, never added to.
#include "slic.h"

namespace imsegm {

constexpr uint32_t EDT3D_NONE = 0xffffffffu;    // boundary.hip's EDT_NONE

// ---------------------------------------------------------------------------------------------------
// mask: skimage.segmentation.find_boundaries(mode='thick') in three dimensions.  A workgroup owns 64 x 4 voxels of one slice, so a
// wave reads 64 neighbouring labels of a row in each of its seven loads.  flags[0] and flags[1 + z] (zeroed by the launcher) are
// raised when a voxel is set.
// ---------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
k_boundary_mask3d(const int32_t *__restrict__ labels, int D, int H, int W, uint8_t *__restrict__ mask, int *__restrict__ flags)
{
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6), z = blockIdx.z;
    const size_t HW = (size_t)H * (size_t)W;
    bool set = false;
    if (x < W && y < H) {
        const size_t i = (size_t)z * HW + (size_t)y * W + x;
        const int c = labels[i];
        const int lf = z > 0 ? labels[i - HW] : c, lb = z + 1 < D ? labels[i + HW] : c;
        const int lu = y > 0 ? labels[i - W] : c, ld = y + 1 < H ? labels[i + W] : c;
        const int ll = x > 0 ? labels[i - 1] : c, lr = x + 1 < W ? labels[i + 1] : c;
        set = lf != c || lb != c || lu != c || ld != c || ll != c || lr != c;
        mask[i] = set ? 1 : 0;
    }
    // two integer atomics per wave that has a set voxel: the words only ever go from 0 to 1
    if (__ballot(set) != 0 && (threadIdx.x & 63) == 0) {
        atomicOr(flags, 1);
        atomicOr(flags + 1 + z, 1);
    }
}

// ---------------------------------------------------------------------------------------------------
// depth pass: one thread per voxel, threads along the H * W voxels of a slice (a wave reads 64 neighbouring words of slice z - k
// and of slice z + k).  A lane looks at k = 1, 2, ... and stops at the first k with k^2 >= its best value (no farther slice can do
// better: s >= 0) or when both slices have left the volume: at most D - 1 steps, with a depth of 64 a few dozen.  Slices without a
// set voxel are skipped by their flag (uniform over the workgroup), their s is NONE anyway.  No mask at all (flags[0] == 0):
// scipy's distance_transform_edt answers as if ONE zero sat at (slice -1, row 0, column 0), d2 = (z + 1)^2 + y^2 + x^2 (see
// k_edt_rows for the two-dimensional form of it) -- restated here, the test compares against scipy at run time.
// ---------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
k_edt_depth(const uint32_t *__restrict__ s, int D, size_t HW, int W, const int *__restrict__ flags, uint32_t *__restrict__ d2_out,
            double *__restrict__ dist_out)
{
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    const int z = blockIdx.y;
    if (p >= HW) return;
    const int *slice_set = flags + 1;
    uint32_t best = EDT3D_NONE;
    if (flags[0] == 0) {                               // (uniform over the grid)
        const uint32_t y = (uint32_t)(p / (size_t)W), x = (uint32_t)(p % (size_t)W);
        best = (uint32_t)(z + 1) * (uint32_t)(z + 1) + y * y + x * x;
    } else {
        if (slice_set[z]) best = s[(size_t)z * HW + p];
        for (int k = 1; k < D; ++k) {
            const uint32_t k2 = (uint32_t)k * (uint32_t)k;
            const bool before = z - k >= 0, after = z + k < D;
            if (k2 >= best || (!before && !after)) break;
            if (before && slice_set[z - k]) {
                const uint32_t v = s[(size_t)(z - k) * HW + p];
                if (v != EDT3D_NONE) best = min(best, k2 + v);
            }
            if (after && slice_set[z + k]) {
                const uint32_t v = s[(size_t)(z + k) * HW + p];
                if (v != EDT3D_NONE) best = min(best, k2 + v);
            }
        }
    }
    const size_t i = (size_t)z * HW + p;
    d2_out[i] = best;
    if (dist_out) dist_out[i] = sqrt((double)best);
}

// ---------------------------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------------------------
int edt3d_size_ok(int D, int H, int W)
{
    if (D < 1 || H < 1 || W < 1) {
        set_error("boundary3d: depth, height and width must be positive");
        return 0;
    }
    // uint32 squared distances: (D - 1)^2 + (H - 1)^2 + (W - 1)^2, and D^2 + (H - 1)^2 + (W - 1)^2 for a volume without a set voxel,
    // must stay below NONE.  The bound also keeps D and H within the 65535 of a launch grid's y and z extent
    const unsigned long long d = (unsigned long long)D, h = (unsigned long long)H, w = (unsigned long long)W;
    if (d * d + h * h + w * w > 0xffffffffull) {
        set_error("boundary3d: D^2 + H^2 + W^2 exceeds 2^32 - 1, squared distances would not fit 32 bits");
        return 0;
    }
    if (d * h * w > 0x40000000ull) {                   // (the cap of a volume session, imsegm_volume_create)
        set_error("boundary3d: more than 2^30 voxels");
        return 0;
    }
    return 1;
}

int launch_boundary_mask3d(const int32_t *labels, int D, int H, int W, uint8_t *mask, int *flags, hipStream_t st)
{
    HIP_TRY(hipMemsetAsync(flags, 0, ((size_t)D + 1) * sizeof(int), st));
    hipLaunchKernelGGL(k_boundary_mask3d, dim3(cdiv(W, 64), cdiv(H, 4), D), 256, 0, st, labels, D, H, W, mask, flags);
    HIP_TRY(hipGetLastError());
    return 0;
}

int launch_edt3d(const uint8_t *mask, const int *flags, int D, int H, int W, uint32_t *g, uint32_t *d2_out, double *dist_out,
                 hipStream_t st)
{
    // columns: mask -> d2_out (as g of the slices), rows: d2_out -> g (the slices' own distances), depth: g -> d2_out
    if (launch_edt_slices(mask, flags + 1, D, H, W, d2_out, g, st)) return -1;
    const size_t HW = (size_t)H * (size_t)W;
    hipLaunchKernelGGL(k_edt_depth, dim3((unsigned)((HW + 255) / 256), D), 256, 0, st, g, D, HW, W, flags, d2_out, dist_out);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // namespace imsegm
