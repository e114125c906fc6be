// morphology.hip -- the smoothing of an egg class map and the rays on its two masks, on the device:
//   split_segm_background_foreground     imsegm/ellipse_fitting.py:400-443 (scipy.ndimage binary_fill_holes, skimage.morphology
//                                        opening with disk(r) for integer r)
//   compute_ray_features_segm_2d         per centre on seg_bg ('up') and seg_fg ('down'), ellipse_fitting.py:385-390, :480-482,
//                                        :531-533, :581 (the walk of raywalk.h)
// Integers only up to the ray walk: a pixel survives the erosion when no 0 of the image lies within dy^2 + dx^2 <= r^2 of it, and is
// set by the dilation when a surviving pixel does; pixels outside the image never count ("Boundary points").
#include "morphology.h"
#include "raywalk.h"
#include "unionfind.h"

namespace imsegm {

// ---- hole filling: one labelling of the zero pixels (segm <= 0), 4-connected -------------------------------------------------
// The run rule of unionfind.h (run_label_init / run_label_merge); workgroup (c, y) covers pixels 256 c .. 256 c + 255 of row y.
__device__ __forceinline__ bool holes_zero(int32_t l) { return l <= 0; }

__global__ void __launch_bounds__(256) k_holes_init(const int32_t *__restrict__ segm, int32_t *__restrict__ parent, int W)
{
    run_label_init(segm, parent, blockIdx.y, blockIdx.x * 256 + threadIdx.x, W, holes_zero);
}

__global__ void __launch_bounds__(256) k_holes_merge(const int32_t *__restrict__ segm, int32_t *parent, int W)
{
    run_label_merge(segm, parent, blockIdx.y, blockIdx.x * 256 + threadIdx.x, W, holes_zero);
}

// the border pixels, one lane each: top row, bottom row, left column, right column
__global__ void __launch_bounds__(256)
k_holes_touch(const int32_t *__restrict__ segm, const int32_t *__restrict__ parent, int H, int W, uint8_t *touches)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= 2 * W + 2 * H) return;
    int y, x;
    if (t < W) {
        y = 0, x = t;
    } else if (t < 2 * W) {
        y = H - 1, x = t - W;
    } else if (t < 2 * W + H) {
        y = t - 2 * W, x = 0;
    } else {
        y = t - 2 * W - H, x = W - 1;
    }
    const int p = y * W + x;
    if (segm[p] <= 0) touches[uf_find(parent, p)] = 1;
}

__global__ void __launch_bounds__(256)
k_holes_write(const int32_t *__restrict__ segm, const int32_t *__restrict__ parent, const uint8_t *__restrict__ touches, int n,
              uint8_t *__restrict__ seg_bg, uint8_t *__restrict__ seg_fg)
{
    const unsigned int p = blockIdx.x * 256u + threadIdx.x;
    if (p >= (unsigned int)n) return;
    const int l = segm[p];
    seg_bg[p] = l <= 0 ? touches[uf_find(parent, (int)p)] : (uint8_t)0;
    seg_fg[p] = l == 1;
}

// ---- disc erosion / dilation ------------------------------------------------------------------------------------------------
// A workgroup of 256 lanes makes a 64 x 64 tile of the output.  It reads the tile with a halo of r pixels into LDS as "is this a
// pixel the search looks for" (a 0 of the image for the erosion, a 1 for the dilation; outside the image: no), then
//   * run[ty][c] = distance along column c from tile row ty to the nearest such pixel, capped at r + 1: a lane takes a column and 16
//     rows and walks down and up once, r + 16 steps each way, carrying the run length;
//   * a pixel has one within the disc when run[ty][c + k]^2 + k^2 <= r^2 for some |k| <= r: at most 2 r + 1 bytes of LDS, leaving at
//     the first hit.
// LDS: (64 + 2 r)^2 + 64 (64 + 2 r) bytes: 14 852 at r = 15, 49 152 at r = 64 (DESIGN.md section 4 on the tile and the occupancy).
constexpr int MO_TILE = 64, MO_SEG = 16;
//
// LABELLED: the same tiles for all objects of a label map at once (center_annotation.hip): the mask of a pixel is that of its OWN
// label -- bit `level` of the code byte for the erosion, the eroded byte for the dilation -- and a pixel of another label is
// outside it; the radius of a pixel is radius[label * MORPH_LEVEL_SLOTS + level] <= r, r being the halo of the launch.  One byte of
// LDS per pixel still: bit 0 as above, bit 1 "the label differs from the pixel above", bit 2 "... from the pixel to the left" (both
// inside the image).  A column run ends at a label change -- as a hit for the erosion, as "nothing beyond" for the dilation -- so
// run[ty][c] is the distance to the nearest hit among the pixels of the label of (ty, c); the row search of a pixel stops on
// either side where the label changes, for the erosion with a hit.  The dilation writes level + 1 into `out` where it finds a
// survivor and leaves every other byte as it is: the levels are launched in ascending order, the highest one stays.
template <int TARGET, bool LABELLED> __device__ __forceinline__ int morph_step(int d, int cap, uint8_t here, uint8_t change)
{
    if (here & 1) return 0;
    if (LABELLED && (change & 2)) return TARGET ? cap : 1;
    return min(d + 1, cap);
}

//
// BOXED: the plain tiles for many small planes at once (the clean-up of watershed.hip): plane blockIdx.z + 1 has the height, width
// and pixel offset of its row in ml.boxes (MORPH_BOX_WORDS words per row: first row, first column, height, width, offset) and lies
// at that offset in `in` and `out`; the grid covers the largest plane and a workgroup outside its own plane leaves at once.
template <int TARGET, bool LABELLED, bool BOXED = false>
__global__ void __launch_bounds__(256) k_disc_morph(const uint8_t *__restrict__ in, int H, int W, int r, uint8_t *__restrict__ out,
                                                    MorphLabels ml)
{
    extern __shared__ uint8_t morph_lds[];
    if (BOXED) {
        const int32_t *box = ml.boxes + (size_t)(blockIdx.z + 1) * MORPH_BOX_WORDS;
        H = min(box[2], H);
        W = min(box[3], W);
        if ((int)blockIdx.x * MO_TILE >= W || (int)blockIdx.y * MO_TILE >= H) return;       // (uniform over the workgroup)
        in += box[4];
        out += box[4];
    }
    const int LW = MO_TILE + 2 * r;
    uint8_t *hit = morph_lds;                          // [LW][LW]
    uint8_t *run = morph_lds + LW * LW;                // [MO_TILE][LW]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int x0 = blockIdx.x * MO_TILE - r, y0 = blockIdx.y * MO_TILE - r;
    for (int ly = wave; ly < LW; ly += 4) {
        const int y = y0 + ly;
        const bool iny = y >= 0 && y < H;
        for (int lx = lane; lx < LW; lx += 64) {
            const int x = x0 + lx;
            uint8_t v = 0;
            if (iny && x >= 0 && x < W) {
                const size_t i = (size_t)y * W + x;
                if (LABELLED) {
                    const int l = ml.labels[i];
                    const bool own = l >= 1 && l <= ml.max_label;
                    const bool set = own && (TARGET ? in[i] != 0 : ((in[i] >> ml.level) & 1) != 0);
                    v = (uint8_t)((set == (TARGET != 0) ? 1 : 0) | (y > 0 && ml.labels[i - W] != l ? 2 : 0) |
                                  (x > 0 && ml.labels[i - 1] != l ? 4 : 0));
                } else {
                    v = (in[i] != 0) == (TARGET != 0);
                }
            }
            hit[ly * LW + lx] = v;
        }
    }
    __syncthreads();
    const int cap = r + 1;
    for (int i = threadIdx.x; i < LW * (MO_TILE / MO_SEG); i += 256) {
        const int seg = i / LW, c = i - seg * LW;
        const int t0 = seg * MO_SEG;                   // first tile row of the lane; LDS row of tile row t is t + r
        int d = cap;
        for (int ly = t0; ly < t0 + r + MO_SEG; ++ly) {
            const uint8_t here = hit[ly * LW + c];
            d = morph_step<TARGET, LABELLED>(d, cap, here, here);                       // (the change between ly - 1 and ly sits on ly)
            if (ly >= t0 + r) run[(ly - r) * LW + c] = (uint8_t)d;
        }
        d = cap;
        for (int ly = t0 + MO_SEG - 1 + 2 * r; ly >= t0 + r; --ly) {
            const uint8_t below = LABELLED && ly + 1 < LW ? hit[(ly + 1) * LW + c] : (uint8_t)0;
            d = morph_step<TARGET, LABELLED>(d, cap, hit[ly * LW + c], below);          // (the change between ly and ly + 1 on ly + 1)
            if (ly <= t0 + MO_SEG - 1 + r) run[(ly - r) * LW + c] = (uint8_t)min(d, (int)run[(ly - r) * LW + c]);
        }
    }
    __syncthreads();
    const int x = blockIdx.x * MO_TILE + lane;
    if (x >= W) return;
    for (int ty = wave; ty < MO_TILE; ty += 4) {
        const int y = blockIdx.y * MO_TILE + ty;
        if (y >= H) break;
        const uint8_t *line = run + ty * LW + lane + r;
        bool found = false;
        if (LABELLED) {
            const int l = ml.labels[(size_t)y * W + x];
            const bool own = l >= 1 && l <= ml.max_label;
            if (own) {
                const int rr = min(ml.radius[l * MORPH_LEVEL_SLOTS + ml.level], r), r2 = rr * rr;
                const uint8_t *flags = hit + (ty + r) * LW + lane + r;
                bool left = true, right = true;                // the side has not met another label yet
                found = (int)line[0] * (int)line[0] <= r2;
                for (int k = 1; k <= rr && !found; ++k) {
                    if (left && (flags[1 - k] & 4)) left = false, found = !TARGET;
                    if (right && (flags[k] & 4)) right = false, found = found || !TARGET;
                    const int lim = r2 - k * k, a = line[-k], b = line[k];
                    found = found || (left && a * a <= lim) || (right && b * b <= lim);
                }
            }
            if (TARGET) {
                if (found) out[(size_t)y * W + x] = (uint8_t)(ml.level + 1);
            } else {
                out[(size_t)y * W + x] = own && !found;
            }
        } else {
            const int r2 = r * r;
            for (int k = 0; k <= r && !found; ++k) {
                const int lim = r2 - k * k, a = line[-k], b = line[k];
                found = a * a <= lim || b * b <= lim;
            }
            out[(size_t)y * W + x] = TARGET ? found : !found;
        }
    }
}

// ---- rays of all centres on both masks ----------------------------------------------------------------------------------------
// blockIdx.y = 0: seg_bg with edge 'up', 1: seg_fg with edge 'down'; the walk is ray_walk (raywalk.h).  One wave per
// (position, mask), one lane per angle.
__global__ void __launch_bounds__(64)
k_boundary_rays(const uint8_t *__restrict__ seg_bg, const uint8_t *__restrict__ seg_fg, int H, int W,
                const int32_t *__restrict__ positions, int P, const float *__restrict__ grad, int A, float *__restrict__ rays_bg,
                float *__restrict__ rays_fg)
{
    const int p = blockIdx.x;
    const int edge = blockIdx.y == 0 ? 1 : -1;
    const uint8_t *seg = blockIdx.y == 0 ? seg_bg : seg_fg;
    float *out = blockIdx.y == 0 ? rays_bg : rays_fg;
    if (p >= P || !out) return;
    const int py = positions[2 * p], px = positions[2 * p + 1];
    const bool inside = py >= 0 && py < H && px >= 0 && px < W;
    auto on_mask = [&](int y, int x) -> bool { return seg[(size_t)y * W + x] != 0; };
    const bool start = inside ? on_mask(py, px) : false;
    const int diag = ray_walk_limit(H, W);
    for (int a = threadIdx.x; a < A; a += blockDim.x)
        out[(size_t)p * A + a] = ray_walk(py, px, inside, start, grad[2 * a], grad[2 * a + 1], H, W, diag, edge, on_mask);
}

int morph_size_ok(int H, int W)
{
    if (H > 65535 || (size_t)H * (size_t)W >= ((size_t)1 << 31)) {
        set_error("morphology: more than 65535 rows or 2^31 pixels");
        return 0;
    }
    return 1;
}

int launch_fill_holes_split(const int32_t *segm, int H, int W, int32_t *parent, uint8_t *touches, uint8_t *seg_bg, uint8_t *seg_fg,
                            hipStream_t st)
{
    const int n = H * W;
    const dim3 rows(cdiv(W, 256), H);
    HIP_TRY(hipMemsetAsync(touches, 0, (size_t)n, st));
    hipLaunchKernelGGL(k_holes_init, rows, 256, 0, st, segm, parent, W);
    hipLaunchKernelGGL(k_holes_merge, rows, 256, 0, st, segm, parent, W);
    hipLaunchKernelGGL(k_holes_touch, cdiv(2L * W + 2L * H, 256), 256, 0, st, segm, parent, H, W, touches);
    hipLaunchKernelGGL(k_holes_write, cdiv(n, 256), 256, 0, st, segm, parent, touches, n, seg_bg, seg_fg);
    HIP_TRY(hipGetLastError());
    return 0;
}

int launch_disc_morph_boxed(const uint8_t *in, int H, int W, int r, int dilate, uint8_t *out, const int32_t *boxes, int n_boxes,
                            hipStream_t st)
{
    if (r < 1 || r > MORPH_MAX_RADIUS || n_boxes < 1 || n_boxes > 65535) {
        set_error("disc morphology: the radius must lie in [1, IMSEGM_MORPH_MAX_RADIUS] and the planes number 1 .. 65535");
        return -1;
    }
    const int LW = MO_TILE + 2 * r;
    const size_t lds = (size_t)LW * LW + (size_t)MO_TILE * LW;
    const dim3 grid(cdiv(W, MO_TILE), cdiv(H, MO_TILE), n_boxes);
    MorphLabels ml;
    ml.boxes = boxes;
    if (dilate)
        hipLaunchKernelGGL((k_disc_morph<1, false, true>), grid, 256, lds, st, in, H, W, r, out, ml);
    else
        hipLaunchKernelGGL((k_disc_morph<0, false, true>), grid, 256, lds, st, in, H, W, r, out, ml);
    HIP_TRY(hipGetLastError());
    return 0;
}

int launch_disc_morph(const uint8_t *in, int H, int W, int r, int dilate, uint8_t *out, hipStream_t st)
{
    if (r < 1 || r > MORPH_MAX_RADIUS) {
        set_error("disc morphology: the radius must lie in [1, IMSEGM_MORPH_MAX_RADIUS]");
        return -1;
    }
    const int LW = MO_TILE + 2 * r;
    const size_t lds = (size_t)LW * LW + (size_t)MO_TILE * LW;
    const dim3 grid(cdiv(W, MO_TILE), cdiv(H, MO_TILE));
    if (dilate)
        hipLaunchKernelGGL((k_disc_morph<1, false>), grid, 256, lds, st, in, H, W, r, out, MorphLabels());
    else
        hipLaunchKernelGGL((k_disc_morph<0, false>), grid, 256, lds, st, in, H, W, r, out, MorphLabels());
    HIP_TRY(hipGetLastError());
    return 0;
}

int launch_disc_morph_labelled(const uint8_t *in, int H, int W, int r, int dilate, uint8_t *out, const MorphLabels &ml, hipStream_t st)
{
    if (r < 0 || r > MORPH_MAX_RADIUS || !ml.labels || !ml.radius || ml.level < 0 || ml.level >= MORPH_LEVEL_SLOTS || ml.max_label < 1) {
        set_error("disc morphology of a label map: a halo outside [0, IMSEGM_MORPH_MAX_RADIUS] or no tables");
        return -1;
    }
    const int LW = MO_TILE + 2 * r;
    const size_t lds = (size_t)LW * LW + (size_t)MO_TILE * LW;
    const dim3 grid(cdiv(W, MO_TILE), cdiv(H, MO_TILE));
    if (dilate)
        hipLaunchKernelGGL((k_disc_morph<1, true>), grid, 256, lds, st, in, H, W, r, out, ml);
    else
        hipLaunchKernelGGL((k_disc_morph<0, true>), grid, 256, lds, st, in, H, W, r, out, ml);
    HIP_TRY(hipGetLastError());
    return 0;
}

int launch_boundary_rays(const uint8_t *seg_bg, const uint8_t *seg_fg, int H, int W, const int32_t *positions, int P, const float *grad,
                         int A, float *rays_bg, float *rays_fg, hipStream_t st)
{
    if (P > 0 && (rays_bg || rays_fg))
        hipLaunchKernelGGL(k_boundary_rays, dim3(P, 2), 64, 0, st, seg_bg, seg_fg, H, W, positions, P, grad, A, rays_bg, rays_fg);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // namespace imsegm
