// volume.hip -- 3-D gray supervoxel path (BASELINE config 5).
//
// Replaces, for D x H x W gray volumes:
//   skimage.segmentation.slic(im, n_segments, compactness, multichannel=False, spacing=space, sigma=1)
//       as called at /root/reference/imsegm/superpixels.py:104-106   (no Lab, anisotropic spacing)
// (skimage.measure.label of the supervoxel map, superpixels.py:111: label_cc.hip; the graph and the centres of the supervoxels,
// superpixels.py:180-242: volume_graph.hip)
// Arithmetic contract of the assignment: identical to oracle orc_slic_iterate (fp64, operation order
// of _slic.pyx with spacing):  d = ((sz*(cz-z))^2 + (sy*(cy-y))^2 + (sx*(cx-x))^2) * (1/step^2) + (v - cv)^2.
//
// Candidate search: the centroids enter their index into the lists of the 64 x 16 x 16 bricks their search window meets
// (k_vol_scatter); an assignment workgroup -- one brick cross-section -- reads the list of its brick only.  Sized for the
// 10^9 voxels / 3 * 10^5 supervoxels of config 5; a float32 volume runs in float32 from end to end, as scikit-image 0.18 does.
#include "slic.h"
#include <hip/hip_ext.h>

namespace imsegm {

__device__ __forceinline__ int vreflect(int i, int n)
{
    if (n == 1) return 0;
    int p = 2 * n;
    i %= p;
    if (i < 0) i += p;
    if (i >= n) i = p - 1 - i;
    return i;
}

template <typename T>
__global__ void __launch_bounds__(256)
k_vol_to_f64(const T *__restrict__ src, size_t n, double off, double scale, double *__restrict__ dst)
{
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    // skimage.img_as_float as an affine map: (v + off) * scale   (uint8: off 0, scale 1 / 255)
    if (i < n) dst[i] = ((double)src[i] + off) * scale;
}

// one scipy correlate1d pass (symmetric taps, 'reflect') along z (0), y (1) or x (2); optional final scale
template <int AXIS>
__global__ void __launch_bounds__(256)
k_vol_blur(const double *__restrict__ src, double *__restrict__ dst, int D, int H, int W, Taps t, double ratio, int scale)
{
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    size_t n = (size_t)D * H * W;
    if (i >= n) return;
    int x = (int)(i % W), y = (int)((i / W) % H), z = (int)(i / ((size_t)W * H));
    double v;
    if (t.r < 0) {
        v = src[i];
    } else {
        v = src[i] * t.w[0];
        for (int j = t.r; j >= 1; --j) {
            size_t a, b;
            if (AXIS == 0) {
                a = ((size_t)vreflect(z - j, D) * H + y) * W + x;
                b = ((size_t)vreflect(z + j, D) * H + y) * W + x;
            } else if (AXIS == 1) {
                a = ((size_t)z * H + vreflect(y - j, H)) * W + x;
                b = ((size_t)z * H + vreflect(y + j, H)) * W + x;
            } else {
                a = ((size_t)z * H + y) * W + vreflect(x - j, W);
                b = ((size_t)z * H + y) * W + vreflect(x + j, W);
            }
            v += (src[a] + src[b]) * t.w[j];
        }
    }
    if (scale) v = v * ratio;
    dst[i] = v;
}

int launch_vol_preprocess(const void *src, int dtype, double off, double scale, int D, int H, int W, const Taps &tz, const Taps &ty,
                          const Taps &tx, double ratio, double *bufA, double *bufB, hipStream_t st)
{
    size_t n = (size_t)D * H * W;
    int grid = cdiv((long)n, 256);
    if (dtype == DT_U8) hipLaunchKernelGGL(k_vol_to_f64<uint8_t>, grid, 256, 0, st, (const uint8_t *)src, n, off, scale, bufA);
    else if (dtype == DT_F32) hipLaunchKernelGGL(k_vol_to_f64<float>, grid, 256, 0, st, (const float *)src, n, off, scale, bufA);
    else hipLaunchKernelGGL(k_vol_to_f64<double>, grid, 256, 0, st, (const double *)src, n, off, scale, bufA);
    hipLaunchKernelGGL(k_vol_blur<0>, grid, 256, 0, st, bufA, bufB, D, H, W, tz, ratio, 0);
    hipLaunchKernelGGL(k_vol_blur<1>, grid, 256, 0, st, bufB, bufA, D, H, W, ty, ratio, 0);
    hipLaunchKernelGGL(k_vol_blur<2>, grid, 256, 0, st, bufA, bufB, D, H, W, tx, ratio, 1);
    HIP_TRY(hipGetLastError());
    return 0;   // result in bufB
}

// ---- centroid table ----------------------------------------------------------------------------------
__device__ __forceinline__ void vol_window(const VolState &s, double cz, double cy, double cx, int *w)
{
    double a;
    a = cz - (double)(2 * s.step_z); w[0] = (int)(a > 0 ? a : 0.0);
    a = cz + (double)(2 * s.step_z); a = a + 1.0; w[1] = (int)(a < (double)s.D ? a : (double)s.D);
    a = cy - (double)(2 * s.step_y); w[2] = (int)(a > 0 ? a : 0.0);
    a = cy + (double)(2 * s.step_y); a = a + 1.0; w[3] = (int)(a < (double)s.H ? a : (double)s.H);
    a = cx - (double)(2 * s.step_x); w[4] = (int)(a > 0 ? a : 0.0);
    a = cx + (double)(2 * s.step_x); a = a + 1.0; w[5] = (int)(a < (double)s.W ? a : (double)s.W);
}

__global__ void k_vol_centroid_init(VolState s)
{
    int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= s.K) return;
    int ix = k % s.grid_n[2], iy = (k / s.grid_n[2]) % s.grid_n[1], iz = k / (s.grid_n[2] * s.grid_n[1]);
    double cz = (double)(s.grid_0[0] + iz * s.grid_d[0]);
    double cy = (double)(s.grid_0[1] + iy * s.grid_d[1]);
    double cx = (double)(s.grid_0[2] + ix * s.grid_d[2]);
    s.cen[(size_t)k * 4 + 0] = cz;
    s.cen[(size_t)k * 4 + 1] = cy;
    s.cen[(size_t)k * 4 + 2] = cx;
    s.cen[(size_t)k * 4 + 3] = 0.0;
    vol_window(s, cz, cy, cx, s.win + (size_t)k * 6);
    for (int j = 0; j < 6; ++j) s.acc[(size_t)k * 6 + j] = 0;
}

__global__ void k_vol_centroid_finalize(VolState s)
{
    int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= s.K) return;
    long long *a = s.acc + (size_t)k * 6;
    long long n = a[0];
    int *w = s.win + (size_t)k * 6;
    if (n == 0) {
        for (int j = 0; j < 6; ++j) w[j] = 0;
    } else {
        double nn = (double)n;
        double cz = i64_to_double(a[1]) / nn, cy = i64_to_double(a[2]) / nn, cx = i64_to_double(a[3]) / nn;
        s.cen[(size_t)k * 4 + 0] = cz;
        s.cen[(size_t)k * 4 + 1] = cy;
        s.cen[(size_t)k * 4 + 2] = cx;
        s.cen[(size_t)k * 4 + 3] = fix_value(a[4], a[5], ldexp(1.0, -fix_bits_of(*s.premax))) / nn;
        vol_window(s, cz, cy, cx, w);
    }
    for (int j = 0; j < 6; ++j) a[j] = 0;
}

// every centroid appends itself to the list of each brick its search window meets (order irrelevant: the
// assignment breaks ties on the centroid index explicitly)
__global__ void __launch_bounds__(256) k_vol_scatter(VolState s)
{
    int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= s.K) return;
    const int *w = s.win + (size_t)k * 6;
    if (w[1] <= w[0] || w[3] <= w[2] || w[5] <= w[4]) return;       // dead centroid: empty window
    const int bz0 = w[0] / VOL_BZ, bz1 = (w[1] - 1) / VOL_BZ;
    const int by0 = w[2] / VOL_BY, by1 = (w[3] - 1) / VOL_BY;
    const int bx0 = w[4] / VOL_BX, bx1 = (w[5] - 1) / VOL_BX;
    for (int bz = bz0; bz <= bz1; ++bz)
        for (int by = by0; by <= by1; ++by)
            for (int bx = bx0; bx <= bx1; ++bx) {
                const int b = (bz * s.nby + by) * s.nbx + bx;
                const int pos = atomicAdd(&s.brick_count[b], 1);
                if (pos < s.brick_cap) s.brick_list[(size_t)b * s.brick_cap + pos] = k;
            }
}

// ---- assignment -----------------------------------------------------------------------------------------
// One wave = 64 consecutive x, VROWS rows of one z slice; a workgroup = four such strips = the cross-section of a brick.
// The workgroup scans the candidate list of its brick (or, if that list overflowed, the whole centroid table) once,
// keeps the windows that meet the cross-section in an LDS list (ballot compaction), and every wave evaluates the
// list for its strip; equal distances go to the lower centroid index, which is what the ascending scan with a
// strict '>' of _slic.pyx yields (the order of evaluation is free: the comparison carries the index).
constexpr int VROWS = 4;

// (round 3: like the float32 kernel below -- the four waves of a workgroup scan the brick's list once, together, stage the records of
// the windows that meet the 64 x 16 cross-section in LDS, and each wave walks them in ascending order of their lower bound over
// its strip, stopping at the first bound above the worst best distance of the strip)
struct VolRec64 {
    double cz, cy, cx, cv;
    int wy0, wy1, wx0, wx1;
};
constexpr int VLIST64 = 512;

template <bool ACCUM>
__global__ void __launch_bounds__(256)
k_vol_assign(VolState s, const double *__restrict__ vol, int32_t *__restrict__ labels)
{
    __shared__ int list[VLIST64];
    __shared__ VolRec64 rec[VLIST64];
    __shared__ int wave_base[4];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int rows_per_block = 4 * VROWS;
    const int yb = cdiv(s.H, rows_per_block);
    const int z = blockIdx.y / yb;
    const int Y0 = (blockIdx.y % yb) * rows_per_block, Y1 = min(Y0 + rows_per_block, s.H);
    const int y0 = Y0 + wave * VROWS;
    const int x = blockIdx.x * 64 + lane;
    const int x0w = blockIdx.x * 64, x1w = min(x0w + 64, s.W);
    const bool alive = y0 < s.H;                              // (a wave below the volume takes part in the barriers only)
    const int y1w = min(y0 + VROWS, s.H);
    const bool xin = x < s.W;
    double pv[VROWS], best_d[VROWS];
    int best_k[VROWS];
#pragma unroll
    for (int r = 0; r < VROWS; ++r) {
        bool ok = alive && xin && (y0 + r) < s.H;
        pv[r] = vol[ok ? ((size_t)z * s.H + y0 + r) * s.W + x : 0];
        best_d[r] = DBL_MAX;
        best_k[r] = -1;
    }
    const double fz = (double)z, fx = (double)x;
    int count = 0;                                         // (uniform over the workgroup)
    double wave_worst = DBL_MAX;          // >= the current best distance of every voxel of this wave
    static_assert(VOL_BX == 64 && VOL_BY == 4 * VROWS, "a workgroup lies inside one brick");
    const int brick = ((z / VOL_BZ) * s.nby + (Y0 / VOL_BY)) * s.nbx + blockIdx.x;
    const int bcount = s.brick_count[brick];
    const bool whole = bcount > s.brick_cap;                   // list overflow: scan every centroid
    const int *__restrict__ blist = s.brick_list + (size_t)brick * s.brick_cap;
    const int nscan = whole ? s.K : bcount;
    const int nblk = cdiv(nscan, 256);
    constexpr int PER = VLIST64 / 64;
    for (int b = 0; b < nblk; ++b) {
        const int i = b * 256 + tid;
        int k = 0;
        bool hit = false;
        if (i < nscan) {
            k = whole ? i : blist[i];
            const int *w = s.win + (size_t)k * 6;
            hit = z >= w[0] && z < w[1] && w[2] < Y1 && w[3] > Y0 && w[4] < x1w && w[5] > x0w;
        }
        const unsigned long long m = __ballot(hit);
        if (lane == 0) wave_base[wave] = __popcll(m);
        __syncthreads();
        int base = count;
        for (int w2 = 0; w2 < wave; ++w2) base += wave_base[w2];
        const int added = wave_base[0] + wave_base[1] + wave_base[2] + wave_base[3];
        if (hit) list[base + __popcll(m & ((1ULL << lane) - 1ULL))] = k;
        count += added;
        __syncthreads();
        if (count <= VLIST64 - 256 && b + 1 < nblk) continue;
        for (int c = tid; c < count; c += 256) {
            const int ck = list[c];
            const int *w = s.win + (size_t)ck * 6;
            VolRec64 rc;
            rc.cz = s.cen[(size_t)ck * 4]; rc.cy = s.cen[(size_t)ck * 4 + 1]; rc.cx = s.cen[(size_t)ck * 4 + 2];
            rc.cv = s.cen[(size_t)ck * 4 + 3];
            rc.wy0 = w[2]; rc.wy1 = w[3]; rc.wx0 = w[4]; rc.wx1 = w[5];
            rec[c] = rc;
        }
        __syncthreads();
        if (alive) {
            // Exact pruning: the spatial part of the distance to the nearest point of the strip is a lower bound of the
            // distance of every voxel of the strip (every operation is monotone in IEEE arithmetic and the colour term
            // is >= 0); a candidate whose bound exceeds the worst current best of the wave can neither win nor tie.
            double lbl[PER];
#pragma unroll
            for (int j = 0; j < PER; ++j) {
                const int c = lane + 64 * j;
                lbl[j] = DBL_MAX;
                if (c < count) {
                    const VolRec64 rc = rec[c];
                    if (rc.wy0 < y1w && rc.wy1 > y0) {
                        const double tz = s.sz * (rc.cz - fz);
                        const double dz = tz * tz;
                        const double yn = fmin(fmax(rc.cy, (double)y0), (double)(y1w - 1));
                        const double xn = fmin(fmax(rc.cx, (double)x0w), (double)(x1w - 1));
                        const double tyl = s.sy * (rc.cy - yn), txl = s.sx * (rc.cx - xn);
                        lbl[j] = (dz + tyl * tyl + txl * txl) * s.spatial_weight;
                    }
                }
            }
            int since_refresh = 0;
            while (true) {
                double mine = lbl[0];
#pragma unroll
                for (int j = 1; j < PER; ++j) mine = fmin(mine, lbl[j]);
                const double wm = wave_min_f64(mine);
                if (!(wm <= wave_worst) || wm == DBL_MAX) break;   // (DBL_MAX: nothing left in the batch)
                const unsigned long long own = __ballot(mine == wm);
                const int src = __ffsll((long long)own) - 1;
                int jsel = 0;
#pragma unroll
                for (int j = PER - 1; j >= 0; --j)
                    if (lbl[j] == wm) jsel = j;
                jsel = __builtin_amdgcn_readlane(jsel, src);
#pragma unroll
                for (int j = 0; j < PER; ++j)
                    if (lane == src && j == jsel) lbl[j] = DBL_MAX;
                const int c = src + 64 * jsel;
                const int ck = list[c];
                const VolRec64 rc = rec[c];
                const double tz = s.sz * (rc.cz - fz);
                const double dz = tz * tz;
                const bool inx = x >= rc.wx0 && x < rc.wx1;
                const double tx = s.sx * (rc.cx - fx);
                const double dx2 = tx * tx;
#pragma unroll
                for (int r = 0; r < VROWS; ++r) {
                    const int y = y0 + r;
                    if (y < rc.wy0 || y >= rc.wy1) continue;
                    const double ty = s.sy * (rc.cy - (double)y);
                    const double dy = ty * ty;
                    double d = (dz + dy + dx2) * s.spatial_weight;
                    const double t = pv[r] - rc.cv;
                    d = d + t * t;
                    const bool take = inx && (best_d[r] > d || (best_d[r] == d && ck < best_k[r]));
                    best_d[r] = take ? d : best_d[r];               // (selects, no change of the exec mask)
                    best_k[r] = take ? ck : best_k[r];
                }
                if (++since_refresh == 2) {                    // refresh the bound
                    since_refresh = 0;
                    double m2 = 0.0;
#pragma unroll
                    for (int r = 0; r < VROWS; ++r)
                        if (xin && (y0 + r) < s.H) m2 = fmax(m2, best_d[r]);
                    wave_worst = wave_max_f64(m2);
                }
            }
        }
        count = 0;
        __syncthreads();
    }
    if (!alive) return;
    // labels (an uncovered voxel keeps its previous assignment) + accumulation
    unsigned pending = 0;
#pragma unroll
    for (int r = 0; r < VROWS; ++r) {
        if (!(xin && (y0 + r) < s.H)) continue;
        size_t p = ((size_t)z * s.H + y0 + r) * s.W + x;
        if (best_k[r] >= 0) labels[p] = best_k[r];
        else best_k[r] = labels[p];
        if (best_k[r] >= 0) pending |= 1u << r;
    }
    if (!ACCUM) return;
    const double fscale = ldexp(1.0, fix_bits_of(*s.premax));
    while (true) {
        int first = -1;
#pragma unroll
        for (int r = VROWS - 1; r >= 0; --r)
            if (pending & (1u << r)) first = best_k[r];
        unsigned long long vote = __ballot(first >= 0);
        if (!vote) break;
        const int k = __shfl(first, __ffsll((long long)vote) - 1, 64);
        long long q[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };
#pragma unroll
        for (int r = 0; r < VROWS; ++r) {
            if ((pending & (1u << r)) && best_k[r] == k) {
                const long long t = (long long)trunc(pv[r] * fscale);     // two limbs of the global sum: t = hi * 2^24 + lo
                q[0] += 1; q[1] += z; q[2] += y0 + r; q[3] += x; q[4] += t >> 24; q[5] += t & 0xffffff;
                pending &= ~(1u << r);
            }
        }
        long long tot = wave_reduce8_i64(q);
        if ((lane & 7) == 0 && (lane >> 3) < 6 && tot != 0) atomic_add_i64(s.acc + (size_t)k * 6 + (lane >> 3), tot);
    }
}

int launch_vol_slic(VolState s, const double *vol, int32_t *labels, int max_iter, hipStream_t st)
{
    size_t n = (size_t)s.D * s.H * s.W;
    HIP_TRY(hipMemsetAsync(labels, 0xff, n * sizeof(int32_t), st));
    hipLaunchKernelGGL(k_vol_centroid_init, cdiv(s.K, 256), 256, 0, st, s);
    dim3 grid(cdiv(s.W, 64), cdiv(s.H, 4 * VROWS) * s.D);
    const size_t n_bricks = (size_t)s.nbz * s.nby * s.nbx;
    for (int it = 0; it < max_iter; ++it) {
        HIP_TRY(hipMemsetAsync(s.brick_count, 0, n_bricks * sizeof(int), st));
        hipLaunchKernelGGL(k_vol_scatter, cdiv(s.K, 256), 256, 0, st, s);
        if (it + 1 < max_iter) {
            hipLaunchKernelGGL(k_vol_assign<true>, grid, 256, 0, st, s, vol, labels);
            hipLaunchKernelGGL(k_vol_centroid_finalize, cdiv(s.K, 256), 256, 0, st, s);
        } else {
            hipLaunchKernelGGL(k_vol_assign<false>, grid, 256, 0, st, s, vol, labels);
        }
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

// ---- float32 volumes: scikit-image 0.18 keeps a float32 input in float32 from end to end ---------------------
// (slic_superpixels.py `dtype = image.dtype` -> `_slic_cython[float32]`; oracle: orc_slic_gray3d_f32).  What that
// means for the arithmetic, all of it reproduced here:
//   * the Gaussian filter computes every line in double and stores float32 after every axis pass;
//   * `image * ratio` is a float32 product;
//   * centroids, spacing, the distance  ((dz + dy) + dx) * (1/step^2) + (v - cv)^2  and the search windows are float32;
//   * the centroid update adds the members of a segment in RASTER ORDER into float32 running sums -- not
//     associative, so no parallel reduction reproduces it.  Here one wave owns one centroid: it walks the
//     bounding box of the segment's voxels (tracked by the assignment kernel with integer atomics) in raster
//     order, 64 voxels per load, and folds the member lanes one by one (ballot bits -> v_readlane) into four
//     float32 accumulators kept in lanes 0..3 (z, y, x, value): the additions happen in exactly the order of the
//     sequential loop of _slic.pyx.
template <int AXIS>
__global__ void __launch_bounds__(256)
k_vol_blur_r32(const float *__restrict__ src, float *__restrict__ dst32, int D, int H, int W, Taps t, float fratio, int last)
{
    // (round 5: the values between two axis passes ARE float32 -- scipy stores every line in the output dtype -- so they are kept
    // as float32, not as doubles that hold float32 values: half the bytes per pass, and the float32 input is read as it is)
    // (grid: x blocks of a row, y, z -- no 64-bit division to find the voxel)
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y, z = blockIdx.z;
    if (x >= W) return;
    const size_t i = ((size_t)z * H + y) * W + x;
    double v;
    if (t.r < 0) {
        v = (double)src[i];                               // axis not filtered: the float32 value passes through
    } else {
        v = (double)src[i] * t.w[0];
        const int pos = AXIS == 0 ? z : AXIS == 1 ? y : x, len = AXIS == 0 ? D : AXIS == 1 ? H : W;
        if (pos - t.r >= 0 && pos + t.r < len) {
            // inside the volume along this axis (all but 2 r positions per line): the taps are i -/+ j * stride, no reflected
            // index, no 64-bit multiply per tap -- the same additions in the same order
            const size_t stride = AXIS == 0 ? (size_t)H * W : AXIS == 1 ? (size_t)W : 1;
            for (int j = t.r; j >= 1; --j) v += ((double)src[i - j * stride] + (double)src[i + j * stride]) * t.w[j];
        } else
        for (int j = t.r; j >= 1; --j) {
            size_t a, b;
            if (AXIS == 0) {
                a = ((size_t)vreflect(z - j, D) * H + y) * W + x;
                b = ((size_t)vreflect(z + j, D) * H + y) * W + x;
            } else if (AXIS == 1) {
                a = ((size_t)z * H + vreflect(y - j, H)) * W + x;
                b = ((size_t)z * H + vreflect(y + j, H)) * W + x;
            } else {
                a = ((size_t)z * H + y) * W + vreflect(x - j, W);
                b = ((size_t)z * H + y) * W + vreflect(x + j, W);
            }
            v += ((double)src[a] + (double)src[b]) * t.w[j];
        }
    }
    const float f = (float)v;                             // scipy stores the line in the output dtype (float32)
    dst32[i] = last ? f * fratio : f;                     // numpy: float32 array * Python float
}

// Round 6: the same three passes with a third of the traffic.  The axis passes above each read and write the whole volume (and the
// z pass fetches every plane nine times from beyond the L2: a plane of config 5 is 64 MB) -- 20.7 ms for 2^30 voxels.
//   * z pass (k_vol_blur_z32): a thread owns a column (four neighbouring columns: one 16-byte load per plane) and walks it along z
//     with the 2 R + 1 planes of its window in registers -- every voxel is read once;
//   * y and x pass together (k_vol_blur_yx32): a 64 x 32 tile of one slice with its halo goes through LDS, the y pass writes the
//     float32 lines scipy would store into a second LDS tile, the x pass reads them from there.
// Same operations in the same order on the same float32 intermediate values as the three passes (tests: both forms, bit for bit).
constexpr int VBLUR_R = 4;                         // largest radius the two kernels take (sigma = 1: radius 4)

template <int R, int VEC>
__global__ void __launch_bounds__(256)
k_vol_blur_z32(const float *__restrict__ src, float *__restrict__ dst, int D, int H, int W, Taps t, int zchunk)
{
    typedef float vec_t __attribute__((ext_vector_type(VEC)));
    const int x = (blockIdx.x * 256 + threadIdx.x) * VEC, y = blockIdx.y;
    const int z0 = blockIdx.z * zchunk, z1 = min(z0 + zchunk, D);
    if (x >= W) return;
    const size_t plane = (size_t)H * W, col = (size_t)y * W + x;
    auto load = [&](int z) { return *reinterpret_cast<const vec_t *>(src + (size_t)vreflect(z, D) * plane + col); };
    vec_t win[2 * R + 1];
#pragma unroll
    for (int j = 0; j <= 2 * R; ++j) win[j] = load(z0 - R + j);
    vec_t ahead = load(z0 + R + 1);                   // the plane the NEXT step needs, requested a step early
    for (int z = z0; z < z1; ++z) {
        vec_t out;
#pragma unroll
        for (int c = 0; c < VEC; ++c) {
            double v = (double)win[R][c] * t.w[0];
#pragma unroll
            for (int j = R; j >= 1; --j) v += ((double)win[R - j][c] + (double)win[R + j][c]) * t.w[j];
            out[c] = (float)v;                       // scipy stores the line in the output dtype (float32)
        }
        *reinterpret_cast<vec_t *>(dst + (size_t)z * plane + col) = out;
#pragma unroll
        for (int j = 0; j < 2 * R; ++j) win[j] = win[j + 1];
        win[2 * R] = ahead;
        if (z + 2 < z1) ahead = load(z + R + 2);
    }
}

// (radii known when compiled, a wave = eight rows of the tile: the y pass slides a window of 8 + 2 RY values down a column -- two LDS
// reads per value written where the loop over runtime radii took 2 RY + 1 --, no division for the coordinates: 6.2 -> see
// profiles/README_r06.md at 2^30 voxels.  Same sums in the same order.)
template <int RY, int RX>
__global__ void __launch_bounds__(256)
k_vol_blur_yx32(const float *__restrict__ src, float *__restrict__ dst, int H, int W, Taps ty, Taps tx, float fratio)
{
    constexpr int TW = 64 + 2 * RX, TH = 32 + 2 * RY;
    __shared__ float A[TH][TW];
    __shared__ float B[32][TW];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int X0 = blockIdx.x * 64, Y0 = blockIdx.y * 32;
    const float *__restrict__ sl = src + (size_t)blockIdx.z * H * W;
    const bool extra = lane < 2 * RX;                          // the lanes that also serve the columns 64 .. TW - 1
    const int xa = vreflect(X0 - RX + lane, W), xb = extra ? vreflect(X0 - RX + 64 + lane, W) : 0;
    // (a compile-time trip count: the rows of a wave are requested together and stored as they arrive -- `for (r = wave; r < TH; r += 4)`
    // was a load, a wait and a store per row, ten trips to memory one after the other)
    constexpr int TR = (TH + 3) / 4;
    float a0[TR], a1[TR];
#pragma unroll
    for (int i = 0; i < TR; ++i) {
        const int r = wave + 4 * i;
        const float *__restrict__ row = sl + (size_t)vreflect(Y0 - RY + min(r, TH - 1), H) * W;
        a0[i] = row[xa];
        a1[i] = extra ? row[xb] : 0.f;
    }
#pragma unroll
    for (int i = 0; i < TR; ++i) {
        const int r = wave + 4 * i;
        if (r < TH) {
            A[r][lane] = a0[i];
            if (extra) A[r][64 + lane] = a1[i];
        }
    }
    __syncthreads();
#pragma unroll
    for (int part = 0; part < 2; ++part) {
        if (part == 1 && !extra) break;
        const int c = part ? 64 + lane : lane;
        float win[8 + 2 * RY];
#pragma unroll
        for (int i = 0; i < 8 + 2 * RY; ++i) win[i] = A[8 * wave + i][c];
#pragma unroll
        for (int o = 0; o < 8; ++o) {
            double v = (double)win[o + RY] * ty.w[0];
#pragma unroll
            for (int j = RY; j >= 1; --j) v += ((double)win[o + RY - j] + (double)win[o + RY + j]) * ty.w[j];
            B[8 * wave + o][c] = (float)v;                     // scipy stores the line in the output dtype (float32)
        }
    }
    __syncthreads();
    float *__restrict__ out = dst + (size_t)blockIdx.z * H * W;
    if (X0 + lane >= W) return;
#pragma unroll
    for (int o = 0; o < 8; ++o) {
        const int yy = 8 * wave + o;
        if (Y0 + yy >= H) break;
        double v = (double)B[yy][lane + RX] * tx.w[0];
#pragma unroll
        for (int j = RX; j >= 1; --j) v += ((double)B[yy][lane + RX - j] + (double)B[yy][lane + RX + j]) * tx.w[j];
        out[(size_t)(Y0 + yy) * W + X0 + lane] = (float)v * fratio;      // numpy: float32 array * Python float
    }
}

template <int RY>
static void launch_blur_yx32(int rx, dim3 grid, hipStream_t st, const float *src, float *dst, int H, int W, const Taps &ty, const Taps &tx,
                             float fratio)
{
    switch (rx) {
    case 0: hipLaunchKernelGGL((k_vol_blur_yx32<RY, 0>), grid, 256, 0, st, src, dst, H, W, ty, tx, fratio); break;
    case 1: hipLaunchKernelGGL((k_vol_blur_yx32<RY, 1>), grid, 256, 0, st, src, dst, H, W, ty, tx, fratio); break;
    case 2: hipLaunchKernelGGL((k_vol_blur_yx32<RY, 2>), grid, 256, 0, st, src, dst, H, W, ty, tx, fratio); break;
    case 3: hipLaunchKernelGGL((k_vol_blur_yx32<RY, 3>), grid, 256, 0, st, src, dst, H, W, ty, tx, fratio); break;
    default: hipLaunchKernelGGL((k_vol_blur_yx32<RY, 4>), grid, 256, 0, st, src, dst, H, W, ty, tx, fratio); break;
    }
}

template <int VEC>
static void launch_blur_z32(int R, dim3 grid, hipStream_t st, const float *src, float *dst, int D, int H, int W, const Taps &t, int zchunk)
{
    switch (R) {
    case 0: hipLaunchKernelGGL((k_vol_blur_z32<0, VEC>), grid, 256, 0, st, src, dst, D, H, W, t, zchunk); break;
    case 1: hipLaunchKernelGGL((k_vol_blur_z32<1, VEC>), grid, 256, 0, st, src, dst, D, H, W, t, zchunk); break;
    case 2: hipLaunchKernelGGL((k_vol_blur_z32<2, VEC>), grid, 256, 0, st, src, dst, D, H, W, t, zchunk); break;
    case 3: hipLaunchKernelGGL((k_vol_blur_z32<3, VEC>), grid, 256, 0, st, src, dst, D, H, W, t, zchunk); break;
    default: hipLaunchKernelGGL((k_vol_blur_z32<4, VEC>), grid, 256, 0, st, src, dst, D, H, W, t, zchunk); break;
    }
}

int launch_vol_preprocess_f32(const float *src, int D, int H, int W, const Taps &tz, const Taps &ty, const Taps &tx, double ratio,
                              double *bufA, double *bufB, hipStream_t st)
{
    float *a32 = reinterpret_cast<float *>(bufA), *b32 = reinterpret_cast<float *>(bufB);
    if (H > 65535 || D > 65535) {
        set_error("volume pre-processing: more than 65 535 rows or slices");
        return -1;
    }
    if (tz.r <= VBLUR_R && ty.r <= VBLUR_R && tx.r <= VBLUR_R && !knobs().pre_3pass) {
        // an axis that is not filtered (radius < 0) passes its values through: the single tap 1.0 (x * 1.0 == x, (float)(double)x == x)
        auto eff = [](const Taps &t) {
            Taps e = t;
            if (e.r < 0) {
                e.r = 0;
                e.w[0] = 1.0;
            }
            return e;
        };
        const float *mid = src;
        if (tz.r >= 0) {
            const int vec = (W % 4 == 0 && (reinterpret_cast<uintptr_t>(src) & 15) == 0) ? 4 : 1;
            // enough columns to fill the device, else the z range in chunks (each re-reads the 2 R planes around it)
            const long columns = (long)cdiv(W, vec) * H;
            int chunks = (int)std::min<long>(std::max<long>(1, (long)(16384L * 64 / std::max<long>(columns, 1))), std::max(1, D / 16));
            const int zchunk = cdiv(D, chunks);
            const dim3 grid(cdiv(cdiv(W, vec), 256), H, cdiv(D, zchunk));
            if (vec == 4) launch_blur_z32<4>(tz.r, grid, st, src, a32, D, H, W, tz, zchunk);
            else launch_blur_z32<1>(tz.r, grid, st, src, a32, D, H, W, tz, zchunk);
            mid = a32;
        }
        const dim3 tiles(cdiv(W, 64), cdiv(H, 32), D);
        const Taps ey = eff(ty), ex = eff(tx);
        switch (ey.r) {
        case 0: launch_blur_yx32<0>(ex.r, tiles, st, mid, b32, H, W, ey, ex, (float)ratio); break;
        case 1: launch_blur_yx32<1>(ex.r, tiles, st, mid, b32, H, W, ey, ex, (float)ratio); break;
        case 2: launch_blur_yx32<2>(ex.r, tiles, st, mid, b32, H, W, ey, ex, (float)ratio); break;
        case 3: launch_blur_yx32<3>(ex.r, tiles, st, mid, b32, H, W, ey, ex, (float)ratio); break;
        default: launch_blur_yx32<4>(ex.r, tiles, st, mid, b32, H, W, ey, ex, (float)ratio); break;
        }
        HIP_TRY(hipGetLastError());
        return 0;   // float32 result in bufB
    }
    const dim3 rows(cdiv(W, 256), H, D);
    hipLaunchKernelGGL(k_vol_blur_r32<0>, rows, 256, 0, st, src, b32, D, H, W, tz, 0.f, 0);
    hipLaunchKernelGGL(k_vol_blur_r32<1>, rows, 256, 0, st, (const float *)b32, a32, D, H, W, ty, 0.f, 0);
    hipLaunchKernelGGL(k_vol_blur_r32<2>, rows, 256, 0, st, (const float *)a32, b32, D, H, W, tx, (float)ratio, 1);
    HIP_TRY(hipGetLastError());
    return 0;   // float32 result in bufB
}

__device__ __forceinline__ void vol_window_f32(const VolState &s, float cz, float cy, float cx, int *w)
{
    // _slic.pyx with float32 centroids: <Py_ssize_t>max(cz - 2 * step_z, 0), <Py_ssize_t>min(cz + 2 * step_z + 1, depth)
    float a;
    a = cz - (float)(2 * s.step_z); w[0] = (int)(a > 0 ? a : 0.f);
    a = cz + (float)(2 * s.step_z); a = a + 1.f; w[1] = (int)(a < (float)s.D ? a : (float)s.D);
    a = cy - (float)(2 * s.step_y); w[2] = (int)(a > 0 ? a : 0.f);
    a = cy + (float)(2 * s.step_y); a = a + 1.f; w[3] = (int)(a < (float)s.H ? a : (float)s.H);
    a = cx - (float)(2 * s.step_x); w[4] = (int)(a > 0 ? a : 0.f);
    a = cx + (float)(2 * s.step_x); a = a + 1.f; w[5] = (int)(a < (float)s.W ? a : (float)s.W);
}

__device__ __forceinline__ void vol_bbox_reset(int *b)
{
    b[0] = b[2] = b[4] = 0x7fffffff;
    b[1] = b[3] = b[5] = -1;
}

__global__ void k_vol_centroid_init_f32(VolState s)
{
    int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= s.K) return;
    int ix = k % s.grid_n[2], iy = (k / s.grid_n[2]) % s.grid_n[1], iz = k / (s.grid_n[2] * s.grid_n[1]);
    float cz = (float)(double)(s.grid_0[0] + iz * s.grid_d[0]);
    float cy = (float)(double)(s.grid_0[1] + iy * s.grid_d[1]);
    float cx = (float)(double)(s.grid_0[2] + ix * s.grid_d[2]);
    s.cen32[(size_t)k * 4 + 0] = cz;
    s.cen32[(size_t)k * 4 + 1] = cy;
    s.cen32[(size_t)k * 4 + 2] = cx;
    s.cen32[(size_t)k * 4 + 3] = 0.f;
    vol_window_f32(s, cz, cy, cx, s.win + (size_t)k * 6);
    vol_bbox_reset(s.bbox + (size_t)k * 6);
}

// Round 3.  (1) The four waves of a workgroup (64 x 16 voxels of one slice = the cross-section of a brick) scan the brick's list
// ONCE, together, and stage the records of the centroids whose window meets the cross-section in LDS; before, every wave scanned
// the whole list (~230 windows of 24 bytes) for itself.  (2) Each wave then walks the staged candidates in ascending order of
// their lower bound over ITS strip (64 x 4) by repeated wave minima, and stops at the first bound above the worst best distance
// of the strip (`wave_worst`): every candidate behind it is at least as far.  ~150 windows meet a strip at sp_size 15, ~30 have a
// bound below the final worst distance; before, the list order decided how many were evaluated in full.  The pruning is exact as
// before: a candidate is skipped only when its bound EXCEEDS what every voxel of the strip already has (float32 operations, all
// monotone; ties go on being evaluated).  (3) The bounding boxes of the segments: the distinct labels of a strip are enumerated
// with ballots (a strip is 4 rows: row masks give the x and y extent), parked one per lane, and the lanes compare with / update
// the boxes in ONE round of loads instead of a serial load-compare-atomic chain per label.
struct VolRec {
    float cz, cy, cx, cv;
    int wy0, wy1, wx0, wx1;
};
constexpr int VLIST32 = 512;          // staged candidates per batch (a batch is walked when fewer than 256 slots are left)

// -DIMSEGM_VOL_PHASE_PROF (tools/build_variant.sh; never in the shipped library): shader-clock ticks per section of the assignment
// kernel, summed over the lane 0 of every wave, + waves and evaluated candidates -> imsegm_debug_vol_phases
#ifdef IMSEGM_VOL_PHASE_PROF
__device__ unsigned long long g_vol_phase[16];
#define VOL_PH_BEGIN unsigned long long ph_t0 = clock64(), ph_t1; int ph_evaluated = 0;
#define VOL_PH(i) do { if (lane == 0) { ph_t1 = clock64(); atomicAdd(&g_vol_phase[i], ph_t1 - ph_t0); ph_t0 = ph_t1; } } while (0)
#define VOL_PH_COUNT(i, v) do { if (lane == 0) atomicAdd(&g_vol_phase[i], (unsigned long long)(v)); } while (0)
#else
#define VOL_PH_BEGIN
#define VOL_PH(i)
#define VOL_PH_COUNT(i, v)
#endif

// Round 6: the walk over one batch of staged candidates, instantiated for the number of list slots a lane really holds (NS =
// ceil(count / 64): ~150 windows meet a cross-section at sp_size 15, i.e. 3 slots, where rounds 3 - 5 always carried the 8 of a full
// list through every minimum, search and clear), and on integer KEYS: the bits of the (non-negative) float32 bound with the slot
// number in their three lowest bits.  The wave minimum of the keys is the next candidate's bound -- rounded down by at most seven
// units in the last place, still a lower bound -- AND its slot: no search for the slot, no second exchange.  Which candidates are
// evaluated can only grow by the rounding; the result does not depend on it (the comparison carries the centroid index).
constexpr int VOL_KEY_INF = 0x7f800000;

__device__ __forceinline__ int wave_min_key(int key)
{
    // keys of real candidates lie in [0, VOL_KEY_INF): as a maximum of VOL_KEY_INF - key, a lane without a source contributes 0
    int x = VOL_KEY_INF - key;
    x = max(x, __builtin_amdgcn_update_dpp(0, x, 0x111, 0xf, 0xf, false));
    x = max(x, __builtin_amdgcn_update_dpp(0, x, 0x112, 0xf, 0xf, false));
    x = max(x, __builtin_amdgcn_update_dpp(0, x, 0x114, 0xf, 0xf, false));
    x = max(x, __builtin_amdgcn_update_dpp(0, x, 0x118, 0xf, 0xf, false));
    x = max(x, __builtin_amdgcn_update_dpp(0, x, 0x142, 0xa, 0xf, false));
    x = max(x, __builtin_amdgcn_update_dpp(0, x, 0x143, 0xc, 0xf, false));
    return VOL_KEY_INF - __builtin_amdgcn_readlane(x, 63);
}

// A workgroup of k_vol_assign_f32 takes the 64 x 16 cross-section of a brick in ONE slice; a lane holds one column of VROWS rows.
// Measured (64 x 4096 x 4096, one box each): 11.4 ms per accumulating sweep; with two consecutive slices per workgroup -- the scan
// of the brick's list, its barriers and the flush of the boxes serving twice the voxels, a candidate selected once for eight rows
// of a lane -- 12.1 ms: 102 registers per lane leave four waves per SIMD where 56 leave eight, and the kernel lives on the waves
// that compute while others wait.
//
// The voxels of a wave inside the cross-section: a 16 x 16 TILE -- lane & 15 in x, rows 4 (lane >> 4) .. + 3 in y.  The walk evaluates
// a candidate for all 256 voxels of the wave; at config 5 a supervoxel is ~35 x 35 voxels of a slice: a 64 x 4 strip (lane in x, four
// rows) met the windows of ~9 centroids whose bound lay below its worst distance, a tile meets ~half of that.  A 32 x 8 tile,
// whose rows are whole 128-byte lines of the label map where the 16 x 16 tile's are half lines, measured 9.93 against 9.38 ms per
// sweep.  Same candidates per VOXEL, same arithmetic, same comparison whatever the shape: the label maps are the same.
constexpr int VT_W = 16, VT_H = 16;
// the neighbour to the left inside the tile's row of voxels (the first lane of a row keeps `first`)
__device__ __forceinline__ int tile_prev(int v, int first) { return __builtin_amdgcn_update_dpp(first, v, 0x111, 0xf, 0xf, false); }      // row_shr:1

template <int NS>
__device__ __forceinline__ void vol_walk_f32(const VolRec *rec, const int *list, int count, int lane, int y0, int y1w, int x0w, int x1w,
                                             int yl, int x, bool xin, int H, bool zin, float fz0, float fx, float sz, float sy, float sx,
                                             float sw, const float (&pv)[VROWS], float (&best_d)[VROWS], int (&best_k)[VROWS],
                                             float &wave_worst)
{
    static_assert(NS >= 1 && NS <= 8, "three bits of a key hold the slot");
    // bounds over this wave's voxels [y0, y1w) x [x0w, x1w); a window that misses them is out.  The bound of a candidate lies below
    // every distance it can give a voxel of this wave (the scan has kept the windows that cover the slice).
    // (yl: the first of the lane's own VROWS rows)
    int key[NS];
#pragma unroll
    for (int j = 0; j < NS; ++j) {
        const int c = lane + 64 * j;
        key[j] = VOL_KEY_INF;
        if (c < count) {
            const VolRec rc = rec[c];
            if (rc.wy0 < y1w && rc.wy1 > y0 && rc.wx0 < x1w && rc.wx1 > x0w) {
                const float yn = fminf(fmaxf(rc.cy, (float)y0), (float)(y1w - 1));
                const float xn = fminf(fmaxf(rc.cx, (float)x0w), (float)(x1w - 1));
                const float tyl = sy * (rc.cy - yn), txl = sx * (rc.cx - xn);
                const float dy2 = tyl * tyl, dx2 = txl * txl;
                const float tz = sz * (rc.cz - fz0);
                const float dz = tz * tz;
                const float lb = ((dz + dy2) + dx2) * sw;              // >= 0, or +inf / NaN (then: not a candidate)
                const int bits = __float_as_int(lb);
                key[j] = (bits >= 0 && bits < VOL_KEY_INF) ? ((bits & ~7) | j) : VOL_KEY_INF;
            }
        }
    }
    int since_refresh = 0;
    while (true) {
        int mine = key[0];
#pragma unroll
        for (int j = 1; j < NS; ++j) mine = min(mine, key[j]);
        const int wk = wave_min_key(mine);
        if (wk >= VOL_KEY_INF) break;                              // nothing left in the batch
        if (!(__int_as_float(wk & ~7) <= wave_worst)) break;       // every candidate left is farther than what the strips have
        const unsigned long long own = __ballot(mine == wk);
        const int src = __ffsll((long long)own) - 1;
        const int jsel = wk & 7;
#pragma unroll
        for (int j = 0; j < NS; ++j)
            if (lane == src && j == jsel) key[j] = VOL_KEY_INF;
        const int c = src + 64 * jsel;
        const int ck = list[c];
        const VolRec rc = rec[c];
        VOL_PH_COUNT(11, 1);
        const bool inx = x >= rc.wx0 && x < rc.wx1;
        const float tx = sx * (rc.cx - fx);
        const float dx2 = tx * tx;
        float dy[VROWS];
#pragma unroll
        for (int r = 0; r < VROWS; ++r) {
            const float ty = sy * (rc.cy - (float)(yl + r));
            dy[r] = ty * ty;
        }
        const float tz = sz * (rc.cz - fz0);
        const float dz = tz * tz;
#pragma unroll
        for (int r = 0; r < VROWS; ++r) {
            const int y = yl + r;
            const bool iny = y >= rc.wy0 && y < rc.wy1;
            float d = ((dz + dy[r]) + dx2) * sw;
            const float t = pv[r] - rc.cv;
            d = d + t * t;
            const bool take = inx && iny && (best_d[r] > d || (best_d[r] == d && ck < best_k[r]));
            // (the compiler guards the arithmetic of a row with the window test -- branches; written with & and | instead, as
            // compares into masks and two selects, every row is computed for every candidate and the kernel spills: 14.7
            // against 8.7 ms per sweep at config 5)
            best_d[r] = take ? d : best_d[r];
            best_k[r] = take ? ck : best_k[r];
        }
        if (++since_refresh == 2) {
            since_refresh = 0;
            float m2 = 0.f;
#pragma unroll
            for (int r = 0; r < VROWS; ++r)
                if (xin && (yl + r) < H && zin) m2 = fmaxf(m2, best_d[r]);
            wave_worst = wave_max_nonneg_f32(m2);           // (distances: never negative; +inf while a voxel has no candidate)
        }
    }
}


// Round 6.  A phase profile of the kernel (shader-clock ticks per section, tools/vol_phase_probe.py) showed where a workgroup's
// 25 us go: 27 % into the scan of the brick list (list entry -> search window of that centroid -> test: two dependent trips to
// global memory), 8 % into fetching the records of the hits (a third), 31 % into the bounding boxes (per strip row, every run
// start loads its label's box and compares: four more dependent trips per wave) and 17 % into the walk itself -- the kernel waits,
// all four waves of a workgroup together, far more than it computes.  So the trips are taken out:
//   * k_vol_scatter_f32 writes everything the assignment needs of a centroid -- position, value, search window, index: one
//     VolEntry of 48 bytes -- into the brick lists; the scan loads an entry with three 16-byte loads, tests it and drops it
//     straight into the LDS records: ONE trip instead of three, and one barrier less;
//   * the bounding boxes of a workgroup's labels meet in an LDS hash table first (a 64 x 16 cross-section sees a dozen labels):
//     run starts update it with LDS atomics, and one thread per label compares with / updates the global box at the end --
//     a dozen box updates per workgroup instead of one per run, row and wave (~100).
// Same candidates, same arithmetic, same order-free comparison: the label maps do not move.
struct VolEntry {
    float cz, cy, cx, cv;
    int wy0, wy1, wx0, wx1;
    int wz0, wz1, k, pad;
};
static_assert(sizeof(VolEntry) == 48, "three 16-byte loads per entry");
constexpr int VT_SLOTS = 64;          // labels of a workgroup's cross-section whose boxes meet in LDS (more: straight to global memory)

// every centroid writes its entry into the list of each brick its search window meets (float32 volumes).  One WAVE per centroid:
// lane j takes the bricks j, j + 64, ... of the window's brick range (~50 at sp_size 15: a thread per centroid walked them one
// after the other, an atomic and three 16-byte stores each -- 0.98 ms per sweep at 298 116 supervoxels)
__global__ void __launch_bounds__(256) k_vol_scatter_f32(VolState s)
{
    const int k = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, lane = threadIdx.x & 63;
    if (k >= s.K) return;
    const int *w = s.win + (size_t)k * 6;
    const int w0 = w[0], w1 = w[1], w2 = w[2], w3 = w[3], w4 = w[4], w5 = w[5];
    if (w1 <= w0 || w3 <= w2 || w5 <= w4) return;       // dead centroid: empty window
    const float4 cen = *reinterpret_cast<const float4 *>(s.cen32 + (size_t)k * 4);
    const int4 e0 = make_int4(__float_as_int(cen.x), __float_as_int(cen.y), __float_as_int(cen.z), __float_as_int(cen.w));
    const int4 e1 = make_int4(w2, w3, w4, w5);
    const int4 e2 = make_int4(w0, w1, k, 0);
    const int bz0 = w0 / VOL_BZ, by0 = w2 / VOL_BY, bx0 = w4 / VOL_BX;
    const int nz = (w1 - 1) / VOL_BZ - bz0 + 1, ny = (w3 - 1) / VOL_BY - by0 + 1, nx = (w5 - 1) / VOL_BX - bx0 + 1;
    const int total = nz * ny * nx;
    for (int j = lane; j < total; j += 64) {
        const int bx = bx0 + j % nx, by = by0 + (j / nx) % ny, bz = bz0 + j / (nx * ny);
        const int b = (bz * s.nby + by) * s.nbx + bx;
        const int pos = atomicAdd(&s.brick_count[b], 1);
        if (pos < s.brick_cap) {
            int4 *dst = reinterpret_cast<int4 *>(s.brick_entries + ((size_t)b * s.brick_cap + pos) * 12);
            dst[0] = e0;
            dst[1] = e1;
            dst[2] = e2;
        }
    }
}

// waves per SIMD the register allocation aims at.  On 64 x 4 strips: 80 registers when left alone (six waves), 72 at seven -- 2.53
// against 2.68 ms per sweep of a quarter volume, alternating on one box --, spills at eight (64 registers: 3.47 ms).  On 16 x 16
// tiles with the labels staged through LDS (more per-lane state: own rows, tile geometry) seven waves spill into scratch inside the
// walk: 6 -> 7.48, 7 -> 8.72, 5 -> 8.37, 8 -> 11.97 ms per sweep at config 5, one box each pair.
constexpr int VOL_ASSIGN_WAVES = 6;
template <bool TRACK>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(VOL_ASSIGN_WAVES, VOL_ASSIGN_WAVES)))
k_vol_assign_f32(VolState s, const float *__restrict__ vol, int32_t *__restrict__ labels)
{
    // A workgroup = the 64 x 16 cross-section of a brick in one slice; a wave = a 16 x 16 tile of it (see VT_W above).
    __shared__ int list[VLIST32];
    __shared__ __attribute__((aligned(16))) VolRec rec[VLIST32];      // (filled with 16-byte stores)
    // (19.7 KB per workgroup, eight of them per CU; with a byte per record for the slices a window covers and z columns in the table
    // of the boxes -- two slices per workgroup -- it was 20.8 KB and seven)
    __shared__ int wave_base[4];
    // the box of a label inside the cross-section as the SET of its columns -- 64 bits, hb_box[][0..1] -- and of its rows -- 16 bits,
    // hb_box[][2] --, joined with OR (hb_box[][3]: padding, the 64-bit set stays 8-byte aligned)
    __shared__ int hb_key[TRACK ? VT_SLOTS : 1];
    __shared__ __attribute__((aligned(8))) int hb_box[TRACK ? VT_SLOTS : 1][4];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    VOL_PH_BEGIN
    const int rows_per_block = 4 * VROWS;
    const int yb = cdiv(s.H, rows_per_block);
    const int z0 = blockIdx.y / yb;
    const int nzv = min(1, s.D - z0);                         // 1: the slice of this workgroup lies inside the volume (else <= 0)
    const bool zin = nzv > 0;
    const int Y0 = (blockIdx.y % yb) * rows_per_block, Y1 = min(Y0 + rows_per_block, s.H);
    // the wave's voxels: [y0, y1w) x [xt0, xt1); the lane's: column x, rows yl .. yl + VROWS - 1
    constexpr int TILES_X = 64 / VT_W;                        // the four tiles of a workgroup lie side by side
    const int y0 = Y0 + (wave / TILES_X) * VT_H;
    const int yl = y0 + (lane / VT_W) * VROWS;
    const int x0w = blockIdx.x * 64, x1w = min(x0w + 64, s.W);                    // the cross-section (the scan of the brick's list)
    const int xt0 = x0w + (wave % TILES_X) * VT_W, xt1 = min(xt0 + VT_W, s.W);
    const int x = xt0 + (lane & (VT_W - 1));
    const bool alive = xt0 < s.W && y0 < s.H;                 // (a wave outside the volume takes part in the barriers only)
    const int y1w = min(y0 + VT_H, s.H);
    const bool xin = x < s.W;
    if (TRACK && tid < VT_SLOTS) {                            // (visible to all after the first barrier of the scan below)
        hb_key[tid] = -1;
#pragma unroll
        for (int j = 0; j < 4; ++j) hb_box[tid][j] = 0;
    }
    float pv[VROWS], best_d[VROWS];
    int best_k[VROWS];
#pragma unroll
    for (int r = 0; r < VROWS; ++r) {
        const bool ok = alive && xin && (yl + r) < s.H && zin;
        pv[r] = vol[ok ? ((size_t)z0 * s.H + yl + r) * s.W + x : 0];
        best_d[r] = INFINITY;
        best_k[r] = -1;
    }
    const float fz0 = (float)z0, fx = (float)x;
    const float sz = (float)s.sz, sy = (float)s.sy, sx = (float)s.sx;
    const float sw = (float)s.spatial_weight;              // = (float)(1 / ((double)step * (double)step))
    int count = 0;                                         // (uniform over the workgroup)
    float wave_worst = INFINITY;
    const int brick = ((z0 / VOL_BZ) * s.nby + (Y0 / VOL_BY)) * s.nbx + blockIdx.x;
    const int bcount = s.brick_count[brick];
    const bool whole = bcount > s.brick_cap;                   // list overflow: scan every centroid
    const int4 *__restrict__ entries = reinterpret_cast<const int4 *>(s.brick_entries + (size_t)brick * s.brick_cap * 12);
    // (requesting the first 256 entries before the length of the list is known -- one trip to memory instead of two -- was built and
    // measured: 3.30 against 2.67 ms per sweep of a 64 x 2048 x 2048 volume on one box, alternating.  Twelve more registers per
    // thread and half the speculative loads wasted cost more than the trip.)
    const int nscan = whole ? s.K : bcount;
    const int nblk = cdiv(nscan, 256);
    static_assert(VLIST32 == 512, "eight list slots per lane: three bits of a key");
    VOL_PH(0);
    VOL_PH_COUNT(8, 1);
    VOL_PH_COUNT(9, nscan);
    if (nblk == 0) __syncthreads();                            // (the table of the boxes is initialised for everybody)
    for (int b = 0; b < nblk; ++b) {
        const int i = b * 256 + tid;
        int4 e0 = make_int4(0, 0, 0, 0), e1 = e0, e2 = e0;
        bool hit = false;
        if (i < nscan) {
            if (whole) {
                const int *w = s.win + (size_t)i * 6;
                const float4 cen = *reinterpret_cast<const float4 *>(s.cen32 + (size_t)i * 4);
                e0 = make_int4(__float_as_int(cen.x), __float_as_int(cen.y), __float_as_int(cen.z), __float_as_int(cen.w));
                e1 = make_int4(w[2], w[3], w[4], w[5]);
                e2 = make_int4(w[0], w[1], i, 0);
            } else {
                e0 = entries[3 * i];
                e1 = entries[3 * i + 1];
                e2 = entries[3 * i + 2];
            }
            hit = e2.x < z0 + nzv && e2.y > z0 && e1.x < Y1 && e1.y > Y0 && e1.z < x1w && e1.w > x0w;
        }
        const unsigned long long m = __ballot(hit);
        if (lane == 0) wave_base[wave] = __popcll(m);
        __syncthreads();
        int base = count;
        for (int w2 = 0; w2 < wave; ++w2) base += wave_base[w2];
        const int added = wave_base[0] + wave_base[1] + wave_base[2] + wave_base[3];
        if (hit) {
            const int pos = base + __popcll(m & ((1ULL << lane) - 1ULL));
            list[pos] = e2.z;
            int4 *dst = reinterpret_cast<int4 *>(&rec[pos]);
            dst[0] = e0;
            dst[1] = e1;
        }
        count += added;
        __syncthreads();                                     // (list and records are complete; wave_base may be rewritten)
        VOL_PH(1);
        if (count <= VLIST32 - 256 && b + 1 < nblk) continue;
        VOL_PH_COUNT(10, count);
        VOL_PH(2);
        if (alive) {
#define VOL_WALK(NS) vol_walk_f32<NS>(rec, list, count, lane, y0, y1w, xt0, xt1, yl, x, xin, s.H, zin, fz0, fx, sz, sy, sx, sw, pv, best_d, best_k, wave_worst)
            switch ((count + 63) >> 6) {
            case 0: break;
            case 1: VOL_WALK(1); break;
            case 2: VOL_WALK(2); break;
            case 3: VOL_WALK(3); break;
            case 4: VOL_WALK(4); break;
            case 5: VOL_WALK(5); break;
            case 6: VOL_WALK(6); break;
            case 7: VOL_WALK(7); break;
            default: VOL_WALK(8); break;
            }
#undef VOL_WALK
        }
        VOL_PH(3);
        count = 0;
        if (b + 1 < nblk) __syncthreads();                   // (everybody is done with this batch's list and records)
        VOL_PH(4);
    }
    unsigned pending = 0;                                    // bit r: the voxel of row r carries a label
    // A tile's row is narrower than a line of the label map (16 voxels = 64 of its 128 bytes): the tiles hand their new labels to
    // the LDS the records have left, and every wave stores four whole rows of the cross-section.  Written half line by half line,
    // straight from the tiles, the map cost 2.3 bytes to memory per byte (WRITE_SIZE, profiles/pmc_r06_cfg5_kernels.txt).
    int *stage = reinterpret_cast<int *>(rec);               // [16][64]
    static_assert(sizeof(rec) >= 16 * 64 * sizeof(int), "the records' LDS holds a cross-section of labels");
    __syncthreads();                                         // (everybody is done with the last batch's records)
#pragma unroll
    for (int r = 0; r < VROWS; ++r) stage[(yl - Y0 + r) * 64 + (x - x0w)] = best_k[r];
    __syncthreads();
#pragma unroll
    for (int r = 0; r < VROWS; ++r) {
        const int ys = Y0 + wave * VROWS + r, xs = x0w + lane;
        const int k = stage[(wave * VROWS + r) * 64 + lane];
        if (k >= 0 && xs < s.W && ys < s.H) labels[((size_t)z0 * s.H + ys) * s.W + xs] = k;
    }
    if (alive) {
#pragma unroll
        for (int r = 0; r < VROWS; ++r) {
            if (!(xin && (yl + r) < s.H && zin)) continue;
            if (best_k[r] < 0) best_k[r] = labels[((size_t)z0 * s.H + yl + r) * s.W + x];      // uncovered voxel keeps its previous assignment
            if (best_k[r] >= 0) pending |= 1u << r;
        }
    }
    VOL_PH(5);
    if (!TRACK) return;
    // bounding box of every segment's voxels (incl. the ones that kept an old label): the region the order-preserving update of
    // that centroid has to walk.  By RUNS: in every row of the tile the first lane of a run of equal labels finds the end of its run
    // in the vote of the run starts and joins the label's SETS of columns and rows in the workgroup's LDS table with two ORs that
    // return nothing; a lane that has found the slot of a label keeps it for the rows below (a label change costs the search
    // again).  The table goes to the global boxes once, below.  Unions, minima and maxima: the boxes are the same whatever the order
    // and however often a label is met.
    // (Measured at config 5, one box: runs that update minima / maxima of y and x in the table 9.49 ms per sweep; label by label --
    // the first waiting lane names a label, four votes give its columns and rows, one lane joins them -- 11.05 ms: a serial chain
    // per label and wave.)
    if (alive) {
        int slot_of = -2, slot = -1;
#pragma unroll
        for (int r = 0; r < VROWS; ++r) {
            const int k = (pending >> r) & 1u ? best_k[r] : -1;
            const int kp = tile_prev(k, -2);                        // (the first lane of a row of the tile: a start)
            const bool start = k >= 0 && kp != k;
            const unsigned long long starts = __ballot(start), valid = __ballot(k >= 0);
            if (start) {
                const unsigned long long stop = (starts | ~valid) & ~((2ULL << lane) - 1ULL);     // the lanes above this one
                const int len = (stop ? __ffsll((long long)stop) - 1 : 64) - lane;                 // (<= 16: the next row starts)
                if (k != slot_of) {
                    slot_of = k;
                    slot = (int)(((unsigned int)k * 2654435761u) >> 26);          // 6 bits
                    bool placed = false;
                    for (int probe = 0; probe < VT_SLOTS; ++probe) {
                        const int old = atomicCAS(&hb_key[slot], -1, k);
                        if (old == -1 || old == k) {
                            placed = true;
                            break;
                        }
                        slot = (slot + 1) & (VT_SLOTS - 1);
                    }
                    slot = placed ? slot : -1;
                }
                const int y = yl + r;
                if (slot >= 0) {
                    atomicOr(reinterpret_cast<unsigned long long *>(&hb_box[slot][0]), ((1ULL << len) - 1ULL) << (x - x0w));
                    atomicOr(reinterpret_cast<unsigned int *>(&hb_box[slot][2]), 1u << (y - Y0));
                } else {                                              // (more than VT_SLOTS labels in a cross-section)
                    int *bb = s.bbox + (size_t)k * 6;
                    atomicMin(&bb[0], z0); atomicMax(&bb[1], z0);
                    atomicMin(&bb[2], y); atomicMax(&bb[3], y);
                    atomicMin(&bb[4], x); atomicMax(&bb[5], x + len - 1);
                }
            }
        }
    }
    __syncthreads();
    if (tid < VT_SLOTS && hb_key[tid] >= 0) {
        int *bb = s.bbox + (size_t)hb_key[tid] * 6;
        const int2 bz = *reinterpret_cast<const int2 *>(bb), by = *reinterpret_cast<const int2 *>(bb + 2),
                   bx = *reinterpret_cast<const int2 *>(bb + 4);
        const unsigned long long colset = *reinterpret_cast<const unsigned long long *>(&hb_box[tid][0]);
        const unsigned rows = (unsigned)hb_box[tid][2];
        const int ylo = Y0 + __ffs(rows) - 1, yhi = Y0 + 31 - __clz(rows);
        const int xlo = x0w + __ffsll((long long)colset) - 1, xhi = x0w + 63 - __clzll((long long)colset);
        if (bz.x > z0) atomicMin(&bb[0], z0);
        if (bz.y < z0) atomicMax(&bb[1], z0);
        if (by.x > ylo) atomicMin(&bb[2], ylo);
        if (by.y < yhi) atomicMax(&bb[3], yhi);
        if (bx.x > xlo) atomicMin(&bb[4], xlo);
        if (bx.y < xhi) atomicMax(&bb[5], xhi);
    }
    VOL_PH(6);
}

// Round 5: one LANE per centroid.  The float32 sums of a segment must be formed in raster order (see above), which makes the sum of
// ONE segment a serial chain -- but the chains of different segments have nothing to do with each other.  Rounds 3 / 4 gave a
// whole wave to one chain: per member voxel a find-first-bit, a bit clear, two v_readlane and two packed additions, i.e. eight
// issue slots of which the wave used one lane's worth (13.2 ms per sweep at 298 116 supervoxels against 3.5 here; A/B in
// profiles/rocprof_r05_cfg5_kernel_stats.txt against rocprof_r04_cfg5_kernel_stats.txt; removed in round 6).  Here a lane walks the
// bounding box of ITS segment voxel by voxel -- labels[p] == k ? add : skip -- and the sixty-four chains of a wave advance together;
// lanes of one wave hold neighbouring centroids of a grid row, whose boxes lie side by side, so the lines a wave touches are shared
// by its lanes and reused by the next steps of the walk (L1 / L2), and the additions of a chain happen in exactly the order of the
// serial loop: z, then y, then x ascending.  Same results bit for bit (the parity tests of the float32 volumes; the full-size
// label map against scikit-image's).
constexpr int VU_STEP = 4;          // voxels of one 16-byte load
// four consecutive 4-byte elements at a 4-byte aligned address: one global_load_dwordx4
template <typename T> struct __attribute__((packed, aligned(4))) Quad {
    T v[4];
};
static_assert(VU_STEP == 4, "a round of the update is one Quad");
// (quads of a lane requested per round, config 5, ms per sweep: 1 -> 3.01, 2 -> 2.03, 4 -> 1.81, 6 -> 1.84, 8 -> 1.82)
// (the walk as one sequence of rounds with the NEXT round's labels requested before this round's values -- one trip per round
// instead of two -- measured 1.84 against 1.80: with four quads per round the trips are no longer what the kernel waits for)
constexpr int VU_QUADS = 4;

// (lanes per workgroup, config 5, one box: 64 -> 3.26, 256 -> 2.93, 512 -> 3.13, 1 024 -> 3.89 ms per sweep; an eighth of the centroids
// per XCD -- block index modulo 8 -> a fixed range -- 3.06 against 2.99: not kept)
constexpr int VOL_UPDATE_BLOCK = 256;
__global__ void __launch_bounds__(VOL_UPDATE_BLOCK)
k_vol_update_f32_lane(VolState s, const float *__restrict__ vol, const int32_t *__restrict__ labels)
{
    const int k = blockIdx.x * VOL_UPDATE_BLOCK + threadIdx.x;
    if (k >= s.K) return;
    int *bb = s.bbox + (size_t)k * 6;
    int *w = s.win + (size_t)k * 6;
    const int z0 = bb[0], z1 = bb[1], y0 = bb[2], y1 = bb[3], x0 = bb[4], x1 = bb[5];
    if (z1 < z0) {                                            // no voxel carries this label: the centroid is dead
#pragma unroll
        for (int j = 0; j < 6; ++j) w[j] = 0;
        return;
    }
    float sz = 0.f, sy = 0.f, sx = 0.f, sv = 0.f;
    int cnt = 0;
    for (int z = z0; z <= z1; ++z) {
        const float fz = (float)z;
        for (int y = y0; y <= y1; ++y) {
            const float fy = (float)y;
            const size_t row = ((size_t)z * s.H + y) * s.W;
            // VU_STEP voxels per round: their labels and values are requested together (eight loads in flight instead of a chain
            // of two per voxel), then added in order.  A voxel of another segment adds +0.0f, which leaves a sum that started at
            // +0.0f bit for bit as it is (a sum of this kind is never -0.0f: (+0) + (-0) = +0).
            // (round 6: the four voxels of a round come in ONE 16-byte load of labels and one of values -- the lanes of a wave walk
            // different boxes, so every load instruction touches 64 cache lines whatever its width; a quarter of the instructions.
            // Voxels past x1 are loaded -- the buffers end in padding -- and masked.  The values of a quad are requested only where
            // one of its labels is the lane's -- under half of a box's voxels: 3.01 against 3.25 ms per sweep at config 5, one box.)
            // (VU_QUADS quads per round, all requested before the first is added: a lane's consecutive quads lie in one or two cache
            // lines, and requested together they are ONE trip to the L2 where one quad per round was a trip each -- the lines a wave
            // touches in a round, 64 lanes x 2 arrays, do not survive in the L1 until its next round)
            for (int x = x0; x <= x1; x += VU_STEP * VU_QUADS) {
                Quad<int> lab[VU_QUADS];
                Quad<float> val[VU_QUADS];
#pragma unroll
                for (int q = 0; q < VU_QUADS; ++q) {
                    lab[q] = { { -1, -1, -1, -1 } };
                    if (x + VU_STEP * q <= x1) lab[q] = *reinterpret_cast<const Quad<int> *>(labels + row + x + VU_STEP * q);
                }
#pragma unroll
                for (int q = 0; q < VU_QUADS; ++q) {
                    val[q] = { { 0.f, 0.f, 0.f, 0.f } };
                    if (lab[q].v[0] == k || lab[q].v[1] == k || lab[q].v[2] == k || lab[q].v[3] == k)
                        val[q] = *reinterpret_cast<const Quad<float> *>(vol + row + x + VU_STEP * q);
                }
#pragma unroll
                for (int q = 0; q < VU_QUADS; ++q)
#pragma unroll
                    for (int j = 0; j < VU_STEP; ++j) {
                        const int xx = x + VU_STEP * q + j;
                        const bool mine = lab[q].v[j] == k && xx <= x1;
                        sz = sz + (mine ? fz : 0.f);
                        sy = sy + (mine ? fy : 0.f);
                        sx = sx + (mine ? (float)xx : 0.f);
                        sv = sv + (mine ? val[q].v[j] : 0.f);
                        cnt += mine ? 1 : 0;
                    }
            }
        }
    }
    const float fc = (float)cnt;                              // seg[c] / (float)cnt   (cnt > 0: the box is not empty)
    const float cz = sz / fc, cy = sy / fc, cx = sx / fc;
    *reinterpret_cast<float4 *>(s.cen32 + (size_t)k * 4) = make_float4(cz, cy, cx, sv / fc);
    vol_window_f32(s, cz, cy, cx, w);
    vol_bbox_reset(bb);
}

int launch_vol_slic_f32(VolState s, const float *vol, int32_t *labels, int max_iter, hipStream_t st, const ProfHook *prof)
{
    size_t n = (size_t)s.D * s.H * s.W;
    HIP_TRY(hipMemsetAsync(labels, 0xff, n * sizeof(int32_t), st));
    hipLaunchKernelGGL(k_vol_centroid_init_f32, cdiv(s.K, 256), 256, 0, st, s);
    dim3 grid(cdiv(s.W, 64), cdiv(s.H, 4 * VROWS) * s.D);      // a workgroup: 64 x 16 voxels of one slice
    const size_t n_bricks = (size_t)s.nbz * s.nby * s.nbx;
    for (int it = 0; it < max_iter; ++it) {
        HIP_TRY(hipMemsetAsync(s.brick_count, 0, n_bricks * sizeof(int), st));
        hipLaunchKernelGGL(k_vol_scatter_f32, cdiv((long)s.K * 64, 256), 256, 0, st, s);
        // (when profiling: the event pair rides on the dispatch of the assignment kernel, group 0 = "slic_assign")
        hipEvent_t ev_a = nullptr, ev_b = nullptr;
        if (prof && prof->pair) prof->pair(prof->user, 0, &ev_a, &ev_b);
        if (it + 1 < max_iter) {
            if (ev_a) hipExtLaunchKernelGGL(k_vol_assign_f32<true>, grid, dim3(256), 0, st, ev_a, ev_b, 0, s, vol, labels);
            else hipLaunchKernelGGL(k_vol_assign_f32<true>, grid, 256, 0, st, s, vol, labels);
            hipLaunchKernelGGL(k_vol_update_f32_lane, cdiv(s.K, VOL_UPDATE_BLOCK), VOL_UPDATE_BLOCK, 0, st, s, vol, labels);
        } else {
            if (ev_a) hipExtLaunchKernelGGL(k_vol_assign_f32<false>, grid, dim3(256), 0, st, ev_a, ev_b, 0, s, vol, labels);
            else hipLaunchKernelGGL(k_vol_assign_f32<false>, grid, 256, 0, st, s, vol, labels);
        }
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

#ifdef IMSEGM_VOL_PHASE_PROF
int vol_phase_read(unsigned long long *out16, int reset)
{
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpyFromSymbol(out16, HIP_SYMBOL(g_vol_phase), 16 * sizeof(unsigned long long)));
    if (reset) {
        unsigned long long zero[16] = { 0 };
        HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_vol_phase), zero, sizeof(zero)));
    }
    return 0;
}
#endif

}  // namespace imsegm

#ifdef IMSEGM_VOL_PHASE_PROF
extern "C" __attribute__((visibility("default"))) int imsegm_debug_vol_phases(unsigned long long *out16, int reset)
{
    return imsegm::vol_phase_read(out16, reset);
}
#endif
