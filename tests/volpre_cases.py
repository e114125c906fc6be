"""Shared by tests/test_volpre_reference_host.py and tests/test_gpu_volpre_reference.py: the pre-processing of the gray-volume SLIC
(csrc/volume.hip: k_vol_to_f64, k_vol_blur, k_vol_blur_z32, k_vol_blur_yx32, k_vol_blur_r32, launch_absmax_f64) and its centroid
update (k_vol_update_f32_lane, k_vol_centroid_finalize), stated three times --

  ``reference64`` / ``reference32``  the definition in ``numpy.longdouble`` (64 mantissa bits) from the uploaded voxels, with the
                   taps ``Volume3D.slic`` hands to the library widened (``taps_of``: for a float32 volume the taps of
                   ``float32(sigma) / float32(spacing)``);
  ``yardstick64`` / ``yardstick32``  ``scipy.ndimage.gaussian_filter(mode='reflect')`` on the float64 / float32 array and the product
                   with ``1 / compactness`` in that type;
  ``model64`` / ``model32``          numpy transcriptions of the device's evaluation in the kernels' operation order -- the z chunks, the
                   ``ahead`` plane, the 64 x 32 tiles with their ``extra`` columns, the interior shortcut as INDEX MAPS -- with a
                   ``defect=`` switch.

No expected number comes from the device code.

Non-float32 volumes (uint8, float64; every other dtype goes up as float64 with ``img_as_float_map``'s offset and scale): the plane
is float64.  Reference: ``(v + off) * scale``, then z, y, x as reflected Toeplitz products (``pre_cases.reflect_matrix``: period 2n,
any distance), then ``* (1 / compactness)``, all in 80 bits.  Deviation: max |got - ref| / S, S = max |ref|.  Tolerance: the
project's rule, ``FACTOR`` x (yardstick against the reference), floor ``FLOOR``.

float32 volumes: scikit-image 0.18 keeps them float32, and scipy stores every line of every axis pass in the output dtype.  The
reference restates that: per pass the 80-bit reflected sum of the float32 inputs with the fp64 taps, rounded ONCE to float32; after
the x pass the float32 product with ``float32(1 / compactness)``.  The device (and scipy) form the sum in fp64 and round that: the
bits can differ from the reference's only where the exact sum of a pass lies next to a float32 rounding midpoint.

  gamma.  A pass computes  v = x0 w0;  v += (a_j + b_j) w_j  for j = r .. 1.  With u = 2^-53 every operation rounds once,
  fl(p op q) = (p op q)(1 + d), |d| <= u.  The centre product passes through 1 multiplication and r additions, the pair j = r
  through its own addition, its multiplication and r additions (r + 2 roundings, the most of any term); so
  |fl(sum) - sum| <= gamma_(r + 2) sum |w_j| |v_j|,  gamma_n = n u / (1 - n u)  (Higham, Accuracy and Stability, Lemma 3.1).  The
  builder uses the looser count of all 2 r + 2 operations the sum is charged with as a dot product of 2 r + 1 terms with one
  pair addition more: GAMMA(r) = gamma_(2 r + 2) >= gamma_(r + 2).  The reference's own 80-bit evaluation of the same sum errs by at
  most (2 r + 2) 2^-64 sum |w_j| |v_j| (same argument, unit roundoff 2^-64); both go into the margin.  Nothing here is tuned.

  A voxel and pass are MARKED when the 80-bit sum lies within that margin of a midpoint between two neighbouring float32 numbers;
  each mark spreads over the footprint (reflected) of the later passes.  Unmarked voxels of the device must equal the reference bit
  for bit; marked voxels are held to two float32 spacings at S.  The builder asserts from the reference alone that at most
  ``MARK_CAP`` of a case's voxels are marked, and that every voxel where scipy's float32 result differs from the reference is marked.

Centroid update: see ``update_reference32`` / ``update_bound64``."""
import functools

import numpy as np

import pre_cases as P
from pre_cases import FACTOR, FLOOR, LD, LONGDOUBLE_OK, reflect_matrix, rel_dev, widen  # noqa: F401  (the tests read them from here)

SEED = 20261019
COMPACTNESS = 10.
MARK_CAP = 0.005
U64 = 2.0**-53
Z_TILE_W, YX_TW, YX_TH, VBLUR_R = 256, 64, 32, 4           # columns of a z-pass workgroup; tile of k_vol_blur_yx32; its largest radius
VU_STEP, VU_QUADS = 4, 4                                   # k_vol_update_f32_lane: voxels of a quad, quads of a round
#: sigma = 1: the spacing that gives each radius int(4 / spacing + 0.5)
SPACING_OF_RADIUS = {0: 10., 1: 5., 2: 2., 3: 1.5, 4: 1., 8: 0.5, 16: 0.25}
REFUSED_SPACING = 0.24                                     # radius 17


def gamma(r):
    """gamma_(2 r + 2) in fp64 (module docstring)"""
    n = 2 * r + 2
    return n * U64 / (1 - n * U64)


def sigma_over_spacing(dtype, sigma, spacing):
    """what ``Volume3D.slic`` computes: in float32 for a float32 volume (scikit-image 0.18 keeps both in the image's dtype)"""
    fdt = np.float32 if np.dtype(dtype) == np.float32 else np.float64
    return [float(s) for s in np.array([sigma, sigma, sigma], dtype=fdt) / np.ascontiguousarray(spacing, dtype=fdt)]


def taps_of(c):
    """the three half kernels (z, y, x) the host hands to the library for a case; None: axis not filtered"""
    from pyimsegm_amd._hip import gaussian_taps
    return [gaussian_taps(s) for s in sigma_over_spacing(c['volume'].dtype if c['dtype'] == 'f32' else np.float64, c['sigma'],
                                                         c['spacing'])]


def radii_of(c):
    return tuple(-1 if t is None else len(t) - 1 for t in taps_of(c))


def affine_of(c):
    from pyimsegm_amd._hip import img_as_float_map
    return img_as_float_map(c['volume'].dtype)


def along(mat, v, axis):
    """mat (n x n) applied along ``axis`` of ``v``"""
    return np.moveaxis(np.tensordot(mat, v, axes=(1, axis)), 0, axis)


# ---- references ------------------------------------------------------------------------------------------------------------
def reference64(c):
    """the float64 plane's definition in longdouble"""
    off, scale = affine_of(c)
    v = (np.asarray(c['volume']).astype(LD) + LD(off)) * LD(scale)
    for axis, t in enumerate(taps_of(c)):
        if t is not None:
            v = along(reflect_matrix(v.shape[axis], t), v, axis)
    return v * (LD(1) / LD(c['compactness']))


def yardstick64(c):
    from scipy import ndimage
    off, scale = affine_of(c)
    v = (widen(c['volume']) + off) * scale
    if c['sigma'] > 0:
        v = ndimage.gaussian_filter(v, sigma_over_spacing(np.float64, c['sigma'], c['spacing']), mode='reflect')
    return v * (1. / c['compactness'])


def midpoint_distance(s):
    """distance of the longdouble values ``s`` to the nearest midpoint between two neighbouring float32 numbers (exact: the float32
    neighbours have 24 bits, their mean 25)"""
    f = s.astype(np.float32)
    up, dn = np.nextafter(f, np.float32(np.inf)), np.nextafter(f, np.float32(-np.inf))
    fl = f.astype(LD)
    return np.minimum(np.abs(s - (fl + up.astype(LD)) / 2), np.abs(s - (fl + dn.astype(LD)) / 2))


def reference32(c):
    """(plane float32, marked bool): the float32 contract in 80 bits, and the voxels whose bits an fp64 evaluation may not share"""
    v = np.asarray(c['volume'])
    assert v.dtype == np.float32
    marked = np.zeros(v.shape, bool)
    for axis, t in enumerate(taps_of(c)):
        if t is None:
            continue
        r, n = len(t) - 1, v.shape[axis]
        mat = reflect_matrix(n, t)
        s = along(mat, v.astype(LD), axis)
        weight = along(np.abs(mat), np.abs(v).astype(LD), axis)
        margin = (LD(gamma(r)) + LD(2 * r + 2) * LD(2.0)**-64) * weight
        footprint = reflect_matrix(n, np.ones(r + 1), dtype=np.float64) > 0
        marked = (along(footprint.astype(np.float64), marked.astype(np.float64), axis) > 0) | (midpoint_distance(s) <= margin)
        v = s.astype(np.float32)                                 # one rounding, 80 bits -> float32
    return v * np.float32(1. / c['compactness']), marked


def yardstick32(c):
    """scipy on the float32 array (it stores every pass in float32), then the float32 product"""
    from scipy import ndimage
    v = np.asarray(c['volume'])
    if c['sigma'] > 0:
        v = ndimage.gaussian_filter(v, sigma_over_spacing(np.float32, c['sigma'], c['spacing']), mode='reflect')
    assert v.dtype == np.float32
    return v * np.float32(1. / c['compactness'])


def check32(got, ref):
    """the float32 comparison: (voxels that differ, largest difference in float32 spacings at S); raises where an unmarked voxel
    differs or a marked one is farther than two spacings"""
    got = np.asarray(got)
    assert got.dtype == np.float32 and got.shape == ref['ref'].shape
    differ = got != ref['ref']
    spacing = float(np.spacing(np.float32(ref['scale'])))
    worst = float(np.abs(got.astype(np.float64) - ref['ref'].astype(np.float64)).max()) / spacing if spacing > 0 else 0.
    assert not np.any(differ & ~ref['marked']), '%d unmarked voxels differ from the reference' % int(np.sum(differ & ~ref['marked']))
    assert worst <= 2, 'a marked voxel is %.3g float32 spacings at S away' % worst
    return int(differ.sum()), worst


# ---- the device's evaluation as index maps ---------------------------------------------------------------------------------
BORDER_DEFECTS = ('nearest', 'mirror', 'single-wrap')


def border(i, n, defect=None):
    """vreflect of volume.hip; with a border defect, another rule (pre_cases.border_index)"""
    return P.border_index(i, n, defect if defect in BORDER_DEFECTS else None)


def z_chunks(shape):
    """(vec, [(z0, z1), ...]) of launch_vol_preprocess_f32's z pass: vector form when W % 4 == 0 (the upload buffer is 16-byte
    aligned), the z range split when the columns do not fill the device and D >= 32"""
    d, h, w = shape
    vec = 4 if w % 4 == 0 else 1
    columns = -(-w // vec) * h
    chunks = min(max(1, (16384 * 64) // max(columns, 1)), max(1, d // 16))
    zchunk = -(-d // chunks)
    return vec, [(z0, min(z0 + zchunk, d)) for z0 in range(0, d, zchunk)]


def z_columns(w, vec):
    """the columns each thread of the z pass owns (x = (block * 256 + thread) * VEC .. + VEC - 1, kept when x < W)"""
    threads = -(-(-(-w // vec)) // Z_TILE_W) * Z_TILE_W
    return [list(range(t * vec, t * vec + vec)) for t in range(threads) if t * vec < w]


def z_window_map(shape, r, defect=None):
    """[D, 2 r + 1]: the plane window slot j holds when k_vol_blur_z32 computes plane z"""
    d = shape[0]
    m = np.zeros((d, 2 * r + 1), np.int64)
    for z0, z1 in z_chunks(shape)[1]:
        for z in range(z0, z1):
            want = np.arange(z - r, z + r + 1)
            idx = border(want, d, defect)
            if defect == 'chunk-seam' and z0 > 0:            # planes below the chunk reflected at the chunk's start
                idx = np.where(want < z0, border(2 * z0 - 1 - want, d), idx)
            if defect == 'ahead-stale' and z == z1 - 1 and z1 - z0 >= 3:
                idx[2 * r] = border(z + r - 1, d)            # the plane requested a step too early: that of z - 1
            m[z] = idx
    return m


def pass_by_map(x32, axis, taps, index_map, last):
    """one axis pass the way every blur kernel of volume.hip evaluates it: centre tap, then the pairs from the farthest in, in fp64;
    ``index_map[pos, r + d]`` = the source index of offset d at output position pos.  Returns fp64 (the caller stores float32)"""
    r = len(taps) - 1
    x = np.asarray(x32).astype(np.float64)
    acc = np.take(x, index_map[:, r], axis) * taps[0]
    for j in range(last, 0, -1):
        a, b = np.take(x, index_map[:, r - j], axis), np.take(x, index_map[:, r + j], axis)
        acc = acc + (a + b) * taps[j]
    return acc


def plain_map(n, r, defect=None):
    pos = np.arange(n)
    return np.stack([border(pos + d, n, defect) for d in range(-r, r + 1)], axis=1)


def shortcut_map(n, r, defect=None):
    """k_vol_blur_r32: positions with pos - r >= 0 and pos + r < len take i -/+ j * stride, the others the reflected index -- the
    same indices.  'shortcut-early': pos = r - 1 takes the shortcut too and reads index -1 (here: numpy's -1, the last element of
    the line -- whatever it is, it is not the reflected element 0)"""
    m = plain_map(n, r, defect)
    if defect == 'shortcut-early' and r >= 1 and 2 * r - 1 < n:
        m[r - 1] = np.arange(-1, 2 * r)
    return m


def last_tap(r, defect):
    return r - 1 if defect == 'tap-dropped' and r == 3 else r


def eff(t):
    """an axis that is not filtered passes through the fast path as the single tap 1.0"""
    return np.array([1.0]) if t is None else t


def yx_tiles32(mid, ty, tx, ratio, defect=None):
    """k_vol_blur_yx32<RY, RX> on [D, H, W] float32: per 64 x 32 tile the rows / columns its LDS tile A holds as index maps"""
    d, h, w = mid.shape
    ry, rx = len(ty) - 1, len(tx) - 1
    tw, th = YX_TW + 2 * rx, YX_TH + 2 * ry
    out = np.zeros(mid.shape, np.float32)
    fratio = np.float32(ratio)
    ly, lx = last_tap(ry, defect), last_tap(rx, defect)
    for y0 in range(0, h, YX_TH):
        rows = np.minimum(np.arange(th), th - (2 if defect == 'row-dup' else 1))
        rowidx = border(y0 - ry + rows, h, defect)
        for x0 in range(0, w, YX_TW):
            cols = np.arange(tw)
            colidx = border(x0 - rx + cols, w, defect)
            if defect == 'extra-neighbour':                  # the lanes that serve columns 64 .. TW - 1 read the column before
                colidx = np.where(cols >= YX_TW, border(x0 - rx + cols - 1, w), colidx)
            a = mid[:, rowidx][:, :, colidx]                                        # A[TH][TW] of every slice
            ymap = np.arange(YX_TH)[:, None] + np.arange(2 * ry + 1)[None, :]       # B[yy] <- A[yy .. yy + 2 RY]
            b = pass_by_map(a, 1, ty, ymap, ly)
            b = b if defect == 'no-f32-store' else b.astype(np.float32)
            xmap = np.arange(YX_TW)[:, None] + np.arange(2 * rx + 1)[None, :]       # out[lane] <- B[lane .. lane + 2 RX]
            v = pass_by_map(b, 2, tx, xmap, lx)
            v = (v * ratio).astype(np.float32) if defect == 'ratio-double' else v.astype(np.float32) * fratio
            ny, nx = min(YX_TH, h - y0), min(YX_TW, w - x0)
            out[:, y0:y0 + ny, x0:x0 + nx] = v[:, :ny, :nx]
    if defect == 'ragged':                                   # the last ragged row / column of the tile grid not written
        if h % YX_TH:
            out[:, h - 1, :] = 0
        if w % YX_TW:
            out[:, :, w - 1] = 0
    return out


def fast_path(c):
    return all(r <= VBLUR_R for r in radii_of(c))


def model32(c, path='default', defect=None):
    """the float32 plane as launch_vol_preprocess_f32 produces it: the z-column / tile kernels when every radius is <= 4 (and
    ``path`` is not 'three-pass'), else the three k_vol_blur_r32 passes"""
    v = np.asarray(c['volume'])
    tz, ty, tx = taps_of(c)
    ratio = 1. / c['compactness']
    fratio = np.float32(ratio)
    if fast_path(c) and path != 'three-pass':
        if tz is not None:
            r = len(tz) - 1
            vec = z_chunks(v.shape)[0]
            assert sorted(x for cols in z_columns(v.shape[2], vec) for x in cols if x < v.shape[2]) == list(range(v.shape[2]))
            v = pass_by_map(v, 0, tz, z_window_map(v.shape, r, defect), last_tap(r, defect)).astype(np.float32)
        return yx_tiles32(v, eff(ty), eff(tx), ratio, defect)
    for axis, t in enumerate((tz, ty, tx)):
        keep = defect == 'no-f32-store' and axis == 1
        if t is not None:
            r = len(t) - 1
            v = pass_by_map(v, axis, t, shortcut_map(v.shape[axis], r, defect), last_tap(r, defect))
            if not keep:
                v = v.astype(np.float32)
    if defect == 'ratio-double':
        return (v.astype(np.float64) * ratio).astype(np.float32)
    return v.astype(np.float32) * fratio


def model64(c, defect=None):
    """k_vol_to_f64 and the three k_vol_blur passes in fp64, ``* ratio`` inside the x pass"""
    off, scale = affine_of(c)
    x = widen(c['volume'])
    v = x * scale + off if defect == 'off-after-scale' else (x + off) * scale
    for axis, t in enumerate(taps_of(c)):
        if t is not None:
            r = len(t) - 1
            v = pass_by_map(v, axis, t, plain_map(v.shape[axis], r, defect), last_tap(r, defect))
    return v * (1. / c['compactness'])


# ---- centroid update -------------------------------------------------------------------------------------------------------
def update_reference32(plane, labels, n_centroids):
    """_slic.pyx on a float32 image: per label the members in raster order added one by one into float32 sums (z, y, x, value),
    each divided by float32(count).  {label: float32[4]} for the labels with members.  A plain loop; nothing of the kernel's"""
    d, h, w = plane.shape
    flat_l, flat_v = labels.ravel(), plane.ravel()
    order = np.argsort(flat_l, kind='stable')                # members of a label stay in raster order
    bounds = np.searchsorted(flat_l[order], np.arange(n_centroids + 1))
    out = {}
    for k in range(n_centroids):
        members = order[bounds[k]:bounds[k + 1]]
        if not len(members):
            continue
        sums = np.zeros(4, np.float32)
        zs, ys, xs = np.unravel_index(members, (d, h, w))
        for z, y, x, val in zip(zs.astype(np.float32), ys.astype(np.float32), xs.astype(np.float32), flat_v[members]):
            sums[0] += z
            sums[1] += y
            sums[2] += x
            sums[3] += val
        out[k] = sums / np.float32(len(members))
    return out


def update_model32(plane, labels, n_centroids, defect=None):
    """k_vol_update_f32_lane: a lane walks the bounding box of its label row by row, four 16-byte quads per round; a voxel of
    another label -- or past the box -- adds +0.0f"""
    d, h, w = plane.shape
    out = {}
    pad_l = np.concatenate([labels.ravel(), np.full(16, -1, labels.dtype)])         # (the buffers end in padding)
    pad_v = np.concatenate([plane.ravel(), np.zeros(16, np.float32)])
    for k in range(n_centroids):
        zz, yy, xx = np.nonzero(labels == k)
        if not len(zz):
            continue
        z0, z1, y0, y1, x0, x1 = zz.min(), zz.max(), yy.min(), yy.max(), xx.min(), xx.max()
        sums = np.zeros(4, np.float32)
        count = 0
        chain = []
        for z in range(z0, z1 + 1):
            for y in range(y0, y1 + 1):
                row = (z * h + y) * w
                for x in range(x0, x1 + 1, VU_STEP * VU_QUADS):
                    for q in range(VU_QUADS):
                        xq = x + VU_STEP * q
                        if xq > x1:
                            continue                         # quad not requested: its four voxels add +0.0f
                        if defect == 'quad-dropped' and xq + VU_STEP - 1 > x1:
                            continue                         # the last, partial quad of the row left out
                        for j in range(VU_STEP):
                            mine = pad_l[row + xq + j] == k and xq + j <= x1
                            term = (np.float32(z), np.float32(y), np.float32(xq + j), pad_v[row + xq + j]) if mine else (np.float32(0), ) * 4
                            chain.append(term)
                            count += int(mine)
        terms = np.array(chain, np.float32)
        if defect == 'pairwise':
            level = list(terms)                              # neighbours added first, then the partial sums
            while len(level) > 1:
                level = [level[i] + level[i + 1] if i + 1 < len(level) else level[i] for i in range(0, len(level), 2)]
            sums = level[0]
        else:
            for t in terms:
                sums = sums + t
        with np.errstate(invalid='ignore'):                  # (a defect can leave a label without a counted member)
            out[k] = sums / np.float32(count)
    return out


def fix_bits_of(premax):
    """common.h: 46 minus the binary exponent of premax (2^e > premax)"""
    return 46 - (int(np.frexp(premax)[1]) if premax > 0 else 1)


def update_model64(plane, labels, n_centroids, premax):
    """k_vol_assign<true> + k_vol_centroid_finalize: integer sums of trunc(v 2^f), exact; one rounding to fp64, one division"""
    f = fix_bits_of(premax)
    out = {}
    for k in range(n_centroids):
        zz, yy, xx = np.nonzero(labels == k)
        if not len(zz):
            continue
        n = float(len(zz))
        total = sum(int(np.trunc(v * 2.0**f)) for v in plane[zz, yy, xx])
        out[k] = np.array([float(zz.sum()) / n, float(yy.sum()) / n, float(xx.sum()) / n, float(total) * 2.0**-f / n])
    return out


def update_bound64(plane, labels, n_centroids, premax):
    """{label: (exact means longdouble[4], bound on the value)}.  Bound: a member enters as t = trunc(v 2^f) -- v 2^f is exact, the
    truncation loses less than 1, i.e. less than 2^-f of v --, the integer sum is exact, so sum / n is below 2^-f from the mean;
    the sum is rounded to fp64 once (i64_to_double, when it exceeds 2^53) and divided by n once: two roundings of at most 2^-53
    relative each, 2^-52 |mean| to first order.  Bound = 2^-f + 2^-52 |mean|, f = fix_bits_of(premax)"""
    f = fix_bits_of(premax)
    out = {}
    for k in range(n_centroids):
        zz, yy, xx = np.nonzero(labels == k)
        if not len(zz):
            continue
        n = LD(len(zz))
        mean = np.array([LD(int(zz.sum())) / n, LD(int(yy.sum())) / n, LD(int(xx.sum())) / n, plane[zz, yy, xx].astype(LD).sum() / n])
        out[k] = mean, float(LD(2.0)**-f + LD(2.0)**-52 * abs(mean[3]))
    return out


def grid_assignment(plane, n_segments, spacing):
    """a stand-in for the first sweep on the CPU: every voxel to the nearest of about ``n_segments`` grid centroids (spacing-weighted
    position plus value).  Only the host file uses it: any label map with ragged segments shows what the update model does"""
    d, h, w = plane.shape
    per = max(1., (d * h * w / float(n_segments)) ** (1. / 3))
    axes = [np.arange(per / 2 if n > per else n / 2., n, max(per, 1.)) for n in (d, h, w)]
    cz, cy, cx = [a.ravel() for a in np.meshgrid(*axes, indexing='ij')]
    cv = plane[cz.astype(int), cy.astype(int), cx.astype(int)].astype(np.float64)
    z, y, x = np.meshgrid(np.arange(d), np.arange(h), np.arange(w), indexing='ij')
    best = np.full(plane.shape, np.inf)
    lab = np.zeros(plane.shape, np.int32)
    for k in range(len(cz)):
        dist = ((spacing[0] * (z - cz[k]))**2 + (spacing[1] * (y - cy[k]))**2 + (spacing[2] * (x - cx[k]))**2) / per**2 + \
               (plane - cv[k])**2 * 400.
        take = dist < best
        best[take], lab[take] = dist[take], k
    return lab, len(cz)


# ---- the cases -------------------------------------------------------------------------------------------------------------
def make_volume(dtype, shape, key=0, lo=None, hi=None):
    """noise on a ramp; floats reach below zero"""
    rng = np.random.RandomState([SEED, key] + list(shape) + [sum(ord(ch) for ch in dtype)])
    d, h, w = shape
    z, y, x = np.meshgrid(np.arange(d), np.arange(h), np.arange(w), indexing='ij')
    ramp = (z / max(d - 1., 1.) + y / max(h - 1., 1.) + 2 * x / max(w - 1., 1.)) / 4.
    v = 0.55 * ramp + 0.45 * rng.random_sample(shape)                              # [0, 1)
    if dtype == 'u8':
        return (v * 256).astype(np.uint8)
    if dtype == 'u16':
        return (v * 65536).astype(np.uint16)
    if dtype == 'i16':
        return (v * 65536 - 32768).astype(np.int16)
    lo, hi = (-0.15, 1.05) if lo is None else (lo, hi)
    return (lo + (hi - lo) * v).astype(np.float32 if dtype == 'f32' else np.float64)


def _case(name, volume, spacing, sigma=1., compactness=COMPACTNESS, **extra):
    volume.setflags(write=False)
    n = volume.size
    out = dict(id=name, volume=volume, spacing=tuple(float(s) for s in spacing), sigma=float(sigma), compactness=float(compactness),
               shape=volume.shape, dtype={'uint8': 'u8', 'float32': 'f32', 'float64': 'f64', 'uint16': 'u16', 'int16': 'i16'}[volume.dtype.name],
               n_segments=4 if n >= 64 else 1, three_pass=False)
    out.update(extra)
    return out


def _sp(rz, ry, rx):
    return tuple(SPACING_OF_RADIUS[r] for r in (rz, ry, rx))


def _f32(name, shape, radii, key=0, **extra):
    return _case(name, make_volume('f32', shape, key), _sp(*radii), **extra)


#: fast-path cases that run once more under IMSEGM_PRE_3PASS
BOTH_PATHS = ['yx00-3x33x65', 'yx13-3x33x65', 'yx24-3x33x65', 'yx44-3x33x65', 'small-2x3x5', 'chunk-33x5x8-r4']
NONF32_SPACINGS = [('r-1', (1., 1., 1.), 0.), ('r013', _sp(0, 1, 3), 1.), ('r4-8-16', _sp(4, 8, 16), 1.), ('r16-3-0', _sp(16, 3, 0), 1.),
                   ('r148', _sp(1, 4, 8), 1.)]


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    # float32, fast path: every (RY, RX), RZ cycling; W % 4 != 0: the scalar z pass
    for ry in range(5):
        for rx in range(5):
            rz = (ry * 5 + rx) % 5
            out.append(_f32('yx%d%d-3x33x65' % (ry, rx), (3, 33, 65), (rz, ry, rx), key=ry * 5 + rx))
    for rz in range(5):                                      # W % 4 == 0: the vector z pass
        out.append(_f32('z%d-3x33x64' % rz, (3, 33, 64), (rz, (rz + 2) % 5, (rz + 3) % 5)))
    for name, shape in [('small-1x1x1', (1, 1, 1)), ('slice-1x50x60', (1, 50, 60)), ('small-2x3x5', (2, 3, 5)), ('tile-9x32x64', (9, 32, 64)),
                        ('ragged-5x31x63', (5, 31, 63)), ('short-h-4x3x130', (4, 3, 130)), ('short-w-4x70x3', (4, 70, 3))]:
        out.append(_f32(name, shape, (4, 4, 4)))
    for shape in [(33, 5, 8), (35, 6, 12), (48, 4, 4), (31, 5, 8)]:
        for rz in (4, 1):
            out.append(_f32('chunk-%dx%dx%d-r%d' % (shape + (rz, )), shape, (rz, 4, 4), key=rz))
    # float32, three passes: radius 8 and 16
    for shape in [(5, 9, 40), (40, 5, 9), (5, 40, 9)]:
        for r in (8, 16):
            if shape == (5, 40, 9) and r == 16:
                continue
            out.append(_f32('r%d-%dx%dx%d' % ((r, ) + shape), shape, (r, r, r)))
    for name in BOTH_PATHS:
        base = [c for c in out if c['id'] == name][0]
        out.append(dict(base, id=name + '-3pass', three_pass=True))
    # every other dtype: the float64 plane
    for dtype in ('u8', 'f64', 'u16'):
        for shape in [(3, 33, 65), (7, 5, 37)]:
            for tag, spacing, sigma in NONF32_SPACINGS:
                out.append(_case('%s-%dx%dx%d-%s' % ((dtype, ) + shape + (tag, )), make_volume(dtype, shape), spacing, sigma))
    for dtype in ('u8', 'f64'):
        out.append(_case('%s-1x1x1' % dtype, make_volume(dtype, (1, 1, 1)), _sp(4, 8, 16)))
        out.append(_case('%s-2x3x5' % dtype, make_volume(dtype, (2, 3, 5)), _sp(4, 8, 16)))
    out.append(_case('f64-beyond-3x33x65', make_volume('f64', (3, 33, 65), 1, -0.2, 1.3), _sp(1, 4, 3)))
    out.append(_case('f64-compactness-0.05', make_volume('f64', (7, 5, 37), 2), _sp(3, 1, 4), compactness=0.05))
    # (beyond the list of the issue: the one dtype whose img_as_float offset is not zero -- `off` and `scale` in the right order)
    out.append(_case('i16-7x5x37', make_volume('i16', (7, 5, 37)), _sp(1, 4, 3)))
    # one session, two volumes
    out.append(_f32('reuse-f32', (6, 20, 37), (2, 4, 1), key=7))
    out.append(_case('reuse-f64', make_volume('f64', (6, 20, 37), 7), _sp(2, 4, 1)))
    assert len({c['id'] for c in out}) == len(out)
    assert all(c['volume'].size <= 150000 for c in out)
    return tuple(out)


def case(name):
    return {c['id']: c for c in cases()}[name]


def is_f32(c):
    return c['dtype'] == 'f32'


_REFERENCES = {}


def reference(name):
    """per case, once per process, read-only.  float64 plane: ``ref`` (longdouble), ``scale``, ``yardstick``, ``tol``.  float32
    plane: ``ref`` (float32), ``marked``, ``scale``, ``scipy`` (the yardstick's plane), ``yardstick`` = voxels of it that differ"""
    base = name[:-len('-3pass')] if name.endswith('-3pass') else name
    if base not in _REFERENCES:
        c = case(base)
        if is_f32(c):
            ref, marked = reference32(c)
            yard = yardstick32(c)
            differ = yard != ref
            # the builder's conditions, from the reference and scipy alone
            assert marked.mean() <= MARK_CAP, '%s: %d of %d voxels marked' % (base, marked.sum(), marked.size)
            assert not np.any(differ & ~marked), '%s: scipy differs from the reference outside the marked set' % base
            for a in (ref, marked, yard):
                a.setflags(write=False)
            _REFERENCES[base] = dict(ref=ref, marked=marked, scale=float(np.abs(ref).max()), scipy=yard, yardstick=int(differ.sum()),
                                     n_marked=int(marked.sum()))
        else:
            ref = reference64(c)
            ref.setflags(write=False)
            yard = rel_dev(yardstick64(c), ref)
            _REFERENCES[base] = dict(ref=ref, scale=float(np.abs(ref).max()), yardstick=yard, tol=max(FACTOR * yard, FLOOR))
    return _REFERENCES[base]


#: (id, dtype, shape, spacing, n_segments): W % 4 == 0 and != 0 (257, 33: a lane's quads straddle row ends), anisotropic, K = 2 .. ~400,
#: a volume of one slice
UPDATE_CASES = [('upd-f32-4x33x257-k400', 'f32', (4, 33, 257), (1., 1., 1.), 400), ('upd-f32-5x20x33-k40', 'f32', (5, 20, 33), (2., 1., 1.), 40),
                ('upd-f32-1x40x64-k30', 'f32', (1, 40, 64), (1., 1., 1.), 30), ('upd-f32-3x16x128-k2', 'f32', (3, 16, 128), (1., 1., 1.), 2),
                ('upd-f64-4x33x257-k400', 'f64', (4, 33, 257), (1., 1., 1.), 400), ('upd-f64-5x20x33-k40', 'f64', (5, 20, 33), (5., 1., 1.5), 40),
                ('upd-f64-1x40x64-k30', 'f64', (1, 40, 64), (1., 1., 1.), 30), ('upd-f64-3x16x128-k2', 'f64', (3, 16, 128), (1., 1., 1.), 2)]


@functools.lru_cache(maxsize=None)
def update_cases():
    return tuple(_case(name, make_volume(dtype, shape, 11), spacing, n_segments=k) for name, dtype, shape, spacing, k in UPDATE_CASES)


# ---- which cases a defect can show on: geometry, radii and dtype only ----------------------------------------------------------
DEFECTS = ['nearest', 'mirror', 'single-wrap', 'tap-dropped', 'chunk-seam', 'ahead-stale', 'extra-neighbour', 'row-dup', 'ragged',
           'shortcut-early', 'no-f32-store', 'ratio-double', 'off-after-scale']
UPDATE_DEFECTS = ['quad-dropped', 'pairwise']


def applies(c, defect):
    d, h, w = c['shape']
    rz, ry, rx = radii_of(c)
    f32 = is_f32(c)
    fast = f32 and fast_path(c) and not c['three_pass']
    if defect in BORDER_DEFECTS:                              # the rule maps some index of some filtered axis elsewhere
        return any(r > 0 and not np.array_equal(border(np.arange(-r, n + r), n, defect), border(np.arange(-r, n + r), n))
                   for n, r in zip((d, h, w), (rz, ry, rx)))
    if defect == 'tap-dropped':
        return 3 in (rz, ry, rx)
    if defect in ('chunk-seam', 'ahead-stale'):               # the window map of the z pass changes
        return fast and rz >= 0 and not np.array_equal(z_window_map(c['shape'], rz, defect), z_window_map(c['shape'], rz))
    if defect == 'extra-neighbour':                           # a written output of some tile reads a column >= 64 of A
        return fast and rx >= 1 and any(min(YX_TW, w - x0) + 2 * rx > YX_TW and
                                        not np.array_equal(border(x0 - rx + np.arange(YX_TW, min(YX_TW, w - x0) + 2 * rx) - 1, w),
                                                           border(x0 - rx + np.arange(YX_TW, min(YX_TW, w - x0) + 2 * rx), w))
                                        for x0 in range(0, w, YX_TW))
    if defect == 'row-dup':                                   # output row 31 of a tile exists (it reads row TH - 1 of A), and the
        th = YX_TH + 2 * max(ry, 0)                           # rows TH - 1 and TH - 2 of A are different rows of the slice
        return fast and any(y0 + YX_TH <= h and border(y0 - max(ry, 0) + th - 1, h) != border(y0 - max(ry, 0) + th - 2, h)
                            for y0 in range(0, h, YX_TH))
    if defect == 'ragged':
        return fast and bool(h % YX_TH or w % YX_TW)
    if defect == 'shortcut-early':
        return f32 and not fast and any(r >= 1 and 2 * r - 1 < n for n, r in zip((d, h, w), (rz, ry, rx)))
    if defect == 'no-f32-store':
        # the y pass really rounds (RY >= 1) and the x pass really sums (RX >= 1: with the single tap 1.0 its float32 store rounds the
        # double to the float32 the y pass would have stored); from 30 voxels: a 2^-25 relative change of the inputs moves the float32
        # rounding of a sum with probability ~ 1 / 4 per voxel
        return f32 and ry >= 1 and rx >= 1 and d * h * w >= 30
    if defect == 'ratio-double':                              # two roundings against one, float32(0.1) against 0.1
        return f32 and d * h * w >= 30
    if defect == 'off-after-scale':
        return not f32 and affine_of(c)[0] != 0
    raise ValueError(defect)
