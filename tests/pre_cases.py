"""Shared by tests/test_pre_reference_host.py and tests/test_gpu_pre_reference.py: the SLIC pre-processing of csrc/slic_pre.hip
(min / max, normalisation, sRGB -> XYZ -> Lab, Gaussian blur, 1 / compactness, premax) stated three times --

  ``reference80``  the definition of ``skimage.color.rgb2lab`` + ``scipy.ndimage.gaussian_filter(mode='reflect')`` + ``* (1 /
                   compactness)`` from the raw pixel in ``numpy.longdouble`` (64 mantissa bits), with the fp64 constants of
                   colorconv.py widened and the taps the host hands to the library widened;
  ``yardstick64``  the same definition in plain numpy / scipy float64 (``np.power(.., 2.4)``, ``np.cbrt``, ``gaussian_filter``): it
                   sizes the tolerance and nothing else;
  ``model64``      a float64 transcription of the device's own functions (det_cbrt, det_pow24, rgb2lab_px, zblur_point, the two
                   blur passes) in the kernel's operation order, with a ``defect=`` switch --

and the cases at which the kernels can go wrong: every blur radius class (none, 4, 5, 8 fused; 9, 16 three-pass), images smaller
than the radius, one tile, one pixel into the next tiles, every input type and normalisation arm, pixels at the two branch
thresholds, the image's extremes where only one code path of the min / max kernels sees them.  No expected number comes from the
device code.  float32 pixels are widened exactly and then treated like float64: that is this library's contract for float32 input
(what scikit-image does with float32 input is out of scope).

Deviation of a case: max |got - ref| over the three planes / S, S = max |ref| over the three planes (1 / compactness scales out).
Tolerance: 16 x (yardstick against the reference), floor 1e-14."""
import functools

import numpy as np

#: 64 mantissa bits (x87 extended); where ``longdouble`` is the platform's fp64 the reference is no reference
LONGDOUBLE_OK = bool(np.finfo(np.longdouble).nmant >= 63)
LONGDOUBLE_REASON = 'numpy.longdouble has %d mantissa bits here, 63 are needed' % np.finfo(np.longdouble).nmant

LD = np.longdouble
SEED = 20261018
FACTOR = 16              # the project's rule: 16 x what plain fp64 library code does on the same input
FLOOR = 1e-14            # about 90 units of 2^-53 relative to S: below that the yardstick of a tiny image is luck
COMPACTNESS = 10.
PF_TX, PF_TY, PF_MAXR = 64, 16, 8          # tile and largest radius of k_pre_fused

SRGB_T, LAB_T = 0.04045, 0.008856
RGB2XYZ = ((0.412453, 0.357580, 0.180423), (0.212671, 0.715160, 0.072169), (0.019334, 0.119193, 0.950227))
WHITE = (0.95047, 1.0, 1.08883)
GUARD = 1e-12            # no value of a case this close to a threshold it is compared with (see ``check_conditions``)

SIGMAS = [0., 1.0, 1.2, 2.0, 2.2, 4.0]                 # radius -1, 4, 5, 8 (last fused), 9 (first three-pass), 16 (largest)
FUSED_SIGMAS = [0., 1.0, 1.2, 2.0]
#: smaller than every radius; one row and one column into the next tiles; ragged on both axes with three tile columns
GRID_SHAPES = [(3, 5), (17, 65), (33, 130)]
OTHER_SHAPES = [(1, 1), (1, 70), (70, 1), (2, 2), (16, 64), (47, 129)]


def radius_of(sigma):
    return int(4.0 * sigma + 0.5) if sigma > 0 else -1


def taps_of(sigma):
    from pyimsegm_amd._hip import gaussian_taps
    return gaussian_taps(float(sigma))


def widen(image):
    """uint8 / float32 / float64 -> float64, exactly"""
    return np.asarray(image).astype(np.float64)


def scaled(normalize, vmin, vmax):
    return normalize == 1 or (normalize == 2 and not (vmin == 0 and vmax == 1))


# ---- the reference ---------------------------------------------------------------------------------------------------------
def reflect_index(i, n):
    """scipy's 'reflect' (d c b a | a b c d | d c b a) at any distance: period 2n"""
    i = np.asarray(i) % (2 * n)
    return np.where(i >= n, 2 * n - 1 - i, i)


def reflect_matrix(n, taps, dtype=LD):
    """n x n matrix of the 1-D correlation with the symmetric kernel whose half is ``taps`` (taps[0] = centre)"""
    taps = np.asarray(taps).astype(dtype)
    idx = np.arange(n)
    mat = np.zeros((n, n), dtype=dtype)
    for d in range(-(len(taps) - 1), len(taps)):
        mat[idx, reflect_index(idx + d, n)] += taps[abs(d)]         # (one column per row and d: no index repeats)
    return mat


def xyz_over_white80(image, normalize):
    """X / Xn, Y / Yn, Z / Zn [3, H, W] and the normalised channel values [H, W, 3], in longdouble from the raw pixel"""
    x = np.asarray(image).astype(LD)
    vmin, vmax = x.min(), x.max()
    if scaled(normalize, vmin, vmax):
        v = (x - vmin) / (vmax - vmin)
    elif np.asarray(image).dtype == np.uint8:
        v = x / LD(255)
    else:
        v = x
    above = v > LD(SRGB_T)
    base = np.where(above, (v + LD(0.055)) / LD(1.055), LD(1))
    lin = np.where(above, np.power(base, LD(12) / LD(5)), v / LD(12.92))
    xyz = [sum(LD(m) * lin[..., c] for c, m in enumerate(row)) / LD(w) for row, w in zip(RGB2XYZ, WHITE)]
    return np.array(xyz), v


def reference80(image, sigma, normalize, compactness=COMPACTNESS):
    """pre-processed planes [3, H, W] in longdouble"""
    t, _ = xyz_over_white80(image, normalize)
    above = t > LD(LAB_T)
    f = np.where(above, np.cbrt(np.where(above, t, LD(1))), LD(7.787) * t + LD(16. / 116.))
    lab = np.array([LD(116) * f[1] - LD(16), LD(500) * (f[0] - f[1]), LD(200) * (f[1] - f[2])])
    taps = taps_of(sigma)
    if taps is not None:
        lab = lab * reflect_matrix(1, taps)[0, 0]                            # the depth-1 z pass: every neighbour is the pixel
        lab = np.einsum('ij,cjk->cik', reflect_matrix(lab.shape[1], taps), lab)    # y
        lab = np.einsum('cik,lk->cil', lab, reflect_matrix(lab.shape[2], taps))    # then x
    return lab * (LD(1) / LD(compactness))


def yardstick64(image, sigma, normalize, compactness=COMPACTNESS):
    """the same definition with numpy's and scipy's own float64 functions"""
    from scipy import ndimage
    image = np.asarray(image)
    x = widen(image)
    vmin, vmax = x.min(), x.max()
    if scaled(normalize, vmin, vmax):
        v = (x - vmin) / (vmax - vmin)
    elif image.dtype == np.uint8:
        v = x / 255.
    else:
        v = x
    above = v > SRGB_T
    lin = np.where(above, np.power(np.where(above, (v + 0.055) / 1.055, 1.), 2.4), v / 12.92)
    t = np.array([(lin @ np.array(row)) / w for row, w in zip(RGB2XYZ, WHITE)])
    above = t > LAB_T
    f = np.where(above, np.cbrt(np.where(above, t, 1.)), 7.787 * t + 16. / 116.)
    lab = np.array([116. * f[1] - 16., 500. * (f[0] - f[1]), 200. * (f[1] - f[2])])
    if sigma > 0:
        lab = np.array([ndimage.gaussian_filter(p[None], sigma, mode='reflect')[0] for p in lab])
    return lab * (1. / compactness)


def rel_dev(got, ref):
    """max |got - ref| over the three planes / max |ref|, in longdouble, as a float"""
    ref = np.asarray(ref).astype(LD)
    return float(np.max(np.abs(np.asarray(got).astype(LD) - ref)) / np.max(np.abs(ref)))


# ---- the device's functions in float64 numpy, operation for operation --------------------------------------------------------
def det_cbrt(x):
    x = np.ascontiguousarray(x, dtype=np.float64)
    y = (np.int64(0x553ef0ff289dd796) - x.view(np.int64) // 3).view(np.float64)          # (x > 0: floor is C's truncation)
    third = 1.0 / 3.0
    for _ in range(5):
        y3 = y * y * y
        r = 1.0 - x * y3
        y = y + y * (r * third)
    yy = y * y
    c = x * yy
    e = c * c * c - x
    return c - e * (yy * third)


def det_pow24(t):
    t = np.ascontiguousarray(t, dtype=np.float64)
    y = (np.int64(0x4cb8a8c154c985f0) - t.view(np.int64) // 5).view(np.float64)
    for _ in range(5):
        y2 = y * y
        y5 = y2 * y2 * y
        r = 1.0 - t * y5
        y = y + y * (r * 0.2)
    p = t * y
    return p * p * p


def ulp_error(got, exact):
    """largest |got - exact| in units of the fp64 spacing at ``exact``"""
    exact = np.asarray(exact, dtype=LD)
    return float(np.max(np.abs(np.asarray(got).astype(LD) - exact) / np.spacing(np.abs(exact).astype(np.float64)).astype(LD)))


@functools.lru_cache(maxsize=None)
def function_ulps(count=200000):
    """measured on the domains the pre-processing uses -- cbrt on (0.008856, 1.2], x^2.4 on [(0.04045 + 0.055) / 1.055, 1.3] -- at
    ``count`` seeded points each plus the 256 uint8 levels: {'det_cbrt', 'np.cbrt', 'det_pow24', 'np.power'} in ulp"""
    rng = np.random.RandomState(SEED)
    levels = np.arange(256) / 255.
    tc = np.concatenate([np.exp(rng.uniform(np.log(LAB_T), np.log(1.2), count)), levels[levels > LAB_T]])
    tc = tc[tc > LAB_T]
    tp = np.concatenate([rng.uniform((SRGB_T + 0.055) / 1.055, 1.3, count), (levels[levels > SRGB_T] + 0.055) / 1.055])
    exact_c, exact_p = np.cbrt(tc.astype(LD)), np.power(tp.astype(LD), LD(12) / LD(5))
    return {'det_cbrt': ulp_error(det_cbrt(tc), exact_c), 'np.cbrt': ulp_error(np.cbrt(tc), exact_c),
            'det_pow24': ulp_error(det_pow24(tp), exact_p), 'np.power': ulp_error(np.power(tp, 2.4), exact_p)}


#: what the construction allows.  det_cbrt: c = x y^2 carries the error of y (Newton's fixed point, about 1 ulp) twice; the final
#: step removes it to second order and leaves its own rounding: the correction e (yy / 3) is tiny, so the subtraction rounds once
#: (0.5 ulp) on top of a residual below 0.5 ulp.  det_pow24: y = t^(-1/5) sits within about 1.5 ulp of its fixed point, p = t y adds
#: 0.5, the cube triples that relative error and adds two roundings: 3 x 2 + 1 = 7.
ULP_BOUND = {'det_cbrt': 1.0, 'det_pow24': 7.0}

DEFECTS = ['nearest', 'mirror', 'single-wrap', 'n1', 'tap-dropped', 'halo-channel', 'seam', 'ragged', 'ge-srgb', 'linear-all',
           'no-scale', 'scale-01', 'lut-clamp', 'min-no-tail', 'max-no-last-vector', 'ratio-early']
#: restatements that must NOT change a bit (the n == 1 return of reflect_idx is a shortcut: the period-2n arithmetic gives 0 for
#: n = 1 anyway; the uint8 wrap of the LUT index is unreachable, v >= vmin), and a permitted reordering that must stay inside
HARMLESS_EQUAL = ['n1', 'lut-clamp']
HARMLESS_INSIDE = ['ratio-early']


def border_index(i, n, defect=None):
    """reflect_idx of slic_pre.hip; with a defect: another border rule"""
    i = np.asarray(i)
    if defect == 'nearest':
        return np.clip(i, 0, n - 1)
    if defect == 'mirror':                                  # whole-sample symmetric: d c b | a b c d | c b a
        if n == 1:
            return np.zeros_like(i)
        i = i % (2 * n - 2)
        return np.where(i >= n, 2 * n - 2 - i, i)
    if defect == 'single-wrap':                             # one reflection, no modulo; what is still outside is clamped
        i = np.where(i < 0, -1 - i, np.where(i >= n, 2 * n - 1 - i, i))
        return np.clip(i, 0, n - 1)
    if n == 1 and defect != 'n1':
        return np.zeros_like(i)
    return reflect_index(i, n)


def device_minmax(image, defect=None):
    """what k_minmax / k_minmax_u8 hand on, as float64; the two defects leave out what one code path of k_minmax_u8 covers"""
    flat = widen(image).ravel()
    lo = hi = flat
    if np.asarray(image).dtype == np.uint8:
        nvec = flat.size // 16
        if defect == 'min-no-tail' and nvec:
            lo = flat[:16 * nvec]
        if defect == 'max-no-last-vector' and nvec:
            hi = np.concatenate([flat[:16 * (nvec - 1)], flat[16 * nvec:]])
    return float(lo.min()), float(hi.max())


def minmax_route(image, element):
    """which code path of the min / max kernel of launch_minmax reads flat element ``element``: 'vector' / 'last-vector' / 'tail'
    for uint8 (16-byte lanes, the byte tail of workgroup 0), 'unrolled' / 'remainder' for the float kernels' loop by four"""
    image = np.asarray(image)
    n = image.size
    if image.dtype == np.uint8:
        nvec = n // 16
        return 'tail' if element >= 16 * nvec else ('last-vector' if element >= 16 * (nvec - 1) else 'vector')
    stride = 256 * max(1, min(128, (n + 4095) // 4096))
    first = element % stride + (element // (4 * stride)) * 4 * stride               # where that thread's round begins
    return 'unrolled' if first + 3 * stride < n else 'remainder'


def lab_z64(image, sigma, normalize, defect=None):
    """first stage of the device: normalise, rgb2lab_px (uint8: through the 256-entry table), zblur_point -> [3, H, W]"""
    image = np.asarray(image)
    vmin, vmax = device_minmax(image, defect)
    norm = scaled(normalize, vmin, vmax)
    if defect == 'no-scale':
        norm = False
    if defect == 'scale-01':
        norm = True

    def linearise(v):
        above = (v >= SRGB_T) if defect == 'ge-srgb' else (v > SRGB_T)
        return np.where(above, det_pow24(np.where(above, (v + 0.055) / 1.055, 1.)), v / 12.92)

    if image.dtype == np.uint8:
        levels = np.arange(256)
        if norm:
            diff = levels - int(vmin)
            index = np.clip(diff, 0, 255) if defect == 'lut-clamp' else diff & 255
            x = index.astype(np.float64) / (vmax - vmin)
        else:
            x = levels.astype(np.float64) * (1.0 / 255)
        lin = linearise(x)[image]
    else:
        v = widen(image)
        if norm:
            v = (v - vmin) / (vmax - vmin)
        lin = linearise(v)
    m = RGB2XYZ
    xyz = [lin[..., 0] * m[r][0] + lin[..., 1] * m[r][1] + lin[..., 2] * m[r][2] for r in range(3)]
    f = []
    for t in (xyz[0] / 0.95047, xyz[1] / 1.0, xyz[2] / 1.08883):
        above = np.zeros(t.shape, bool) if defect == 'linear-all' else (t > LAB_T)
        f.append(np.where(above, det_cbrt(np.where(above, t, 1.)), 7.787 * t + 16.0 / 116.0))
    lab = np.array([(116.0 * f[1]) - 16.0, 500.0 * (f[0] - f[1]), 200.0 * (f[1] - f[2])])
    taps = taps_of(sigma)
    if taps is None:
        return lab
    last = len(taps) - 1 - (1 if defect == 'tap-dropped' else 0)
    tmp = lab * taps[0]
    for j in range(last, 0, -1):
        tmp = tmp + (lab + lab) * taps[j]
    return tmp


def blur_yx64(planes, sigma, ratio, defect=None):
    """the y pass, the x pass and ``* ratio`` the way k_pre_fused / k_blur_axis evaluate them"""
    taps = taps_of(sigma)
    _, h, w = planes.shape
    out = planes
    if taps is not None:
        last = len(taps) - 1 - (1 if defect == 'tap-dropped' else 0)
        rows, cols = np.arange(h), np.arange(w)
        acc = out * taps[0]
        for j in range(last, 0, -1):
            a, b = out[:, border_index(rows - j, h, defect)], out[:, border_index(rows + j, h, defect)]
            if defect == 'halo-channel' and j == len(taps) - 1:          # top halo row of every tile: the next channel's row
                top = rows % PF_TY == 0
                a = np.where(top[None, :, None], np.roll(a, -1, axis=0), a)
            acc = acc + (a + b) * taps[j]
        out = acc
        if defect == 'ratio-early':
            out = out * ratio
        acc = out * taps[0]
        for j in range(last, 0, -1):
            acc = acc + (out[:, :, border_index(cols - j, w, defect)] + out[:, :, border_index(cols + j, w, defect)]) * taps[j]
        out = acc
    if not (defect == 'ratio-early' and taps is not None):
        out = out * ratio
    return out


def model64(image, sigma, normalize, compactness=COMPACTNESS, defect=None):
    """the device's planes [3, H, W] in float64 numpy, with one ``defect`` or none"""
    ratio = 1.0 / compactness
    planes = lab_z64(image, sigma, normalize, defect)
    out = blur_yx64(planes, sigma, ratio, defect)
    _, h, w = out.shape
    if defect == 'seam' and w > PF_TX:                       # input column 64 read as column 63 by the outputs right of the seam
        moved = np.array(planes)
        moved[:, :, PF_TX] = moved[:, :, PF_TX - 1]
        out = np.array(out)
        out[:, :, PF_TX:] = blur_yx64(moved, sigma, ratio)[:, :, PF_TX:]
    if defect == 'ragged':                                   # the last ragged row / column of the tile grid not written
        out = np.array(out)
        if h % PF_TY:
            out[:, h - 1, :] = 0.
        if w % PF_TX:
            out[:, :, w - 1] = 0.
    return out


# ---- the cases -------------------------------------------------------------------------------------------------------------
def _rng(*key):
    return np.random.RandomState([SEED] + [int(k) for k in key])


def _pin(image, lo, hi):
    """first element ``lo``, last element ``hi`` (both inside the value range of the rest)"""
    flat = image.reshape(-1)
    flat[0], flat[-1] = lo, hi
    return image


def make_image(kind, shape, key=0):
    """seeded H x W x 3 image of one of the input kinds"""
    h, w = shape
    rng = _rng(h, w, key, sum(ord(ch) for ch in kind))
    full = (h, w, 3)
    ftype = np.float32 if kind.startswith('f32') else np.float64
    if kind == 'u8-full':                       # 0 .. 255: scaled by (v - 0) / 255
        return _pin(rng.randint(0, 256, full).astype(np.uint8), 0, 255)
    if kind == 'u8-mid':                        # 37 .. 201: the table under normalisation with vmin > 0
        return _pin(rng.randint(37, 202, full).astype(np.uint8), 37, 201)
    if kind == 'u8-01':                         # {0, 1}: min == 0 and max == 1, no scaling, v / 255
        return _pin(rng.randint(0, 2, full).astype(np.uint8), 0, 1)
    if kind == 'u8-raw':                        # normalize = 0
        return _pin(rng.randint(3, 250, full).astype(np.uint8), 3, 249)
    if kind in ('f64-unit', 'f32-unit'):        # [0, 1] with min exactly 0 and max exactly 1: no scaling under normalize = 2
        return _pin(rng.random_sample(full).astype(ftype), 0, 1)
    if kind in ('f64-wide', 'f32-wide'):        # [-1, 2], normalize = 1
        return _pin((rng.random_sample(full) * 3 - 1).astype(ftype), -1, 2)
    if kind in ('f64-beyond', 'f32-beyond'):    # [-0.2, 1.3], normalize = 0: negative (linear arm) and beyond white
        return _pin((rng.random_sample(full) * 1.5 - 0.2).astype(ftype), ftype(-0.2), ftype(1.3))
    if kind == 'gray':                          # R = G = B
        return np.repeat(rng.random_sample((h, w, 1)), 3, axis=2)
    raise ValueError(kind)


NORMALIZE_OF = {'u8-full': 2, 'u8-mid': 2, 'u8-01': 2, 'u8-raw': 0, 'f64-unit': 2, 'f32-unit': 2, 'f64-wide': 1, 'f32-wide': 1,
                'f64-beyond': 0, 'f32-beyond': 0, 'gray': 0}


def block_image():
    """16 x 16 blocks: every one of the 256 levels occurs in every channel (the whole table is read)"""
    rng = _rng(256)
    return np.stack([rng.permutation(256).astype(np.uint8).reshape(16, 16) for _ in range(3)], axis=2)


def threshold_image():
    """float64, normalize = 0, no blur (pixels independent): channel values at 0.04045, its two fp64 neighbours and 1e-3 to either
    side, alone and mixed with other channels; dark pixels whose Y lands in [0.0088, 0.0089] on both sides of 0.008856; black, white"""
    t = SRGB_T
    values = [np.nextafter(t, 0.), t, np.nextafter(t, 1.), t - 1e-3, t + 1e-3]
    pixels = [(v, v, v) for v in values] + [(v, 0.5, 0.2) for v in values] + [(0.7, v, 0.01) for v in values] + \
             [(0.3, 0.9, v) for v in values]
    for y in (0.00880, 0.00884, 0.008855, 0.008857, 0.00887, 0.00890):
        g = 1.055 * y**(1 / 2.4) - 0.055                     # gray: X / Xn, Y and Z / Zn all next to the threshold
        pixels += [(g, g, g), (g + 0.03, g - 0.005, g - 0.02), (0., g * 1.16, 0.)]
    pixels += [(0., 0., 0.), (1., 1., 1.)]
    return np.array(pixels, dtype=np.float64).reshape(4, 10, 3)


def threshold_image_u8():
    """uint8, normalize = 0: (1, 0, 0) has the smallest non-zero Z of a uint8 image (5.9e-6), (0, 0, 1) the smallest X; levels 10 and
    11 lie on the two sides of 0.04045 x 255 = 10.3; black and white"""
    pixels = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 0, 0), (255, 255, 255), (10, 10, 10), (11, 11, 11), (10, 11, 200), (24, 24, 24),
              (25, 25, 25)]
    return np.array(pixels, dtype=np.uint8).reshape(2, 5, 3)


def extreme_image(dtype, shape, at_min, at_max):
    """mid-gray with exactly one minimum and one maximum channel value, at flat elements ``at_min`` / ``at_max`` (negative: from the
    end): a wrong minimum or maximum changes every output pixel"""
    h, w = shape
    if dtype == 'u8':
        image = np.full((h, w, 3), 128, np.uint8)
        lo, hi = 3, 250
    else:
        image = np.full((h, w, 3), 0.5, np.float32)
        lo, hi = np.float32(-0.75), np.float32(1.625)
    flat = image.reshape(-1)
    flat[at_min], flat[at_max] = lo, hi
    return image


def corner_image():
    """17 x 65 uint8, mid-gray with a pure-blue pixel in the last corner (the one pixel of the last ragged tile): its B value, about
    -107.9, is the largest |value| of the three planes and negative"""
    image = np.full((17, 65, 3), 128, np.uint8)
    image[0, 0] = (0, 0, 0)
    image[-1, -1] = (0, 0, 255)
    return image


def _case(name, image, sigma, normalize, compactness=COMPACTNESS, **extra):
    image.setflags(write=False)
    out = dict(id=name, image=image, sigma=float(sigma), normalize=int(normalize), compactness=float(compactness),
               shape=image.shape[:2], dtype={'uint8': 'u8', 'float32': 'f32', 'float64': 'f64'}[image.dtype.name], extremes=None)
    out.update(extra)
    return out


def _extreme_cases():
    """(dtype, shape, element of the minimum, element of the maximum, routes expected of (minimum, maximum))"""
    plan = [
        # n = 81: n % 16 = 1, the tail is the last element alone
        ('u8', (3, 9), 0, -1, ('vector', 'tail')), ('u8', (3, 9), -1, 0, ('tail', 'vector')),
        ('u8', (3, 9), 70, 66, ('last-vector', 'last-vector')),
        # n = 63: n % 16 = 15, elements 48 .. 62 are the tail, 32 .. 47 the last vector
        ('u8', (3, 7), 49, 40, ('tail', 'last-vector')), ('u8', (3, 7), 33, 61, ('last-vector', 'tail')),
        # n = 12 870: four workgroups, 804 vectors, a 6-byte tail that workgroup 0 alone reads
        ('u8', (33, 130), 12866, 12860, ('tail', 'last-vector')), ('u8', (33, 130), 12850, 12869, ('last-vector', 'tail')),
        # float32: n = 81 (no unrolled round at all), n = 3 315 (elements from 3 072 on), n = 12 870 (from 12 288 on)
        ('f32', (3, 9), 0, -1, ('remainder', 'remainder')),
        ('f32', (17, 65), 0, -1, ('unrolled', 'remainder')), ('f32', (17, 65), 3200, 1500, ('remainder', 'unrolled')),
        ('f32', (33, 130), 12300, 0, ('remainder', 'unrolled')), ('f32', (33, 130), 12287, -1, ('unrolled', 'remainder')),
    ]
    out = []
    for dtype, shape, at_min, at_max, routes in plan:
        image = extreme_image(dtype, shape, at_min, at_max)
        where = tuple(e % image.size for e in (at_min, at_max))
        assert tuple(minmax_route(image, e) for e in where) == routes, (dtype, shape, at_min, at_max)
        out.append(_case('extreme-%s-%dx%d-min%d-max%d' % (dtype, shape[0], shape[1], where[0], where[1]), image, 1.0, 1,
                         extremes=dict(at_min=where[0], at_max=where[1], routes=routes)))
    return out


@functools.lru_cache(maxsize=None)
def cases():
    """every case, built once; images are read-only"""
    out = []
    grid_kind = {'u8': 'u8-full', 'f32': 'f32-unit', 'f64': 'f64-beyond'}
    for shape in GRID_SHAPES:                   # every radius class x the three dtypes
        for sigma in SIGMAS:
            for dtype, kind in grid_kind.items():
                out.append(_case('grid-%dx%d-s%g-%s' % (shape + (sigma, dtype)), make_image(kind, shape), sigma, NORMALIZE_OF[kind]))
    for i, shape in enumerate(OTHER_SHAPES):    # the other shapes: a fused and a three-pass radius each, dtypes in rotation
        for j, sigma in enumerate((1.0, 2.0, 4.0)):
            kind = ['u8-mid', 'f64-wide', 'f32-beyond'][(i + j) % 3]
            out.append(_case('shape-%dx%d-s%g-%s' % (shape + (sigma, kind)), make_image(kind, shape, 1), sigma, NORMALIZE_OF[kind]))
    for kind in sorted(NORMALIZE_OF):           # every input kind and normalisation arm: r = 5 (fused) and r = 9 (three-pass)
        out.append(_case('kind-%s-17x65-s1.2' % kind, make_image(kind, (17, 65), 2), 1.2, NORMALIZE_OF[kind], gray=kind == 'gray'))
        out.append(_case('kind-%s-33x130-s2.2' % kind, make_image(kind, (33, 130), 2), 2.2, NORMALIZE_OF[kind], gray=kind == 'gray'))
    out.append(_case('blocks-16x16-s1', block_image(), 1.0, 2))
    out.append(_case('blocks-16x16-s2.2', block_image(), 2.2, 2))
    out.append(_case('threshold-f64', threshold_image(), 0., 0))
    out.append(_case('threshold-u8', threshold_image_u8(), 0., 0))
    out += _extreme_cases()
    out.append(_case('corner-negative-b', corner_image(), 0., 2, corner=True))
    out.append(_case('compactness-0.05', make_image('u8-full', (17, 65), 3), 1.0, 2, compactness=0.05))
    # one session, two images: the extremes of the second lie inside those of the first
    out.append(_case('reuse-first', make_image('u8-full', (17, 65), 4), 1.0, 2))
    out.append(_case('reuse-second', make_image('u8-mid', (17, 65), 4), 1.0, 2))
    for c in out:
        check_conditions(c)
    assert len({c['id'] for c in out}) == len(out)
    return tuple(out)


def case(name):
    return {c['id']: c for c in cases()}[name]


def check_conditions(c):
    """decided by the reference alone: no normalised channel value of a NORMALISED case within 1e-12 of 0.04045 (a raw value may sit
    on it: both sides compare the same fp64 number), no X / Xn, Y, Z / Zn of any case within 1e-12 of 0.008856 (a computed value: the
    two formulas meet to about 1e-7 only, so a pixel there may legitimately take either branch); extremes unique where they are placed"""
    t, v = xyz_over_white80(c['image'], c['normalize'])
    x = np.asarray(c['image']).astype(LD)
    if scaled(c['normalize'], x.min(), x.max()) or c['dtype'] == 'u8':
        assert float(np.min(np.abs(v - LD(SRGB_T)))) > GUARD, c['id']
    assert float(np.min(np.abs(t - LD(LAB_T)))) > GUARD, c['id']
    if c['extremes']:
        flat = c['image'].ravel()
        assert np.sum(flat == flat.min()) == 1 and np.sum(flat == flat.max()) == 1
        assert flat.argmin() == c['extremes']['at_min'] and flat.argmax() == c['extremes']['at_max']
    if c.get('corner'):
        ref = _reference_of(c)['ref']
        h, w = c['shape']
        assert float(ref[2, h - 1, w - 1]) < 0 and float(np.abs(ref).max()) == float(-ref[2, h - 1, w - 1])
        assert (h - 1) % PF_TY == 0 and (w - 1) % PF_TX == 0


_REFERENCES = {}


def reference(name):
    """per case, computed once per process and read-only: ``ref`` (longdouble planes), ``scale`` S, ``yardstick`` (fp64 library code
    against the reference), ``tol``"""
    if name not in _REFERENCES:
        _REFERENCES[name] = _reference_of(case(name))
    return _REFERENCES[name]


def _reference_of(c):
    ref = reference80(c['image'], c['sigma'], c['normalize'], c['compactness'])
    ref.setflags(write=False)
    yard = rel_dev(yardstick64(c['image'], c['sigma'], c['normalize'], c['compactness']), ref)
    return dict(ref=ref, scale=float(np.abs(ref).max()), yardstick=yard, tol=max(FACTOR * yard, FLOOR))


def n_segments_of(c):
    """K = 1 .. 4 centroids"""
    return 4 if c['shape'][0] * c['shape'][1] >= 64 else 1


def applies(c, defect):
    """the cases a defect can show on, decided by geometry, dtype and the reference's own values -- never by a kernel's output"""
    h, w = c['shape']
    r = radius_of(c['sigma'])
    image = c['image']
    x = widen(image)
    vmin, vmax = float(x.min()), float(x.max())
    norm = scaled(c['normalize'], vmin, vmax)
    if defect in ('nearest', 'mirror', 'single-wrap'):          # the border rule maps some index elsewhere
        return any(not np.array_equal(border_index(np.arange(-r, n + r), n, defect), border_index(np.arange(-r, n + r), n))
                   for n in (h, w)) if r > 0 else False
    if defect == 'tap-dropped':
        return r in (5, 8)
    if defect == 'halo-channel':
        return r > 0
    if defect == 'seam':                                        # (the flat images of the extremes: columns 63 and 64 are equal)
        return w > PF_TX and not c['extremes']
    if defect == 'ragged':
        return bool(h % PF_TY or w % PF_TX)
    if defect == 'ge-srgb':                                     # a channel value exactly on the threshold
        return bool(np.any(xyz_over_white80(image, c['normalize'])[1] == LD(SRGB_T)))
    if defect == 'linear-all':
        return bool(np.any(xyz_over_white80(image, c['normalize'])[0] > LD(LAB_T)))
    if defect == 'no-scale':                                    # scaling that changes values by more than a rounding
        return norm and (vmin, vmax) != ((0., 255.) if c['dtype'] == 'u8' else (0., 1.))
    if defect == 'scale-01':
        return c['dtype'] == 'u8' and not norm and c['normalize'] == 2
    if defect == 'min-no-tail':
        return bool(c['extremes']) and c['dtype'] == 'u8' and c['extremes']['routes'][0] == 'tail'
    if defect == 'max-no-last-vector':
        return bool(c['extremes']) and c['dtype'] == 'u8' and c['extremes']['routes'][1] == 'last-vector'
    return True                                                 # n1, lut-clamp, ratio-early: every case
