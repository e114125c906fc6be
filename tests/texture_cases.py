"""Shared by tests/test_texture_reference_host.py and tests/test_gpu_texture_reference.py: an 80-bit (``numpy.longdouble``)
restatement of the Leung-Malik stage -- the sigma = 150 high-pass, the responses of a filter battery (true convolution, scipy's
'reflect' border at any distance, maximum over the kernels, upper-side clip), the sum of squares and the statistics of the
normalised response -- and the batteries, routes and shapes at which every kernel instantiation of csrc/texture.hip is reached.
No expected number comes from the device code; scipy's own fp64 deviation from the reference is the yardstick of the tolerances.

Routes (how the Python layer reaches a kernel; argued from ``Image2D._pack_bank`` and the dispatch of ``launch_battery_dense`` /
``launch_battery_sep``, asserted per case by both test modules):
  'battery'   ``lm_battery``: everything dense, padded to 1 / 2 / 4 / 8 kernels, parity 0 -> ``k_conv_battery<NK>``
  'features'  ``lm_features([battery])``: ONE battery, so its response lies at the start of the response buffer and
              ``get_response()`` returns it.  The split (kernels, parity, groups, rank) picks the kernels: parity 0 ->
              ``k_conv_battery<kernels>``, +-1 -> ``k_conv_battery_sym<kernels>``, +-2 -> ``k_conv_battery_quad<kernels / 2, 16>``;
              groups > 0 -> side 33: ``k_sep_battery_tall`` (``wide``: ``k_sep_battery<33>``), another side: ``k_sep_battery<0>``."""
import functools

import numpy as np

#: x87 extended precision (eps 1.08e-19); where ``longdouble`` is the fp64 of the platform the reference is no reference
LONGDOUBLE_OK = bool(np.finfo(np.longdouble).eps < 1e-18)
LONGDOUBLE_REASON = 'numpy.longdouble is not an 80-bit format here (eps %.3g)' % float(np.finfo(np.longdouble).eps)

LD = np.longdouble

SEED = 20261018

#: crosses the 96-row seam of the tall tile (16 x 96), the 64-column seam of the dense tiles (64 x 16), several 16-row and 16-column
#: seams, ragged on both axes
SHAPE = (113, 83)
#: narrower than the kernel radius on one axis (the reflected border is crossed more than once); one row (reflect_index's n == 1);
#: exactly one dense tile; exactly one tall tile
BORDER_SHAPES = [(9, 150), (97, 7), (1, 70), (16, 64), (96, 16)]

#: colour images of the high-pass test: (shape, dtype); see tests/test_gpu_texture_reference.py for what each one crosses
HIGHPASS_IMAGES = [((70, 131), 'u8'), ((5, 203), 'f32'), ((131, 67), 'f64'), ((1, 40), 'u8'), ((33, 1300), 'u8')]
#: volumes (slices independent, no channel pass): 6068 voxels (not divisible by 3); D = 1; D = 2
HIGHPASS_VOLUMES = [((4, 41, 37), 'u8'), ((1, 20, 90), 'f64'), ((2, 70, 19), 'f32')]

FLOOR = 1e-13            # 1089 terms of unit-L1 weights in fp64: 1089 x 1.1e-16 = 1.2e-13, whatever the order of the sum
FACTOR = 16              # another order of the sums (the project's rule)


def noise(shape, dtype, seed=SEED):
    """seeded noise, every tap matters: uint8 0 .. 255, or standard normal x 40 as float32 / float64"""
    rng = np.random.RandomState([seed] + list(shape))
    if dtype == 'u8':
        return rng.randint(0, 256, shape).astype(np.uint8)
    return (rng.standard_normal(shape) * 40).astype({'f32': np.float32, 'f64': np.float64}[dtype])


# ---- the reference ---------------------------------------------------------------------------------------------------------
def shifted_sum(planes, flipped, pad_mode='symmetric', dtype=LD):
    """sum_{a, b} flipped[a, b] * padded[..., y + a, x + b]: the correlation with ``flipped`` (odd sides, square or not) as shifted
    additions over a padded copy; ``pad_mode`` of numpy.pad ('symmetric' is scipy's 'reflect') at any distance"""
    planes = np.asarray(planes)
    weights = np.atleast_2d(np.asarray(flipped)).astype(dtype)
    ra, rb = weights.shape[0] // 2, weights.shape[1] // 2
    h, w = planes.shape[-2:]
    padded = np.pad(planes.astype(dtype), [(0, 0)] * (planes.ndim - 2) + [(ra, ra), (rb, rb)], mode=pad_mode)
    out = np.zeros(planes.shape, dtype=dtype)
    for a in range(weights.shape[0]):
        for b in range(weights.shape[1]):
            if weights[a, b] != 0:
                out += weights[a, b] * padded[..., a:a + h, b:b + w]
    return out


def conv80(planes, kernel):
    """true convolution of every plane with ``kernel`` (odd side), scipy's 'reflect' border, in longdouble"""
    return shifted_sum(planes, np.asarray(kernel)[::-1, ::-1])


def clip_upper(resp, clip):
    return np.where(resp > clip, np.asarray(clip, dtype=resp.dtype), resp)


def response80(planes, battery, clip):
    """maximum over the kernels of the battery, then the clip of the upper side (descriptors.py: ``response[response > clip] = clip``)"""
    return clip_upper(np.max([conv80(planes, k) for k in battery], axis=0), clip)


def sumsq80(resp):
    x = np.asarray(resp).astype(LD)
    return np.sum(x * x)


def reflect_matrix(n, taps):
    """n x n longdouble matrix of the 1-D correlation with the symmetric kernel whose half is ``taps`` (taps[0] = centre), border
    'reflect' at any distance"""
    taps = np.asarray(taps).astype(LD)
    r = len(taps) - 1
    idx = np.arange(n)
    mat = np.zeros((n, n), dtype=LD)
    for d in range(-r, r + 1):
        j = (idx + d) % (2 * n)
        j = np.where(j >= n, 2 * n - 1 - j, j)
        mat[idx, j] += taps[abs(d)]             # (one column per row and d: no index repeats within the statement)
    return mat


def highpass80(image, sigma=150., channel_pass=True):
    """``image - gaussian_filter(image.astype(float), sigma)`` in longdouble from the taps the host hands to ``lm_prepare``.
    H x W x 3 image: all three axes (the 3-element channel axis too), returned as planes [3, H, W]"""
    from pyimsegm_amd._hip import gaussian_taps
    taps = gaussian_taps(float(sigma))
    x = np.asarray(image).astype(LD)
    blur = np.tensordot(reflect_matrix(x.shape[0], taps), x, axes=(1, 0))
    blur = np.tensordot(reflect_matrix(x.shape[1], taps), blur, axes=(1, 1)).transpose(1, 0, 2)
    if channel_pass:
        blur = np.tensordot(blur, reflect_matrix(x.shape[2], taps), axes=(2, 1))
    return np.ascontiguousarray(np.rollaxis(x - blur, -1, 0))


def highpass80_volume(volume, sigma=150.):
    """slice by slice, the two in-plane axes only (image_subtract_gauss_smooth): [D, H, W]"""
    from pyimsegm_amd._hip import gaussian_taps
    taps = gaussian_taps(float(sigma))
    x = np.asarray(volume).astype(LD)
    my, mx = reflect_matrix(x.shape[1], taps), reflect_matrix(x.shape[2], taps)
    blur = np.einsum('ij,djk->dik', my, x)
    blur = np.einsum('dik,lk->dil', blur, mx)
    return x - blur


def highpass_scipy(image):
    from scipy import ndimage
    image = np.asarray(image)
    return np.rollaxis(image - ndimage.gaussian_filter(image.astype(float), 150), -1, 0)


def highpass_scipy_volume(volume):
    from scipy import ndimage
    volume = np.asarray(volume)
    return volume - np.array([ndimage.gaussian_filter(plane.astype(float), 150) for plane in volume])


def rel_dev(got, ref, scale):
    """max |got - ref| / scale in longdouble, as a float"""
    return float(np.max(np.abs(np.asarray(got).astype(LD) - ref)) / LD(scale)) if np.size(ref) else 0.


def rule(reference_deviation):
    """the tolerance: 16 x the fp64 yardstick's own deviation from the reference, floor 1e-13"""
    return max(FACTOR * reference_deviation, FLOOR)


def stats80(resp, norm):
    """(mean, energy) per channel over ALL pixels (one label) of the normalised response as stats.hip stages it: the value
    ``(r * (log(1 + norm) / 0.03)) / norm`` rounded to float32, squares in float32, sums exact (here: longdouble); and ``mul``"""
    norm = LD(norm)
    mul = np.log(1 + norm) / LD(0.03)
    v32 = ((np.asarray(resp).astype(LD) * mul) / norm).astype(np.float32)
    flat = v32.reshape(v32.shape[0], -1)
    mean = flat.astype(LD).sum(axis=1) / flat.shape[1]
    energy = (flat * flat).astype(LD).sum(axis=1) / flat.shape[1]
    return mean, energy, float(mul)


# ---- batteries and cases ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def banks():
    """the banks the cases draw from, built once (read-only): 'normal' (8 orientations, 4 sigmas), 'short' (4 orientations),
    'six', 'sixteen' (6 / 16 orientations, the normal sigmas), 'side17' (radius 8, sigma 1.4, 8 orientations)"""
    from pyimsegm_amd import descriptors as D
    out = {'normal': D.create_filter_bank_lm_2d()[0],
           'short': D.create_filter_bank_lm_2d(sigmas=D.SHORT_FILTERS_SIGMAS, nb_orient=4)[0],
           'six': D.create_filter_bank_lm_2d(nb_orient=6)[0],
           'sixteen': D.create_filter_bank_lm_2d(nb_orient=16)[0],
           'side17': D.create_filter_bank_lm_2d(radius=8, sigmas=(1.4, ), nb_orient=8)[0]}
    for bank in out.values():
        for battery in bank:
            battery.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def battery(name):
    """a battery by name: '<bank>:<index>' or '<bank>:<index>:<orientations joined by ,>'; 'centre': the side-33 kernel that is 1
    at the centre (``lm_battery`` with it copies the high-pass planes into the response, bit for bit: every other product is 0 x)"""
    if name == 'centre':
        out = np.zeros((1, 33, 33))
        out[0, 16, 16] = 1.
    else:
        parts = name.split(':')
        out = np.asarray(banks()[parts[0]][int(parts[1])])
        if len(parts) > 2:
            out = np.ascontiguousarray(out[[int(k) for k in parts[2].split(',')]])
    out.setflags(write=False)
    return out


# the batteries of a bank per sigma: edge, bar, Gauss, GaussLap, GaussLap2 (index 5 s + 0 .. 4)
QUAD4 = '1,15,2,14,3,13,5,11'              # four mirror pairs of the 16-orientation bank
NONAXIS8 = '1,2,3,4,5,6,7,9'               # (0 and 8 are the axis orientations, rank 1)


def case(name, bat, route, expect, kernels, separable=True, mirror=True, wide=False):
    """``expect``: (dense kernels after padding, parity, separable groups, rank) of ``_pack_bank`` for the 'features' route, the
    padded kernel count alone for 'battery'; ``kernels``: what the dispatch launches for it"""
    return dict(id=name, battery=bat, route=route, expect=expect, kernels=kernels, separable=separable, mirror=mirror, wide=wide)


#: every instantiation at SHAPE.  Edge batteries are odd under the point reflection (sign -1), bar batteries even (+1).
CASES = [
    # k_conv_battery<1, 2, 4, 8>: lm_battery with 1, 2, 3 -> 4 and 8 kernels
    case('plain1', 'normal:4', 'battery', 1, ['k_conv_battery<1>']),
    case('plain2', 'sixteen:0:3,7', 'battery', 2, ['k_conv_battery<2>']),
    case('plain3to4', 'sixteen:6:2,5,11', 'battery', 4, ['k_conv_battery<4>']),
    case('plain8', 'normal:0', 'battery', 8, ['k_conv_battery<8>']),
    # k_conv_battery<6>: lm_features(separable=False) on six kernels
    case('plain6', 'six:1', 'features', (6, 0, 0, 0), ['k_conv_battery<6>'], separable=False),
    # k_conv_battery_sym<1, 2, 4, 6, 8>: mirror=False
    case('sym1-edge', 'sixteen:0:3', 'features', (1, -1, 0, 0), ['k_conv_battery_sym<1>'], mirror=False),
    case('sym2-bar', 'short:1', 'features', (2, 1, 2, 1), ['k_conv_battery_sym<2>', 'k_sep_battery_tall'], mirror=False),
    case('sym4-bar', 'sixteen:6:1,2,3,5', 'features', (4, 1, 0, 0), ['k_conv_battery_sym<4>'], mirror=False),
    case('sym6-edge', 'normal:0', 'features', (6, -1, 2, 1), ['k_conv_battery_sym<6>', 'k_sep_battery_tall'], mirror=False),
    case('sym8-edge', 'sixteen:5:' + NONAXIS8, 'features', (8, -1, 0, 0), ['k_conv_battery_sym<8>'], mirror=False),
    case('sym8-bar', 'sixteen:1:' + NONAXIS8, 'features', (8, 1, 0, 0), ['k_conv_battery_sym<8>'], mirror=False),
    # k_conv_battery_quad<1, 2, 3, 4>, each on an edge and a bar battery; the 0 / 90 degree kernels go through k_sep_battery_tall
    # and merge with the quad kernel's output
    case('quad1-edge', 'short:0', 'features', (2, -2, 2, 1), ['k_conv_battery_quad<1,16>', 'k_sep_battery_tall']),
    case('quad1-bar', 'short:1', 'features', (2, 2, 2, 1), ['k_conv_battery_quad<1,16>', 'k_sep_battery_tall']),
    case('quad2-edge', 'six:5', 'features', (4, -2, 2, 1), ['k_conv_battery_quad<2,16>', 'k_sep_battery_tall']),
    case('quad2-bar', 'six:1', 'features', (4, 2, 2, 1), ['k_conv_battery_quad<2,16>', 'k_sep_battery_tall']),
    case('quad3-edge', 'normal:0', 'features', (6, -2, 2, 1), ['k_conv_battery_quad<3,16>', 'k_sep_battery_tall']),
    case('quad3-bar', 'normal:6', 'features', (6, 2, 2, 1), ['k_conv_battery_quad<3,16>', 'k_sep_battery_tall']),
    case('quad4-edge', 'sixteen:0:' + QUAD4, 'features', (8, -2, 0, 0), ['k_conv_battery_quad<4,16>']),
    case('quad4-bar', 'sixteen:6:' + QUAD4, 'features', (8, 2, 0, 0), ['k_conv_battery_quad<4,16>']),
    # k_sep_battery_tall alone: a Gaussian (rank 1), both Laplacians (rank 2)
    case('tall-gauss', 'normal:2', 'features', (0, 0, 1, 1), ['k_sep_battery_tall']),
    case('tall-lap', 'normal:3', 'features', (0, 0, 1, 2), ['k_sep_battery_tall']),
    case('tall-lap2', 'normal:9', 'features', (0, 0, 1, 2), ['k_sep_battery_tall']),
    # k_sep_battery<33>: the same on the 64 x 16 tile, and the merge
    case('wide-gauss', 'normal:2', 'features', (0, 0, 1, 1), ['k_sep_battery<33>'], wide=True),
    case('wide-lap', 'normal:3', 'features', (0, 0, 1, 2), ['k_sep_battery<33>'], wide=True),
    case('wide-lap2', 'normal:9', 'features', (0, 0, 1, 2), ['k_sep_battery<33>'], wide=True),
    case('wide-edge', 'normal:0', 'features', (6, -2, 2, 1), ['k_conv_battery_quad<3,16>', 'k_sep_battery<33>'], wide=True),
    case('wide-bar', 'normal:6', 'features', (6, 2, 2, 1), ['k_conv_battery_quad<3,16>', 'k_sep_battery<33>'], wide=True),
    # another kernel side (17): the run-time radius k_sep_battery<0>, the dense and symmetric kernels, never the quad form
    case('side17-edge', 'side17:0', 'features', (6, -1, 2, 1), ['k_conv_battery_sym<6>', 'k_sep_battery<0>']),
    case('side17-bar', 'side17:1', 'features', (6, 1, 2, 1), ['k_conv_battery_sym<6>', 'k_sep_battery<0>']),
    case('side17-gauss', 'side17:2', 'features', (0, 0, 1, 1), ['k_sep_battery<0>']),
    case('side17-lap', 'side17:3', 'features', (0, 0, 1, 2), ['k_sep_battery<0>']),
    case('side17-lap2', 'side17:4', 'features', (0, 0, 1, 2), ['k_sep_battery<0>']),
    case('side17-plain8', 'side17:0', 'battery', 8, ['k_conv_battery<8>']),
    case('side17-plain6', 'side17:1:1,2,3,5,6,7', 'features', (6, 0, 0, 0), ['k_conv_battery<6>'], separable=False),
]
CASE = {c['id']: c for c in CASES}

#: the tall / wide pairs whose responses must also agree with each other
TALL_WIDE = [('tall-gauss', 'wide-gauss'), ('tall-lap', 'wide-lap'), ('tall-lap2', 'wide-lap2'), ('quad3-edge', 'wide-edge'),
             ('quad3-bar', 'wide-bar')]

#: at every border shape: one quad (merged with its separable kernels), one point-symmetric, one plain dense, one rank-2 separable,
#: one separable-with-merge battery
BORDER_CASES = ['quad1-edge', 'sym4-bar', 'plain2', 'tall-lap', 'sym2-bar']

#: with the clip at the median of the positive responses: one quad, one symmetric, one plain, one tall-separable battery (few
#: kernels each: the maximum over many orientations is rarely negative, and negative responses beyond the clip must occur)
CLIP_CASES = ['quad1-edge', 'sym1-edge', 'plain3to4', 'tall-lap2']

#: the five batteries of one sigma of the bank: one launch of k_sep_battery_tall with SEP_MAX_JOBS = 5 jobs
ONE_SIGMA = ['normal:0', 'normal:1', 'normal:2', 'normal:3', 'normal:4']


def split_of(c):
    """what the host makes of a case: (kernels, parity, groups, rank) for 'features', the padded count for 'battery'"""
    from pyimsegm_amd._hip import Image2D
    bat = battery(c['battery'])
    if c['route'] == 'battery':
        return Image2D._battery_weights(bat)[1]
    packed = Image2D._pack_bank([bat], c['separable'], c['mirror'])
    return tuple(int(packed[k][0]) for k in ('kernels', 'parity', 'groups', 'ranks'))


def sep_truncation(bat, separable=True):
    """what the host's SVD split leaves out: the largest L1 norm of K_flipped - sum_i y_i x_i^T over the battery's separable
    kernels, in longdouble (|sum dK x| <= L1(dK) max|x|: a relative error of the response in units of max|plane|)"""
    from pyimsegm_amd._hip import Image2D
    _, _, taps, groups, rank, _, _ = Image2D._split_battery(bat, separable)
    flipped = np.asarray(bat)[:, ::-1, ::-1].astype(LD)
    worst = 0.
    for g in range(groups):
        rebuilt = sum(np.outer(taps[g, i, 1].astype(LD), taps[g, i, 0].astype(LD)) for i in range(rank))
        worst = max(worst, min(float(np.abs(k - rebuilt).sum()) for k in flipped))
    return worst


_REFERENCES = {}


def reference(name, planes):
    """per battery name and plane shape, computed once per process and never modified: the longdouble response of every kernel
    (``each``), their maximum (``raw``, before the clip), scipy's fp64 deviation from it relative to max|plane| (``scipy``) and
    the planes they were computed on -- the same planes every time (the high-pass of a seeded image is deterministic)"""
    from scipy import ndimage
    planes = np.asarray(planes, dtype=np.float64)
    key = (name, planes.shape)
    if key not in _REFERENCES:
        bat = battery(name)
        each = np.array([conv80(planes, k) for k in bat])
        scale = float(np.abs(planes).max())
        scipy_dev = max(rel_dev([ndimage.convolve(p, k) for p in planes], e, scale) for k, e in zip(bat, each))
        raw = np.max(each, axis=0)
        held = np.array(planes)
        for a in (each, raw, held):
            a.setflags(write=False)
        _REFERENCES[key] = dict(each=each, raw=raw, scipy=scipy_dev, planes=held, scale=scale)
    ref = _REFERENCES[key]
    assert np.array_equal(ref['planes'], planes), 'the planes of %s changed between two tests' % name
    return ref


def tolerance(c, ref):
    """relative to max|plane|: 16 x scipy's deviation on the same planes (floor 1e-13), plus the truncation of the SVD split where
    kernels run as separable passes"""
    tol = rule(ref['scipy'])
    if c['route'] == 'features' and c['separable']:
        tol += sep_truncation(battery(c['battery']))
    return tol


def host_planes(shape, dtype='u8'):
    """fp64 high-pass planes of the seeded image of ``shape`` from scipy: what the CPU test convolves (the GPU test convolves the
    device's own planes)"""
    return np.ascontiguousarray(highpass_scipy(noise(tuple(shape) + (3, ), dtype)), dtype=np.float64)
