"""Descriptor stage: per-superpixel colour / texture statistics.

Host-side mirror of the hot-path part of the reference module ``imsegm/descriptors.py`` (lines
1-1285: colour statistics, Leung-Malik texture bank, feature-set selection).  The segmented
reductions the reference delegates to ``imsegm/features_cython.pyx`` run as HIP kernels
(``csrc/stats.hip``); the function names ``cython_*`` are kept so that callers of the reference do
not change, ``hip_*`` are the same functions under an honest name.

Host (numpy / scipy) code remains where the reference itself is numpy / scipy and the device does not
take the input: the ``numpy_*`` alternatives, the median / mean gradient of dtypes a device session does
not hold, and the Leung-Malik filter responses of batteries of more than 8 kernels (``scipy.ndimage``
convolutions, exactly as ``descriptors.py:903-1106``; see DESIGN.md, "what runs where").
"""
import functools
import itertools
import logging

import numpy as np
from scipy import ndimage
from sklearn import preprocessing

from pyimsegm_amd import _hip
from pyimsegm_amd.utilities import ImageDimensionError, reference_attribute

#: kept for API compatibility: the driver script assigns it (run_segm_slic_model_graphcut.py:59).
#: It no longer selects an implementation: the native path is always the HIP library.
USE_CYTHON = True
#: the segmented reductions run on the GPU through libimsegm_hip.so (there is no CPU fallback)
USE_HIP = True

#: define all available statistic computed on superpixels
NAMES_FEATURE_FLAGS = ('mean', 'std', 'energy', 'median', 'meanGrad')
#: define sigmas for Leung-Malik filter bank
DEFAULT_FILTERS_SIGMAS = (np.sqrt(2), 2, 2 * np.sqrt(2), 4)
#: define small list/range of sigmas for Leung-Malik filter bank
SHORT_FILTERS_SIGMAS = (np.sqrt(2), 2, 4)
#: define the richest version of computed superpixel features
FEATURES_SET_ALL = {
    'color': ('mean', 'std', 'energy', 'median', 'meanGrad'),
    'tLM': ('mean', 'std', 'energy', 'median', 'meanGrad'),
}
#: define basic color features for superpixels
FEATURES_SET_COLOR = {'color': ('mean', 'std', 'energy')}
#: define basic texture features (complete LM filter bank) for superpixels
FEATURES_SET_TEXTURE = {'tLM': ('mean', 'std', 'energy')}
#: define basic texture features (small LM filter bank) for superpixels
FEATURES_SET_TEXTURE_SHORT = {'tLM_short': ('mean', 'std', 'energy')}
#: define circular diameters for computing label histogram
HIST_CIRCLE_DIAGONALS = (10, 20, 30, 40, 50)
#: maximal response is bounded by fix number to prevent overflowing (for LM filter bank)
MAX_SIGNAL_RESPONSE = 1.e6


# ------------------------------------------------------------------------------------------------
# input validation (messages as the reference, descriptors.py:128-206)
# ------------------------------------------------------------------------------------------------


def _fail_unless(condition, template, *values):
    if not condition:
        raise ImageDimensionError(template % tuple(repr(v) for v in values))
    return True


def _same_plane(image, segm):
    """ image - segmentation compatibility for colour images (message of descriptors.py:128-146) """
    return _fail_unless(image.shape[:2] == segm.shape, 'ndarrays - image and segmentation do not match %s vs %s', image.shape, segm.shape)


def _same_shape(image, segm):
    """ image - segmentation compatibility for gray images / volumes (descriptors.py:149-167) """
    return _fail_unless(image.shape == segm.shape, 'ndarrays - image and segmentation do not match %s vs %s', image.shape, segm.shape)


def _three_channels(image):
    """ the image has to be H x W x 3 (descriptors.py:170-184) """
    return _fail_unless(image.ndim == 3 and image.shape[2] == 3, 'image is not RGB with dims %s', image.shape)


def _unknown(kind, given, known):
    """reports (does not raise) the entries of ``given`` that ``known`` does not accept (descriptors.py:187-206)"""
    strangers = [item for item in given if not known(item)]
    if strangers:
        logging.warning('unrecognised following feature %s: %r', kind, strangers)
    return strangers


def _report_unknown_groups(feature_flags):
    return _unknown('groups', feature_flags, lambda key: key.startswith(('color', 'tLM')))


def _report_unknown_names(feature_flags):
    return _unknown('names', feature_flags, lambda name: name in NAMES_FEATURE_FLAGS)


def _finished(features, names):
    """the closing step every feature table of the reference goes through: negative zeros become zeros
    (``features[features == 0] = 0``, descriptors.py:860,1034,1102,1165,1265) and the column count is checked against the names"""
    np.add(features, 0., out=features, where=features == 0)          # (-0. + 0. = +0.)
    if names is not None and len(names) != features.shape[1]:
        raise ValueError('features: %r and names %r' % (features.shape, names))
    return features, names



# ------------------------------------------------------------------------------------------------
# HIP segmented statistics, colour 2D  (reference: cython_img2d_color_*, descriptors.py:209-296)
# ------------------------------------------------------------------------------------------------


def _stats_session(img, seg):
    img = np.asarray(img)
    seg = np.asarray(seg)
    _same_plane(img, seg)
    _three_channels(img)
    return _hip.Image2D(seg.shape[0], seg.shape[1]).upload(img).set_labels(seg)


def hip_img2d_color_mean(img, seg):
    """ mean colour per superpixel (float32 staging, 64-bit accumulation as features_cython.pyx:81-98)

    :param ndarray img: input RGB image H x W x 3
    :param ndarray seg: segmentation H x W
    :return ndarray: np.array<nb_lbs, 3>
    """
    logging.debug('HIP: computing Colour means for image %r & segm %r', np.shape(img), np.shape(seg))
    sess = _stats_session(img, seg)
    mean, _, _ = sess.color_stats(mean=True, energy=False, var=False)
    sess.close()
    return mean


def hip_img2d_color_energy(img, seg):
    """ mean squared colour per superpixel (features_cython.pyx:101-119) """
    logging.debug('HIP: computing Colour energy for image %r & segm %r', np.shape(img), np.shape(seg))
    sess = _stats_session(img, seg)
    _, energy, _ = sess.color_stats(mean=False, energy=True, var=False)
    sess.close()
    return energy


def hip_img2d_color_std(img, seg, means=None):
    """ colour standard deviation per superpixel (features_cython.pyx:122-141, descriptors.py:264-296)

    The variance kernel subtracts the float32-rounded means, exactly as the reference does.
    ``means`` is accepted for API compatibility; the means are (re)computed on the device, which is
    what the reference does when ``means`` is None and what its callers pass anyway.
    """
    logging.debug('HIP: computing Colour STD for image %r & segm %r', np.shape(img), np.shape(seg))
    sess = _stats_session(img, seg)
    _, _, var = sess.color_stats(mean=False, energy=False, var=True)
    sess.close()
    return np.sqrt(var)


cython_img2d_color_mean = hip_img2d_color_mean
cython_img2d_color_energy = hip_img2d_color_energy
cython_img2d_color_std = hip_img2d_color_std

# ------------------------------------------------------------------------------------------------
# the reference's numpy alternatives (numpy_img2d_color_* / numpy_img3d_gray_*, descriptors.py:299-455, :569-702: what
# USE_CYTHON = False selects there) are not part of this module: the names resolve to the reference's own functions when a
# reference package is installed behind the overlay (module __getattr__ below).  What stays is the median of the dtypes a
# device session does not hold unchanged.
# ------------------------------------------------------------------------------------------------


def __getattr__(name):
    """names of the reference module that are not part of the path: the reference's own, when one is installed"""
    return reference_attribute('descriptors', name)


def _median_by_label(values, labels, nb_labels):
    """median of ``values`` per label (both flat); NaN for labels without samples, as np.median([])"""
    order = np.lexsort((values, labels))
    ranked = values[order]
    counts = np.bincount(labels, minlength=nb_labels)
    first = np.cumsum(counts) - counts
    out = np.full(nb_labels, np.nan)
    some = counts > 0
    out[some] = 0.5 * (ranked[first[some] + (counts[some] - 1) // 2] + ranked[first[some] + counts[some] // 2])
    return out


def _channel_medians(image, segm):
    """per label and channel (a gray volume: one channel) by numpy, float64"""
    image, labels = np.asarray(image, dtype=np.float64), np.asarray(segm).ravel()
    nb = int(labels.max()) + 1
    if image.ndim == np.ndim(segm):
        return _median_by_label(image.ravel(), labels, nb)
    return np.stack([_median_by_label(image[..., c].ravel(), labels, nb) for c in range(image.shape[-1])], axis=1)


# ------------------------------------------------------------------------------------------------
# gray 3D statistics (reference: cython_img3d_gray_* / numpy_img3d_gray_*, descriptors.py:458-702)
# ------------------------------------------------------------------------------------------------


def _gray_stats_session(img, seg):
    img, seg = np.asarray(img), np.asarray(seg)
    _same_shape(img, seg)
    return _hip.Volume3D(*seg.shape).upload(img).set_labels(seg)


def hip_img3d_gray_mean(img, seg):
    """ mean intensity per supervoxel (float32 staging, 64-bit accumulation as features_cython.pyx:144-166)

    :param ndarray img: gray volume D x H x W
    :param ndarray seg: segmentation D x H x W
    :return ndarray: np.array<nb_lbs>
    """
    logging.debug('HIP: computing Gray means for image %r and segm %r', np.shape(img), np.shape(seg))
    sess = _gray_stats_session(img, seg)
    mean, _, _ = sess.gray_stats(mean=True, energy=False, var=False)
    sess.close()
    return mean


def hip_img3d_gray_energy(img, seg):
    """ mean squared intensity per supervoxel (features_cython.pyx:169-191)
    """
    logging.debug('HIP: computing Gray energy for image %r and segm %r', np.shape(img), np.shape(seg))
    sess = _gray_stats_session(img, seg)
    _, energy, _ = sess.gray_stats(mean=False, energy=True, var=False)
    sess.close()
    return energy


def hip_img3d_gray_std(img, seg, mean=None):
    """ intensity STD per supervoxel (features_cython.pyx:194-219; float32-rounded mean, descriptors.py:547)

    ``mean`` is accepted for API compatibility; the means are (re)computed on the device, which is
    what the reference does when ``mean`` is None and what its callers pass anyway.
    """
    logging.debug('HIP: computing Gray STD for image %r and segm %r', np.shape(img), np.shape(seg))
    sess = _gray_stats_session(img, seg)
    _, _, var = sess.gray_stats(mean=False, energy=False, var=True)
    sess.close()
    return np.sqrt(var)


cython_img3d_gray_mean = hip_img3d_gray_mean
cython_img3d_gray_energy = hip_img3d_gray_energy
cython_img3d_gray_std = hip_img3d_gray_std


def _device_keeps(image, plane_axes):
    """median / mean gradient run on the device for the dtypes a session holds unchanged (the gradient image keeps the dtype of the
    source, descriptors.py:767-769 / :842-844: integer data truncate / wrap) and planes of at least 2 x 2; else the numpy route"""
    image = np.asarray(image)
    return image.dtype in (np.uint8, np.float32, np.float64) and min(image.shape[a] for a in plane_axes) >= 2


def _ordered_columns(by_flag, feature_flags):
    """the statistics that were asked for, in the column order of the reference (NAMES_FEATURE_FLAGS)"""
    return [by_flag[flag]() for flag in NAMES_FEATURE_FLAGS if flag in feature_flags]


def compute_image3d_gray_statistic(image, segm, feature_flags=NAMES_FEATURE_FLAGS, ch_name='gray', sess=None):
    """ statistics of a gray volume per supervoxel (reference descriptors.py:705-784); ``sess``: a device session that already holds
    the volume and its supervoxels
    """
    image = np.asarray(image)
    if sess is None:
        segm = np.asarray(segm)
    _same_shape(image, segm)
    if len(feature_flags) == 0:
        raise ValueError('some features has to be selected')
    on_device = _device_keeps(image, (1, 2))
    sums = {'mean', 'std', 'energy'} & set(feature_flags)
    needs_session = bool(sums) or (on_device and bool({'median', 'meanGrad'} & set(feature_flags)))
    if sess is None or {'median', 'meanGrad'} & set(feature_flags):
        image = np.nan_to_num(image)       # (a resident session already holds the caller-checked finite volume)
    own = needs_session and sess is None
    if own:
        sess = _hip.Volume3D(*segm.shape).upload(image).set_labels(segm)
    try:
        mean = energy = var = None
        if sums:
            mean, energy, var = sess.gray_stats(mean='mean' in sums, energy='energy' in sums, var='std' in sums)

        def mean_gradient():
            if on_device:
                return sess.mean_gradient()
            slopes = np.zeros_like(image)
            for z, plane in enumerate(image):
                slopes[z] = np.sum(np.gradient(plane), axis=0)
            return hip_img3d_gray_mean(slopes, segm)

        columns = _ordered_columns({'mean': lambda: mean, 'std': lambda: np.sqrt(var), 'energy': lambda: energy,
                                    'median': lambda: sess.median() if on_device else _channel_medians(image, segm),
                                    'meanGrad': mean_gradient}, feature_flags)
    finally:
        if own:
            sess.close()
    _report_unknown_names(feature_flags)
    names = ['%s_%s' % (ch_name, flag) for flag in NAMES_FEATURE_FLAGS if flag in feature_flags]
    return _finished(np.nan_to_num(np.array(columns)).T, names)


def _color_statistic_session(sess, image, segm, feature_flags, color_name):
    """colour statistics (reference descriptors.py:787-863) from a device session that already holds ``image`` and ``segm``"""
    sums = {'mean', 'std', 'energy'} & set(feature_flags)
    mean = energy = var = None
    if sums:
        mean, energy, var = sess.color_stats(mean='mean' in sums, energy='energy' in sums, var='std' in sums)
    on_device = _device_keeps(image, (0, 1))

    def mean_gradient():
        if on_device:
            return sess.mean_gradient()
        slopes = np.zeros_like(image)
        for c in range(3):
            slopes[..., c] = np.sum(np.gradient(image[..., c]), axis=0)
        return hip_img2d_color_mean(slopes, segm)

    blocks = _ordered_columns({'mean': lambda: mean, 'std': lambda: np.sqrt(var), 'energy': lambda: energy,
                               'median': lambda: sess.median() if on_device else _channel_medians(image, segm),
                               'meanGrad': mean_gradient}, feature_flags)
    _report_unknown_names(feature_flags)
    names = ['%s-ch%i_%s' % (color_name, c + 1, flag) for flag in NAMES_FEATURE_FLAGS if flag in feature_flags for c in range(3)]
    table = np.hstack(blocks) if blocks else np.empty((sess.n_labels, 0))
    return _finished(np.nan_to_num(table), names)


def compute_image2d_color_statistic(image, segm, feature_flags=NAMES_FEATURE_FLAGS, color_name='color'):
    """ statistics of a colour image per superpixel, columns ordered mean, std, energy, median, meanGrad with the three channels
    of a statistic side by side (reference descriptors.py:787-863)

    :return tuple(ndarray,list(str)): K x (3 * number of statistics) table, column names
    """
    image, segm = np.asarray(image), np.asarray(segm)
    _three_channels(image)
    _same_plane(image, segm)
    finite = np.nan_to_num(image)
    sess = _hip.Image2D(segm.shape[0], segm.shape[1]).upload(finite).set_labels(segm)
    try:
        return _color_statistic_session(sess, finite, segm, feature_flags, color_name)
    finally:
        sess.close()


def norm_features(features, scaler=None):
    """ features standardised to zero mean and unit variance by ``scaler`` -- fitted here when none is given
    (reference descriptors.py:866-877); returns (features, scaler) """
    scaler = scaler or preprocessing.StandardScaler().fit(features)
    return scaler.transform(features), scaler


# ------------------------------------------------------------------------------------------------
# Leung-Malik texture bank (reference descriptors.py:880-1106) -- host scipy, as the reference
# ------------------------------------------------------------------------------------------------


def make_gaussian_filter1d(vals, sigma, order=0):
    """ a Gaussian (order 0) or -- up to a constant -- its first / second derivative sampled at ``vals``, scaled to unit L1 norm
    (reference descriptors.py:880-900).  Operation by operation the reference's arithmetic: the bank decides the last bits of
    every filter response, and the point symmetry the device kernels rely on holds bit for bit only that way. """
    if not order <= 2:
        raise ValueError("Only orders up to 2 are supported")
    bell = np.exp(-vals**2 / (2. * sigma**2))
    shaped = {1: lambda: -bell * vals, 2: lambda: bell * (vals**2 - sigma**2)}.get(order, lambda: bell)()
    return shaped / np.abs(shaped).sum()


def make_edge_filter2d(sig, phase, points, sup):
    """ an elongated Gaussian (3 sig along x) times the ``phase``-th derivative of a Gaussian across it on the (rotated) grid
    ``points`` (2 x sup^2), unit L1 norm (reference descriptors.py:903-912) """
    along = make_gaussian_filter1d(points[0], sigma=3 * sig)
    across = make_gaussian_filter1d(points[1], sigma=sig, order=phase)
    kernel = (along * across).reshape(sup, sup)
    return kernel / np.abs(kernel).sum()


def create_filter_bank_lm_2d(radius=16, sigmas=DEFAULT_FILTERS_SIGMAS, nb_orient=8):
    """ Leung-Malik bank (reference descriptors.py:915-948): per sigma a battery of ``nb_orient`` edge filters and one of bar
    filters over half a circle (the filters are symmetric), a Gaussian, and the Laplacians of Gaussians of sigma and sigma^2 --
    five batteries per sigma, named 'sigma<s>-edge' ... 'sigma<s>-GaussLap2'
    """
    logging.debug('creating Leung-Malik filter bank')
    side = 2 * radius + 1
    cols, rows = np.mgrid[-radius:radius + 1, radius:-radius - 1:-1]
    grid = np.vstack([cols.ravel(), rows.ravel()])
    turned = []                     # the grid rotated by every orientation (the same for all sigmas)
    for k in range(nb_orient):
        theta = np.pi * k / nb_orient
        cos, sin = np.cos(theta), np.sin(theta)
        turned.append(np.dot(np.array([[cos, -sin], [sin, cos]]), grid))
    dot = np.zeros((side, side))
    dot[radius, radius] = 1
    filters, names = [], []
    for sigma in sigmas:
        for phase in (1, 2):        # edge, bar
            filters.append(np.asarray([make_edge_filter2d(sigma, phase, points, side) for points in turned]))
        filters += [ndimage.gaussian_filter(dot, sigma)[None], ndimage.gaussian_laplace(dot, sigma)[None],
                    ndimage.gaussian_laplace(dot, sigma**2)[None]]
        names += ['sigma%.1f-%s' % (sigma, kind) for kind in ('edge', 'bar', 'Gauss', 'GaussLap', 'GaussLap2')]
    return filters, names


def compute_img_filter_response2d(img, filter_battery):
    """ response of one battery on a 2D image: the maximum over its kernels (reference descriptors.py:951-966) """
    if np.ndim(filter_battery) != 3:
        raise ValueError('wrong battery dim %r' % filter_battery.shape)
    each = [ndimage.convolve(img, kernel) for kernel in filter_battery]
    return np.max(np.array(each), axis=0) if len(each) > 1 else each[0]


def compute_img_filter_response3d(img, filter_battery):
    """ :func:`compute_img_filter_response2d` slice by slice (reference descriptors.py:969-978) """
    logging.debug('compute image filter response in 3D')
    return np.array([compute_img_filter_response2d(plane, filter_battery) for plane in img])


def image_subtract_gauss_smooth(img, sigma):
    """ every slice minus its Gaussian-smoothed copy (reference descriptors.py:981-994) """
    if not sigma > 0:
        return img
    return img - np.array([ndimage.gaussian_filter(plane.astype(float), sigma) for plane in img])


@functools.lru_cache(maxsize=4)
def _select_bank(bank_type):
    """the bank of a ``tLM`` / ``tLM_short`` group, built once per process (the arrays are shared: read-only for every caller;
    their identity is what :meth:`_hip.Image2D.lm_features` keys its factorisation on)"""
    if bank_type == 'short':
        filters, names = create_filter_bank_lm_2d(sigmas=SHORT_FILTERS_SIGMAS, nb_orient=4)
    else:
        filters, names = create_filter_bank_lm_2d()
    for battery in filters:
        battery.setflags(write=False)
    return filters, names


def _normalise_response(response):
    """clip and rescale one battery response globally, descriptors.py:1088-1094"""
    response[response > MAX_SIGNAL_RESPONSE] = MAX_SIGNAL_RESPONSE
    norm = np.sqrt(np.sum(response**2))
    if norm == 0 or abs(norm) == np.inf:
        return np.zeros(response.shape)
    return (response * (np.log(1 + norm) / 0.03)) / norm


def compute_texture_desc_lm_img3d_val(img, seg, feature_flags, bank_type='normal'):
    """ Leung-Malik texture statistics of a gray volume (reference descriptors.py:997-1038) """
    img, seg = np.asarray(img), np.asarray(seg)
    _same_shape(img, seg)
    logging.debug('compute texture descriptors using Leung-Malik')
    filters, fl_names = _select_bank(bank_type)
    if _texture_on_device(feature_flags, filters):
        return _texture_desc_lm_device3d(img, seg, feature_flags, filters, fl_names)
    img = image_subtract_gauss_smooth(img, 150)
    features, names = [], []
    for battery, fl_name in zip(filters, fl_names):
        response = _normalise_response(compute_img_filter_response3d(img, battery))
        fts, n = compute_image3d_gray_statistic(response, seg, feature_flags, fl_name)
        features.append(fts)
        names += n
    return _finish_texture(features, names)


def compute_texture_desc_lm_img2d_clr(img, seg, feature_flags, bank_type='normal'):
    """ Leung-Malik texture statistics of a colour image (reference descriptors.py:1041-1106)
    """
    img, seg = np.asarray(img), np.asarray(seg)
    _three_channels(img)
    logging.debug('compute texture descriptors using Leung-Malik')
    filters, fl_names = _select_bank(bank_type)
    if _texture_on_device(feature_flags, filters):
        return _texture_desc_lm_device(img, seg, feature_flags, filters, fl_names)
    # host path (batteries of more than 8 kernels, unknown statistic names): scipy as the reference
    # scalar sigma on all three axes, channel axis included (descriptors.py:1078)
    img = img - ndimage.gaussian_filter(img.astype(float), 150)
    img_roll = np.rollaxis(img, -1, 0)
    sess = _hip.Image2D(seg.shape[0], seg.shape[1]).set_labels(seg)
    features, names = [], []
    for battery, fl_name in zip(filters, fl_names):
        response = np.rollaxis(_normalise_response(compute_img_filter_response3d(img_roll, battery)), 0, 3)
        response = np.nan_to_num(np.ascontiguousarray(response))
        sess.upload(response)
        fts, ns = _color_statistic_session(sess, response, seg, feature_flags, fl_name)
        features.append(fts)
        names += ns
    sess.close()
    return _finish_texture(features, names)


def _texture_on_device(feature_flags, filters):
    """the statistics the device forms of a filter response (all five of NAMES_FEATURE_FLAGS), and batteries it takes (at most
    8 kernels)"""
    return set(feature_flags) <= set(NAMES_FEATURE_FLAGS) and all(len(f) <= 8 for f in filters)


def _convert_on_device(image, convert_on):
    """whether a 'color_<space>' group of ``image`` is converted on the device: asked for (``convert_on='device'``; ``'host'`` and
    None are the numpy conversion) and the conversion of the uploaded pixels is the conversion the host would make -- uint8
    images, and float images whose sum is finite (NaN / inf are replaced BEFORE the upload but AFTER the host's conversion);
    planes of at least 2 x 2 (the mean gradient needs them)"""
    if convert_on not in (None, 'host', 'device'):
        raise ValueError('convert_on is %r, expected \'host\' or \'device\'' % (convert_on, ))
    if convert_on != 'device':
        return False
    image = np.asarray(image)
    return image.ndim == 3 and min(image.shape[:2]) >= 2 \
        and (image.dtype == np.uint8 or bool(np.isfinite(image.sum(dtype=np.float64))))


def _convert_session(sess, space):
    """the session's uploaded RGB image converted to ``space`` on the device; its statistics read the result from now on"""
    from pyimsegm_amd.utilities.data_io import _HED_FROM_RGB
    return sess.convert_color(space, _HED_FROM_RGB if space == 'hed' else None)


def resident_feature_groups(feature_flags, convert_on=None):
    """the descriptor groups of ``feature_flags`` in the column order of :func:`compute_selected_features_color2d` (the colour
    statistics, then the Leung-Malik ones) as ``[(kind, flags, batteries, columns)]`` when ALL of them can be formed and kept on
    the device -- 'color' in RGB, with ``convert_on='device'`` also 'color_<space>' (``batteries`` is the name of the space then),
    and 'tLM' / 'tLM_<bank>', each with mean / std / energy; otherwise None (median, meanGrad, colour spaces converted on the
    host: the general path)"""
    order = [k for k in feature_flags if k.startswith('color')] + [k for k in feature_flags if k.startswith('tLM')]
    if not order or len(order) != len(feature_flags):
        return None
    groups = []
    for key in order:
        flags = set(feature_flags[key])
        if not flags or not flags <= {'mean', 'std', 'energy'}:
            return None
        if key == 'color':
            groups.append(('color', flags, None, 3 * len(flags)))
        elif convert_on == 'device' and key.startswith('color_') and key.split('_')[-1] in _hip.COLOR_SPACES:
            groups.append(('color', flags, key.split('_')[-1], 3 * len(flags)))
        elif key == 'tLM' or key.startswith('tLM_'):
            filters, _ = _select_bank(key.split('_')[-1] if '_' in key else 'normal')
            if not _texture_on_device(flags, filters) or len({np.shape(f)[1:] for f in filters}) != 1:
                return None
            groups.append(('tLM', flags, filters, 3 * len(flags) * len(filters)))
        else:
            return None
    return groups


def resident_feature_table(sess, groups):
    """forms the K x F table of ``groups`` (:func:`resident_feature_groups`) on the device session that holds the image and its
    label map -- nothing comes to the host, nothing is waited for; returns F"""
    total = sum(g[3] for g in groups)
    column, prepared = 0, False
    for kind, flags, filters, width in groups:
        sess.features_place(total, column)
        want = dict(mean='mean' in flags, std='std' in flags, energy='energy' in flags)
        if kind == 'color' and filters is not None:         # a colour space: converted where the RGB image already is
            _convert_session(sess, filters)
            try:
                sess.features_color(to_host=False, **want)
            finally:
                sess.convert_color(0)
        elif kind == 'color':
            sess.features_color(to_host=False, **want)
        else:
            if not prepared:
                sess.lm_prepare(150.)
                prepared = True
            sess.lm_features(filters, MAX_SIGNAL_RESPONSE, to_host=False, **want)
        column += width
    return total


def _finish_texture(blocks, names):
    """the blocks of the batteries side by side, NaN / inf replaced, names prefixed (descriptors.py:1031-1038, :1099-1106)"""
    return _finished(np.nan_to_num(np.concatenate(tuple(blocks), axis=1)), ['tLM_' + name for name in names])


def _battery_blocks(sess, battery, feature_flags):
    """the statistics of ``feature_flags`` (mean, std, energy, median, meanGrad; in that order) of the normalised response of ONE
    battery on a session that holds the high-passed planes, with the norm of the response brought to the host in between
    (descriptors.py:1088-1096: a response of norm 0 or inf counts as all zeros).  The median and the mean gradient leave the
    prepared planes as they are: the next battery needs no lm_prepare."""
    norm = sess.lm_battery(battery, MAX_SIGNAL_RESPONSE)
    flags = set(feature_flags)
    if not 0 < abs(norm) < np.inf:
        zeros = np.zeros(sess.n_labels if isinstance(sess, _hip.Volume3D) else (sess.n_labels, 3))
        return _ordered_columns(dict.fromkeys(NAMES_FEATURE_FLAGS, lambda: zeros), flags)
    mul = np.log(1 + norm) / 0.03
    mean = energy = var = None
    if flags & {'mean', 'std', 'energy'}:
        mean, energy, var = sess.response_stats(mul, norm, mean='mean' in flags, energy='energy' in flags, var='std' in flags)
    return _ordered_columns({'mean': lambda: mean, 'std': lambda: np.sqrt(var), 'energy': lambda: energy,
                             'median': lambda: sess.response_median(mul, norm),
                             'meanGrad': lambda: sess.response_mean_gradient(mul, norm)}, flags)


def _texture_desc_lm_device(img, seg, feature_flags, filters, fl_names, sess=None):
    """Leung-Malik statistics of a colour image entirely on the GPU: high-pass, filter batteries with the maximum over the
    orientations, the norm of a battery's response, per-superpixel statistics (texture.hip + stats.hip)"""
    borrowed = sess is not None
    if not borrowed:
        sess = _hip.Image2D(seg.shape[0], seg.shape[1]).upload(np.nan_to_num(img)).set_labels(seg)
    try:
        sess.lm_prepare(150.)
        sums = {'mean', 'std', 'energy'} & set(feature_flags)
        fused = sums and not {'median', 'meanGrad'} & set(feature_flags)
        if fused and len({np.shape(f)[1:] for f in filters}) == 1 and hasattr(sess, 'lm_features'):
            # all batteries in one call: the norm of a battery never comes to the host (60 synchronisations per image less)
            blocks = [sess.lm_features(filters, MAX_SIGNAL_RESPONSE, mean='mean' in sums, std='std' in sums, energy='energy' in sums)]
        else:       # battery by battery (the median and the mean gradient are formed of one response at a time)
            blocks = [_finished(np.nan_to_num(np.hstack(_battery_blocks(sess, battery, feature_flags))), None)[0]
                      for battery in filters]
    finally:
        if not borrowed:
            sess.close()
    names = ['%s-ch%i_%s' % (name, c + 1, flag) for name in fl_names for flag in NAMES_FEATURE_FLAGS if flag in feature_flags
             for c in range(3)]
    _report_unknown_names(feature_flags)
    return _finish_texture(blocks, names)


def _texture_desc_lm_device3d(img, seg, feature_flags, filters, fl_names):
    """Leung-Malik statistics of a gray volume on the GPU: per-slice high-pass and filter batteries (the slices are the
    planes the 2-D kernels work on), one norm over the volume, per-supervoxel statistics"""
    sess = _hip.Volume3D(*seg.shape).upload(np.nan_to_num(img)).set_labels(seg)
    try:
        sess.lm_prepare(150.)
        blocks = [_finished(np.nan_to_num(np.array(_battery_blocks(sess, battery, feature_flags))).T, None)[0] for battery in filters]
    finally:
        sess.close()
    names = ['%s_%s' % (name, flag) for name in fl_names for flag in NAMES_FEATURE_FLAGS if flag in feature_flags]
    _report_unknown_names(feature_flags)
    return _finish_texture(blocks, names)


# ------------------------------------------------------------------------------------------------
# feature-set selection (reference descriptors.py:1109-1285)
# ------------------------------------------------------------------------------------------------


def _groups(feature_flags, prefix):
    """(key, suffix or None) of the descriptor groups of one kind in the order of ``feature_flags``: 'color_hsv' -> 'hsv'"""
    return [(key, key.split('_')[-1] if '_' in key else None) for key in feature_flags if key.startswith(prefix)]


def _side_by_side(blocks, names, feature_flags):
    """the closing step of every compute_selected_features_* (descriptors.py:1160-1166, :1262-1270): unknown groups reported,
    the blocks of the groups concatenated (no block at all: the ValueError of numpy, as there), NaN / inf replaced"""
    _report_unknown_groups(feature_flags)
    if not blocks:
        logging.error('not supported features: %r', feature_flags)
    return _finished(np.nan_to_num(np.concatenate(tuple(blocks), axis=1)), names)


def compute_selected_features_gray3d(img, segments, feature_flags=FEATURES_SET_COLOR, sess=None):
    """ selected features of a gray volume (reference descriptors.py:1109-1166): the intensity statistics of ALL 'color*' groups
    together (their flags united), then one Leung-Malik block per 'tLM*' group
    """
    img = np.asarray(img)
    if sess is None:
        segments = np.asarray(segments)
    _same_shape(img, segments)
    if not feature_flags:
        raise ValueError('some features has to be selected')
    blocks, names = [], []
    colour = _groups(feature_flags, 'color')
    if colour:
        flags = np.unique([feature_flags[key] for key, _ in colour])
        part, part_names = compute_image3d_gray_statistic(img, segments, flags, sess=sess)
        blocks.append(part)
        names += part_names
    for key, bank in _groups(feature_flags, 'tLM'):
        part, part_names = compute_texture_desc_lm_img3d_val(img, segments, feature_flags[key], bank or 'normal')
        blocks.append(part)
        names += part_names
    return _side_by_side(blocks, names, feature_flags)


def compute_selected_features_gray2d(img, segments, features_flags=FEATURES_SET_ALL):
    """ selected features of a gray 2D image: a volume of one slice (reference descriptors.py:1169-1204)
    """
    img, segments = np.asarray(img), np.asarray(segments)
    _same_shape(img, segments)
    return compute_selected_features_gray3d(img[None], segments[None], features_flags)


def _selected_features_color2d(img, segments, feature_flags, sess=None, convert_on=None):
    """reference descriptors.py:1207-1270 with ONE device session for all groups that read the RGB image; with
    ``convert_on='device'`` that includes the 'color_<space>' groups, whose conversion then runs on that session"""
    _three_channels(img)
    borrowed = sess is not None
    blocks, names = [], []
    on_device = _convert_on_device(img, convert_on)

    def session():
        nonlocal sess
        if sess is None:
            sess = _hip.Image2D(segments.shape[0], segments.shape[1]).upload(np.nan_to_num(img)).set_labels(segments)
        return sess

    try:
        for key, space in _groups(feature_flags, 'color'):
            if space is None:
                part, part_names = _color_statistic_session(session(), img, segments, feature_flags[key], 'rgb')
            elif on_device and space in _hip.COLOR_SPACES:
                _convert_session(session(), space)
                try:    # (the converted image is float64 on the device whatever the upload is: that is all the statistics ask of it)
                    stand_in = np.broadcast_to(np.float64(0.), tuple(np.shape(img)[:2]) + (3, ))
                    part, part_names = _color_statistic_session(sess, stand_in, segments, feature_flags[key], space)
                finally:
                    sess.convert_color(0)
            else:           # a colour space converted on the host: its own upload
                from pyimsegm_amd.utilities.data_io import convert_img_color_from_rgb
                converted = np.nan_to_num(convert_img_color_from_rgb(img, space))
                part, part_names = compute_image2d_color_statistic(converted, segments, feature_flags[key], color_name=space)
            blocks.append(part)
            names += part_names
        for key, bank in _groups(feature_flags, 'tLM'):
            filters, filter_names = _select_bank(bank or 'normal')
            if _texture_on_device(feature_flags[key], filters):
                part, part_names = _texture_desc_lm_device(img, segments, feature_flags[key], filters, filter_names, sess=session())
            else:
                part, part_names = compute_texture_desc_lm_img2d_clr(img, segments, feature_flags[key], bank or 'normal')
            blocks.append(part)
            names += part_names
    finally:
        if sess is not None and not borrowed:
            sess.close()
    return _side_by_side(blocks, names, feature_flags)


def compute_selected_features_color2d(img, segments, feature_flags=FEATURES_SET_ALL, convert_on=None):
    """ selected features of a colour 2D image (reference descriptors.py:1207-1270)

    :param str convert_on: (not in the reference) where a 'color_<space>' group is converted from RGB: ``'host'`` (numpy, then
        a second upload; the default) or ``'device'`` (on the session that holds the RGB image; last digits may differ)
    """
    return _selected_features_color2d(np.asarray(img), np.asarray(segments), feature_flags, convert_on=convert_on)


def compute_selected_features_img2d(image, segm, features_flags=FEATURES_SET_COLOR, convert_on=None):
    """ by the kind of image: H x W x 3 colour or H x W gray (reference descriptors.py:1273-1285); ``convert_on``: see
    :func:`compute_selected_features_color2d` (colour images only) """
    image, segm = np.asarray(image), np.asarray(segm)
    colour = image.ndim == 3 and image.shape[2] == 3
    if not colour and image.ndim != 2:
        logging.error('invalid image size - %r', image.shape)
        return None
    if colour:
        return compute_selected_features_color2d(image, segm, features_flags, convert_on=convert_on)
    return compute_selected_features_gray2d(image, segm, features_flags)


# ------------------------------------------------------------------------------------------------
# label histograms around positions and ray features (reference descriptors.py:1371-1660); the
# natives behind them (features_cython.pyx:222-282) run batched on the device
# ------------------------------------------------------------------------------------------------


def adjust_bounding_box_crop(image_size, bbox_size, position):
    """ clip a box of ``bbox_size`` centred at ``position`` to the image (reference ``descriptors.py:1371-1409``)

    :return (), (), (), (): begin / end of the crop in the image, begin / end of the matching part of the box
    """
    if len(image_size) != len(bbox_size):
        raise ValueError('incompatible sizes %r != %r' % (image_size, bbox_size))
    im_begin, im_end, bb_begin, bb_end = [], [], [], []
    for size, box, pos in zip(image_size, bbox_size, position):
        size, box, pos = int(size), int(box), int(pos)
        half_lo, half_hi = box // 2, box - box // 2             # floor(box / 2), ceil(box / 2)
        lo, hi = max(pos - half_lo, 0), min(pos + half_hi, size)
        im_begin.append(lo)
        im_end.append(hi)
        bb_begin.append(half_lo - pos if lo == 0 else 0)
        bb_end.append(half_lo + (size - pos) if hi == size else box)
    if [e - b for b, e in zip(im_begin, im_end)] != [e - b for b, e in zip(bb_begin, bb_end)]:
        raise ValueError('different sizes of image %r and bounding box %r mask'
                         % ([e - b for b, e in zip(im_begin, im_end)], [e - b for b, e in zip(bb_begin, bb_end)]))
    return tuple(im_begin), tuple(im_end), tuple(bb_begin), tuple(bb_end)


def hip_label_hist_seg2d(segm_select, struc_elem, nb_labels):
    """ histogram of the labels under a structuring element (``computeLabelHistogram2d``) on the device
    """
    segm_select, struc_elem = np.asarray(segm_select), np.asarray(struc_elem)
    if segm_select.shape != struc_elem.shape:
        raise ValueError('segm. %r and mask %r sizes do not match' % (segm_select.shape, struc_elem.shape))
    if segm_select.dtype.kind == 'f':
        segm_select = np.where(np.isnan(segm_select), -1, segm_select)      # NaN marks "no label" (descriptors.py:1490)
    h, w = segm_select.shape
    hist = _hip.label_hist2d(segm_select, [[0, 0, h, w, 0, 0]], struc_elem, nb_labels)[0]
    return np.array(hist, dtype=float)


cython_label_hist_seg2d = hip_label_hist_seg2d


def compute_label_hist_segm(segm, position, struc_elem, nb_labels):
    """ label histogram of the neighbourhood ``struc_elem`` around ``position`` and the size of that neighbourhood
    (reference ``descriptors.py:1411-1461``)
    """
    hists, sizes = compute_label_hist_positions(segm, [position], struc_elem, nb_labels)
    return hists[0], sizes[0]


def compute_label_hist_positions(segm, positions, struc_elem, nb_labels):
    """ :func:`compute_label_hist_segm` for many positions in ONE launch (a wave per position)

    :return tuple(ndarray,ndarray): histograms P x nb_labels (float), sizes of the clipped neighbourhoods P
    """
    segm, struc_elem = np.asarray(segm), np.asarray(struc_elem)
    windows, sizes = [], []
    for position in positions:
        if segm.ndim != len(position):
            raise ValueError('dim of position %r should match the segmentation %r dim' % (position, segm.shape))
        position = [int(p) for p in position]
        im_begin, im_end, bb_begin, bb_end = adjust_bounding_box_crop(segm.shape, struc_elem.shape, position)
        windows.append([im_begin[0], im_begin[1], im_end[0] - im_begin[0], im_end[1] - im_begin[1], bb_begin[0], bb_begin[1]])
        sizes.append(np.sum(struc_elem[bb_begin[0]:bb_end[0], bb_begin[1]:bb_end[1]]))
    hists = _hip.label_hist2d(segm, windows, struc_elem, nb_labels)
    return np.array(hists, dtype=float), np.array(sizes, dtype=float)


def _ray_directions(angle_step):
    """per-angle step (d_row, d_col) of ``computeRayFeaturesBinary2d`` with the precision chain of features_cython.pyx:253-269:
    the float32 angle goes through ``np.deg2rad`` as a Python float (float64), the result is stored in a C ``float``; its
    sine / cosine are again formed in float64 and stored as ``float``; the division by the larger magnitude is float32"""
    angles = np.arange(0, 360, angle_step, dtype=np.float32)
    dirs = np.empty((len(angles), 2), dtype=np.float32)
    for i, ang in enumerate(angles):
        rad = np.float32(np.deg2rad(float(ang)))
        g0, g1 = np.float32(np.sin(float(rad))), np.float32(np.cos(float(rad)))
        gmax = max(abs(g0), abs(g1))
        dirs[i] = g0 / gmax, g1 / gmax
    return dirs


def ray_walk_host(mask, positions, directions, edge):
    """``computeRayFeaturesBinary2d(mask, position, edge)`` in numpy for all positions and angles: float32 [P, A]; float32 positions
    advanced by the float32 ``directions`` [A, 2], the walk of csrc/raywalk.h operation by operation -- the one host statement of
    it (``ellipse_fitting.ray_walk_host`` is this function, ``region_growing.ray_distances_down`` its one-position 'down' call).
    ``edge`` is 1 ('up': the first mask pixel) or -1 ('down': the first pixel off the mask after one on it)."""
    mask = np.asarray(mask, dtype=bool)
    height, width = mask.shape
    directions = np.asarray(directions, dtype=np.float32).reshape(-1, 2)
    positions = np.asarray(positions, dtype=np.int64).reshape(-1, 2)
    rays = np.full((len(positions), len(directions)), -1, dtype=np.float32)
    steps = int(np.sqrt(float(width) * width + float(height) * height))
    for p, (py, px) in enumerate(positions):
        if not (0 <= py < height and 0 <= px < width):
            continue
        if edge == 1 and mask[py, px]:
            rays[p] = 0
            continue
        pos0 = np.full(len(directions), py, dtype=np.float32)
        pos1 = np.full(len(directions), px, dtype=np.float32)
        last = np.full(len(directions), mask[py, px], dtype=bool)
        active = np.ones(len(directions), dtype=bool)
        for _ in range(steps):
            if not active.any():
                break
            pos0 = pos0 + directions[:, 0]
            pos1 = pos1 + directions[:, 1]
            r0, r1 = np.floor(pos0.astype(np.float64) + 0.5), np.floor(pos1.astype(np.float64) + 0.5)
            active &= ~((pos0 < 0) | (r0 >= height) | (pos1 < 0) | (r1 >= width))
            idx = np.nonzero(active)[0]
            actual = mask[r0[idx].astype(int), r1[idx].astype(int)]
            hit = actual if edge == 1 else last[idx] & ~actual
            dx, dy = pos0[idx[hit]] - np.float32(py), pos1[idx[hit]] - np.float32(px)
            rays[p, idx[hit]] = np.sqrt(((dx * dx) + (dy * dy)).astype(np.float64)).astype(np.float32)
            last[idx] = actual
            active[idx[hit]] = False
    return rays


def hip_ray_features_positions(seg_binary, positions, angle_step=5., edge='up'):
    """ ray features of many positions in ONE launch (``computeRayFeaturesBinary2d`` per position): float32 P x A """
    edge_int = {'down': -1, 'up': 1}[edge]
    return _hip.ray_features_binary2d(np.asarray(seg_binary) != 0, positions, _ray_directions(float(angle_step)), edge_int)


def hip_ray_features_seg2d(seg_binary, position, angle_step=5., edge='up'):
    """ distances from ``position`` to the object boundary along rays (reference ``descriptors.py:1630-1659``)
    """
    return np.array(hip_ray_features_positions(seg_binary, [position], angle_step, edge)[0])


cython_ray_features_seg2d = hip_ray_features_seg2d


def compute_ray_features_segm_2d(seg_binary, position, angle_step=5., smooth_coef=0, edge='up'):
    """ ray features of one position, optionally smoothed along the angle (reference ``descriptors.py:1715-1758``:
    the ray casting followed by ``gaussian_filter1d``) """
    seg_binary = np.asarray(seg_binary)
    if seg_binary.ndim != len(position):
        raise ValueError('Segmentation dim of %r and position (%i) does not match' % (seg_binary.ndim, len(position)))
    ray_dist = hip_ray_features_seg2d(seg_binary.astype(bool), tuple(map(int, position)), angle_step, edge)
    if smooth_coef is not None and smooth_coef > 0:
        ray_dist = ndimage.gaussian_filter1d(ray_dist, smooth_coef)
    return ray_dist


# ------------------------------------------------------------------------------------------------
# centre-candidate point descriptors (reference descriptors.py:1288-1369, :1498-1528, :1761-1895): label histograms in
# concentric rings and ray features against border labels, one launch for all positions (csrc/points.hip)
# ------------------------------------------------------------------------------------------------


def _disc(radius):
    """``skimage.morphology.disk(radius)``: 1 where dy^2 + dx^2 <= radius^2 on the (2 radius + 1)^2 grid"""
    axis = np.arange(-radius, radius + 1)
    return np.array(axis[:, None] ** 2 + axis[None, :] ** 2 <= radius ** 2, dtype=np.uint8)


def _positions_inside(positions, shape):
    return bool(np.all((positions >= 0) & (positions < np.asarray(shape[:2]))))


def _device_radii(diameters):
    """the radii as the ring kernels take them (sorted, distinct) and the place of every given radius among them; None when the
    radii are not integers the kernels accept"""
    radii = np.asarray(diameters)
    if radii.ndim != 1 or radii.dtype.kind not in 'iu' or len(radii) == 0 or radii.min() < 0 or radii.max() > 16384:
        return None
    return np.unique(radii, return_inverse=True)


def _disc_label_hists(segm, positions, diameters, nb_labels):
    """label counts P x D x nb_labels under the discs and the sizes P x D of the clipped discs, both float64 of exact integers"""
    if segm.dtype.kind == 'f':
        segm = np.where(np.isnan(segm), -1, segm)                 # NaN marks "no label" (descriptors.py:1490)
    device = _device_radii(diameters) if _positions_inside(positions, segm.shape) else None
    if device is not None and len(device[0]) * (int(nb_labels) + 1) <= _hip.RING_MAX_BINS:
        hist, size = _hip.ring_hist2d(segm, positions, device[0], nb_labels)
        return hist[:, device[1], :].astype(float), size[:, device[1]].astype(float)
    # more counters than a lane's LDS columns hold ("Point descriptors"), radii that are no integers, or a position
    # outside the map: one batched launch per disc
    per_disc = [compute_label_hist_positions(segm, positions, _disc(d), nb_labels) for d in diameters]
    return np.stack([h for h, _ in per_disc], axis=1), np.stack([s for _, s in per_disc], axis=1)


def _disc_layer_sums(segm, positions, diameters):
    """layer sums P x D x C under the discs (float64) and the sizes P x D of the clipped discs"""
    device = _device_radii(diameters) if _positions_inside(positions, segm.shape) else None
    if device is None:
        per_pos = [[compute_label_hist_proba(segm, pos, _disc(d)) for d in diameters] for pos in positions]
        return (np.array([[h for h, _ in row] for row in per_pos], dtype=float).reshape(len(positions), len(diameters), segm.shape[-1]),
                np.array([[s for _, s in row] for row in per_pos], dtype=float).reshape(len(positions), len(diameters)))
    radii, place = device
    sums, sizes = [], []
    for first in range(0, len(radii), _hip.RING_PROBA_MAX_DISCS):   # the discs of a launch are complete on their own
        total, size = _hip.ring_hist_proba2d(segm, positions, radii[first:first + _hip.RING_PROBA_MAX_DISCS])
        sums.append(total)
        sizes.append(size)
    return np.concatenate(sums, axis=1)[:, place, :], np.concatenate(sizes, axis=1)[:, place].astype(float)


def compute_label_hist_proba(segm, position, struc_elem):
    """ sums of the layers of ``segm`` (H x W x C, one layer per label) under ``struc_elem`` around ``position`` and the size of
    the clipped element (reference ``descriptors.py:1498-1528``)

    A single position under an arbitrary element is numpy on the host, as in the reference; the discs of
    :func:`compute_label_histograms_positions` are summed on the device for all positions at once.

    >>> seg = np.zeros((50, 50, 2), dtype=float)
    >>> seg[15:35, 20:40, 1] = 1
    >>> seg[:, :, 0] = 1 - seg[:, :, 1]
    >>> hist, size = compute_label_hist_proba(seg, (15, 20), np.ones((12, 13), dtype=int))
    >>> hist.tolist(), int(size)
    ([114.0, 42.0], 156)
    """
    segm, struc_elem = np.asarray(segm), np.asarray(struc_elem)
    if segm.ndim != (len(position) + 1):
        raise ValueError('segment. (%r) should have larger (+1) dim than position %i' % (segm.shape, len(position)))
    position = [int(p) for p in position]
    im_begin, im_end, bb_begin, bb_end = adjust_bounding_box_crop(segm.shape[:struc_elem.ndim], struc_elem.shape, position)
    crop = segm[im_begin[0]:im_end[0], im_begin[1]:im_end[1], :]
    elem = struc_elem[bb_begin[0]:bb_end[0], bb_begin[1]:bb_end[1]]
    if crop.shape[:-1] != elem.shape:
        raise ValueError('initial dim of segmentation %r should match element %r' % (crop.shape, elem))
    layers = np.rollaxis(crop, -1, 0) * np.tile(elem, (crop.shape[-1], 1, 1))
    return np.sum(layers, axis=(1, 2)), np.sum(elem)


def compute_label_histograms_positions(segm, positions, diameters=HIST_CIRCLE_DIAGONALS, nb_labels=None):
    """ label histograms in consecutive rings around the positions (reference ``descriptors.py:1288-1369``)

    Ring d lies between the discs ``skimage.morphology.disk(diameters[d - 1])`` and ``disk(diameters[d])`` (the reference hands
    its "diameters" to ``disk`` as radii), clipped to the map; its value per label is the difference of the two discs' counts
    over the difference of their sizes.  For a label map ``segm`` (H x W) the counts, for probability layers (H x W x C) the
    float64 sums of all positions and discs come from ONE launch that reads every window once (``imsegm_ring_hist2d`` /
    ``imsegm_ring_hist_proba2d``); the division is float64 on the host.

    :param ndarray segm: H x W labels or H x W x C layers
    :param list(tuple(int,int)) positions: (row, col)
    :param list(int) diameters: radii of the discs
    :param int nb_labels: number of labels (the maximum + 1, or C)
    :return tuple(ndarray,list(str)): features P x (D * nb_labels), names 'hist-d_%i-lb_%i'
    """
    segm = np.asarray(segm)
    pos_dim = np.asarray(positions).shape[1]
    if (segm.ndim - pos_dim) not in (0, 1):
        raise ValueError('dimension %r and %r difference should be 0 or 1' % (segm.ndim, pos_dim))
    if pos_dim != 2:
        raise ValueError('positions have to be (row, col), not %r values' % pos_dim)
    layers = segm.ndim == pos_dim + 1
    if nb_labels is None:
        nb_labels = segm.shape[-1] if layers else segm.max() + 1
    diameters = list(diameters)
    # int(p) of the reference: towards zero
    points = np.array([[int(p) for p in pos] for pos in positions], dtype=np.int64).reshape(-1, 2)
    if layers:
        hist, size = _disc_layer_sums(segm, points, diameters)
    else:
        hist, size = _disc_label_hists(segm, points, diameters, int(nb_labels))
    # the rings, with the two checks of the reference's loop at the first position and disc that fails one
    hist_last = np.concatenate([np.zeros_like(hist[:, :1]), hist[:, :-1]], axis=1)
    inter_size = size - np.concatenate([np.zeros_like(size[:, :1]), size[:, :-1]], axis=1)
    empty, shrinks = inter_size <= 0, ~np.all(hist >= hist_last, axis=2)
    if np.any(empty | shrinks):
        pos, disc = np.unravel_index(np.argmax(empty | shrinks), empty.shape)
        if empty[pos, disc]:
            raise ValueError('norm or element should be positive')
        raise ValueError('outer elem should have more labels %r then the inter %r'
                         % (hist[pos, disc].tolist(), hist_last[pos, disc].tolist()))
    with np.errstate(invalid='ignore', divide='ignore'):
        pos_hists = ((hist - hist_last) / inter_size[:, :, None]).reshape(len(points), hist.shape[1] * hist.shape[2])
    feature_names = ['hist-d_%i-lb_%i' % (d, lb) for d in diameters for lb in range(nb_labels)]
    if pos_hists.shape[1] != len(feature_names):
        raise ValueError('histogram: %r and names %r' % (pos_hists.shape, feature_names))
    return pos_hists, feature_names


def shift_ray_features(ray_dist, method='phase'):
    """ rotate ray features to start at their main direction (reference ``descriptors.py:1761-1802``): the phase of the strongest
    component of the spectrum of five periods (``method='phase'``), or the maximum; numpy on the host (an FFT of 5 A points)

    >>> vec = np.array([43, 46, 44, 39, 28, 18, 12, 10,  9, 12, 22, 28])
    >>> ray, shift = shift_ray_features(vec)
    >>> ray.tolist(), round(float(shift), 1)
    ([46, 44, 39, 28, 18, 12, 10, 9, 12, 22, 28, 43], 41.5)

    :return tuple(ndarray,float): the rotated features, the shift in degrees
    """
    ray_dist = np.asarray(ray_dist)
    angle_step = 360 / len(ray_dist)
    if method == 'phase':
        periods = np.hstack([ray_dist] * 5)
        spectrum = np.fft.fft(periods - np.mean(periods)) / float(len(periods))
        strongest = np.argmax(np.abs(spectrum)[:len(periods) // 2])
        shift = np.rad2deg(-np.angle(spectrum)[:len(periods) // 2][strongest])
        shift = (360 + shift) if shift < 0 else shift
    else:
        shift = float(np.argmax(ray_dist) * angle_step)
    steps = int(round(shift / angle_step))
    return np.array(ray_dist[steps:].tolist() + ray_dist[:steps].tolist()), shift


def shift_ray_features_rows(rays, method='phase'):
    """ :func:`shift_ray_features` of every row of a P x A table at once: the five periods side by side, the mean taken off per row,
    ONE ``np.fft.fft(axis=1)`` and one ``argmax`` for the whole table instead of P small ones (numpy transforms every row of a batch
    with the routine it takes for a single vector, so the spectra are the bits of the row loop); the rotation per row keeps the
    loop's Python ``round``.  The table has the dtype ``np.array`` gives the loop's lists (float64 for any float table).

    >>> rays, shifts = shift_ray_features_rows(np.array([[43, 46, 44, 39, 28, 18, 12, 10,  9, 12, 22, 28]] * 2))
    >>> rays.tolist()[1], [round(float(s), 1) for s in shifts]
    ([46, 44, 39, 28, 18, 12, 10, 9, 12, 22, 28, 43], [41.5, 41.5])

    :param ndarray rays: P x A
    :return tuple(ndarray,list(float)): the rotated rows, the shifts in degrees
    """
    rays = np.asarray(rays)
    if rays.ndim != 2 or rays.size == 0:
        return rays, [0.] * (len(rays) if rays.ndim == 2 else 0)
    nb_angles = rays.shape[1]
    angle_step = 360 / nb_angles
    if method == 'phase':
        periods = np.hstack([rays] * 5)
        half = periods.shape[1] // 2
        spectrum = np.fft.fft(periods - np.mean(periods, axis=1, keepdims=True), axis=1) / float(periods.shape[1])
        rows = np.arange(len(rays))
        strongest = np.argmax(np.abs(spectrum)[:, :half], axis=1)
        shifts = np.rad2deg(-np.angle(spectrum)[:, :half][rows, strongest])
        shifts = [(360 + shift) if shift < 0 else shift for shift in shifts]
    else:
        shifts = [float(best * angle_step) for best in np.argmax(rays, axis=1)]
    steps = np.array([int(round(shift / angle_step)) for shift in shifts], dtype=np.int64)
    # row[steps:] + row[:steps] of the loop: a step at or beyond the row's end leaves the row as it is, a negative one counts from it
    steps = np.where(steps >= nb_angles, 0, np.where(steps < 0, np.maximum(steps + nb_angles, 0), steps))
    turned = np.take_along_axis(rays, (np.arange(nb_angles)[None, :] + steps[:, None]) % nb_angles, axis=1)
    if turned.dtype.kind == 'f' and turned.dtype.itemsize <= 8:
        return turned.astype(np.float64), shifts
    if turned.dtype.kind == 'b' or (turned.dtype.kind == 'i' and turned.dtype.itemsize <= 8):
        return turned.astype(np.bool_ if turned.dtype.kind == 'b' else np.int64), shifts
    return np.array(turned.tolist()), shifts


def _border_table(segm, border_labels):
    """the label map and the label table ``imsegm_ray_features_labels2d`` takes; a map that int32 does not hold exactly, or more
    labels than the table has room for: the mask, formed on the host, against the table [1]"""
    if segm.dtype.kind in 'iub' and len(border_labels) <= _hip.RAY_MAX_BORDER_LABELS:
        info = np.iinfo(np.int32)
        if segm.dtype.itemsize <= 2 or segm.dtype == np.int32 or (segm.size and info.min <= segm.min() and segm.max() <= info.max):
            return segm, [int(lb) for lb in border_labels if lb == int(lb) and info.min <= lb <= info.max]
    return np.isin(segm, list(border_labels)), [1]


def compute_ray_features_positions(segm, list_positions, angle_step=5., border_labels=None, segm_open=None, smooth_ray=None,
                                   shifting=True, edge='up'):
    """ ray features of many positions against the labels ``border_labels`` (reference ``descriptors.py:1805-1895``)

    One launch (``imsegm_ray_features_labels2d``) serves all positions: the mask ``segm in border_labels`` is formed on the device
    from the label table, the rays are walked as ``computeRayFeaturesBinary2d`` walks them, and ``smooth_ray`` is
    ``scipy.ndimage.gaussian_filter1d`` along the angle, in the same kernel.  What stays on the host: ``np.argmax`` over the layers
    of an H x W x C ``segm``; the phase shift (:func:`shift_ray_features`, row by row); and ``segm_open``, which is not moved to
    the device -- the mask is formed and opened with ``skimage.morphology.opening`` on the host (imported only then, as in the
    reference) before the upload.

    :param ndarray segm: H x W labels or H x W x C layers
    :param list(tuple(int,int)) list_positions: (row, col)
    :param float angle_step: degrees between two rays
    :param list(int) border_labels: the labels the rays stop at, [0] by default
    :param int segm_open: radius of the disc the mask is opened with
    :param float smooth_ray: sigma of the smoothing along the angle
    :param bool shifting: rotate every row to its main phase
    :param str edge: 'up' or 'down'
    :return tuple(ndarray,list(float),list(str)): distances P x A, shifts, names 'ray-lb_%s-agl_%i'
    """
    logging.debug('compute Ray features with border label=%r and angle step=%f', border_labels, angle_step)
    segm = np.asarray(segm)
    pos_dim = np.asarray(list_positions).shape[1]
    if (segm.ndim - pos_dim) not in (0, 1):
        raise ValueError('dimension %s and %s difference should be 0 or 1' % (segm.ndim, pos_dim))
    border_labels = border_labels if border_labels is not None else [0]
    if segm.ndim > pos_dim:
        segm = np.argmax(segm, axis=-1)
    if segm.ndim != pos_dim:
        raise ValueError('Segmentation dim of %r and position (%i) does not match' % (segm.ndim, pos_dim))
    if pos_dim != 2:
        raise ValueError('positions have to be (row, col), not %r values' % pos_dim)
    if isinstance(segm_open, int):
        from skimage import morphology
        segm, table = morphology.opening(np.isin(segm, list(border_labels)), morphology.disk(segm_open)), [1]
    else:
        segm, table = _border_table(segm, border_labels)
    points = np.array([[int(p) for p in pos] for pos in list_positions], dtype=np.int64).reshape(-1, 2)
    taps = _hip.gaussian_taps(smooth_ray) if smooth_ray is not None and smooth_ray > 0 else None
    rays = _hip.ray_features_labels2d(segm, table, points, _ray_directions(float(angle_step)), {'down': -1, 'up': 1}[edge], taps)
    pos_shift = [0.] * len(rays)
    if shifting and len(rays):
        shifted = [shift_ray_features(row) for row in rays]
        rays, pos_shift = np.array([row for row, _ in shifted]), [float(shift) for _, shift in shifted]
    feature_names = ['ray-lb_%s-agl_%i' % (''.join(map(str, border_labels)), int(a))
                     for a in np.linspace(0, 360 - angle_step, rays.shape[1])]
    return rays, pos_shift, feature_names


def reduce_close_points(points, dist_thr):
    """ drop points until no two are closer than ``dist_thr`` (reference ``descriptors.py:2005-2041``): of the closest pair (the first
    in row-major order of the distance matrix) the point with the larger index goes.  numpy on the host: at most a few dozen points

    >>> reduce_close_points(np.array([range(10), range(10)]).T, 2).tolist()
    [[0, 0], [2, 2], [4, 4], [6, 6], [8, 8]]
    >>> reduce_close_points(np.array([[0, 0], [1, 1], [0, 2]]), 2).tolist()
    [[0, 0], [0, 2]]
    >>> reduce_close_points(np.ones((10, 2)), 2).tolist()
    [[1.0, 1.0]]

    :param ndarray points: N x 2, more than 2, in their order along the contour
    :param float dist_thr: the smallest distance that may remain
    :return ndarray: the points kept
    """
    from scipy.spatial.distance import cdist
    if len(points) <= 2:
        raise ValueError('too few point to be reduced')
    dist = cdist(points, points, metric='euclidean')
    np.fill_diagonal(dist, np.inf)
    while dist.size and np.min(dist) < dist_thr:
        worse = max(np.unravel_index(dist.argmin(), dist.shape))
        points = np.delete(points, worse, axis=0)
        dist = np.delete(np.delete(dist, worse, axis=0), worse, axis=1)
    return points


def interpolate_ray_dist(ray_dists, order='spline'):
    """the ray distances with those that met no edge (``-1``) filled in from the others (reference ``descriptors.py:1898-1962``; its
    examples are in tests/doctests/region_growing.py).  On the host: it is reached only when a ray leaves the image.

    :param list(float) ray_dists: one distance per angle
    :param str|int order: degree of a polynomial through the known rays (``np.polyfit``), or 'spline' for an interpolating spline
        through three turns of them (``InterpolatedUnivariateSpline``)
    :return ndarray: a copy; unchanged when no ray is known
    """
    rays = np.array(ray_dists)
    known, holes = np.nonzero(rays != -1)[0], np.nonzero(rays == -1)[0]
    if len(known) == 0:
        return rays
    if isinstance(order, int):
        rays[holes] = np.polyval(np.polyfit(known, rays[known], order), holes)
    elif order == 'spline':
        from scipy.interpolate import InterpolatedUnivariateSpline
        # the angle is periodic: the known rays once more a turn before and a turn after
        turns = np.concatenate([known - len(rays), known, known + len(rays)])
        rays[holes] = InterpolatedUnivariateSpline(turns, np.tile(rays[known], 3))(holes)
    elif order == 'cos':
        raise NotImplementedError("interpolate_ray_dist: order 'cos' (a least-squares sine fit) is not provided")
    return rays
