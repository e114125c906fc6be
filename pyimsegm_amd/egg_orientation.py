"""Orientation of egg cut-outs: the reference's ``experiments_ovary_detect/run_egg_swap_orientation.py`` without files and process
pools.  A per-pixel median over the whole stack of cut-outs of a stage gives a template, and every cut-out is turned by 180 degrees
when it agrees better with the template that way ('cc'), or when its bright pixels crowd its left third ('density').

* :func:`compute_mean_image` -- the template: the images cropped to their common minimum size, the median of channel 0;
* :func:`perform_orientation_swap` -- one cut-out against a template;
* :func:`swap_orientations` -- the whole of the script's ``main`` in one call: template, decisions and turned cut-outs;
* :func:`correlation_coefficient`, :func:`condition_swap_correl`, :func:`condition_swap_density` -- the reference's float statements
  restated in numpy.  They are the host definitions: ``on='host'`` or ``IMSEGM_ORIENTATION_ON=host`` computes with them.

**The device decides by an integer rule** ("Egg orientation"; :func:`stack_median2_host`,
:func:`orientation_sums_host` and :func:`orientation_flags_host` state it in numpy and the device equals them byte for byte).  The
template is kept as ``template2 = 2 * median``, a whole number.  A turned image has the mean and the deviation of the original, so
``cc < cc_swap`` holds exactly when ``P = sum(a * template2)`` is smaller than ``Pf = sum(a[::-1, ::-1] * template2)``, and both
coefficients are 0 when the image or the template is constant; at ``P == Pf`` the answer is "no swap".  ``a > mean`` of the density
test is ``a * cnt > S`` without a division.  The integer rule can differ from the float statement only where ``|cc - cc_swap|`` is
of the order of 1e-16, a rounding tie of the float statement; the median and the density test never differ.

The device takes uint8 images of 3 dimensions with 1 to 4 channels, at most 65 535 of them, and a given template only when
``2 * template`` is a whole number in 0 .. 510 everywhere (true of every median of a uint8 stack).  Anything else takes the host
statements, silently."""
import numpy as np

from . import _hip

__all__ = ['IMAGE_CHANNEL', 'SWAP_CONDITION', 'compute_mean_image', 'perform_orientation_swap', 'swap_orientations',
           'correlation_coefficient', 'condition_swap_correl', 'condition_swap_density', 'stack_median2_host',
           'orientation_sums_host', 'orientation_flags_host']

IMAGE_CHANNEL = 0  # image channel for mass extraction
SWAP_CONDITION = 'cc'
#: columns of :func:`orientation_sums_host` (``IMSEGM_ORIENT_SUM_WORDS`` words per image)
SUM_A, SUM_MIN, SUM_MAX, SUM_P, SUM_PF, SUM_CNT, SUM_S, SUM_L, SUM_R = range(9)


def _place(on):
    """'host' or 'device': ``_hip.resolve_place`` on IMSEGM_ORIENTATION_ON ('device' without a device raises)"""
    return _hip.resolve_place(on, 'IMSEGM_ORIENTATION_ON', True)[0]


def _load(images):
    """the list of arrays; entries that are paths go through ``load_image_2d`` of the ``imsegm.utilities.data_io`` in use (the
    reference's when one is installed: this package reads no image files itself)"""
    loaded = []
    for img in images:
        if isinstance(img, (str, bytes)) or hasattr(img, '__fspath__'):
            from imsegm.utilities import data_io
            if not hasattr(data_io, 'load_image_2d'):
                raise ValueError('an image given as a path needs imsegm.utilities.data_io.load_image_2d of an installed reference')
            img = data_io.load_image_2d(img)[0]
        loaded.append(np.asarray(img))
    return loaded


# ------------------------------------------------------------------------------------------------
# the float statements of the reference
# ------------------------------------------------------------------------------------------------


def correlation_coefficient(patch1, patch2):
    """the reference's ``correlation_coefficient`` (:83-89): 0 when a deviation is 0"""
    product = np.mean((patch1 - patch1.mean()) * (patch2 - patch2.mean()))
    stds = patch1.std() * patch2.std()
    if stds == 0:
        return 0
    product /= stds
    return product


def condition_swap_correl(img, img_template):
    """the reference's ``condition_swap_correl`` (:77-80): the turned image correlates better with the template"""
    cc = correlation_coefficient(img[:, :, IMAGE_CHANNEL], img_template)
    cc_swap = correlation_coefficient(img[::-1, ::-1, IMAGE_CHANNEL], img_template)
    return cc < cc_swap


def condition_swap_density(img):
    """the reference's ``condition_swap_density`` (:65-74): more pixels above the mean of the non-minimum pixels in the left third
    than in the right third.  A third of 0 columns makes the right part the whole image (``img[:, -0:]``); a division by zero
    gives inf or NaN, as numpy does, without a warning"""
    part = int(img.shape[1] / 3)
    sel_mask = img[:, :, IMAGE_CHANNEL] > np.min(img[:, :, IMAGE_CHANNEL])
    with np.errstate(all='ignore'):
        norm_val = np.mean(img[sel_mask, IMAGE_CHANNEL]) if sel_mask.any() else np.nan
        val_left = np.sum(img[:, :part, IMAGE_CHANNEL] > norm_val)
        val_right = np.sum(img[:, -part:, IMAGE_CHANNEL] > norm_val)
        ration = np.float64(val_left) / np.float64(val_right)
    return bool(ration > 1.)


# ------------------------------------------------------------------------------------------------
# the integer statements: what the device computes
# ------------------------------------------------------------------------------------------------


def _planes(stack):
    stack = np.asarray(stack)
    if stack.dtype != np.uint8 or stack.ndim != 3 or stack.size == 0:
        raise ValueError('the stack has to be a non-empty uint8 array [N, h, w] (one channel), not %s %r' % (stack.dtype, stack.shape))
    return stack


def stack_median2_host(stack):
    """``template2``: with ``s`` the N values of a pixel sorted, ``s[(N - 1) // 2] + s[N // 2]`` as uint16 [h, w] -- exactly
    ``2 * np.median(stack, axis=0)`` for a uint8 stack [N, h, w]"""
    stack = _planes(stack)
    n = len(stack)
    low, high = (n - 1) // 2, n // 2
    part = np.partition(stack, sorted({low, high}), axis=0)
    return part[low].astype(np.uint16) + part[high]


def orientation_sums_host(stack, template2):
    """the nine words of every image of a uint8 stack [N, h, w] against ``template2`` [h, w] as int64 [N, 9]: ``A = sum a``,
    ``min a``, ``max a``, ``P = sum a t``, ``Pf = sum a[::-1, ::-1] t``, ``cnt = #{a > min}``, ``S = sum of the a > min``, and with
    ``g = a * cnt > S`` and ``part = w // 3``: ``L = sum g[:, :part]``, ``R = sum g[:, w - part:]`` (``part == 0``: all of ``g``)"""
    stack = _planes(stack)
    template2 = np.asarray(template2).astype(np.int64)
    n, h, w = stack.shape
    if template2.shape != (h, w):
        raise ValueError('template2 %r and the images %r differ in size' % (template2.shape, (h, w)))
    part = w // 3
    sums = np.zeros((n, 9), dtype=np.int64)
    step = max(1, (1 << 20) // (h * w))
    for first in range(0, n, step):
        a = stack[first:first + step].astype(np.int64)
        out = sums[first:first + step]
        out[:, SUM_A] = a.sum(axis=(1, 2))
        out[:, SUM_MIN] = a.min(axis=(1, 2))
        out[:, SUM_MAX] = a.max(axis=(1, 2))
        out[:, SUM_P] = (a * template2).sum(axis=(1, 2))
        out[:, SUM_PF] = (a[:, ::-1, ::-1] * template2).sum(axis=(1, 2))
        above = a > out[:, SUM_MIN, None, None]
        out[:, SUM_CNT] = above.sum(axis=(1, 2))
        out[:, SUM_S] = (a * above).sum(axis=(1, 2))
        g = a * out[:, SUM_CNT, None, None] > out[:, SUM_S, None, None]
        out[:, SUM_L] = g[:, :, :part].sum(axis=(1, 2))
        out[:, SUM_R] = g[:, :, w - part:].sum(axis=(1, 2)) if part > 0 else g.sum(axis=(1, 2))
    return sums


def orientation_flags_host(sums, template2, swap_type=SWAP_CONDITION):
    """the decisions from the nine words, bool [N]: 'cc' = the image is not constant, the template is not constant and ``P < Pf``;
    anything else (density) = ``L > R``"""
    sums = np.asarray(sums)
    if swap_type == 'cc':
        template2 = np.asarray(template2)
        varies = template2.min() != template2.max()
        return (sums[:, SUM_MIN] != sums[:, SUM_MAX]) & varies & (sums[:, SUM_P] < sums[:, SUM_PF])
    return sums[:, SUM_L] > sums[:, SUM_R]


# ------------------------------------------------------------------------------------------------
# what the device takes
# ------------------------------------------------------------------------------------------------


def _device_stack(imgs, size):
    """the images cropped to ``size`` as one uint8 array [N, h, w, C], or None for what ``imsegm_orient_stack`` does not take"""
    height, width = size
    if not imgs or len(imgs) > _hip.ORIENT_MAX_IMAGES or height < 1 or width < 1 or height * width > 2 ** 30:
        return None
    channels = imgs[0].shape[2] if imgs[0].ndim == 3 else 0
    if not 1 <= channels <= 4 or len(imgs) * height * width * channels > 2 ** 31 - 1:
        return None
    for img in imgs:
        if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != channels or img.shape[0] < height or img.shape[1] < width:
            return None
    stack = np.empty((len(imgs), height, width, channels), dtype=np.uint8)
    for i, img in enumerate(imgs):
        stack[i] = img[:height, :width]
    return stack


def _template2_of(img_template):
    """``2 * template`` as uint16 when that is a whole number in 0 .. 510 everywhere, else None"""
    template = np.asarray(img_template)
    if template.ndim != 2 or template.size == 0 or template.dtype.kind not in 'biuf':
        return None
    doubled = template.astype(np.float64) * 2
    if not np.all(np.isfinite(doubled)) or doubled.min() < 0 or doubled.max() > 510 or np.any(doubled != np.rint(doubled)):
        return None
    return doubled.astype(np.uint16)


def _min_size(imgs):
    return tuple(int(v) for v in np.min([img.shape[:2] for img in imgs], axis=0))


# ------------------------------------------------------------------------------------------------
# the public functions
# ------------------------------------------------------------------------------------------------


def compute_mean_image(images, on=None):
    """ the template of a stage (the reference's ``compute_mean_image``): channel 0 of every image cropped to the per-axis minimum
    of the sizes, and the per-pixel median over the images.  On the device (``imsegm_stack_median_u8``): one lane per pixel, a
    radix selection over the stack.

    :param list images: arrays [h_i, w_i, C]; entries that are paths are loaded through ``data_io.load_image_2d``
    :return ndarray: float64 [h, w]
    """
    imgs = _load(images)
    if _place(on) == 'device' and imgs and all(img.ndim == 3 for img in imgs):
        stack = _device_stack(imgs, _min_size(imgs))
        template2 = None if stack is None else _hip.stack_median(stack, IMAGE_CHANNEL)
        if template2 is not None:
            return template2 / 2.
    planes = [img[:, :, IMAGE_CHANNEL] for img in imgs]
    min_size = np.min([img.shape for img in planes], axis=0)
    planes = [img[:min_size[0], :min_size[1]] for img in planes]
    return np.median(planes, axis=0)


def _decide(img, img_template, swap_type):
    if swap_type == 'cc':
        return bool(condition_swap_correl(img, img_template))
    return bool(condition_swap_density(img))


def perform_orientation_swap(img, img_template, swap_type=SWAP_CONDITION):
    """ compute the density in front and back part of the egg and rotate eventually (the reference's function without its files):
    the image cropped to the size of the template, turned as ``img[::-1, ::-1, :]`` when the swap condition holds.  The float
    statements decide.  An image smaller than the template raises the ``ValueError`` numpy raises for the correlation.

    :param ndarray img: input image [h, w, C] (a path is loaded)
    :param ndarray img_template: template / mean image
    :param str swap_type: used swap condition, 'cc' or density
    :return ndarray: the cropped, possibly turned image
    """
    img = _load([img])[0]
    img_size = np.asarray(img_template).shape
    img = img[:img_size[0], :img_size[1]]
    if _decide(img, img_template, swap_type):
        img = img[::-1, ::-1, :]
    return img


def _swap_device(imgs, swap_type, img_template):
    if not all(img.ndim == 3 for img in imgs):
        return None
    template2 = None
    if img_template is None:
        size = _min_size(imgs)
    else:
        template2 = _template2_of(img_template)
        if template2 is None:
            return None
        size = template2.shape
    stack = _device_stack(imgs, size)
    if stack is None:
        return None
    got = _hip.orient_stack(stack, IMAGE_CHANNEL, 'cc' if swap_type == 'cc' else 'density', template2, in_place=True)
    if got is None:
        return None
    template2, flags, _, turned = got
    return list(turned), flags, (template2 / 2. if img_template is None else np.asarray(img_template))


def swap_orientations(images, swap_type=SWAP_CONDITION, img_template=None, on=None):
    """ bring all cut-outs of a stage to one orientation: the whole of the reference's ``main`` (:101-128) in one call.  Without a
    given template it is :func:`compute_mean_image` of the images; every image goes through :func:`perform_orientation_swap`.

    With ``on='device'`` (the default where a device is present; ``IMSEGM_ORIENTATION_ON``) this is one ``imsegm_orient_stack``
    call: the stack goes up once, the median, the sums of the swap test and the turn run on it, and the integer rule of this
    module's docstring decides.  What the device does not take runs the host statements.

    :param list images: arrays [h_i, w_i, C]; entries that are paths are loaded through ``data_io.load_image_2d``
    :param str swap_type: 'cc' (correlation with the template) or density
    :param ndarray img_template: template [h, w], or None
    :return tuple(list,ndarray,ndarray): the oriented images, the swap flags bool [N], the template
    """
    imgs = _load(images)
    if _place(on) == 'device' and imgs:
        got = _swap_device(imgs, swap_type, img_template)
        if got is not None:
            return got
    template = compute_mean_image(imgs, on='host') if img_template is None else np.asarray(img_template)
    flags = np.zeros(len(imgs), dtype=bool)
    oriented = []
    for i, img in enumerate(imgs):
        img = img[:template.shape[0], :template.shape[1]]
        flags[i] = _decide(img, template, swap_type)
        oriented.append(img[::-1, ::-1, :] if flags[i] else img)
    return oriented, flags, template
