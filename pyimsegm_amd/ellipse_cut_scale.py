"""Cut-outs of ellipse-annotated eggs, scaled to the normal size of their stage: the reference's
``experiments_ovary_detect/run_ellipse_cut_scale.py`` without files, tables and process pools.  Per egg the script rasterises the
matched ellipse (``add_overlap_ellipse`` on an empty map), cuts the egg out under that mask (``cut_object``), resizes the cut-out
with ``skimage.transform.resize`` to ``(int(median b), int(median a))`` of the stage and writes it as an 8-bit image
(``export_image``).  The result is exactly what :mod:`pyimsegm_amd.egg_orientation` reads.

* :func:`resize_image_host` -- ``skimage.transform.resize(img, output_shape)`` with the defaults of scikit-image 0.18.3 for uint8
  images, restated in numpy and scipy.  **This statement is the definition**; scikit-image is not needed.
* :func:`resize_images` -- a list of uint8 images of any sizes to one float64 stack.
* :func:`export_image_array` -- the array half of the reference's ``export_image``.
* :func:`stage_norm_size` -- the normal size of a stage from its ellipses.
* :func:`extract_ellipse_objects`, :func:`extract_ellipse_objects_host` -- the loop of ``extract_ellipse_object`` over all ellipses
  of one image.

**The resize** ("Cut and scale").  The anti-aliasing blur is integer-typed: ``resize`` hands the *uint8* image
to ``scipy.ndimage.gaussian_filter(image, sigma, mode='mirror')`` with ``sigma = max(0, (in / out - 1) / 2)`` per axis; the filter
runs along the rows' axis, then the columns' axis, and after each the fp64 sum is cast back to uint8 by truncation, so that a
constant area of value ``v`` can come out as ``v - 1``.  Then the image becomes ``uint8 * (1 / 255)`` in fp64, a bilinear lookup
runs at ``r = (H / h) (y + 0.5) - 0.5``, ``c = (W / w) (x + 0.5) - 0.5`` with neighbours beyond the edge mirrored without repeating
the edge, and the result is clipped to the range of the blurred image.  scikit-image takes its two factors from a least-squares
``AffineTransform.estimate``; the statement here takes the exact quotients, which differs from scikit-image by some 1e-14.

The device (``imsegm_ellipse_cut_scale``, ``imsegm_resize_crops``; csrc/resize.hip) equals the host statements byte for byte.  It
takes uint8 images of 1 to 4 channels, at most ``CUT_OBJECTS_MAX_LABELS`` ellipses per call and blur radii up to
``RESIZE_MAX_RADIUS``; anything else takes the host statements, silently.  ``on='host'`` or ``IMSEGM_CUT_SCALE_ON=host`` asks for
the host statements."""
import numpy as np

from . import _hip
from .ellipse_fitting import _int_params, ellipse_geometry, ellipse_pixels_host
from .utilities.data_io import _hook_geometry, cut_object_host, get_image2d_boundary_color

__all__ = ['COLUMNS_ELLIPSE', 'NORM_FUNC', 'resize_image_host', 'resize_images', 'export_image_array', 'stage_norm_size',
           'extract_ellipse_objects', 'extract_ellipse_objects_host', 'blur_taps']

#: the columns of an ellipse row, as the script names them: centre (first and second image axis), the two radii, the angle
COLUMNS_ELLIPSE = ['ellipse_xc', 'ellipse_yc', 'ellipse_a', 'ellipse_b', 'ellipse_theta']
NORM_FUNC = np.median  # other options - mean, max, ...


#: where a call runs that asks for nothing, when a device is present: what tools/time_cut_scale.py measured
DEFAULT_PLACE = 'device'


def _place(on):
    """'host' or 'device': ``_hip.resolve_place`` on IMSEGM_CUT_SCALE_ON ('device' without a device raises); with nothing asked
    and a device present, ``DEFAULT_PLACE``"""
    place, explicit = _hip.resolve_place(on, 'IMSEGM_CUT_SCALE_ON', True)
    return place if explicit or place == 'host' else DEFAULT_PLACE


# ------------------------------------------------------------------------------------------------
# the host statements
# ------------------------------------------------------------------------------------------------


def _blur_sigmas(in_shape, out_shape):
    """scikit-image's ``anti_aliasing_sigma`` of the two image axes: ``max(0, (in / out - 1) / 2)``"""
    factors = np.asarray(in_shape[:2], dtype=float) / np.asarray(out_shape[:2], dtype=float)
    return np.maximum(0, (factors - 1) / 2)


def blur_taps(sigma):
    """(radius, weights float64 [radius + 1]) of ``scipy.ndimage.gaussian_filter1d(..., sigma)`` as the device takes them:
    ``weights[j]`` is the weight at distance ``j`` from the centre -- ``exp(-0.5 / sigma^2 * x^2)`` over ``arange(-r, r + 1)``
    divided by its sum, ``r = int(4 sigma + 0.5)``.  An axis that scipy skips (sigma <= 1e-15) is radius 0 with the weight 1, which
    leaves every byte as it is."""
    sigma = float(sigma)
    if not sigma > 1e-15:
        return 0, np.ones(1)
    radius = int(4.0 * sigma + 0.5)
    x = np.arange(-radius, radius + 1)
    phi_x = np.exp(-0.5 / (sigma * sigma) * x ** 2)
    phi_x = phi_x / phi_x.sum()
    return radius, np.ascontiguousarray(phi_x[radius:])


def blur_image_host(img, output_shape, anti_aliasing_sigma=None):
    """the anti-aliasing step of ``resize``: ``ndi.gaussian_filter`` on the uint8 image itself, sigma 0 on the channel axis;
    ``anti_aliasing_sigma``: the two sigmas, as scikit-image's parameter of that name, instead of ``max(0, (in / out - 1) / 2)``"""
    from scipy import ndimage as ndi
    sigmas = _blur_sigmas(img.shape, output_shape) if anti_aliasing_sigma is None else anti_aliasing_sigma
    sigmas = tuple(float(sigma) for sigma in sigmas) + (0, ) * (img.ndim - 2)
    return ndi.gaussian_filter(img, sigmas, cval=0, mode='mirror')


def _mirror(index, size):
    """indices beyond 0 .. size - 1 mirrored without repeating the edge (-1 -> 1); an axis of length 1 reads its single pixel"""
    if size == 1:
        return np.zeros_like(index)
    period = 2 * (size - 1)
    index = np.abs(index) % period
    return np.where(index > size - 1, period - index, index)


def _lookup_axis(size_in, size_out, single):
    """(low index, high index, weight of the high one) of the bilinear lookup along one axis"""
    if single:
        coords = np.array([size_in / 2.0 - 0.5])
    else:
        coords = (float(size_in) / float(size_out)) * (np.arange(size_out, dtype=np.float64) + 0.5) - 0.5
    low, high = np.floor(coords), np.ceil(coords)
    return _mirror(low.astype(np.int64), size_in), _mirror(high.astype(np.int64), size_in), coords - low


def resize_image_host(img, output_shape, anti_aliasing_sigma=None):
    """ the numpy / scipy statement of ``skimage.transform.resize(img, output_shape)`` with the defaults of scikit-image 0.18.3
    (order 1, mode 'reflect', anti-aliasing, clip) for a uint8 image [H, W] or [H, W, C]; see the module's docstring.

    >>> img = np.arange(48, dtype=np.uint8).reshape(6, 8) * 5
    >>> out = resize_image_host(img, (3, 4))
    >>> out.shape, out.dtype
    ((3, 4), dtype('float64'))
    >>> export_image_array(out)
    array([[ 33,  45,  57,  68],
           [127, 138, 151, 162],
           [220, 232, 244, 255]], dtype=uint8)

    :param ndarray img: uint8 image [H, W] or [H, W, C]
    :param tuple(int,int) output_shape: (h, w)
    :param tuple(float,float) anti_aliasing_sigma: the sigmas of the blur along the two image axes; None: scikit-image's default
    :return ndarray: float64 [h, w] or [h, w, C], values in [0, 1]
    """
    img = np.asarray(img)
    if img.dtype != np.uint8 or img.ndim not in (2, 3) or img.size == 0:
        raise ValueError('a non-empty uint8 image [H, W] or [H, W, C] is expected, not %s %r' % (img.dtype, img.shape))
    h, w = int(output_shape[0]), int(output_shape[1])
    if h < 1 or w < 1:
        raise ValueError('the output shape %r has to be positive' % (tuple(output_shape), ))
    blurred = blur_image_host(img, (h, w), anti_aliasing_sigma)
    a = np.multiply(blurred, 1. / 255, dtype=np.float64)
    single = h == 1 and w == 1
    r0, r1, dr = _lookup_axis(img.shape[0], h, single)
    c0, c1, dc = _lookup_axis(img.shape[1], w, single)
    if a.ndim == 3:
        dr, dc = dr[:, None, None], dc[None, :, None]
    else:
        dr, dc = dr[:, None], dc[None, :]
    p00, p01 = a[r0[:, None], c0[None, :]], a[r0[:, None], c1[None, :]]
    p10, p11 = a[r1[:, None], c0[None, :]], a[r1[:, None], c1[None, :]]
    out = (1 - dr) * ((1 - dc) * p00 + dc * p01) + dr * ((1 - dc) * p10 + dc * p11)
    return np.clip(out, a.min(), a.max())


def export_image_array(img, stretch_range=True):
    """ the array half of the reference's ``export_image`` (``utilities/data_io.py:453-462``) for 2-D and 3-channel images: with
    ``stretch_range`` and a maximum above 0 the image is divided by its maximum and multiplied by 255, then truncated to uint8

    >>> export_image_array(np.array([[0., 0.5], [0.25, 0.125]]))
    array([[  0, 255],
           [127,  63]], dtype=uint8)
    >>> export_image_array(np.zeros((2, 2)))
    array([[0, 0],
           [0, 0]], dtype=uint8)
    """
    img = np.asarray(img)
    if img.ndim < 2:
        raise ValueError('wrong image dim: %r' % (img.shape, ))
    if stretch_range and img.max() > 0:
        img = img / float(img.max()) * 255
    return img.astype(np.uint8)


def stage_norm_size(ellipses, norm_func=NORM_FUNC):
    """ the normal size of a development stage (``perform_stage`` :85-87): ``(int(norm_func(b)), int(norm_func(a)))`` of the rows
    ``xc, yc, a, b, theta`` (:data:`COLUMNS_ELLIPSE`)

    >>> stage_norm_size([(50, 60, 30.5, 20, 0.), (10, 10, 40, 25.8, 1.), (30, 30, 33, 21, 2.)])
    (21, 33)
    """
    ellipses = np.asarray(ellipses, dtype=np.float64).reshape(-1, 5)
    return int(norm_func(ellipses[:, 3])), int(norm_func(ellipses[:, 2]))


def _ellipse_mask_host(shape, ellipse):
    """``add_overlap_ellipse(np.zeros(shape, dtype=int), ellipse, 1)``: an empty map has no label to overlap"""
    mask = np.zeros(shape[:2], dtype=int)
    c1, c2, h, w, phi = _int_params(ellipse)
    rr, cc = ellipse_pixels_host(c1, c2, h, w, orientation=phi, shape=mask.shape)
    mask[rr, cc] = 1
    return mask


def _bg_color(img):
    return get_image2d_boundary_color(img)


def extract_ellipse_objects_host(img, ellipses, norm_size, as_uint8=True):
    """:func:`extract_ellipse_objects` from the host statements alone: ``ellipse_pixels_host``, ``cut_object_host``,
    :func:`resize_image_host` and :func:`export_image_array`"""
    img = np.asarray(img)
    ellipses = [tuple(ell) for ell in ellipses]
    bg_color = _bg_color(img)
    cuts = []
    for ell in ellipses:
        mask = _ellipse_mask_host(img.shape, ell)
        cut = cut_object_host(img, mask, 0, use_mask=True, bg_color=bg_color)
        norm = resize_image_host(cut, norm_size)
        cuts.append(export_image_array(norm) if as_uint8 else norm)
    return _as_stack(cuts, img, norm_size, as_uint8)


def _as_stack(cuts, img, norm_size, as_uint8):
    channels = () if img.ndim == 2 else (img.shape[2], )
    shape = (len(cuts), int(norm_size[0]), int(norm_size[1])) + channels
    return np.asarray(cuts, dtype=np.uint8 if as_uint8 else np.float64).reshape(shape)


# ------------------------------------------------------------------------------------------------
# what the device takes
# ------------------------------------------------------------------------------------------------


def _taps_of(sizes, norm_size):
    """radii int32 [n, 2] and weights float64 [n, 2, RESIZE_MAX_RADIUS + 1] of crops of ``sizes`` [n, 2]; None: a radius above the
    cap"""
    radii = np.zeros((len(sizes), 2), dtype=np.int32)
    weights = np.zeros((len(sizes), 2, _hip.RESIZE_MAX_RADIUS + 1), dtype=np.float64)
    known = {}
    for k, size in enumerate(sizes):
        for axis in (0, 1):
            key = (int(size[axis]), int(norm_size[axis]))
            if key not in known:
                known[key] = blur_taps(max(0., (float(key[0]) / float(key[1]) - 1) / 2))
            radius, taps = known[key]
            if radius > _hip.RESIZE_MAX_RADIUS:
                return None
            radii[k, axis] = radius
            weights[k, axis, :radius + 1] = taps
    return radii, weights


def _device_images(images):
    """the images as C-contiguous uint8 arrays [H_i, W_i, C] of one channel count 1 .. 4, or None"""
    out, channels = [], None
    for img in images:
        if not isinstance(img, np.ndarray) or img.dtype != np.uint8 or img.ndim not in (2, 3) or img.size == 0:
            return None
        img = np.ascontiguousarray(img).reshape(img.shape[0], img.shape[1], -1)
        if channels is None:
            channels = img.shape[2]
        if img.shape[2] != channels or not 1 <= channels <= _hip.CUT_OBJECTS_MAX_CHANNELS:
            return None
        out.append(img)
    return out


def resize_images(images, output_shape, on=None, as_uint8=False):
    """ :func:`resize_image_host` of every image of a list -- uint8 images of any sizes with one channel count -- as one stack.  On
    the device (``imsegm_resize_crops``) the images go up packed, the blur, the lookup and the export run on all of them in one
    launch each, and the stack comes down once.

    :param list(ndarray) images: uint8 images [H_i, W_i] or [H_i, W_i, C]
    :param tuple(int,int) output_shape: (h, w)
    :param str on: ``'device'``, ``'host'`` or None (``IMSEGM_CUT_SCALE_ON``)
    :param bool as_uint8: return the bytes of :func:`export_image_array` of every image instead
    :return ndarray: float64 (or uint8) [n, h, w] or [n, h, w, C]
    """
    images = [np.asarray(img) for img in images]
    h, w = int(output_shape[0]), int(output_shape[1])
    if not images:
        return np.zeros((0, h, w), dtype=np.uint8 if as_uint8 else np.float64)
    if len({img.ndim for img in images}) != 1 or len({img.shape[2:] for img in images}) != 1:
        raise ValueError('the images have to agree in their channels')
    if _place(on) == 'device' and h >= 1 and w >= 1:
        packed = _device_images(images)
        taps = None if packed is None else _taps_of([img.shape[:2] for img in packed], (h, w))
        if taps is not None:
            got = _hip.resize_crops(packed, (h, w), taps[0], taps[1], want_u8=as_uint8)
            if got is not None:
                stack = got[1] if as_uint8 else got[0]
                return stack if images[0].ndim == 3 else stack[..., 0]
    out = [resize_image_host(img, (h, w)) for img in images]
    return _as_stack([export_image_array(o) for o in out] if as_uint8 else out, images[0], (h, w), as_uint8)


def _hook_taps(norm_size):
    def taps(sizes):
        return _taps_of(sizes, norm_size)
    return taps


def extract_ellipse_objects(img, ellipses, norm_size, as_uint8=True, on=None):
    """ the loop of the reference's ``extract_ellipse_object`` (:46-72) over all ellipses of one image, without files: per ellipse
    the mask of ``add_overlap_ellipse(zeros, ell, 1)`` (so ellipses may overlap one another), ``cut_object(img, mask, 0,
    use_mask=True, bg_color=None)``, ``transform.resize`` to ``norm_size`` and, with ``as_uint8``, the bytes ``export_image``
    writes.  ``bg_color`` is taken once from the image.  The stack is what ``egg_orientation.swap_orientations`` takes as is.

    ``on='device'`` (``IMSEGM_CUT_SCALE_ON``): one ``imsegm_ellipse_cut_scale`` call -- the image goes up once, no mask is uploaded,
    the crops stay on the device between the cut and the resize, and the stack comes down once.  Images that are not uint8 or have
    more than 4 channels, more ellipses than ``CUT_OBJECTS_MAX_LABELS``, ellipses ``ellipse_geometry`` refuses and blur radii above
    ``RESIZE_MAX_RADIUS`` take :func:`extract_ellipse_objects_host`.  An ellipse whose clipped mask is empty raises ``IndexError``,
    as ``cut_object`` does.

    :param ndarray img: image [H, W] or [H, W, C]
    :param list(tuple) ellipses: rows ``xc, yc, a, b, theta`` (:data:`COLUMNS_ELLIPSE`)
    :param tuple(int,int) norm_size: (h, w), e.g. :func:`stage_norm_size`
    :param bool as_uint8: the exported bytes (default) or the float64 images
    :param str on: ``'device'``, ``'host'`` or None
    :return ndarray: uint8 or float64 [n, h, w, C] ([n, h, w] for a 2-D image)
    """
    img = np.asarray(img)
    ellipses = [tuple(ell) for ell in ellipses]
    h, w = int(norm_size[0]), int(norm_size[1])
    if ellipses and h >= 1 and w >= 1 and len(ellipses) <= _hip.CUT_OBJECTS_MAX_LABELS and _place(on) == 'device':
        image = _device_images([img])
        geometry = None if image is None or img.size >= 2 ** 31 else ellipse_geometry([_int_params(ell) for ell in ellipses], img.shape)
        if geometry is not None:
            got = _hip.ellipse_cut_scale(image[0], geometry[0], geometry[1], _bg_color(img), (h, w), _hook_geometry,
                                         _hook_taps((h, w)), want_u8=as_uint8)
            if got is not None:
                return got if img.ndim == 3 else got[..., 0]
    return extract_ellipse_objects_host(img, ellipses, (h, w), as_uint8)
