"""Colour-space helpers used by the descriptor stage (numpy restatements of the few
``skimage.color`` conversions the reference reaches through
``imsegm/utilities/data_io.py:28-58``; scikit-image itself is not a dependency of this package).
Image file I/O of the reference (PNG / TIFF / NIfTI / ZVI readers) is out of scope."""
import numpy as np

_XYZ_FROM_RGB = np.array([[0.412453, 0.357580, 0.180423], [0.212671, 0.715160, 0.072169],
                          [0.019334, 0.119193, 0.950227]])
_XYZ_WHITE_D65 = np.array([0.95047, 1., 1.08883])


def _as_float_rgb(image):
    image = np.asarray(image)
    if image.dtype == np.uint8:
        return image[..., :3].astype(np.float64) / 255.
    return image[..., :3].astype(np.float64)


def rgb2hsv(rgb):
    """ RGB -> HSV, all channels in [0, 1] (same formulas as ``skimage.color.rgb2hsv``)
    """
    arr = _as_float_rgb(rgb)
    out = np.empty_like(arr)
    v = arr.max(-1)
    delta = arr.max(-1) - arr.min(-1)
    with np.errstate(invalid='ignore', divide='ignore'):
        s = delta / v
        s[delta == 0.] = 0.
        h = np.empty_like(v)
        idx = arr[..., 0] == v
        h[idx] = ((arr[..., 1] - arr[..., 2]) / delta)[idx]
        idx = arr[..., 1] == v
        h[idx] = 2. + ((arr[..., 2] - arr[..., 0]) / delta)[idx]
        idx = arr[..., 2] == v
        h[idx] = 4. + ((arr[..., 0] - arr[..., 1]) / delta)[idx]
        h = (h / 6.) % 1.
        h[delta == 0.] = 0.
    out[..., 0], out[..., 1], out[..., 2] = h, s, v
    out[np.isnan(out)] = 0
    return out


def rgb2xyz(rgb):
    arr = _as_float_rgb(rgb).copy()
    mask = arr > 0.04045
    arr[mask] = np.power((arr[mask] + 0.055) / 1.055, 2.4)
    arr[~mask] /= 12.92
    return arr @ _XYZ_FROM_RGB.T


def rgb2lab(rgb):
    arr = rgb2xyz(rgb) / _XYZ_WHITE_D65
    mask = arr > 0.008856
    arr[mask] = np.cbrt(arr[mask])
    arr[~mask] = 7.787 * arr[~mask] + 16. / 116.
    x, y, z = arr[..., 0], arr[..., 1], arr[..., 2]
    return np.stack([116. * y - 16., 500. * (x - y), 200. * (y - z)], axis=-1)


def rgb2luv(rgb):
    xyz = rgb2xyz(rgb)
    x, y, z = xyz[..., 0], xyz[..., 1], xyz[..., 2]
    eps = np.finfo(np.float64).eps
    L = y / _XYZ_WHITE_D65[1]
    mask = L > 0.008856
    L = np.where(mask, 116. * np.cbrt(np.where(mask, L, 1.)) - 16., 903.3 * L)
    u0 = 4 * _XYZ_WHITE_D65[0] / np.dot([1, 15, 3], _XYZ_WHITE_D65)
    v0 = 9 * _XYZ_WHITE_D65[1] / np.dot([1, 15, 3], _XYZ_WHITE_D65)
    denom = x + 15 * y + 3 * z + eps
    u = 13. * L * (4. * x / denom - u0)
    v = 13. * L * (9. * y / denom - v0)
    return np.stack([L, u, v], axis=-1)


_HED_FROM_RGB = np.linalg.inv(np.array([[0.65, 0.70, 0.29], [0.07, 0.99, 0.11], [0.27, 0.57, 0.78]]))


def rgb2hed(rgb):
    """ RGB -> Haematoxylin-Eosin-DAB (colour deconvolution as ``skimage.color.rgb2hed`` of scikit-image 0.18: the
    stain values are not clipped at zero; newer releases clip them) """
    arr = np.maximum(_as_float_rgb(rgb), 1e-6)
    return (np.log(arr) / np.log(1e-6)) @ _HED_FROM_RGB


#: conversion function from RGB color space
DICT_CONVERT_COLOR_FROM_RGB = {'hsv': rgb2hsv, 'luv': rgb2luv, 'lab': rgb2lab, 'hed': rgb2hed, 'xyz': rgb2xyz}


def convert_img_color_from_rgb(image, color_space):
    """ convert image colour space from RGB to ``color_space`` (unknown names: image returned as is)
    """
    image = np.asarray(image)
    if image.ndim == 3 and image.shape[-1] in (3, 4) and color_space in DICT_CONVERT_COLOR_FROM_RGB:
        image = DICT_CONVERT_COLOR_FROM_RGB[color_space](image)
    return image


def get_image2d_boundary_color(image, size=1):
    """ the dominant value on the image border of width ``size`` (reference ``utilities/data_io.py:1002-1036``):
    the most frequent label of a 2D (label) image, the per-channel median of a colour image
    """
    import logging
    image = np.asarray(image)
    size = int(size)
    strips = [image[:size, :], image[:, :size], image[-size:, :], image[:, -size:]]
    if image.ndim == 2:
        pixels = np.concatenate([strip.ravel() for strip in strips])
        colour = np.argmax(np.bincount(pixels))
    elif image.ndim == 3:
        pixels = np.concatenate([strip.reshape(-1, image.shape[-1]) for strip in strips], axis=0)
        colour = np.median(pixels, axis=0)
    else:
        logging.error('not supported image dim: %r', image.shape)
        colour = np.array(0)
    return np.asarray(colour).astype(image.dtype)


# ------------------------------------------------------------------------------------------------
# cutting segmented objects out of an image (reference ``utilities/data_io.py:1039-1128``, the step behind
# experiments_ovary_detect/run_cut_segmented_objects.py and run_ellipse_cut_scale.py)
#
# ``cut_object`` centres the object (``scipy.ndimage.shift``, order 0), turns its main axis level (``scipy.ndimage.rotate``, order 0,
# reshape) and crops the padded bounding box of the turned mask.  What the reference does is restated here in numpy as
# ``cut_object_host`` -- neither scikit-image nor the reference is needed -- and ``cut_objects`` does it for all labels of a map in
# one device call (``imsegm_cut_objects``, csrc/cut_objects.hip).  The geometry of an object is ONE function, ``_cut_geometry``:
# the host statement and the device entry (through its geometry hook) both take it from there.
#
# * The region is all pixels of the mask as one region; count, sum r, sum c, sum r^2, sum c^2, sum rc are exact integers.  The
#   centroid is sum / count, one fp64 division per axis (scikit-image 0.18.3: ``coords.mean``).  The orientation is scikit-image
#   0.18.3's: inertia tensor a = mu02 / mu00, b = -mu11 / mu00, c = mu20 / mu00; +-pi/4 by the sign of b when a - c == 0, else
#   0.5 atan2(-2 b, c - a).  Here the central moments come from the integer sums scaled by count^2 (exact), which differs from
#   scikit-image's float moments in the last bits at the most; the golden cases are chosen away from rounding ties.
# * Two nearest-neighbour resamplings are composed, as scipy does them: per axis the coordinate ``x`` is outside the source when
#   x < 0 or x > n - 1 (scipy's mode 'constant'), otherwise the source index is floor(x + 0.5).  Shift: x = k + s with s = centroid
#   - n / 2.  Rotation: x = ((0 + i m0) + j m1) + offset, three fp64 operations in this order, never fused.
# * Outside the source the shift brings in 0 / False.  The rotation is called with ``cval=nan``: a float image gets nan, a uint8
#   image 0 -- that is what x86 makes of nan cast to uint8, the golden vectors record it --, a boolean mask False, and an int64
#   mask INT64_MIN, which counts as True under ``use_mask``.  That is why integer masks never go to the device: the host
#   statement reproduces it.
#
# The device takes uint8 images (H x W or H x W x C, C <= 4) with boolean masks or an integer label map; other image dtypes,
# integer and float masks and C > 4 take the host statement, silently.
# ------------------------------------------------------------------------------------------------

#: labels one ``imsegm_cut_objects`` call takes (``IMSEGM_CUT_OBJECTS_MAX_LABELS``); more are cut in several calls
CUT_OBJECTS_MAX_LABELS = 1024
#: canvas pixels around the forward image of the source box that the device still evaluates: each of the two roundings moves a
#: pixel by at most 0.5 per axis, 0.71 after the turn; 3 covers both with the floor / ceil of the corners
_CUT_WINDOW_MARGIN = 3


def add_padding(img_size, padding, min_row, min_col, max_row, max_col):
    """ add some padding but still be inside image (reference ``utilities/data_io.py:1039-1057``)

    :param tuple(int,int) img_size:
    :param int padding: set padding around segmented object
    :param int min_row: setting top left corner of bounding box
    :param int min_col: setting top left corner of bounding box
    :param int max_row: setting bottom right corner of bounding box
    :param int max_col: setting bottom right corner of bounding box
    :return tuple(int,int,int,int):

    >>> add_padding((50, 50), 5, 15, 25, 35, 55)
    (10, 20, 40, 50)
    """
    min_row = max(0, min_row - padding)
    min_col = max(0, min_col - padding)
    max_row = min(img_size[0], max_row + padding)
    max_col = min(img_size[1], max_col + padding)
    return min_row, min_col, max_row, max_col


def _region_moments(region):
    """count, sum r, sum c, sum r^2, sum c^2, sum rc and the closed box (r min, r max, c min, c max) of a boolean map as Python
    integers -- the ten words per label the device reduces"""
    rows, cols = np.nonzero(region)
    if len(rows) == 0:
        raise IndexError('list index out of range')          # regionprops(...)[0] of the reference
    rows, cols = rows.astype(np.int64), cols.astype(np.int64)
    return (len(rows), int(rows.sum()), int(cols.sum()), int((rows * rows).sum()), int((cols * cols).sum()), int((rows * cols).sum()),
            int(rows.min()), int(rows.max()), int(cols.min()), int(cols.max()))


def _orientation(moments):
    """scikit-image 0.18.3's ``RegionProperties.orientation`` from the integer sums: the tensor entries times count^2, exactly"""
    n, sr, sc, srr, scc, src = moments[:6]
    a = n * scc - sc * sc                                     # mu02 count
    c = n * srr - sr * sr                                     # mu20 count
    b = -(n * src - sr * sc)                                  # -mu11 count
    if a - c == 0:
        return -np.pi / 4. if b < 0 else np.pi / 4.
    return 0.5 * np.arctan2(float(-2 * b), float(c - a))


#: the orientation of one horizontal segment: what the reference subtracts (its PROP_ROTATION_OFFSET, data_io.py:1093-1096)
PROP_ROTATION_OFFSET = _orientation(_region_moments(np.array([[0] * 20, [1] * 20, [0] * 20], dtype=bool)))


def _cut_geometry(moments, shape, allow_rotate=True):
    """everything between the ten integer words of an object and its two index maps, in fp64 as the reference, scikit-image 0.18.3
    and scipy form it: a dict with ``centroid``, ``angle`` (degrees, what ``ndimage.rotate`` is handed), ``shift`` (s per axis),
    ``matrix`` (2 x 2), ``offset`` (2), ``canvas`` (shape of the turned frame) and ``window`` (r0, r1, c0, c1, half open, on the
    canvas: outside it the turned mask is False).  Without rotation both maps are the identity and the window is the source box."""
    height, width = int(shape[0]), int(shape[1])
    n, sr, sc = moments[:3]
    r_min, r_max, c_min, c_max = moments[6:10]
    centroid = (sr / float(n), sc / float(n))
    if not allow_rotate:
        return {'centroid': centroid, 'angle': 0., 'shift': np.zeros(2), 'matrix': np.eye(2), 'offset': np.zeros(2),
                'canvas': (height, width), 'window': (r_min, r_max + 1, c_min, c_max + 1)}
    from scipy import special
    rotate = np.rad2deg(_orientation(moments) - PROP_ROTATION_OFFSET)
    shift = np.array(centroid) - (np.array([height, width]) / 2.)
    # scipy.ndimage.rotate(..., angle, reshape=True), operation by operation
    angle = -rotate
    cos, sin = special.cosdg(angle), special.sindg(angle)
    matrix = np.array([[cos, sin], [-sin, cos]])
    in_plane_shape = np.array([height, width])
    out_bounds = matrix @ [[0, 0, height, height], [0, width, 0, width]]
    out_plane_shape = (np.ptp(out_bounds, axis=1) + 0.5).astype(int)
    out_center = matrix @ ((out_plane_shape - 1) / 2)
    in_center = (in_plane_shape - 1) / 2
    offset = in_center - out_center
    # where the source box can land on the canvas: canvas = matrix^T (shifted - offset), shifted = source - s
    corners = np.array([[r, c] for r in (r_min - 1, r_max + 1) for c in (c_min - 1, c_max + 1)], dtype=np.float64)
    landed = (corners - shift - offset) @ matrix
    low = np.floor(landed.min(axis=0)).astype(int) - _CUT_WINDOW_MARGIN
    high = np.ceil(landed.max(axis=0)).astype(int) + _CUT_WINDOW_MARGIN + 1
    canvas = (int(out_plane_shape[0]), int(out_plane_shape[1]))
    window = (max(0, int(low[0])), min(canvas[0], int(high[0])), max(0, int(low[1])), min(canvas[1], int(high[1])))
    return {'centroid': centroid, 'angle': float(angle), 'shift': shift, 'matrix': matrix, 'offset': offset, 'canvas': canvas,
            'window': window}


def _nearest_index(coordinate, size):
    """scipy's order-0 lookup along one axis in mode 'constant': (index, inside)"""
    inside = (coordinate >= 0) & (coordinate <= size - 1)
    return np.where(inside, np.floor(coordinate + 0.5), 0).astype(np.intp), inside


def _nan_as(dtype):
    """what scipy stores for ``cval=nan`` in an array of ``dtype`` on x86-64"""
    dtype = np.dtype(dtype)
    if dtype.kind == 'f':
        return dtype.type(np.nan)
    if dtype.kind == 'i' and dtype.itemsize >= 4:
        return np.iinfo(dtype).min
    return dtype.type(0)


def _shift_host(arr, shift):
    """``ndimage.shift(arr, -shift, order=0)`` along the first two axes"""
    rows, rows_in = _nearest_index(np.arange(arr.shape[0]) + shift[0], arr.shape[0])
    cols, cols_in = _nearest_index(np.arange(arr.shape[1]) + shift[1], arr.shape[1])
    out = arr[rows[:, None], cols[None, :]]
    out[~(rows_in[:, None] & cols_in[None, :])] = 0
    return out


def _rotate_host(arr, geometry):
    """``ndimage.rotate(arr, angle, order=0, mode='constant', cval=nan)`` in the plane of the first two axes"""
    matrix, offset = geometry['matrix'], geometry['offset']
    i = np.arange(geometry['canvas'][0], dtype=np.float64)[:, None]
    j = np.arange(geometry['canvas'][1], dtype=np.float64)[None, :]
    rows, rows_in = _nearest_index(((0. + i * matrix[0, 0]) + j * matrix[0, 1]) + offset[0], arr.shape[0])
    cols, cols_in = _nearest_index(((0. + i * matrix[1, 0]) + j * matrix[1, 1]) + offset[1], arr.shape[1])
    out = arr[rows, cols]
    out[~(rows_in & cols_in)] = _nan_as(arr.dtype)
    return out


def _first_region(mask):
    """the pixels of ``regionprops(mask.astype(int))[0]``: those of the smallest positive value"""
    lab = np.asarray(mask).astype(int)
    positive = lab[lab > 0]
    if positive.size == 0:
        raise IndexError('list index out of range')
    return lab == positive.min()


def cut_object_host(img, mask, padding, use_mask=False, bg_color=None, allow_rotate=True):
    """the numpy statement of the reference's ``cut_object`` (``utilities/data_io.py:1060-1128`` with scikit-image 0.18.3 and
    scipy), for every dtype the reference takes: see the comment above"""
    img, mask = np.asarray(img), np.asarray(mask)
    if mask.shape[:2] != img.shape[:2]:
        raise ValueError
    if mask.ndim != 2:
        raise ValueError('the mask must be 2-D')
    moments = _region_moments(_first_region(mask))
    bg_pixels = np.hstack([mask[0, :], mask[:, 0], mask[-1, :], mask[:, -1]])
    bg_mask = np.argmax(np.bincount(bg_pixels))
    if not (isinstance(bg_color, np.ndarray) and bg_color.size > 1) and not bg_color:
        bg_color = get_image2d_boundary_color(img)
    if allow_rotate:
        geometry = _cut_geometry(moments, mask.shape)
        mask = _rotate_host(_shift_host(mask, geometry['shift']), geometry)
        img = _rotate_host(_shift_host(img, geometry['shift']), geometry)
    img_cut = img.copy()
    if mask.dtype.kind == 'f':
        img_cut[np.isnan(mask), ...] = bg_color
        mask = mask.copy()
        mask[np.isnan(mask)] = bg_mask
    box = _region_moments(_first_region(mask))[6:10]
    min_row, min_col, max_row, max_col = add_padding(img_cut.shape, padding, box[0], box[2], box[1] + 1, box[3] + 1)
    img_cut = img_cut[min_row:max_row, min_col:max_col, ...]
    if use_mask:
        use_mask = mask[min_row:max_row, min_col:max_col, ...].astype(bool)
        img_cut[~use_mask, ...] = bg_color
    return img_cut


def _place(on):
    """'host' or 'device': ``_hip.resolve_place`` on IMSEGM_CUT_OBJECTS_ON"""
    from .. import _hip
    return _hip.resolve_place(on, 'IMSEGM_CUT_OBJECTS_ON', False)[0]


def _device_image(img):
    """``img`` as the C-contiguous uint8 [H, W, C] array the device reads, or None: not a non-empty uint8 image of 1 to 4 channels"""
    if not isinstance(img, np.ndarray) or img.dtype != np.uint8 or img.ndim not in (2, 3) or img.size == 0:
        return None
    if img.ndim == 3 and not 1 <= img.shape[2] <= 4:
        return None
    return np.ascontiguousarray(img).reshape(img.shape[0], img.shape[1], -1)


def _device_map(segm):
    """the label map as C-contiguous int32, or None: not a 2-D map of booleans or of integers inside int32"""
    if not isinstance(segm, np.ndarray) or segm.ndim != 2 or segm.size == 0 or segm.dtype.kind not in 'biu':
        return None
    if segm.dtype.kind != 'b' and segm.dtype.itemsize >= 4 and segm.dtype != np.int32:
        info = np.iinfo(np.int32)
        if segm.min() < info.min or segm.max() > info.max:
            return None
    return np.ascontiguousarray(segm, dtype=np.int32)


def _cut_objects_device(img, image, segm, labels, padding, use_mask, bg_color, allow_rotate):
    """the crops of ``labels`` (any order, repeats allowed) by ``imsegm_cut_objects``, ``CUT_OBJECTS_MAX_LABELS`` distinct labels per
    call; None: outside the caps of the entry"""
    from .. import _hip
    distinct = sorted(set(labels))
    crops = {}
    for start in range(0, len(distinct), CUT_OBJECTS_MAX_LABELS):
        chunk = distinct[start:start + CUT_OBJECTS_MAX_LABELS]
        result = _hip.cut_objects(image, segm, chunk, padding, use_mask, bg_color, allow_rotate, _hook_geometry)
        if result is None:
            return None
        crops.update(zip(chunk, result[0]))
    if img.ndim == 2:
        crops = {label: crop[:, :, 0] for label, crop in crops.items()}
    return [crops[label] if labels.count(label) == 1 else crops[label].copy() for label in labels]


def _hook_geometry(moments, shape, allow_rotate):
    if moments[0] == 0:
        raise IndexError('list index out of range')          # regionprops(...)[0] of the reference: the label has no pixel
    return _cut_geometry(moments, shape, allow_rotate)


def cut_objects(img, segm, labels=None, padding=0, use_mask=False, bg_color=None, allow_rotate=True, on=None):
    """ cut all objects of a label map out of one image: the list
    ``[cut_object(img, segm == l, padding, use_mask, bg_color, allow_rotate) for l in labels]``, the loop of
    experiments_ovary_detect/run_cut_segmented_objects.py:93-101, with ``bg_color`` taken once from the image.

    ``on='device'`` (the default when a device is present; ``IMSEGM_CUT_OBJECTS_ON``): one ``imsegm_cut_objects`` call for all labels
    -- the image and the map go up once, the packed crops come down once.  ``on='host'``: :func:`cut_object_host` per label.  The
    device takes uint8 images (H x W, or H x W x C with C <= 4) and maps of booleans or integers inside int32 with labels inside
    int32; everything else is evaluated by the host statement ("Cut objects").

    :param ndarray img: input image
    :param ndarray segm: label map of the height and width of the image
    :param list(int) labels: the objects; None: the positive values of the map in ascending order
    :param int padding: set padding around segmented object
    :param bool use_mask: fill BG values also outside the mask
    :param bg_color: set as default values outside bounding box; falsy: the dominant colour of the image border
    :param bool allow_rotate: allowing rotate object to get minimal bbox
    :param str on: ``'device'``, ``'host'`` or None
    :return list(ndarray):
    """
    img, segm = np.asarray(img), np.asarray(segm)
    if segm.shape[:2] != img.shape[:2]:
        raise ValueError
    if labels is None:
        values = np.unique(segm)
        labels = values[values > 0]
    labels = [int(label) for label in labels]
    if not labels:
        return []
    if not (isinstance(bg_color, np.ndarray) and bg_color.size > 1) and not bg_color:
        bg_color = get_image2d_boundary_color(img)
    if _place(on) == 'device':
        image, segm32 = _device_image(img), _device_map(segm)
        info = np.iinfo(np.int32)
        if image is not None and segm32 is not None and info.min <= min(labels) and max(labels) <= info.max:
            crops = _cut_objects_device(img, image, segm32, labels, padding, use_mask, bg_color, allow_rotate)
            if crops is not None:
                return crops
    return [cut_object_host(img, segm == label, padding, use_mask, bg_color, allow_rotate) for label in labels]


def cut_object(img, mask, padding, use_mask=False, bg_color=None, allow_rotate=True, on=None):
    """ cut an object from image according binary object segmentation (reference ``utilities/data_io.py:1060-1128``; its examples
    are in tests/doctests/utilities_cut_objects.py): the object is centred, turned so that its main axis is level, and the bounding
    box of the turned mask, widened by ``padding``, is cut out

    A uint8 image with a boolean mask runs on the device when one is present (:func:`cut_objects` with the one label); every other
    combination -- integer and float masks among them, see the comment above -- is :func:`cut_object_host`.

    :param ndarray img: inout image
    :param ndarray mask: segmentation
    :param int padding: set padding around segmented object
    :param bool use_mask: fill BG values also outside the mask
    :param bg_color: set as default values outside bounding box
    :param bool allow_rotate: allowing rotate object to get minimal bbox
    :param str on: ``'device'``, ``'host'`` or None (``IMSEGM_CUT_OBJECTS_ON``)
    :return ndarray:
    """
    img, mask = np.asarray(img), np.asarray(mask)
    if mask.shape[:2] != img.shape[:2]:
        raise ValueError
    if mask.dtype == np.bool_ and mask.ndim == 2 and _device_image(img) is not None and _place(on) == 'device':
        return cut_objects(img, mask, [1], padding, use_mask, bg_color, allow_rotate, on='device')[0]
    return cut_object_host(img, mask, padding, use_mask, bg_color, allow_rotate)
