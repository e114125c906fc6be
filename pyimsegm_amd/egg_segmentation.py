"""Egg segmentation by marker watershed: the tenth method of the reference's
``experiments_ovary_detect/run_ovary_egg-segmentation.py`` (``segment_watershed``, 'watershed_morph') without scikit-image.

* :func:`watershed_markers` -- the flood alone: integer markers spread inside a boolean mask over integer keys, 4-connected;
* :func:`watershed_post_morph` -- the clean-up alone: per label a closing with ``disk(5)``, hole filling and an opening with
  ``disk(15)``, painted in ascending label order;
* :func:`segment_watershed` -- the reference's function: ``seg > 0`` with its holes filled, one marker per centre, the flood over
  minus the squared distance to the background, optionally the clean-up.

Every function has a numpy / scipy statement ``..._host`` in this module, which is the definition (it needs neither scikit-image nor
the reference), and runs on the device by default when one is present: ``on='host'`` or the environment variable
``IMSEGM_WATERSHED_ON=host`` asks for the statement.  What the device entries do not take runs the statement silently: labels
outside 1 .. 1024, radii above ``IMSEGM_MORPH_MAX_RADIUS``, maps beyond the size limits of the distance kernels or with
height^2 + width^2 >= 2^31 ("Watershed").

The flood is defined by rounds, not by scikit-image's queue (whose order is the global push count): see
:func:`watershed_markers_host`."""
import heapq

import numpy as np

from . import _hip
from .ellipse_fitting import fill_holes_host, opening_host

__all__ = ['segment_watershed', 'segment_watershed_host', 'watershed_markers', 'watershed_markers_host', 'watershed_post_morph',
           'watershed_post_morph_host', 'closing_host', 'squared_distances_host']


def _place(on):
    """'host' or 'device': ``_hip.resolve_place`` on IMSEGM_WATERSHED_ON ('device' without a device raises)"""
    return _hip.resolve_place(on, 'IMSEGM_WATERSHED_ON', True)[0]


def _map_2d(seg, what, kinds):
    seg = np.asarray(seg)
    if seg.ndim != 2 or seg.dtype.kind not in kinds:
        raise ValueError('%s has to be a 2-D array of kind %r, not %s %r' % (what, kinds, seg.dtype, seg.shape))
    return seg


def _size_ok(shape):
    """what ``imsegm_watershed*`` take: the caps of the morphology and distance kernels, and keys -d^2 that fit an int32"""
    height, width = shape
    return 1 <= height <= 65535 and width >= 1 and height * width < 2 ** 31 and height * height + width * width < 2 ** 31


def _radius(radius):
    radius = int(radius)
    if radius < 0:
        raise ValueError('a radius must not be negative')
    return radius


# ------------------------------------------------------------------------------------------------
# the host statements
# ------------------------------------------------------------------------------------------------


def squared_distances_host(mask):
    """the exact squared Euclidean distance of every pixel of ``mask`` to its nearest zero pixel as int64: the square of what
    ``scipy.ndimage.distance_transform_edt`` answers (the correctly rounded root of an integer, whose square rounds back to it)"""
    from scipy import ndimage
    distance = ndimage.distance_transform_edt(np.asarray(mask, dtype=bool))
    return np.rint(distance * distance).astype(np.int64)


def closing_host(mask, radius):
    """``skimage.morphology.binary_closing(mask, disk(radius))`` of scikit-image 0.18.3 for an integer radius as two thresholds of
    exact distances: the dilation sets a pixel whose squared distance to the nearest set pixel is <= radius^2 (pixels outside the
    image are clear), the erosion keeps a pixel whose squared distance to the nearest clear pixel is > radius^2 (pixels outside the
    image are set: ``border_value=True``)"""
    from scipy import ndimage
    mask = np.asarray(mask, dtype=bool)
    radius = int(radius)
    if not mask.any():
        return mask
    mask = ndimage.distance_transform_edt(~mask) <= radius
    if mask.all():
        return mask
    return ndimage.distance_transform_edt(mask) > radius


def watershed_markers_host(mask, markers, keys=None):
    """the definition of the flood.  ``markers`` (integers, 0: none) inside ``mask`` are the first labelled pixels; ``keys`` are
    integers, by default minus the squared distance to the background of ``mask`` (:func:`squared_distances_host`).  The frontier
    is the set of labelled pixels that have not spread yet.  Until it is empty:

    1. take the smallest key on the frontier;
    2. all frontier pixels with that key spread at once and leave the frontier;
    3. every unlabelled mask pixel that is a 4-neighbour of a spreading pixel takes the smallest label among its spreading
       neighbours and joins the frontier with its own key.

    Nothing here depends on an order of execution.  scikit-image's ``watershed`` orders its queue by (key, global push count); the
    two agree wherever two labels never reach a pixel in the same round.

    :return ndarray: int32 map of the shape of ``mask``, 0 outside the mask and where no marker arrives"""
    mask = _map_2d(mask, 'the mask', 'biu') != 0
    markers = _map_2d(markers, 'the markers', 'biu')
    if markers.shape != mask.shape:
        raise ValueError('mask %r and markers %r differ in shape' % (mask.shape, markers.shape))
    height, width = mask.shape
    if keys is None:
        keys = -squared_distances_host(mask)
    keys = _map_2d(keys, 'the keys', 'iu').astype(np.int64).ravel()
    if keys.size != mask.size:
        raise ValueError('mask and keys differ in shape')
    out = np.where(mask, markers, 0).astype(np.int64).ravel()
    free = mask.ravel() & (out == 0)
    buckets, heap = {}, []

    def push(pixels):
        order = np.argsort(keys[pixels], kind='stable')
        pixels = pixels[order]
        values, first = np.unique(keys[pixels], return_index=True)
        for value, part in zip(values.tolist(), np.split(pixels, first[1:])):
            if value not in buckets:
                buckets[value] = []
                heapq.heappush(heap, value)
            buckets[value].append(part)

    push(np.flatnonzero(out))
    steps = ((-width, lambda p: p >= width), (width, lambda p: p < (height - 1) * width), (-1, lambda p: p % width > 0),
             (1, lambda p: p % width < width - 1))
    while heap:
        spreading = np.concatenate(buckets.pop(heapq.heappop(heap)))
        targets, labels = [], []
        for step, inside in steps:
            source = spreading[inside(spreading)]
            source = source[free[source + step]]
            targets.append(source + step)
            labels.append(out[source])
        targets, labels = np.concatenate(targets), np.concatenate(labels)
        if not targets.size:
            continue
        order = np.lexsort((labels, targets))
        targets, labels = targets[order], labels[order]
        first = np.ones(len(targets), dtype=bool)
        first[1:] = targets[1:] != targets[:-1]
        targets, labels = targets[first], labels[first]
        out[targets] = labels
        free[targets] = False
        push(targets)
    return out.reshape(mask.shape).astype(np.int32)


def watershed_post_morph_host(segm, radius_close=5, radius_open=15):
    """the clean-up loop of the reference (``run_ovary_egg-segmentation.py:265-274``) in scipy: for every label 1 .. max in
    ascending order ``segm == label`` closed with ``disk(radius_close)`` (:func:`closing_host`), its holes filled, opened with
    ``disk(radius_open)`` (``opening_host``; radius 0: the mask as it is) and painted over what earlier labels painted"""
    segm = _map_2d(segm, 'the label map', 'iu')
    radius_close, radius_open = _radius(radius_close), _radius(radius_open)
    clean = np.zeros(segm.shape, dtype=np.int32)
    top = int(segm.max()) if segm.size else 0
    present = np.flatnonzero(np.bincount(segm[segm > 0].ravel().astype(np.int64), minlength=2)[1:]) + 1 if top > 0 else []
    for label in present:
        part = fill_holes_host(closing_host(segm == label, radius_close))
        if radius_open > 0:
            part = opening_host(part, radius_open)
        clean[part] = label
    return clean


def _centre_pixels(centers, shape):
    """the (row, column) of every centre as the reference's marker loop indexes them: ``int()`` of both coordinates, numpy's
    negative indices resolved"""
    height, width = shape
    pixels = np.zeros((len(centers), 2), dtype=np.int32)
    for i, pos in enumerate(centers):
        row, col = int(pos[0]), int(pos[1])
        if not (-height <= row < height and -width <= col < width):
            raise IndexError('centre %d (%d, %d) lies outside the map %r' % (i, row, col, (height, width)))
        pixels[i] = row % height, col % width
    return pixels


def segment_watershed_host(seg, centers, post_morph=False):
    """the numpy / scipy statement of :func:`segment_watershed` from the statements above"""
    seg = _map_2d(seg, 'the segmentation', 'biuf')
    mask = fill_holes_host(seg > 0)
    markers = np.zeros(seg.shape, dtype=np.int32)
    for i, (row, col) in enumerate(_centre_pixels(centers, seg.shape)):
        markers[row, col] = i + 1                       # (a later centre replaces an earlier one)
    segm = watershed_markers_host(mask, markers) if seg.size else markers
    if post_morph:
        segm = watershed_post_morph_host(segm)
    return segm, centers, None


# ------------------------------------------------------------------------------------------------
# the public functions
# ------------------------------------------------------------------------------------------------


def watershed_markers(mask, markers, keys=None, on=None):
    """ the flood of integer ``markers`` inside the boolean ``mask`` over integer ``keys``, 4-connected, as
    :func:`watershed_markers_host` defines it (scikit-image's ``watershed(keys, markers, mask=mask)`` away from the ridge lines).
    With ``keys=None`` the keys are minus the exact squared distances to the background of ``mask``, computed where the flood runs.

    On the device (``imsegm_watershed_markers``): one workgroup per component of the mask.  Markers outside 0 .. 1024, keys outside
    int32 and maps beyond the size caps run the host statement.

    :param ndarray mask: H x W, boolean or integer (non-zero: inside)
    :param ndarray markers: H x W, integer, 0 for no marker
    :param ndarray keys: H x W, integer, or None
    :return ndarray: int32 H x W
    """
    mask = _map_2d(mask, 'the mask', 'biu') != 0
    markers = _map_2d(markers, 'the markers', 'biu')
    if markers.shape != mask.shape:
        raise ValueError('mask %r and markers %r differ in shape' % (mask.shape, markers.shape))
    if keys is not None:
        keys = _map_2d(keys, 'the keys', 'iu')
        if keys.shape != mask.shape:
            raise ValueError('mask and keys differ in shape')
    if _place(on) == 'device' and mask.size and _size_ok(mask.shape):
        seeds = np.flatnonzero(mask & (markers != 0))
        labels = markers.ravel()[seeds]
        fits = not len(seeds) or (int(labels.min()) >= 1 and int(labels.max()) <= _hip.WATERSHED_MAX_LABELS)
        if fits and (keys is None or (int(keys.min()) >= -2 ** 31 + 1 and int(keys.max()) <= 2 ** 31 - 2)):
            got = _hip.watershed_markers(mask, seeds, labels, keys)
            if got is not None:
                return got
    return watershed_markers_host(mask, markers, keys)


def watershed_post_morph(segm, radius_close=5, radius_open=15, on=None):
    """ the clean-up of a label map after the flood (the reference's loop ``run_ovary_egg-segmentation.py:265-274``): see
    :func:`watershed_post_morph_host` for the definition.  On the device (``imsegm_watershed_post_morph``) every stage is one launch
    over all labels, each inside the plane of its padded bounding box.  Labels above 1024, radii above ``IMSEGM_MORPH_MAX_RADIUS`` and maps beyond the size caps run
    the host statement.

    :param ndarray segm: label map H x W, integer
    :return ndarray: int32 H x W
    """
    segm = _map_2d(segm, 'the label map', 'iu')
    radius_close, radius_open = _radius(radius_close), _radius(radius_open)
    if (_place(on) == 'device' and segm.size and _size_ok(segm.shape) and max(radius_close, radius_open) <= _hip.MORPH_MAX_RADIUS
            and int(segm.max()) <= _hip.WATERSHED_MAX_LABELS):
        got = _hip.watershed_post_morph(segm, radius_close, radius_open)
        if got is not None:
            return got
    return watershed_post_morph_host(segm, radius_close, radius_open)


def segment_watershed(seg, centers, post_morph=False, on=None):
    """ perform watershed segmentation on input imsegm and optionally run some postprocessing using morphological operations (the
    reference's ``segment_watershed``): the mask ``seg > 0`` with its holes filled, marker ``i + 1`` on the pixel
    ``(int(row), int(col))`` of centre ``i`` -- a later centre on the same pixel replaces an earlier one, a centre outside the
    mask yields no label --, :func:`watershed_markers` over minus the squared distance to the background and, with ``post_morph``,
    :func:`watershed_post_morph` with the reference's radii 5 and 15.  One upload, one chain of launches and one download on the
    device (``imsegm_watershed``); more than 1024 centres and maps beyond the size caps run :func:`segment_watershed_host`.

    :param ndarray seg: input image / segmentation H x W, boolean or numeric
    :param list(tuple(int,int)) centers: position of centres / seeds as (row, column)
    :param bool post_morph: apply morphological postprocessing
    :return tuple(ndarray,list,None): resulting segmentation (int32), the centres as given, None
    """
    seg = _map_2d(seg, 'the segmentation', 'biuf')
    if _place(on) == 'device' and seg.size and _size_ok(seg.shape) and len(centers) <= _hip.WATERSHED_MAX_LABELS:
        got = _hip.watershed(seg > 0, _centre_pixels(centers, seg.shape), bool(post_morph))
        if got is not None:
            return got, centers, None
    return segment_watershed_host(seg, centers, post_morph)
