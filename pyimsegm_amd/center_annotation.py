"""Centre-level annotations from maps of annotated eggs: the step in front of the centre detector's training, the reference's
``experiments_ovary_centres/run_create_annotation.py`` without its file I/O and its pandas table.

* :func:`correct_segm` -- ``load_correct_segm`` after the read: threshold, opening with ``disk(sel_radius)``, small 4-connected
  components removed, 8-connected labelling in raster order;
* :func:`compute_eggs_center` -- the centres of mass of the labels as (X, Y) rows;
* :func:`segm_center_levels` -- ``segm_set_center_levels`` without the save: per object the relative distance to its boundary cut at
  ``levels``, every level above the first inside a disc of the level's own area and opened;
* :func:`create_annot_centers` -- the three in one call.

Every function has a numpy / scipy statement ``..._host`` in this module, which is the definition (it needs neither scikit-image nor
the reference), and runs on the device by default when one is present: ``on='host'`` or the environment variable
``IMSEGM_CENTER_ANNOT_ON=host`` asks for the statement.  What the device entries do not take runs the statement silently: more than
1024 labels, more than 8 levels, levels that do not ascend, an opening radius above ``IMSEGM_MORPH_MAX_RADIUS``, maps beyond the
size limits of the morphology and distance kernels ("Centre annotations")."""
import numpy as np

from . import _hip
from .ellipse_fitting import ellipse_pixels_host, opening_host

#: relative distances from the object boundary of the three annotation levels (the reference's constant)
DISTANCE_LEVELS = [0., 0.4, 0.8]

__all__ = ['DISTANCE_LEVELS', 'correct_segm', 'correct_segm_host', 'compute_eggs_center', 'compute_eggs_center_host',
           'segm_center_levels', 'segm_center_levels_host', 'create_annot_centers', 'create_annot_centers_host']


def _place(on):
    """'host' or 'device': ``_hip.resolve_place`` on IMSEGM_CENTER_ANNOT_ON ('device' without a device raises)"""
    return _hip.resolve_place(on, 'IMSEGM_CENTER_ANNOT_ON', True)[0]


def _image_2d(img):
    img = np.asarray(img)
    if img.ndim != 2 or img.dtype.kind not in 'biuf':
        raise ValueError('the egg map has to be a 2-D numeric array, not %s %r' % (img.dtype, img.shape))
    return img


def _label_map(seg_labels):
    seg_labels = np.asarray(seg_labels)
    if seg_labels.ndim != 2 or seg_labels.dtype.kind not in 'iu':
        raise ValueError('the label map has to be a 2-D integer array, not %s %r' % (seg_labels.dtype, seg_labels.shape))
    return seg_labels


def _levels(levels):
    levels = np.asarray(levels, dtype=np.float64).ravel()
    if np.isnan(levels).any():
        raise ValueError('a level is not a number')
    return levels


def _size_ok(shape):
    """what ``morph_size_ok`` and ``edt_size_ok`` of the library take"""
    height, width = shape
    return 1 <= height <= 65535 and width >= 1 and height * width < 2 ** 31 and height * height + width * width <= 0xffffffff


# ------------------------------------------------------------------------------------------------
# the host statements
# ------------------------------------------------------------------------------------------------


def correct_segm_host(img, sel_radius=25, min_size=64):
    """the numpy / scipy statement of :func:`correct_segm`: ``img > 0`` opened with ``disk(sel_radius)`` (:func:`opening_host`),
    scikit-image's ``remove_small_objects`` (the 4-connected components with fewer than ``min_size`` pixels go) and its
    ``measure.label`` of a boolean map (8-connected, numbered from 1 in raster order of every component's first pixel)"""
    from scipy import ndimage
    seg = _image_2d(img) > 0
    if sel_radius > 0:
        seg = opening_host(seg, sel_radius)
    parts, _ = ndimage.label(seg)
    sizes = np.bincount(parts.ravel())
    seg = seg & ~(sizes < min_size)[parts]
    seg_lb, _ = ndimage.label(seg, structure=np.ones((3, 3), dtype=bool), output=np.int32)
    return seg, seg_lb


def _moments(seg_label):
    """pixel count, row sum and column sum of the labels 0 .. max as exact integers"""
    flat = seg_label.ravel()
    keep = flat > 0
    flat = flat[keep].astype(np.int64)
    size = int(flat.max()) + 1 if flat.size else 1
    rows, cols = np.divmod(np.flatnonzero(keep), seg_label.shape[1])
    # (weights are float64 in bincount: exact below 2^53, far above H * W * max(H, W) of any map the library takes)
    return (np.bincount(flat, minlength=size), np.bincount(flat, weights=rows, minlength=size).astype(np.int64),
            np.bincount(flat, weights=cols, minlength=size).astype(np.int64))


def compute_eggs_center_host(seg_label):
    """the numpy statement of :func:`compute_eggs_center`: ``ndimage.center_of_mass(seg_label == lb)`` of every present label --
    the quotient of two exact integer sums in float64 -- as a row (X, Y) = (column mean, row mean)"""
    seg_label = _label_map(seg_label)
    count, sum_r, sum_c = _moments(seg_label)
    present = np.flatnonzero(count[1:] > 0) + 1
    centres = np.empty((len(present), 2), dtype=np.float64)
    centres[:, 0] = sum_c[present].astype(np.float64) / count[present].astype(np.float64)
    centres[:, 1] = sum_r[present].astype(np.float64) / count[present].astype(np.float64)
    return centres


def level_geometry(count):
    """what a level above the first draws with: the disc radius ``int(sqrt(count / pi))`` of a mask of ``count`` pixels and the
    radius ``int(radius * 0.15)`` of the opening"""
    radius = int(np.sqrt(count / np.pi))
    return radius, int(radius * 0.15)


def object_levels_host(im_bin, levels):
    """the level masks of ONE object: a list of (mask after the opening, count of ``probab > level``, disc radius, opening radius),
    radii None for the first level"""
    from scipy import ndimage
    distance = ndimage.distance_transform_edt(im_bin)
    probab = distance / np.max(distance)
    rows, cols = np.nonzero(im_bin)
    center = (float(rows.sum()) / float(len(rows)), float(cols.sum()) / float(len(rows)))
    out = []
    for i, level in enumerate(levels):
        mask = probab > level
        count, radius, opening = int(mask.sum()), None, None
        if i > 0:
            radius, opening = level_geometry(count)
            disc = np.zeros(im_bin.shape, dtype=bool)
            disc[ellipse_pixels_host(center[0], center[1], radius, radius, 0., im_bin.shape)] = True
            mask = opening_host(np.logical_and(mask, disc), opening)
        out.append((mask, count, radius, opening))
    return out


def segm_center_levels_host(seg_labels, levels=DISTANCE_LEVELS):
    """the numpy / scipy statement of :func:`segm_center_levels`, object by object as the reference: the exact Euclidean distance
    inside ``seg_labels == label`` (the image border is no background) over its maximum, level 0 where it is ``> levels[0]``, every
    later level ``i`` where it is ``> levels[i]`` inside scikit-image 0.18.3's disc (:func:`ellipse_pixels_host` with equal radii)
    around the centre of mass with ``radius = int(sqrt(count / pi))``, opened with ``disk(int(radius * 0.15))``; written as
    ``i + 1``, later levels over earlier ones"""
    seg_labels, levels = _label_map(seg_labels), _levels(levels)
    seg = np.zeros_like(seg_labels)
    top = int(seg_labels.max()) if seg_labels.size else 0
    present = np.flatnonzero(np.bincount(seg_labels[seg_labels > 0].ravel().astype(np.int64), minlength=2)[1:]) + 1 if top > 0 else []
    for obj_id in present:
        for i, (mask, _, _, _) in enumerate(object_levels_host(seg_labels == obj_id, levels)):
            seg[mask] = i + 1
    return seg


def create_annot_centers_host(img, levels=DISTANCE_LEVELS, sel_radius=25, min_size=64):
    """the statement of :func:`create_annot_centers` from the three statements above"""
    _, seg_lb = correct_segm_host(img, sel_radius, min_size)
    return segm_center_levels_host(seg_lb, levels).astype(np.uint8), compute_eggs_center_host(seg_lb)


# ------------------------------------------------------------------------------------------------
# the public functions
# ------------------------------------------------------------------------------------------------


def _device_image(img):
    """the egg map as ``imsegm_correct_segm`` reads it: uint8 or int32 as they are, anything else as its ``> 0`` bytes"""
    if img.dtype in (np.uint8, np.int32):
        return np.ascontiguousarray(img)
    return np.ascontiguousarray(img > 0).view(np.uint8)


def _correct_on_device(img, sel_radius, min_size):
    return img.size > 0 and 0 <= sel_radius <= _hip.MORPH_MAX_RADIUS and _size_ok(img.shape)


def _levels_on_device(seg_labels, levels):
    """the caps of ``imsegm_center_levels`` that show before the call; (take it, max label)"""
    if not (seg_labels.size and _size_ok(seg_labels.shape) and len(levels) <= _hip.CENTER_ANNOT_MAX_LEVELS and np.all(np.diff(levels) >= 0)):
        return False, 0
    top = int(seg_labels.max())
    return top <= _hip.CENTER_ANNOT_MAX_LABELS, top


def correct_segm(img, sel_radius=25, min_size=64, on=None):
    """ correct a map of annotated eggs with simple morphology and label it (the reference's ``load_correct_segm`` after the read):
    ``img > 0``, binary opening with ``disk(sel_radius)``, 4-connected components with fewer than ``min_size`` pixels removed,
    8-connected components numbered from 1 in raster order of their first pixels.  ``sel_radius`` and ``min_size`` are the
    reference's constants 25 and 64.

    On the device (``imsegm_correct_segm``) for radii up to ``IMSEGM_MORPH_MAX_RADIUS``; ``on='host'`` (or
    ``IMSEGM_CENTER_ANNOT_ON=host``, no device, a larger radius) runs :func:`correct_segm_host`.

    :param ndarray img: map of eggs H x W, numeric
    :param int sel_radius: radius of the disc of the opening
    :param int min_size: the smallest 4-connected component that stays
    :return tuple(ndarray,ndarray): seg (bool), seg_lb (int32, as scikit-image's ``label`` returns it)
    """
    img = _image_2d(img)
    sel_radius = int(sel_radius)
    if sel_radius < 0:
        raise ValueError('the radius of the opening must not be negative')
    if _place(on) == 'device' and _correct_on_device(img, sel_radius, min_size):
        seg, seg_lb, _ = _hip.correct_segm(_device_image(img), sel_radius, min_size)
        return seg.view(np.bool_), seg_lb
    return correct_segm_host(img, sel_radius, min_size)


def compute_eggs_center(seg_label, on=None):
    """ the centres of mass of all objects of a label map, one row (X, Y) per label of ``1 .. max`` that is present, in label order
    (the reference's ``compute_eggs_center`` as an array: ``ndimage.center_of_mass``, column mean first).

    :param ndarray seg_label: label map H x W, integer
    :return ndarray: float64 (n, 2)
    """
    seg_label = _label_map(seg_label)
    if _place(on) == 'device':
        take, top = _levels_on_device(seg_label, [])
        if take and top >= 1:
            got = _hip.center_levels(seg_label, top, [])
            if got is not None:
                _, count, centres = got
                return centres[count > 0]
    return compute_eggs_center_host(seg_label)


def segm_center_levels(seg_labels, levels=DISTANCE_LEVELS, on=None):
    """ the centre-zone map of a label map (the reference's ``segm_set_center_levels`` without the save): see
    :func:`segm_center_levels_host` for the definition.  All objects of the map in one chain of launches on the device
    (``imsegm_center_levels``); what its caps exclude runs the host statement.

    :param ndarray seg_labels: label map H x W, integer
    :param list(float) levels: relative distances from the object boundary, ascending on the device
    :return ndarray: map of the dtype and shape of ``seg_labels`` with values 0 .. len(levels)
    """
    seg_labels, levels = _label_map(seg_labels), _levels(levels)
    if _place(on) == 'device':
        take, top = _levels_on_device(seg_labels, levels)
        if take and top < 1:
            return np.zeros_like(seg_labels)
        if take and len(levels):
            got = _hip.center_levels(seg_labels, top, levels)
            if got is not None:
                return got[0].astype(seg_labels.dtype)
    return segm_center_levels_host(seg_labels, levels)


def create_annot_centers(img, levels=DISTANCE_LEVELS, on=None, sel_radius=25, min_size=64):
    """ the centre-zone map and the centres of a map of annotated eggs (the reference's ``create_annot_centers`` without the
    files): :func:`correct_segm`, :func:`segm_center_levels` and :func:`compute_eggs_center` with one upload and one download
    (``imsegm_create_annot_centers``).

    :param ndarray img: map of eggs H x W, numeric
    :param list(float) levels: relative distances from the object boundary
    :return tuple(ndarray,ndarray): level map (uint8), centres float64 (n, 2) as (X, Y)
    """
    img, levels = _image_2d(img), _levels(levels)
    sel_radius = int(sel_radius)
    if sel_radius < 0:
        raise ValueError('the radius of the opening must not be negative')
    if (_place(on) == 'device' and _correct_on_device(img, sel_radius, min_size) and 1 <= len(levels) <= _hip.CENTER_ANNOT_MAX_LEVELS
            and np.all(np.diff(levels) >= 0)):
        got = _hip.create_annot_centers(_device_image(img), sel_radius, min_size, levels)
        if got is not None:
            level_map, count, centres = got
            return level_map, centres[count > 0]
    return create_annot_centers_host(img, levels, sel_radius, min_size)
