"""Handling annotations: hand-painted RGB annotation images <-> integer label maps, the colours an image holds and the quantisation of
a painted image to the colours of a legend -- every public name of the reference's ``imsegm/annotation.py`` with its signature,
defaults, result dtypes and errors, the per-pixel work on the device (csrc/annotation.hip).

* ``convert_img_colors_to_labels`` / ``_reverted`` -- one pass of ``imsegm_annot_match`` (exact mode) over the image against the colour
  table.
* ``convert_img_labels_to_colors`` -- ``imsegm_annot_paint``.
* ``unique_image_colors`` / ``image_frequent_colors`` / ``group_images_frequent_colors`` -- ``imsegm_annot_color_hist``: one bin per
  24-bit colour, compacted in key order.
* ``image_color_2_labels`` / ``quantize_image_nearest_color`` -- ``imsegm_annot_match`` (nearest modes): L1 distance, first colour wins.
* ``image_inpaint_pixels`` -- ``imsegm_annot_nearest_valid``, an exact nearest-feature transform; ``quantize_image_nearest_pixel`` --
  exact match, transform and colour gather in one call (``imsegm_annot_quantize_nearest_pixel``).

Every pixel function takes ``on=None | 'host' | 'device'`` (environment: ``IMSEGM_ANNOTATION_ON``; the rules of the switch are
``_hip.resolve_place``, and ``'device'`` without a device raises).  ``'host'`` runs the numpy / scipy statement of the same definition, and so does -- whatever ``on`` says -- every call the device does not take: an image that is not
``[H, W, 3]`` or whose values are not integers in 0 .. 255, colours with a component outside 0 .. 255 or more than
``IMSEGM_ANNOT_MAX_COLORS`` = 256 of them, labels that are not non-negative int32 integers, a map beyond the uint32 limit of the
squared distances (``H^2 + W^2 > 2^32 - 1``) or with more than 65535 rows.  With ``on=None`` the functions named in
``HOST_BY_DEFAULT`` run on the host although a device is present: there the transfers cost more than the host statement
(tools/time_annotation.py).

Differences from the reference, all documented in DESIGN.md:

* ``unique_image_colors`` returns the colours in ascending order of ``r << 16 | g << 8 | b`` (the reference: PIL's internal order), and
  ``image_frequent_colors`` builds its dict in that order; ``image_color_2_labels`` without ``colors`` therefore numbers the frequent
  colours in that order (the reference: in PIL's).
* ``quantize_image_nearest_pixel`` / ``image_inpaint_pixels`` among several valid pixels at the same distance: on the device the one
  with the smallest row-major index (:func:`nearest_valid_host` states the rule in numpy); on the host scipy's choice.
* ``convert_img_labels_to_colors`` with a gap in the label range (labels 0 and 2, none 1) fills the unused table entry with zeros,
  where ``np.array`` of the reference's ragged list fails on numpy >= 1.24.

The examples of the reference's docstrings are not repeated here; their inputs and recorded results are a test
(tests/test_annotation_reference_host.py).
"""
import collections
import logging
import math
import os

import numpy as np

from pyimsegm_amd import _hip
from pyimsegm_amd.utilities import ImageDimensionError

#: columns of the position table that ``load_info_group_by_slices`` collects: anterior, posterior and lateral point of an egg
COLUMNS_POSITION = ('ant_x', 'ant_y', 'post_x', 'post_y', 'lat_x', 'lat_y')
#: column of the position table that names the stack an image is a slice of
SLICE_NAME_GROUPING = 'stack_path'
#: development stage of an egg -> how many slices away an annotation of that stage still shows the same egg
ANNOT_SLICE_DIST_TOL = dict(zip(range(1, 7), (1, 2, 2, 3, 3, 0)))
#: label -> colour of the legend the annotation drivers paint with
DICT_COLOURS = dict(enumerate([(0, 0, 255), (255, 0, 0), (0, 255, 0), (255, 229, 0), (142, 68, 173), (127, 140, 141), (0, 212, 255),
                               (128, 0, 0)]))

#: functions that run on the host with ``on=None`` although a device is present: their device median was not below their host
#: median at 1024 x 768 (profiles/annotation_time.json); ``on='device'`` still takes the device
HOST_BY_DEFAULT = frozenset()


def _place(on, name):
    """'host' or 'device' for the public function ``name``: ``_hip.resolve_place`` on IMSEGM_ANNOTATION_ON ('device' without a
    device raises) and -- when neither the keyword nor the variable says anything -- ``HOST_BY_DEFAULT``"""
    place, explicit = _hip.resolve_place(on, 'IMSEGM_ANNOTATION_ON', True)
    return place if explicit or name not in HOST_BY_DEFAULT else 'host'


# ------------------------------------------------------------------------------------------------
# what the device takes
# ------------------------------------------------------------------------------------------------

def _device_image(img):
    """``img`` as the C-contiguous uint8 [H, W, 3] array the device reads (``img`` itself when it is one), or None: not a non-empty
    3-channel array of integers in 0 .. 255, or 2^32 pixels and more"""
    if not isinstance(img, np.ndarray) or img.ndim != 3 or img.shape[2] != 3 or img.size == 0 or img.size // 3 >= 2 ** 32:
        return None
    if img.dtype != np.uint8:
        if img.dtype.kind not in 'biu' or img.min() < 0 or img.max() > 255:
            return None
    return np.ascontiguousarray(img, dtype=np.uint8)


def _device_colors(colors):
    """the colours as uint8 [K, 3], or None: not 1 .. 256 triples of integers in 0 .. 255, or one-byte integers (whose differences
    to a uint8 pixel wrap in the host statement)"""
    try:
        listed = [np.asarray(clr) for clr in colors]
    except (TypeError, ValueError):
        return None
    if not 1 <= len(listed) <= _hip.ANNOT_MAX_COLORS:
        return None
    for clr in listed:
        if clr.shape != (3, ) or clr.dtype.kind not in 'iu' or clr.dtype.itemsize < 2 or clr.min() < 0 or clr.max() > 255:
            return None
    return np.array(listed, dtype=np.uint8)


def _device_labels(labels):
    """the labels as int32, or None when one is not a non-negative integer below 2^31"""
    try:
        values = np.asarray(list(labels))
    except (TypeError, ValueError):
        return None
    if values.ndim != 1 or values.dtype.kind not in 'biu' or (len(values) and (values.min() < 0 or values.max() > np.iinfo(np.int32).max)):
        return None
    return values.astype(np.int32)


def _nearest_size_ok(shape):
    return len(shape) == 2 and 1 <= shape[0] <= 65535 and shape[1] >= 1 and shape[0] ** 2 + shape[1] ** 2 <= 2 ** 32 - 1


def _keys_to_colors(keys):
    """packed keys -> list of (r, g, b) tuples of Python ints"""
    keys = np.asarray(keys, dtype=np.int64)
    return list(map(tuple, np.stack([keys >> 16, (keys >> 8) & 255, keys & 255], axis=1).tolist()))


# ------------------------------------------------------------------------------------------------
# colours of an image
# ------------------------------------------------------------------------------------------------

def color_counts_host(img):
    """the numpy statement of ``imsegm_annot_color_hist``: (keys uint32 [n] ascending, counts [n]) of a uint8 image [H, W, 3]"""
    flat = img.reshape(-1, 3).astype(np.uint32)
    return np.unique((flat[:, 0] << 16) | (flat[:, 1] << 8) | flat[:, 2], return_counts=True)


def _rgb_bytes(img):
    """what PIL makes of ``Image.fromarray(img).convert('RGB')`` for a uint8 array: a gray image three times, the first three of
    four channels"""
    if img.ndim == 2:
        return np.repeat(img[:, :, None], 3, axis=2)
    if img.ndim == 3 and img.shape[2] in (3, 4):
        return img[:, :, :3]
    raise TypeError('cannot read an array of shape %r as an image' % (img.shape, ))


def _color_counts(img, on, name):
    """(keys, counts) of a uint8 [H, W, 3] array for the public function ``name``, on the device when it takes the image"""
    work = _device_image(img) if _place(on, name) == 'device' else None
    if work is None:
        return color_counts_host(np.ascontiguousarray(img))
    return _hip.annot_color_hist(work)


def unique_image_colors(img, on=None):
    """The distinct colours of an image as a list of (r, g, b) tuples of ints, in ascending order of ``r << 16 | g << 8 | b`` (the
    reference lists them in the order of PIL's colour table).  ``img`` [H, W, 3] is cast to uint8 first, whatever it holds, as the
    reference does; a gray image [H, W] counts as r = g = b and of four channels the first three count.  More than 256 colours are
    worth a warning in the log, nothing else."""
    image = _rgb_bytes(np.asarray(img, dtype=np.uint8))
    three_channels = np.ndim(img) == 3 and np.shape(img)[2] == 3
    keys, _ = _color_counts(image, on if three_channels else 'host', 'unique_image_colors')
    if len(keys) > 256:
        logging.warning('the image holds %i distinct colours, more than an annotation legend has', len(keys))
    return _keys_to_colors(keys)


def image_frequent_colors(img, ratio_threshold=1e-3, on=None):
    """The colours of a uint8 image that are painted on at least ``ratio_threshold`` of its pixels: a dict (r, g, b) -> number of
    pixels, in ascending order of ``r << 16 | g << 8 | b``.  A fourth channel is dropped.  A gray image [H, W] gives its gray values
    as keys, as PIL's colour list does.  Anything PIL does not read as bytes is a TypeError, as it is there."""
    channels = img[..., :3] if img.ndim == 3 else img
    if channels.dtype != np.uint8 or channels.ndim not in (2, 3) or channels.shape[2:] not in ((), (3, )):
        raise TypeError('an image of bytes [H, W] or [H, W, 3] is needed, not %r of %s' % (channels.shape, channels.dtype))
    fewest = math.prod(channels.shape[:2]) * ratio_threshold
    if channels.ndim == 2:
        values, counts = np.unique(channels, return_counts=True)
        return {int(v): int(nb) for v, nb in zip(values, counts) if nb >= fewest}
    keys, counts = _color_counts(channels, on, 'image_frequent_colors')
    kept = counts >= fewest
    found = dict(zip(_keys_to_colors(keys[kept]), counts[kept].tolist()))
    logging.debug('%i of %i colours reach %g pixels: %r', len(found), len(keys), fewest, found)
    return found


def group_images_frequent_colors(paths_img, ratio_threshold=1e-3, on=None):
    """:func:`image_frequent_colors` of every image file of ``paths_img``, summed per colour: a dict (r, g, b) -> number of pixels
    over all images in which the colour reaches ``ratio_threshold``."""
    from PIL import Image
    total = collections.Counter()
    for path in paths_img:
        with Image.open(path) as handle:
            total.update(image_frequent_colors(np.asarray(handle), ratio_threshold, on=on))
    logging.info('%i images hold the frequent colours %r', len(paths_img), dict(total))
    return dict(total)


# ------------------------------------------------------------------------------------------------
# colours <-> labels
# ------------------------------------------------------------------------------------------------

def colors_to_labels_host(img_rgb, colors, labels):
    """the numpy statement of ``imsegm_annot_match`` in exact mode on any array [..., C]: (float64 map with ``labels[k]`` of the last
    of ``colors`` the pixel equals and 0 for none, number of pixels that equal a colour -- counted once per colour)"""
    label_map = np.zeros(img_rgb.shape[:-1])
    n_matched = 0
    for color, label in zip(colors, labels):
        same = np.all(img_rgb == color, axis=-1)
        label_map[same] = label
        n_matched += int(np.count_nonzero(same))
    return label_map, n_matched


def convert_img_colors_to_labels(img_rgb, lut_label_color, on=None):
    """The label map [H, W] (int) of an annotation image [H, W, 3] painted with the colours of ``lut_label_color``, a dict
    label -> colour: :func:`convert_img_colors_to_labels_reverted` with the dict turned round, so of two labels with one colour the
    later one is found."""
    return _colors_to_labels(img_rgb, {color: label for label, color in lut_label_color.items()}, on, 'convert_img_colors_to_labels')


def convert_img_colors_to_labels_reverted(img_rgb, dict_color_label, on=None):
    """The label map [H, W] (int) of an annotation image [H, W, 3] painted with the colours of ``dict_color_label``, a dict
    colour -> label: every pixel gets the label of the colour it equals exactly.  A pixel that has none of the colours is a
    ValueError.  Float images and float colours are compared as they are (on the host)."""
    return _colors_to_labels(img_rgb, dict_color_label, on, 'convert_img_colors_to_labels_reverted')


def _colors_to_labels(img_rgb, dict_color_label, on, name):
    """the exact match behind the public function ``name``"""
    colors, labels = list(dict_color_label.keys()), list(dict_color_label.values())
    work = table = device_labels = None
    if _place(on, name) == 'device':
        work, table, device_labels = _device_image(img_rgb), _device_colors(colors), _device_labels(labels)
    if work is None or table is None or device_labels is None:
        label_map, n_matched = colors_to_labels_host(img_rgb, colors, labels)
        n_missing = label_map.size - n_matched
    else:
        label_map, n_missing = _hip.annot_match(work, table, device_labels, _hip.ANNOT_MATCH_EXACT)
    if n_missing != 0:
        raise ValueError('%i pixels (pixels of several equal colours counted per colour) have none of the colours' % n_missing)
    return label_map.astype(int, copy=False)


def labels_to_colors_host(segm, min_label, table):
    """the numpy statement of ``imsegm_annot_paint``: ``table[segm - min_label]``"""
    return table[np.asarray(segm - min_label, dtype=int)]


def convert_img_labels_to_colors(segm, lut_label_colors, on=None):
    """The image [H, W, C] of a label map [H, W] painted with ``lut_label_colors``, a dict label -> colour, in the dtype ``np.array``
    gives the colours (int64 for tuples of ints).  A label of the map that the dict does not hold is a ValueError.  A label between
    the smallest and the largest of the map that neither the map nor the dict holds has a row of zeros in the colour table."""
    segm = np.asarray(segm)
    orphans = [label for label in np.unique(segm).tolist() if label not in lut_label_colors]
    if orphans:
        raise ValueError('the labels %r of the map have no colour among %r' % (orphans, list(lut_label_colors)))
    first = segm.min()
    has_color = np.array([label in lut_label_colors for label in range(int(first), int(segm.max()) + 1)])
    known = np.array([lut_label_colors[int(first) + i] for i in np.flatnonzero(has_color)])
    table = np.zeros((len(has_color), ) + known.shape[1:], dtype=known.dtype)
    table[has_color] = known
    device_table = None
    if (_place(on, 'convert_img_labels_to_colors') == 'device' and segm.dtype.kind in 'biu' and len(table) <= _hip.ANNOT_MAX_COLORS
            and np.iinfo(np.int32).min <= first and segm.max() <= np.iinfo(np.int32).max and table.ndim == 2):
        device_table = _device_colors(list(table))
    if device_table is None:
        return labels_to_colors_host(segm, first, table)
    painted = _hip.annot_paint(np.ascontiguousarray(segm, dtype=np.int32), int(first), device_table, has_color.astype(np.uint8))
    return painted.astype(table.dtype)


# ------------------------------------------------------------------------------------------------
# nearest colour
# ------------------------------------------------------------------------------------------------

def nearest_color_index_host(img, colors):
    """the numpy statement of ``imsegm_annot_match`` in nearest mode: per pixel of ``img`` [..., 3] the index of the first of
    ``colors`` with the smallest sum of absolute differences (``np.argmin`` over the colours in their order), intp [pixels]"""
    flat = np.reshape(img, (-1, 3))
    best = best_dist = None
    for i, clr in enumerate(colors):
        dist = np.abs(flat - clr).sum(axis=1)
        if best is None:
            best, best_dist = np.zeros(len(flat), dtype=np.intp), dist
            continue
        # (what np.argmin does with a NaN: the first one is the minimum)
        closer = (dist < best_dist) | (np.isnan(dist) & ~np.isnan(best_dist)) if dist.dtype.kind == 'f' else dist < best_dist
        best[closer] = i
        best_dist = np.where(closer, dist, best_dist)
    if best is None:
        raise ValueError('attempt to get argmin of an empty sequence')
    return best


def _nearest_color_inputs(img, colors, on, name):
    """(uint8 image, uint8 table) when the device takes the call of the public function ``name``, else (None, None)"""
    if _place(on, name) != 'device':
        return None, None
    work, table = _device_image(img), _device_colors(colors)
    return (work, table) if work is not None and table is not None else (None, None)


def image_color_2_labels(img, colors=None, on=None):
    """Per pixel of ``img`` [H, W, 3] the index of the nearest of ``colors`` (sum of absolute channel differences, the first among
    equally near ones): intp [H, W].  Without ``colors`` the frequent colours of the image (:func:`image_frequent_colors`) are
    taken, numbered in ascending order of ``r << 16 | g << 8 | b``."""
    table_colors = list(colors) if colors else list(image_frequent_colors(img, on=on))
    work, table = _nearest_color_inputs(img, table_colors, on, 'image_color_2_labels')
    if work is None:
        return nearest_color_index_host(img, table_colors).reshape(img.shape[:2])
    return _hip.annot_match(work, table, mode=_hip.ANNOT_MATCH_NEAREST).astype(np.intp)


def quantize_image_nearest_color(img, colors, on=None):
    """``img`` [H, W, 3] with every pixel replaced by the nearest of ``colors`` (sum of absolute channel differences, the first
    among equally near ones), in the dtype of ``img``."""
    table_colors = list(colors)
    work, table = _nearest_color_inputs(img, table_colors, on, 'quantize_image_nearest_color')
    if work is None:
        index = nearest_color_index_host(img, table_colors)
        return np.asarray(table_colors)[index].astype(img.dtype).reshape(img.shape)
    return _hip.annot_match(work, table, mode=_hip.ANNOT_MATCH_NEAREST_COLOR).astype(img.dtype, copy=False)


# ------------------------------------------------------------------------------------------------
# nearest valid pixel
# ------------------------------------------------------------------------------------------------

def nearest_valid_host(labels, valid_mask, rows_per_chunk=16):
    """the numpy statement of ``imsegm_annot_nearest_valid`` by brute force (for tests and small maps): every pixel of the 2-D array
    ``labels`` outside ``valid_mask`` gets the value of the valid pixel at the smallest squared Euclidean distance (exact, in
    integers), among several at that distance of the one with the smallest row-major index.  Works in chunks of rows: the distance
    table of a chunk holds ``rows_per_chunk * width * n_valid`` int64.

    :raises ValueError: no pixel is valid
    """
    labels, valid_mask = np.asarray(labels), np.asarray(valid_mask, dtype=bool)
    rows, cols = np.nonzero(valid_mask)                # (row-major order: np.argmin keeps the first, the smallest index)
    if len(rows) == 0:
        raise ValueError('no valid pixel')
    values = labels[rows, cols]
    out = np.empty_like(labels)
    xs = np.arange(labels.shape[1], dtype=np.int64)
    for y0 in range(0, labels.shape[0], rows_per_chunk):
        ys = np.arange(y0, min(y0 + rows_per_chunk, labels.shape[0]), dtype=np.int64)
        d2 = (ys[:, None, None] - rows[None, None, :]) ** 2 + (xs[None, :, None] - cols[None, None, :]) ** 2
        out[ys[0]:ys[-1] + 1] = values[np.argmin(d2, axis=2)]
    return out


def inpaint_host(img, valid_mask):
    """the scipy statement: ``NearestNDInterpolator`` over the valid pixels, asked at every pixel in row-major order; which of
    several equally near pixels it takes is scipy's choice"""
    from scipy import interpolate
    nearest = interpolate.NearestNDInterpolator(np.argwhere(valid_mask), img[valid_mask])
    everywhere = np.indices(img.shape).reshape(img.ndim, -1).T
    return nearest(everywhere).reshape(img.shape)


def image_inpaint_pixels(img, valid_mask, on=None):
    """``img`` [H, W] with every pixel outside the bool mask ``valid_mask`` [H, W] replaced by the value of the nearest pixel inside
    it (Euclidean distance), in the dtype of ``img``.  On the device (a 2-D map whose valid values are integers of int32 other than
    -1) ties go to the smallest row-major index, on the host to scipy's choice.  Different shapes are an ImageDimensionError."""
    if img.shape != valid_mask.shape:
        raise ImageDimensionError('the mask %r does not cover the image %r' % (valid_mask.shape, img.shape))
    work = None
    if (_place(on, 'image_inpaint_pixels') == 'device' and _nearest_size_ok(img.shape) and valid_mask.dtype == bool
            and img.dtype.kind in 'biuf' and valid_mask.any()):
        values = img[valid_mask]
        whole = values.astype(np.int64) if values.dtype.kind != 'f' or np.all(np.isfinite(values)) else None
        if (whole is not None and np.array_equal(whole, values) and whole.min() >= np.iinfo(np.int32).min
                and whole.max() <= np.iinfo(np.int32).max and not np.any(whole == -1)):
            work = np.full(img.shape, -1, dtype=np.int32)
            work[valid_mask] = whole
    if work is None:
        return inpaint_host(img, valid_mask)
    return _hip.annot_nearest_valid(work).astype(img.dtype)


def exact_color_index_host(img, colors):
    """float64 [H, W]: the index of the last of ``colors`` the pixel equals, NaN for none"""
    index = np.full(img.shape[:-1], np.nan)
    for i, clr in enumerate(colors):
        apart = np.abs(img - np.asarray(clr).reshape((1, ) * (img.ndim - 1) + (-1, ))).sum(axis=-1)
        index[apart == 0] = i
    return index


def quantize_image_nearest_pixel(img, colors, on=None):
    """``img`` [H, W, 3] reduced to ``colors``: a pixel that has exactly one of the colours keeps it, every other pixel takes the
    colour of the nearest pixel that has one (Euclidean distance in the image plane).  The result has the dtype of
    ``np.asarray(colors)``.  Ties: see :func:`image_inpaint_pixels`.  An image without any pixel of the colours: what the host
    statement does on either place -- scipy answers NaN for an empty point set, the cast to int turns that into an index no colour
    table has, an IndexError."""
    table_colors = list(colors)
    work = table = None
    if _place(on, 'quantize_image_nearest_pixel') == 'device' and _nearest_size_ok(np.shape(img)[:2]):
        work, table = _device_image(img), _device_colors(table_colors)
    refused = None
    if work is not None and table is not None:
        try:
            return _hip.annot_quantize_nearest_pixel(work, table).astype(np.asarray(table_colors).dtype)
        except _hip.HipError as ex:
            refused = ex
    index = exact_color_index_host(img, table_colors)
    exact = ~np.isnan(index)
    if refused is not None and exact.any():
        raise refused          # (the entry point refuses an image without any pixel of the colours and nothing else the checks let through)
    return np.asarray(table_colors)[image_inpaint_pixels(index, exact, on='host').astype(int)]


# ------------------------------------------------------------------------------------------------
# annotated positions (host only)
# ------------------------------------------------------------------------------------------------

def load_info_group_by_slices(path_txt, stages, pos_columns=COLUMNS_POSITION, dict_slice_tol=ANNOT_SLICE_DIST_TOL):
    """The egg positions that belong to every annotated image of the stages ``stages``, from the tab-separated table ``path_txt``
    with the columns ``stage``, ``stack_path``, ``slice_index``, ``image_path`` and ``pos_columns``: a pandas DataFrame indexed by
    the image name without its extension (index name ``image``), one row per image of a selected stage, and per position column
    the array of the values of all annotations of the same stack and the selected stages whose slice is at most
    ``dict_slice_tol[stage of that annotation]`` slices from the image's.  No image of these stages: an empty DataFrame."""
    import pandas as pd
    table = pd.read_table(path_txt, index_col=0)
    table = table.loc[table['stage'].isin(list(stages))].sort_values(['stage'], ascending=False)
    logging.debug('%i annotations of the stages %r in %s', len(table), list(stages), path_txt)
    names, rows = [], []
    for _, stack in table.groupby(SLICE_NAME_GROUPING):
        z = stack['slice_index'].to_numpy()
        reach = np.array(list(map(dict_slice_tol.__getitem__, stack['stage'])))
        near = np.abs(z[:, None] - z[None, :]) <= reach[None, :]      # [image, annotation]
        positions = {column: stack[column].to_numpy() for column in pos_columns}
        for i, image_path in enumerate(stack['image_path']):
            names.append(os.path.splitext(image_path)[0])
            rows.append({column: values[near[i]] for column, values in positions.items()})
    if not rows:
        return pd.DataFrame()
    return pd.DataFrame(rows, index=pd.Index(names, name='image'))
