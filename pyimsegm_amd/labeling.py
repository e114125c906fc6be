"""The part of the reference module ``imsegm/labeling.py`` that is restated on the device.

* Superpixel x annotation histograms of the supervised SLIC -> features -> classifier -> GraphCut path
  (``histogram_regions_labels_counts`` :208, ``histogram_regions_labels_norm`` :250, called at ``imsegm/pipelines.py:284``).
  The reference counts with a per-pixel Python loop (``labeling.py:244-245``); here the pairs are counted by the HIP kernel
  ``k_label_hist`` (``csrc/stats.hip``) through ``imsegm_image2d_label_hist``.
* ``assume_bg_on_boundary`` (:719).
* Scoring of label maps: ``contour_binary_map`` (:34), ``contour_coords`` (:82), ``binary_image_from_coords`` (:120, plain numpy),
  ``compute_distance_map`` (:146), ``compute_labels_overlap_matrix`` (:490), ``relabel_max_overlap_unique`` (:526),
  ``relabel_max_overlap_merge`` (:617) and ``compute_boundary_distances`` (:684).  The reference walks the pixels in Python and
  calls ``scipy.ndimage.distance_transform_edt``; here the masks, the exact Euclidean distance transform, the row-major list of
  boundary points and the overlap counts come from ``csrc/boundary.hip`` and ``k_label_hist`` (``imsegm_boundary_mask``,
  ``imsegm_distance_map``, ``imsegm_boundary_distances``, ``imsegm_labels_overlap``); the look-up tables of the two relabellings
  are a few lines on the host.

2-D integer label maps whose values fit int32 go through the device.  There is no CPU fallback for them: without the HIP library
or a GPU the calls raise.  Inputs the device cannot take (float labels, labels outside int32, maps whose squared diagonal does not
fit 32 bits) are answered by numpy / scipy statements of the same definitions, as ``assume_bg_on_boundary`` does.
``compute_boundary_distances`` also takes 3-D integer maps to the device (``csrc/boundary3d.hip``, ``imsegm_boundary_distances3d``)
when one is present, and to the host statement otherwise (``on``, IMSEGM_BOUNDARY3D_ON).
"""
import numpy as np

from pyimsegm_amd import _hip
from pyimsegm_amd.utilities import ImageDimensionError


def _flat2d(arr):
    """any-dimensional label array as rows x columns (the histogram only sees the flat order)"""
    arr = np.asarray(arr)
    if arr.ndim == 0:
        return arr.reshape(1, 1)
    return arr.reshape(-1, arr.shape[-1]) if arr.ndim != 2 else arr


def histogram_regions_labels_counts(slic, segm, _session=None):
    """ histogram of overlapping regions between two segmentations,
    the typical usage is labelling superpixels from an annotation

    :param ndarray slic: superpixel map
    :param ndarray segm: annotation of the same shape, non-negative labels
    :param _session: (internal) device session that already holds ``slic`` as its label map
    :return ndarray: float matrix, rows = superpixels ``0..max(slic)``, columns = labels ``0..max(segm)``
    """
    segm = np.asarray(segm)
    if _session is None:
        slic = np.asarray(slic)
        if slic.shape != segm.shape:
            raise ImageDimensionError('dimension does not agree')
    elif tuple(_session.shape) != segm.shape:
        raise ImageDimensionError('dimension does not agree')
    if segm.size and segm.min() < 0:
        raise ValueError('only positive labels are allowed')
    nb_annot = int(segm.max()) + 1 if segm.size else 1
    if _session is not None:
        counts = _session.label_hist(segm, nb_annot)
    else:
        slic2d = _flat2d(slic)
        if slic2d.size and slic2d.min() < 0:
            raise ValueError('only positive superpixel labels are allowed')
        sess = _hip.Image2D(slic2d.shape[0], slic2d.shape[1]).set_labels(slic2d)
        try:
            counts = sess.label_hist(_flat2d(segm), nb_annot)
        finally:
            sess.close()
    return counts.astype(np.float64)


def histogram_regions_labels_norm(slic, segm, _session=None):
    """ normalised histogram of overlapping regions between two segmentations: the relative overlap of every
    superpixel with every annotation label (rows of superpixels without pixels stay zero)

    :param ndarray slic: superpixel map
    :param ndarray segm: annotation of the same shape
    :return ndarray: rows = superpixels, columns = labels; every non-empty row sums to one
    """
    shape = tuple(_session.shape) if _session is not None else np.shape(slic)
    if shape != np.shape(segm):
        raise ImageDimensionError('dimension of SLIC %r and segm %r should match' % (shape, np.shape(segm)))
    matrix_hist = histogram_regions_labels_counts(slic, segm, _session=_session)
    region_sums = matrix_hist.sum(axis=1, keepdims=True)
    region_sums[region_sums == 0] = -1.            # no division by zero
    matrix_hist = np.nan_to_num(matrix_hist / region_sums)
    matrix_hist[matrix_hist == 0] = 0              # no negative zeros
    return matrix_hist


def assume_bg_on_boundary(segm, bg_label=0, boundary_size=1):
    """ swap labels such that the background label is the one that dominates the image boundary
    (reference ``labeling.py:719-753``, called by the driver at ``run_segm_slic_model_graphcut.py:373,422``)

    2-D integer label images whose values fit int32 go through the device (``imsegm_assume_bg_on_boundary``: the histogram
    of the four border strips and the label exchange are two kernels on the uploaded map); anything else -- other
    dimensions, float labels -- through the numpy statements of the reference.

    :param ndarray segm: label image
    :param int bg_label: the label the background is to carry
    :param float boundary_size: width of the border that is looked at
    :return ndarray: segmentation with the boundary label and ``bg_label`` exchanged
    """
    arr = np.asarray(segm)
    size = int(boundary_size)
    if arr.ndim == 2 and arr.size and 0 < size <= min(arr.shape) and arr.dtype.kind in 'iu' and 0 <= int(bg_label) < 2**31 \
            and int(arr.min()) >= 0 and int(arr.max()) < 2**28:
        # (negative labels wrap around in the reference's ``np.array(lut)[segm]``, values of 2^28 and more do not fit the
        # device's border histogram: both take the numpy statements below)
        height, width = arr.shape
        # the four strips of data_io.py:1026 (0 < size <= min(shape): the only sizes np.hstack accepts there)
        rows_top, cols_left = slice(None, size).indices(height), slice(None, size).indices(width)
        rows_bottom, cols_right = slice(-size, None).indices(height), slice(-size, None).indices(width)
        strips = np.array([rows_top[0], max(rows_top[1], rows_top[0]), 0, width,
                           0, height, cols_left[0], max(cols_left[1], cols_left[0]),
                           rows_bottom[0], max(rows_bottom[1], rows_bottom[0]), 0, width,
                           0, height, cols_right[0], max(cols_right[1], cols_right[0])], dtype=np.int32)
        work = np.ascontiguousarray(arr, dtype=np.int32)
        if work is arr or np.shares_memory(work, arr):
            work = work.copy()
        _hip.assume_bg_on_boundary(work, strips, bg_label)
        # the reference indexes a Python list of ints: the result is an int64 array
        return work.astype(np.int64)
    from pyimsegm_amd.utilities.data_io import get_image2d_boundary_color
    on_border = int(get_image2d_boundary_color(segm, size=boundary_size))
    present = np.unique(segm)
    if on_border not in present:                   # (cannot happen for integer labels; the reference's statements in that case)
        segm[segm == on_border] = bg_label
        return segm
    # the exchange as a look-up table over 0 .. max(label, bg_label) (when the background label is not in use the reference's
    # table may be too short for it)
    lut = np.arange(max(int(present.max()), int(bg_label)) + 1)
    lut[[on_border, bg_label]] = bg_label, on_border
    return lut[segm]


# ---------------------------------------------------------------------------------------------------------------------
# scoring label maps: boundaries, distance maps, overlaps (reference labeling.py:34-169, :490-716)
# ---------------------------------------------------------------------------------------------------------------------
def _device_labels(arr):
    """the label array as contiguous int32 when the device can take it (integers that fit int32, not empty), else None"""
    arr = np.asarray(arr)
    if arr.dtype.kind not in 'iu' or not arr.size:
        return None
    if (arr.dtype.itemsize > 4 or arr.dtype == np.uint32) and (int(arr.min()) < -2**31 or int(arr.max()) >= 2**31):
        return None
    return np.ascontiguousarray(arr, dtype=np.int32)


def _device_map(arr):
    """a 2-D label map the distance kernels take: ``_device_labels`` and squared distances that fit 32 bits"""
    arr = np.asarray(arr)
    if arr.ndim != 2 or arr.shape[0] > 65535 or arr.shape[0]**2 + arr.shape[1]**2 > 2**32 - 1:
        return None
    return _device_labels(arr)


def _device_volume(arr):
    """a 3-D label map the volume kernels take: ``_device_labels`` and a shape within ``_hip.boundary3d_fits``"""
    arr = np.asarray(arr)
    if not _hip.boundary3d_fits(arr.shape):
        return None
    return _device_labels(arr)


def _device_label(label):
    """the selected label as an int the device compares with, or None (not a whole number, outside int32)"""
    try:
        whole = int(label)
    except (TypeError, ValueError, OverflowError):
        return None
    return whole if whole == label and -2**31 <= whole < 2**31 else None


def _thick_boundaries(segm):
    """``skimage.segmentation.find_boundaries(segm, mode='thick')`` in numpy, any dimension: a neighbour along an axis differs"""
    segm = np.asarray(segm)
    mask = np.zeros(segm.shape, dtype=bool)
    for axis in range(segm.ndim):
        front, back = [slice(None)] * segm.ndim, [slice(None)] * segm.ndim
        front[axis], back[axis] = slice(1, None), slice(None, -1)
        differs = segm[tuple(front)] != segm[tuple(back)]
        mask[tuple(front)] |= differs
        mask[tuple(back)] |= differs
    return mask


def _contour_mask_host(seg, label, include_boundary):
    """the definition of ``contour_binary_map`` in numpy (boolean map)"""
    seg = np.asarray(seg)
    height, width = seg.shape[:2]
    own = seg == label
    mask = np.zeros((height, width), dtype=bool)
    mask[1:-1, 1:-1] = own[1:-1, 1:-1] & ~(own[:-2, 1:-1] & own[2:, 1:-1] & own[1:-1, :-2] & own[1:-1, 2:])
    if include_boundary:
        for edge in (np.s_[:, 0], np.s_[:, -1], np.s_[0, :], np.s_[-1, :]):
            mask[edge] |= own[edge]
    return mask


def _contour_mask(seg, label, include_boundary):
    work, whole = _device_map(seg), _device_label(label)
    if work is None or whole is None:
        return _contour_mask_host(seg, label, include_boundary)
    return _hip.boundary_mask(work, _hip.BOUNDARY_CONTOUR_BORDER if include_boundary else _hip.BOUNDARY_CONTOUR, whole)


def contour_binary_map(seg, label=1, include_boundary=False):
    """ get object boundaries: the pixels of ``label`` inside the image that touch (4-connected) another label
    (reference ``labeling.py:34-79``)

    2-D integer maps go through the device (``imsegm_boundary_mask``), anything else -- float labels, labels outside int32 --
    through numpy statements of the same definition.

    :param ndarray seg: integer image, typically a segmentation
    :param int label: selected single label in the segmentation
    :param bool include_boundary: assume that the object ends with the image boundary
    :return ndarray: int64 map, 1 on the contour
    """
    return _contour_mask(seg, label, include_boundary).astype(np.int64)


def contour_coords(seg, label=1, include_boundary=False):
    """ coordinates of the object boundaries (reference ``labeling.py:82-117``): the interior contour in row-major order
    (from the device mask), then -- with ``include_boundary`` -- the border pixels of ``label`` in the reference's order:
    per row the first and the last column, then per column the first and the last row (corners appear twice)

    :param ndarray seg: integer image, typically a segmentation
    :param int label: selected single label in the segmentation
    :param bool include_boundary: assume that the object ends with the image boundary
    :return list(list(int)): ``[i, j]`` pairs
    """
    coords = np.argwhere(_contour_mask(seg, label, False)).tolist()
    if include_boundary:
        own = np.asarray(seg) == label
        height, width = own.shape[:2]
        rows, cols = np.arange(height), np.arange(width)
        # [i, 0], [i, width - 1] for every row, then [0, j], [height - 1, j] for every column
        by_row = np.stack([np.stack([rows, np.zeros_like(rows)], axis=1), np.stack([rows, np.full_like(rows, width - 1)], axis=1)], axis=1)
        by_col = np.stack([np.stack([np.zeros_like(cols), cols], axis=1), np.stack([np.full_like(cols, height - 1), cols], axis=1)], axis=1)
        coords += by_row[np.stack([own[:, 0], own[:, -1]], axis=1)].tolist()
        coords += by_col[np.stack([own[0, :], own[-1, :]], axis=1)].tolist()
    return coords


def binary_image_from_coords(coords, size):
    """ binary image from contour points (reference ``labeling.py:120-143``); points outside the image are dropped

    :param coords: sequence of ``[i, j]``
    :param tuple(int,int) size: image size
    :return ndarray: int64 map, 1 at the points
    """
    contour_map = np.zeros(size, dtype=np.int64)
    height, width = size
    points = np.asarray(coords)
    if points.size:
        points = points.reshape(len(points), -1)
        inside = (points[:, 0] >= 0) & (points[:, 0] < height) & (points[:, 1] >= 0) & (points[:, 1] < width)
        contour_map[points[inside, 0], points[inside, 1]] = 1
    return contour_map


def compute_distance_map(seg, label=1):
    """ Euclidean distance of every pixel from the contour of ``label`` (reference ``labeling.py:146-169``:
    ``distance_transform_edt`` of the complement of the contour; a map without a contour gets scipy's answer for it,
    the distance to row -1, column 0)

    2-D integer maps go through the device (``imsegm_distance_map``: exact integer squared distances, one square root), anything
    else through the numpy mask and ``scipy.ndimage.distance_transform_edt``.

    :param ndarray seg: integer image, typically a segmentation
    :param int label: selected single label in the segmentation
    :return ndarray: float64 map
    """
    work, whole = _device_map(seg), _device_label(label)
    if work is None or whole is None:
        from scipy import ndimage
        return ndimage.distance_transform_edt(~_contour_mask_host(seg, label, False))
    return _hip.distance_map(work, _hip.BOUNDARY_CONTOUR, whole)


def compute_labels_overlap_matrix(seg1, seg2):
    """ overlap of two segmentations of the same size (reference ``labeling.py:490-523``): ``overlap[a, b]`` = number of
    pixels with ``seg1 == a`` and ``seg2 == b``; pairs with a negative label are skipped

    Integer arrays (any dimension) whose values fit int32 are counted on the device (``imsegm_labels_overlap``), anything else by
    the numpy statement of the same count.

    :param ndarray seg1: label array
    :param ndarray seg2: label array of the same shape
    :return ndarray: int64 matrix ``(max(seg1) + 1) x (max(seg2) + 1)``
    """
    seg1, seg2 = np.asarray(seg1), np.asarray(seg2)
    if seg1.shape != seg2.shape:
        raise ImageDimensionError('segm %r and segm %r should match' % (seg1.shape, seg2.shape))
    extents = [np.max(seg1) + 1, np.max(seg2) + 1]
    work1, work2 = _device_labels(seg1), _device_labels(seg2)
    if work1 is None or work2 is None or min(extents) < 1 or int(extents[0]) * int(extents[1]) > 2**28:
        overlap = np.zeros(extents, dtype=np.int64)
        flat1, flat2 = seg1.ravel(), seg2.ravel()
        counted = (flat1 >= 0) & (flat2 >= 0)
        np.add.at(overlap, (flat1[counted], flat2[counted]), 1)
        return overlap
    return _hip.labels_overlap(work1, work2, int(extents[0]), int(extents[1]))


def _keep_negative(seg_new, seg_relabel):
    negative = seg_relabel < 0
    seg_new[negative] = seg_relabel[negative]
    return seg_new


def relabel_max_overlap_unique(seg_ref, seg_relabel, keep_bg=False):
    """ relabel the second segmentation such that the overlap with the reference is maximal, one label to one label
    (reference ``labeling.py:526-614``; the overlap matrix comes from the device, the table is built here)

    :param ndarray seg_ref: reference segmentation
    :param ndarray seg_relabel: segmentation to relabel
    :param bool keep_bg: label 0 stays
    :return ndarray: int64 segmentation; negative labels are kept
    """
    seg_ref, seg_relabel = np.asarray(seg_ref), np.asarray(seg_relabel)
    if seg_ref.shape != seg_relabel.shape:
        raise ImageDimensionError('Reference segm. %r and input segm. %r should match' % (seg_ref.shape, seg_relabel.shape))
    lut = max_overlap_unique_lut(compute_labels_overlap_matrix(seg_ref, seg_relabel), keep_bg)
    return _keep_negative(np.array(lut)[seg_relabel].astype(np.int64), seg_relabel)


def max_overlap_unique_lut(overlap, keep_bg=False):
    """the look-up table of :func:`relabel_max_overlap_unique` from the overlap matrix of the two maps (rows: reference labels,
    columns: labels ``0 .. max`` of the map to relabel; the matrix is used up): a list with the new label of every column"""
    lut = [-1] * overlap.shape[1]
    if keep_bg:
        lut[0] = 0
        overlap[0, :] = 0
        overlap[:, 0] = 0
    # greedy: the largest remaining count pairs its two labels (the first one in row-major order on ties) and retires both
    for _ in range(max(overlap.shape) + 1):
        if not overlap.any():
            break
        lb_ref, lb_est = np.unravel_index(np.argmax(overlap), overlap.shape)
        lut[lb_est] = int(lb_ref)
        overlap[lb_ref, :] = 0
        overlap[:, lb_est] = 0
    taken = set(lut) - {-1}
    # a label without a partner keeps its own number while nobody has taken it ...
    for idx in range(len(lut)):
        if lut[idx] == -1 and idx not in taken:
            lut[idx] = idx
            taken.add(idx)
    # ... and otherwise gets the largest number below len(lut) nobody has (the reference's inner loop runs on to the last one)
    for idx in range(len(lut)):
        if lut[idx] == -1:
            lut[idx] = max(free for free in range(len(lut)) if free not in taken)
            taken.add(lut[idx])
    return lut


def relabel_max_overlap_merge(seg_ref, seg_relabel, keep_bg=False):
    """ relabel the second segmentation such that every label takes the reference label it overlaps most; several labels may
    merge into one (reference ``labeling.py:617-681``; the overlap matrix comes from the device, the table is built here)

    :param ndarray seg_ref: reference segmentation
    :param ndarray seg_relabel: segmentation to relabel
    :param bool keep_bg: label 0 stays
    :return ndarray: int64 segmentation; negative labels are kept
    """
    seg_ref, seg_relabel = np.asarray(seg_ref), np.asarray(seg_relabel)
    if seg_ref.shape != seg_relabel.shape:
        raise ImageDimensionError('Ref. segm %r and segm %r should match' % (seg_ref.shape, seg_relabel.shape))
    overlap = compute_labels_overlap_matrix(seg_ref, seg_relabel)
    # (the reference looks along the columns when the reference map has more labels than the other one)
    axis = 1 if overlap.shape[0] > overlap.shape[1] else 0
    if keep_bg:
        lut = np.concatenate([[0], np.argmax(overlap[1:, 1:], axis=axis) + 1])
    else:
        lut = np.argmax(overlap, axis=axis)
    untouched = overlap.sum(axis=0) == 0               # labels that overlap nothing keep their number
    if untouched.any():
        lut[untouched] = np.flatnonzero(untouched)
    return _keep_negative(lut[seg_relabel].astype(np.int64), seg_relabel)


def compute_boundary_distances(segm_ref, segm, _session=None, on=None):
    """ distances between the boundaries of two segmentations (reference ``labeling.py:684-716``, the superpixel measure of
    ``run_eval_superpixels.py:108-131``): the pixels of the thick boundary of ``segm_ref`` in row-major order and their
    Euclidean distance to the thick boundary of ``segm``

    2-D integer maps go through the device (``imsegm_boundary_distances``: masks, exact distance transform, stable compaction;
    only the points come back).  3-D integer maps that fit int32 and the limits of the volume kernels (``_hip.boundary3d_fits``)
    go through the device when one is present (``imsegm_boundary_distances3d``: the same with a depth pass; points are ``n x 3``)
    and through the host statement otherwise; ``on`` or the variable IMSEGM_BOUNDARY3D_ON choose for them.  Anything else -- float
    labels, labels outside int32, other dimensions, oversized volumes -- takes the host statement: numpy and
    ``scipy.ndimage.distance_transform_edt``, which work in any dimension (points are then ``n x ndim``).

    :param ndarray segm_ref: reference segmentation
    :param ndarray segm: input segmentation
    :param _session: (internal) device session that already holds ``segm`` as its label map (an image or a volume session)
    :param str on: for 3-D maps None (the device when there is one), 'host' or 'device' (raises without one)
    :return tuple(ndarray,ndarray): points int64 ``n x ndim`` and distances float64 ``n``
    """
    if on not in (None, 'host', 'device'):
        raise ValueError("on is 'host' or 'device', not %r" % (on, ))
    segm_ref = np.asarray(segm_ref)
    shape = tuple(_session.shape) if _session is not None else np.shape(segm)
    if segm_ref.shape != shape:
        raise ImageDimensionError('Ref. segm %r and segm %r should match' % (segm_ref.shape, shape))
    volume = segm_ref.ndim == 3
    work_ref = _device_volume(segm_ref) if volume else _device_map(segm_ref)
    if _session is not None:
        if work_ref is None:
            raise ValueError('the reference segmentation must hold integer labels that fit int32')
        points, dist = _session.boundary_distances(work_ref)
        return points.astype(np.int64), dist
    if volume:
        on_device = _hip.resolve_place(on, 'IMSEGM_BOUNDARY3D_ON', True)[0] == 'device'
        work = _device_volume(segm) if on_device and work_ref is not None else None
    else:
        work = _device_map(segm)
    if work_ref is None or work is None:
        from scipy import ndimage
        on_ref = _thick_boundaries(segm_ref)
        return np.argwhere(on_ref).astype(np.int64), ndimage.distance_transform_edt(~_thick_boundaries(segm))[on_ref].ravel()
    points, dist = (_hip.boundary_distances3d if volume else _hip.boundary_distances)(work_ref, work)
    return points.astype(np.int64), dist
