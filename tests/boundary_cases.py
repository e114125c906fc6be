"""Shared by tests/test_boundary_reference_host.py, tests/test_gpu_boundary.py and tests/golden/make_golden_boundary.py: the
seeded label maps and a numpy / scipy restatement of the definitions behind the scoring functions of ``pyimsegm_amd.labeling``
(``contour_binary_map``, ``contour_coords``, ``compute_distance_map``, ``compute_boundary_distances``,
``compute_labels_overlap_matrix``, ``relabel_max_overlap_unique``, ``relabel_max_overlap_merge``).

Restatement.  scikit-image is not a dependency of the tests: ``find_boundaries(mode='thick')`` is "a 4-neighbour inside the image
carries another label", written with shifted comparisons (``thick``; ``thick_morphology`` is the grey dilation != grey erosion
form with the cross footprint that scikit-image evaluates, the host test shows the two agree).  Distances are
``scipy.ndimage.distance_transform_edt`` of the complement; ``edt_brute`` is the square root of the brute-force integer minimum,
which scipy equals bit for bit (host test).  Every result is exact -- integers up to one correctly rounded square root -- so all
comparisons are ``np.array_equal`` with dtype and shape.  No expected number comes from the device code.

Cases: the smallest shapes at which the kernels can go wrong -- one row, one column, widths on both sides of the 64-lane wave and
of the 256-pixel row tile (63, 65, 257, 300, 700), heights on both sides of the 4-row mask block, 1 / 2 / 5 / 40 labels, block
maps that look like superpixels, a single set pixel in the far corner of 64 x 300 (the longest search, two tiles away), masks
confined to one column and to one row, one 512 x 700 map of jittered blocks (more than one 2048-pixel compaction chunk per row
group, more than 256 chunks for the scan's carry), negative labels on either side and very different label counts."""
import functools

import numpy as np
from scipy import ndimage

SEED = 20261018
SHAPES = ((1, 1), (1, 7), (7, 1), (2, 65), (33, 65), (65, 63), (64, 257))
LABEL_COUNTS = (1, 2, 5, 40)


def _rng(*key):
    return np.random.default_rng([SEED] + [int(k) for k in key])


# ---- label maps ---------------------------------------------------------------------------------------------------------------
def random_map(shape, n_labels, seed=0):
    return _rng(seed, n_labels, *shape).integers(0, n_labels, shape).astype(np.int64)


def block_map(shape, step=(9, 11), seed=0, jitter=0.0):
    """rectangular blocks of `step` pixels numbered in raster order; jitter: that share of the pixels takes the label of the
    pixel one to the right (ragged edges, as superpixels have)"""
    rows, cols = np.indices(shape)
    seg = (rows // step[0]) * (-(-shape[1] // step[1])) + cols // step[1]
    if jitter:
        moved = _rng(seed, *shape).random(shape) < jitter
        seg = np.where(moved, np.roll(seg, -1, axis=1), seg)
    return seg.astype(np.int64)


@functools.lru_cache(maxsize=None)
def maps():
    """name -> label map (int64, read-only)"""
    out = {}
    for shape in SHAPES:
        for count in LABEL_COUNTS:
            out['rand_%dx%d_L%d' % (shape + (count, ))] = random_map(shape, count)
    for shape, step in (((33, 65), (8, 11)), ((65, 63), (9, 7)), ((64, 257), (16, 40)), ((64, 96), (13, 17))):
        out['blocks_%dx%d' % shape] = block_map(shape, step)
        out['ragged_%dx%d' % shape] = block_map(shape, step, seed=1, jitter=0.15)
    far = np.zeros((64, 300), dtype=np.int64)
    far[62, 298] = 1                                    # contour of label 1: exactly this pixel
    out['far_corner_64x300'] = far
    corner = np.zeros((64, 300), dtype=np.int64)
    corner[63, 299] = 3                                 # thick boundary: the corner and its two neighbours
    out['corner_64x300'] = corner
    column = np.zeros((33, 300), dtype=np.int64)
    column[:, 5] = 1                                    # contour of label 1: rows 1 .. 31 of column 5
    out['one_column_33x300'] = column
    row = np.zeros((65, 63), dtype=np.int64)
    row[60, :] = 1                                      # contour of label 1: columns 1 .. 61 of row 60
    out['one_row_65x63'] = row
    out['slic_like_512x700'] = block_map((512, 700), (44, 47), seed=2, jitter=0.1)
    out['annot_512x700'] = block_map((512, 700), (170, 233))
    for seg in out.values():
        seg.setflags(write=False)
    return out


def contour_cases():
    """(map name, label): every map with label 1, the many-label maps also with a label that sits on the border"""
    names = list(maps())
    return [(name, 1) for name in names] + [(name, 0) for name in names if name.startswith(('blocks', 'rand_33x65', 'far'))]


def pair_cases():
    """(reference map, other map) of one shape for the boundary distances, the overlap matrix and the relabellings: equal and
    different label counts, no boundary on either side (0 points / scipy's answer for an empty mask), many against few labels"""
    pairs = []
    for shape in SHAPES:
        tag = '%dx%d' % shape
        pairs += [('rand_%s_L5' % tag, 'rand_%s_L2' % tag), ('rand_%s_L2' % tag, 'rand_%s_L40' % tag), ('rand_%s_L40' % tag, 'rand_%s_L5' % tag),
                  ('rand_%s_L1' % tag, 'rand_%s_L5' % tag), ('rand_%s_L5' % tag, 'rand_%s_L1' % tag), ('rand_%s_L1' % tag, 'rand_%s_L1' % tag)]
    pairs += [('blocks_33x65', 'ragged_33x65'), ('ragged_65x63', 'blocks_65x63'), ('blocks_64x257', 'ragged_64x257'),
              ('ragged_64x96', 'blocks_64x96'), ('blocks_64x96', 'ragged_64x96'), ('ragged_64x257', 'rand_64x257_L2'),
              ('ragged_64x257', 'rand_64x257_L1'), ('far_corner_64x300', 'corner_64x300'),
              ('corner_64x300', 'far_corner_64x300'), ('annot_512x700', 'slic_like_512x700'), ('slic_like_512x700', 'annot_512x700')]
    return pairs


@functools.lru_cache(maxsize=None)
def negative_pairs():
    """name -> (seg1, seg2) with negative labels on the first, the second and both sides"""
    out = {}
    for which, sides in enumerate(((True, False), (False, True), (True, True))):
        seg1, seg2 = random_map((33, 65), 5, seed=10 + which).copy(), random_map((33, 65), 7, seed=20 + which).copy()
        for side, seg in zip(sides, (seg1, seg2)):
            if side:
                seg[_rng(30 + which, seg.max()).random(seg.shape) < 0.1] = -1
                seg[0, 0] = -3
        out['negative_%d%d' % sides] = (seg1, seg2)
    return out


GOLDEN_MAPS = ('rand_1x7_L2', 'rand_7x1_L2', 'rand_2x65_L5', 'rand_33x65_L1', 'rand_33x65_L2', 'rand_33x65_L5', 'rand_33x65_L40',
               'blocks_33x65', 'ragged_33x65', 'blocks_64x96', 'ragged_64x96')
GOLDEN_PAIRS = (('rand_1x7_L2', 'rand_1x7_L2'), ('rand_7x1_L2', 'rand_7x1_L2'), ('rand_33x65_L5', 'rand_33x65_L2'),
                ('rand_33x65_L2', 'rand_33x65_L40'), ('rand_33x65_L40', 'rand_33x65_L5'), ('rand_33x65_L1', 'rand_33x65_L5'),
                ('rand_33x65_L5', 'rand_33x65_L1'), ('blocks_33x65', 'ragged_33x65'), ('ragged_64x96', 'blocks_64x96'),
                ('blocks_64x96', 'ragged_64x96'))


# ---- the definitions in numpy / scipy -----------------------------------------------------------------------------------------
def thick(seg):
    """find_boundaries(seg, mode='thick'): a 4-neighbour inside the image carries another label"""
    seg = np.asarray(seg)
    out = np.zeros(seg.shape, dtype=bool)
    out[:-1, :] |= seg[:-1, :] != seg[1:, :]
    out[1:, :] |= seg[1:, :] != seg[:-1, :]
    out[:, :-1] |= seg[:, :-1] != seg[:, 1:]
    out[:, 1:] |= seg[:, 1:] != seg[:, :-1]
    return out


def thick_morphology(seg):
    """the form scikit-image evaluates: grey dilation != grey erosion under the 4-connected cross"""
    cross = ndimage.generate_binary_structure(2, 1)
    return ndimage.grey_dilation(seg, footprint=cross) != ndimage.grey_erosion(seg, footprint=cross)


def contour(seg, label=1, include_boundary=False):
    """interior pixels of `label` with a 4-neighbour of another label; with include_boundary also its pixels on the image border"""
    seg = np.asarray(seg)
    own = seg == label
    padded = np.pad(own, 1, constant_values=True)
    all_neighbours_own = padded[:-2, 1:-1] & padded[2:, 1:-1] & padded[1:-1, :-2] & padded[1:-1, 2:]
    on_border = np.ones(seg.shape, dtype=bool)
    on_border[1:-1, 1:-1] = False
    out = own & ~all_neighbours_own & ~on_border
    if include_boundary:
        out |= own & on_border
    return out.astype(np.int64)


def contour_points(seg, label=1, include_boundary=False):
    """the interior contour in row-major order, then the border pixels of `label`: for every row its first and its last column,
    then for every column its first and its last row (a pixel can appear more than once)"""
    seg = np.asarray(seg)
    height, width = seg.shape
    out = [[int(i), int(j)] for i, j in zip(*np.nonzero(contour(seg, label)))]
    if include_boundary:
        for i in range(height):
            out += [[i, j] for j in (0, width - 1) if seg[i, j] == label]
        for j in range(width):
            out += [[i, j] for i in (0, height - 1) if seg[i, j] == label]
    return out


def edt(mask):
    """distance of every pixel to the nearest True pixel of `mask`"""
    return ndimage.distance_transform_edt(~np.asarray(mask, dtype=bool))


def edt_brute(mask):
    """sqrt of the brute-force minimum of the integer squared distances (small masks with a set pixel only)"""
    mask = np.asarray(mask, dtype=bool)
    ys, xs = np.nonzero(mask)
    rows, cols = np.indices(mask.shape)
    squared = ((rows[..., None] - ys)**2 + (cols[..., None] - xs)**2).min(axis=-1)
    return np.sqrt(squared.astype(np.float64))


def distance_map(seg, label=1):
    return edt(contour(seg, label))


def boundary_distances(seg_ref, seg):
    on_ref = thick(seg_ref)
    return np.argwhere(on_ref).astype(np.int64).reshape(-1, 2), edt(thick(seg))[on_ref]


def overlap_matrix(seg1, seg2):
    seg1, seg2 = np.asarray(seg1).ravel(), np.asarray(seg2).ravel()
    extents = (int(seg1.max()) + 1, int(seg2.max()) + 1)
    counted = (seg1 >= 0) & (seg2 >= 0)
    flat = np.bincount(seg1[counted] * extents[1] + seg2[counted], minlength=extents[0] * extents[1])
    return flat.reshape(extents).astype(np.int64)


def relabel_unique(seg_ref, seg, keep_bg=False):
    """one-to-one: repeatedly pair the two labels of the largest remaining overlap (first in row-major order); labels left over
    keep their own number if it is free, else take the largest free number below the table's length"""
    seg = np.asarray(seg)
    counts = overlap_matrix(seg_ref, seg)
    table = np.full(int(seg.max()) + 1, -1, dtype=np.int64)
    if keep_bg:
        table[0] = 0
        counts[0, :] = 0
        counts[:, 0] = 0
    while counts.any():
        ref_label, own_label = divmod(int(counts.argmax()), counts.shape[1])
        table[own_label] = ref_label
        counts[ref_label, :] = 0
        counts[:, own_label] = 0
    for own_label in np.flatnonzero(table < 0):
        if own_label not in table:
            table[own_label] = own_label
    for own_label in np.flatnonzero(table < 0):
        table[own_label] = np.setdiff1d(np.arange(len(table)), table)[-1]
    out = table[seg]
    out[seg < 0] = seg[seg < 0]
    return out


def relabel_merge(seg_ref, seg, keep_bg=False):
    """many-to-one: every label takes the reference label of its largest overlap -- looked up along the OTHER axis when the
    reference has more labels than the map (the reference's `max_axis`; an IndexError there when a label overlaps nothing)"""
    seg = np.asarray(seg)
    counts = overlap_matrix(seg_ref, seg)
    axis = int(counts.shape[0] > counts.shape[1])
    if keep_bg:
        table = np.r_[0, counts[1:, 1:].argmax(axis=axis) + 1].astype(np.int64)
    else:
        table = counts.argmax(axis=axis).astype(np.int64)
    alone = counts.sum(axis=0) == 0
    if alone.any():
        if len(alone) != len(table):
            raise IndexError('boolean index did not match')
        table[alone] = np.flatnonzero(alone)
    out = table[seg]
    out[seg < 0] = seg[seg < 0]
    return out


def outcome(call, *args, **kwargs):
    """('ok', value) or ('raises', exception type): the relabellings fail on some label layouts, in the reference too"""
    try:
        return 'ok', call(*args, **kwargs)
    except Exception as ex:        # noqa: B902 -- the type is what is compared
        return 'raises', type(ex)


def same(a, b):
    """bit for bit, dtype and shape included"""
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)


def same_outcome(a, b):
    return a[0] == b[0] and (a[1] is b[1] if a[0] == 'raises' else same(a[1], b[1]))
