"""Inputs of the centre-annotation tests (tests/test_center_annotation_reference_host.py, tests/test_gpu_center_annotation.py) and
of tests/golden/make_golden_center_annotation.py, which runs the reference's ``run_create_annotation`` on them.  Ellipses are painted
with the package's own ``ellipse_pixels_host``; no scikit-image is needed.  Every case is built at the smallest shape that crosses
the rule it is named for; the tests assert that it does.

``ROW_CASES``, ``CORRECT_EDGE_CASES`` and the run-rule maps of tests/cut_objects_cases.py (``run_level_maps``) are the edge tables: plain
arrays at the wave, workgroup and search-window edges of csrc/center_annotation.hip, with numpy / scipy expectations formed in the tests.
``LEVEL_CASES``: name -> builder of ``dict(seg=int32 label map, levels=list)`` for ``segm_center_levels`` / ``compute_eggs_center``.
``CORRECT_CASES``: name -> builder of ``dict(img=uint8 map, sel_radius=int, min_size=int)`` for ``correct_segm`` /
``create_annot_centers``.  ``HOST_ONLY``: cases beyond a cap of the device entry."""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden', 'center_annotation.npz')
LEVELS = [0., 0.4, 0.8]


def _paint(seg, label, r, c, r_radius, c_radius, orientation=0.):
    from pyimsegm_amd.ellipse_fitting import ellipse_pixels_host
    seg[ellipse_pixels_host(r, c, r_radius, c_radius, orientation, seg.shape)] = label
    return seg


def _touching():
    """two eggs that share a straight edge: the distance of either has to see the other as background"""
    seg = np.zeros((50, 86), dtype=np.int32)
    seg[8:42, 6:44] = 1
    seg[12:40, 44:80] = 2
    return dict(seg=seg, levels=LEVELS)


def _border():
    """eggs cut by the image border on two sides: the border is no background, so the distance grows towards it"""
    seg = np.zeros((60, 90), dtype=np.int32)
    _paint(seg, 1, 4., 30., 22, 17, 0.3)
    _paint(seg, 2, 40., 86., 15, 24, 1.1)
    return dict(seg=seg, levels=LEVELS)


def _hole():
    seg = np.zeros((70, 75), dtype=np.int32)
    _paint(seg, 1, 34., 37., 30, 33, 0.)
    _paint(seg, 0, 30., 46., 5, 4, 0.)
    return dict(seg=seg, levels=LEVELS)


def _missing_label():
    """labels 1, 3 and 6 of 1 .. 6"""
    seg = np.zeros((64, 96), dtype=np.int32)
    _paint(seg, 1, 20., 22., 15, 18, 0.4)
    _paint(seg, 3, 40., 66., 19, 22, 2.0)
    _paint(seg, 6, 52., 14., 9, 11, 0.)
    return dict(seg=seg, levels=LEVELS)


def _row_segment():
    """a label that fills whole rows of a map wider than two search windows of the row pass: no row holds a foreign pixel, every
    distance comes from the columns"""
    seg = np.zeros((41, 700), dtype=np.int32)
    seg[6:35, :] = 1
    seg[0:3, 300:340] = 2
    return dict(seg=seg, levels=LEVELS)


def _whole_map():
    """one label and nothing else: scipy's distance transform has no background pixel to measure from"""
    return dict(seg=np.full((9, 13), 1, dtype=np.int32), levels=LEVELS)


def _small_egg():
    """discs so small that int(radius * 0.15) == 0 at both upper levels, and a single pixel"""
    seg = np.zeros((30, 40), dtype=np.int32)
    _paint(seg, 1, 10., 10., 8, 8)
    _paint(seg, 2, 20., 30., 3, 3)
    seg[27, 4] = 3
    return dict(seg=seg, levels=LEVELS)


def _open1():
    """a disc whose level 2 (0-based 1) is opened with disk(1)"""
    return dict(seg=_paint(np.zeros((40, 41), dtype=np.int32), 1, 19., 20., 16, 16), levels=LEVELS)


def _big_disc(radius):
    side = 2 * radius + 21
    seg = _paint(np.zeros((side, side), dtype=np.int32), 1, side // 2 + 0.5, side // 2, radius, radius)
    seg[2:7, 3:9] = 2
    return dict(seg=seg, levels=[0., 0.])


def _tie():
    """a 9 x 9 square: distances 1 .. 5, and 2 / 5 is the double 0.4: those pixels stay out of level 2"""
    seg = np.zeros((15, 17), dtype=np.int32)
    seg[3:12, 4:13] = 1
    return dict(seg=seg, levels=LEVELS)


def _split():
    """two overlapping discs: the level mask is one piece with a neck that the opening removes"""
    seg = np.zeros((60, 100), dtype=np.int32)
    _paint(seg, 1, 30., 30., 21, 21)
    _paint(seg, 1, 30., 68., 21, 21)
    return dict(seg=seg, levels=LEVELS)


def _many_levels():
    """eight levels, the cap of the device entry, two of them equal"""
    seg = np.zeros((64, 96), dtype=np.int32)
    _paint(seg, 2, 30., 30., 25, 28, 0.5)
    _paint(seg, 5, 34., 74., 22, 17, 1.9)
    return dict(seg=seg, levels=[0., 0.1, 0.25, 0.25, 0.5, 0.6, 0.75, 0.9])


LEVEL_CASES = {
    'touching': _touching, 'border': _border, 'hole': _hole, 'missing_label': _missing_label, 'row_segment': _row_segment,
    'whole_map': _whole_map, 'small_egg': _small_egg, 'open1': _open1, 'open64': lambda: _big_disc(430), 'tie': _tie,
    'split': _split, 'many_levels': _many_levels,
}
#: beyond a cap of ``imsegm_center_levels``: an opening radius of 65, levels that descend, nine levels
HOST_ONLY = {
    'open65': lambda: _big_disc(436),
    'descending': lambda: dict(seg=_missing_label()['seg'], levels=[0., 0.8, 0.4]),
    'nine_levels': lambda: dict(seg=_open1()['seg'], levels=[0., 0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8]),
}


def _disc(radius):
    y, x = np.ogrid[-radius:radius + 1, -radius:radius + 1]
    return x * x + y * y <= radius * radius


def _stamp(img, radius, centres, value=255):
    """the union of the discs around ``centres``, clipped by the image: an opening with that disc leaves it as it is"""
    height, width = img.shape
    for r, c in centres:
        for dy, dx in zip(*np.nonzero(_disc(radius))):
            y, x = r + dy - radius, c + dx - radius
            if 0 <= y < height and 0 <= x < width:
                img[y, x] = value
    return img


def _line(r, c, n):
    return [(r, c + i) for i in range(n)]


def _correct(radius):
    """sel_radius 1 or 2.  Blobs, in raster order of their first pixels:
    * a U whose right arm starts above its left arm and above everything else, its base far below: label 1;
    * a blob inside the U: label 2 (a numbering by the first pixel of every row run would give it 3);
    * a blob on the left and one on the top border;
    * components of exactly min_size - 1 (removed) and min_size pixels (kept);
    * two blobs of at least min_size pixels that touch only diagonally: one label;
    * specks that the opening removes."""
    img = np.zeros((78, 120), dtype=np.uint8)
    step = radius + 1                                   # discs (a, a) and (a + step, a + step) touch only diagonally
    min_size = {1: 20, 2: 38}[radius]
    under, exact = {1: (_line(0, 0, 5) + [(1, 0)], _line(0, 0, 6)), 2: (_line(0, 0, 5) + [(2, 2)], _line(0, 0, 5) + [(2, 1)])}[radius]
    # the U: arms of stamps going down, a base of stamps
    _stamp(img, radius, [(r, 44) for r in range(9, 40)] + [(r, 8) for r in range(12, 40)] + _line(40, 8, 37))
    _stamp(img, radius, _line(14, 20, 12) + _line(15, 20, 12))
    _stamp(img, radius, _line(0, 60, 9) + _line(1, 66, 3))
    _stamp(img, radius, [(r, 0) for r in range(50, 62)])
    _stamp(img, radius, [(50 + r, 20 + c) for r, c in under])
    _stamp(img, radius, [(50 + r, 40 + c) for r, c in exact])
    _stamp(img, radius, _line(60, 70, 14) + _line(61, 70, 14))
    _stamp(img, radius, _line(61 + step, 83 + step, 14) + _line(62 + step, 83 + step, 14))
    img[70:72, 100:103] = 9                             # specks below the disc
    img[5, 110] = 1
    img[30:45, 100] = 200
    return dict(img=img, sel_radius=radius, min_size=min_size)


def _eggs_default():
    """the reference's constants on three eggs, one thinner than the disc of 25 and one joined to a neighbour by a thin bridge"""
    img = np.zeros((150, 200), dtype=np.uint8)
    _paint(img, 255, 60., 55., 42, 38, 0.3)
    _paint(img, 255, 95., 150., 45, 36, 1.2)
    _paint(img, 255, 20., 150., 14, 30, 0.)
    img[70:74, 80:130] = 255
    return dict(img=img, sel_radius=25, min_size=64)


CORRECT_CASES = {'correct_r1': lambda: _correct(1), 'correct_r2': lambda: _correct(2), 'eggs_default': _eggs_default}


def level_case(name):
    return (LEVEL_CASES[name] if name in LEVEL_CASES else HOST_ONLY[name])()


def correct_case(name):
    return CORRECT_CASES[name]()


def load_golden():
    return np.load(GOLDEN, allow_pickle=False)


def same(got, want):
    return got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()


# ------------------------------------------------------------------------------------------------
# edge cases from plain arrays (tests/test_gpu_center_annotation_edges.py and the CPU twins in
# tests/test_center_annotation_reference_host.py)
# ------------------------------------------------------------------------------------------------

#: the row pass searches outward in windows of 256 columns, a workgroup owns 256 columns of a row
WINDOW = 256
#: the distances along a row at which the search hands over from one window to the next
HANDOVER = (255, 256, 257, 511, 512, 513)
ROW_W = 780                                             # four workgroups per row, the last one of 12 columns


def _egg_but(shape, holes, value=0):
    """one egg over the whole map but for the pixels ``holes``"""
    seg = np.full(shape, 1, dtype=np.int32)
    for r, c in holes:
        seg[r, c] = value
    return dict(seg=seg, levels=LEVELS)


def _row_case(shape, holes, value=0):
    """probes: the pixels (r, c, dc, side, dr) at a hand-over distance dc along the row from a hole that is their nearest foreign
    pixel, dr rows off it: their squared distance is dc^2 + dr^2; side: where the hole lies"""
    case = _egg_but(shape, holes, value)
    probes = []
    for hr, hc in holes:
        for dc in HANDOVER:
            for c, side in ((hc + dc, 'left'), (hc - dc, 'right')):
                for r in range(shape[0]):
                    nearest = min((r - qr) ** 2 + (c - qc) ** 2 for qr, qc in holes)
                    if 0 <= c < shape[1] and nearest == dc * dc + (r - hr) ** 2:
                        probes.append((r, c, dc, side, abs(r - hr)))
    case['probes'] = probes
    return case


def _none_columns():
    """columns 100 .. 299 hold a foreign pixel in row 0 (g is a number there), all other columns hold one label from top to bottom
    (g == NONE): the search of a pixel of row 3 runs over both kinds"""
    case = _egg_but((4, 600), [(0, c) for c in range(100, 300)])
    case['probes'] = [(3, 100 - dc, dc, 'right', 3) for dc in (1, 99)] + [(3, 299 + dc, dc, 'left', 3) for dc in (255, 256, 257)]
    return case


def _alternate_columns():
    seg = np.zeros((3, 515), dtype=np.int32)
    seg[:, 0::2], seg[:, 1::2] = 1, 2
    return dict(seg=seg, levels=LEVELS, probes=[])


ROW_CASES = {
    'left_end': lambda: _row_case((3, ROW_W), [(1, 0)]),                 # the foreign pixel on the left only
    'right_end': lambda: _row_case((3, ROW_W), [(1, ROW_W - 1)]),        # on the right only
    'at_266': lambda: _row_case((3, ROW_W), [(1, 266)]),                 # probes in the first (right) and in the last workgroup (left)
    'at_513': lambda: _row_case((4, ROW_W), [(0, 513)]),                 # probes at columns 0, 1, 2 and 256 .. 258 (right)
    'at_513_egg': lambda: _row_case((4, ROW_W), [(3, 513)], value=2),    # the foreign pixel is another egg
    'two_corners': lambda: _row_case((5, ROW_W), [(0, 0), (4, ROW_W - 1)]),
    'none_columns': _none_columns,
    'alternate_columns': _alternate_columns,
    'one_row': lambda: _row_case((1, ROW_W), [(0, 513)]),
    'one_row_left_end': lambda: _row_case((1, ROW_W), [(0, 0)]),
    'one_column': lambda: dict(seg=np.array([[1], [1], [0], [1], [2]], dtype=np.int32), levels=LEVELS, probes=[]),
    'no_foreign_3x257': lambda: dict(seg=np.full((3, 257), 1, dtype=np.int32), levels=LEVELS, probes=[]),
}


def row_case(name):
    return ROW_CASES[name]()


def run_level_maps():
    """the run-rule maps of tests/cut_objects_cases.py as label maps of ``center_levels``: ((width, layout), int32 map of the values
    0 .. 3)"""
    import cut_objects_cases
    for key in cut_objects_cases.RUN_MAPS:
        yield key, cut_objects_cases.run_map(*key)


def brute_force_d2(seg, block=8):
    """the squared distance of every pixel to the nearest pixel of another value, by the integer minimum over ALL such pixels, in
    blocks of rows; a map of one value has no such pixel: None"""
    height, width = seg.shape
    rows, cols = (a.ravel().astype(np.int64) for a in np.indices(seg.shape))
    flat = seg.ravel()
    out = np.zeros(seg.size, dtype=np.int64)
    if (flat == flat[0]).all():
        return None
    for start in range(0, seg.size, block * width):
        here = slice(start, min(seg.size, start + block * width))
        d2 = (rows[here, None] - rows[None, :]) ** 2 + (cols[here, None] - cols[None, :]) ** 2
        d2[flat[here, None] == flat[None, :]] = np.iinfo(np.int64).max
        out[here] = d2.min(axis=1)
    return out.reshape(seg.shape)


def edt_d2(seg):
    """the same by ``scipy.ndimage.distance_transform_edt(seg == value)``, squared and rounded, value by value"""
    from scipy import ndimage
    out = np.zeros(seg.shape, dtype=np.int64)
    for value in np.unique(seg):
        mask = seg == value
        out[mask] = np.rint(ndimage.distance_transform_edt(mask) ** 2).astype(np.int64)[mask]
    return out


def expected_d2(seg, max_label):
    """what ``imsegm_debug_center_distances`` answers: the brute-force minimum for the labels 1 .. max_label, 0 for every other pixel;
    (y + 1)^2 + x^2 on a map of one value (the rule of the case ``whole_map``)"""
    d2 = brute_force_d2(seg)
    if d2 is None:
        rows, cols = np.indices(seg.shape).astype(np.int64)
        d2 = (rows + 1) ** 2 + cols ** 2
    return np.where((seg >= 1) & (seg <= max_label), d2, 0).astype(np.uint32)


def expected_words(seg, d2, max_label):
    """max2 and (count, row sum, column sum) of the labels 1 .. max_label as Python integers from int64 numpy sums"""
    rows, cols = np.indices(seg.shape).astype(np.int64)
    max2, sums = [], []
    for label in range(1, max_label + 1):
        mask = seg == label
        max2.append(int(d2[mask].max()) if mask.any() else 0)
        sums.append([int(mask.sum()), int(rows[mask].sum()), int(cols[mask].sum())])
    return max2, sums


CORRECT_W = 320


def _correct_edge(radius):
    """width 320, two workgroups per row.  Without an opening (radius 0) the pixel counts are what is painted: a single row of exactly
    ``min_size`` pixels across columns 255 / 256 (kept), one of ``min_size - 1`` (removed), a blob across the boundary, and two blobs
    that touch only diagonally at (r, 255) / (r + 1, 256).  With radius 1 everything is painted three rows thick with the disc."""
    min_size = 12 if radius == 0 else 29
    img = np.zeros((22, CORRECT_W), dtype=np.uint8)
    if radius == 0:
        img[1, 250:262] = 255                           # 12 pixels, 6 in either workgroup
        img[3, 251:262] = 255                           # 11 pixels
        img[5:8, 240:275] = 7                           # a blob across the boundary
        img[9:11, 244:256] = 255                        # ends at column 255 ...
        img[11:13, 256:268] = 255                       # ... and begins at (11, 256): a diagonal across the boundary
        img[15, 300:320] = 1                            # a run that ends with the row
        img[17:19, 0:9] = 1                             # 18 pixels at the left border
    else:
        _stamp(img, 1, _line(2, 250, 9))                # 3 * 9 + 2 = 29 pixels in columns 249 .. 259
        _stamp(img, 1, _line(6, 251, 7))                # 23 pixels
        _stamp(img, 1, _line(10, 245, 10) + _line(11, 245, 10))          # its last pixels are (10, 255) and (11, 255) ...
        _stamp(img, 1, _line(12, 257, 10) + _line(13, 257, 10))          # ... its first ones (12, 256) and (13, 256)
        _stamp(img, 1, _line(18, 310, 9))               # ends with the row
        img[20, 100:140] = 255                          # one row: the opening removes it
    return dict(img=img, sel_radius=radius, min_size=min_size)


CORRECT_EDGE_CASES = {'edge_r0': lambda: _correct_edge(0), 'edge_r1': lambda: _correct_edge(1)}


def correct_edge_case(name):
    return CORRECT_EDGE_CASES[name]()


def scipy_correct(img, sel_radius, min_size):
    """``correct_segm`` restated with scipy's own parts: threshold, ``binary_opening`` with the disc, 4-connected labels with
    ``bincount >= min_size``, labels with the full 3 x 3 structure (numbered by first pixel in raster order)"""
    from scipy import ndimage
    seg = img > 0
    if sel_radius > 0:
        seg = ndimage.binary_opening(seg, structure=_disc(sel_radius))
    parts, _ = ndimage.label(seg)
    seg = seg & (np.bincount(parts.ravel()) >= min_size)[parts]
    seg_lb, _ = ndimage.label(seg, structure=np.ones((3, 3), dtype=bool), output=np.int32)
    return seg, seg_lb
