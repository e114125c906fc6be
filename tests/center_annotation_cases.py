"""Inputs of the centre-annotation tests (tests/test_center_annotation_reference_host.py, tests/test_gpu_center_annotation.py) and
of tests/golden/make_golden_center_annotation.py, which runs the reference's ``run_create_annotation`` on them.  Ellipses are painted
with the package's own ``ellipse_pixels_host``; no scikit-image is needed.  Every case is built at the smallest shape that crosses
the rule it is named for; the tests assert that it does.

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
