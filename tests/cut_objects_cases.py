"""Seeded inputs of the cut_object / cut_objects tests (tests/test_cut_objects_reference_host.py, tests/test_gpu_cut_objects.py) and of
tests/golden/make_golden_cut_objects.py, which runs the reference's ``cut_object`` on them and picks the seeds.  Ellipses are painted
with the package's own ``ellipse_pixels_host``; no scikit-image is needed.

A case is ``case(name, seed) -> dict(img, segm, labels, padding, use_mask, bg_color, allow_rotate)``: the reference is called once
per label with the boolean mask ``segm == label``.  ``kind`` of ``CASES``: 'fixed' inputs do not depend on the seed beyond the image
noise; 'seeded' ones are re-seeded by the generator until the reference's result is stable (see the generator)."""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden', 'cut_objects.npz')


def _noise(rng, shape, channels):
    return rng.randint(0, 256, tuple(shape) + ((channels, ) if channels else ())).astype(np.uint8)


def _paint(segm, label, r, c, r_radius, c_radius, orientation):
    from pyimsegm_amd.ellipse_fitting import ellipse_pixels_host
    rr, cc = ellipse_pixels_host(r, c, r_radius, c_radius, orientation, segm.shape)
    segm[rr, cc] = label


def _three_ellipses(rng, shape=(61, 83)):
    segm = np.zeros(shape, dtype=np.int32)
    for label, (r, c) in enumerate(((17, 20), (40, 44), (20, 64)), 1):
        _paint(segm, label, r + rng.uniform(-2, 2), c + rng.uniform(-2, 2), rng.uniform(9, 13), rng.uniform(4, 6.5),
               rng.uniform(0.15, np.pi - 0.15))
    return segm


def _ellipses(channels, padding, use_mask, allow_rotate=True, bg_color=None):
    def make(seed):
        rng = np.random.RandomState(seed)
        segm = _three_ellipses(rng)
        return dict(img=_noise(rng, segm.shape, channels), segm=segm, labels=[1, 2, 3], padding=padding, use_mask=use_mask,
                    bg_color=bg_color, allow_rotate=allow_rotate)
    return make


def _doctest(kwargs, dtype):
    def make(seed):
        img = np.ones((10, 20), dtype=dtype)
        img[3:7, 4:16] = 2
        segm = np.zeros((10, 20), dtype=np.int32)
        segm[4:6, 5:15] = 1
        return dict(img=img, segm=segm, labels=[1], padding=2, use_mask=kwargs.get('use_mask', False), bg_color=None,
                    allow_rotate=kwargs.get('allow_rotate', True))
    return make


def _border(seed):
    """ellipses that leave the map on three sides: the shift brings zeros in and the crops reach beyond the turned frame"""
    rng = np.random.RandomState(seed)
    segm = np.zeros((61, 83), dtype=np.int32)
    _paint(segm, 1, 3 + rng.uniform(-1, 1), 30, 11, 5, rng.uniform(0.3, 1.2))
    _paint(segm, 2, 40, 80 + rng.uniform(-1, 1), 12, 6, rng.uniform(1.9, 2.8))
    _paint(segm, 3, 57 + rng.uniform(-1, 1), 4, 10, 4.5, rng.uniform(0.3, 1.2))
    return dict(img=_noise(rng, segm.shape, 3), segm=segm, labels=[1, 2, 3], padding=3, use_mask=False, bg_color=None, allow_rotate=True)


def _two_pieces(seed):
    """one label in two pieces (one region for regionprops), beside a second label"""
    rng = np.random.RandomState(seed)
    segm = np.zeros((61, 83), dtype=np.int32)
    _paint(segm, 5, 15, 18, 8, 4, rng.uniform(0.2, 1.3))
    _paint(segm, 5, 44, 60, 9, 5, rng.uniform(1.8, 2.9))
    _paint(segm, 2, 45, 20, 7, 4, rng.uniform(0.2, 2.9))
    return dict(img=_noise(rng, segm.shape, 3), segm=segm, labels=[2, 5], padding=2, use_mask=True, bg_color=None, allow_rotate=True)


def _axis_aligned(seed):
    """a level and an upright rectangle and a single row, centroids exact in binary: angles of exactly 0 and +-90 degrees"""
    rng = np.random.RandomState(seed)
    segm = np.zeros((40, 50), dtype=np.int32)
    segm[5:9, 6:26] = 1
    segm[14:36, 34:40] = 2
    segm[30, 4:21] = 3
    return dict(img=_noise(rng, segm.shape, 3), segm=segm, labels=[1, 2, 3], padding=1, use_mask=True, bg_color=(7, 8, 9), allow_rotate=True)


def _one_pixel(seed):
    rng = np.random.RandomState(seed)
    segm = np.zeros((21, 30), dtype=np.int32)
    segm[13, 22] = 4
    segm[0, 0] = 9
    return dict(img=_noise(rng, segm.shape, 0), segm=segm, labels=[4, 9], padding=2, use_mask=False, bg_color=None, allow_rotate=False)


def _sparse33(seed):
    """33 small tilted ellipses on a grid, label values with gaps and above 1000"""
    rng = np.random.RandomState(seed)
    segm = np.zeros((97, 155), dtype=np.int32)          # (odd: the canvas centre is no rounding tie)
    labels = sorted(rng.choice(np.arange(3, 5000), 33, replace=False).tolist())
    for k, label in enumerate(labels):
        r, c = 8 + 16 * (k // 7), 11 + 22 * (k % 7)
        _paint(segm, label, r + rng.uniform(-1, 1), c + rng.uniform(-1, 1), rng.uniform(7, 9.5), rng.uniform(2.5, 4.5),
               rng.uniform(0.15, np.pi - 0.15))
    return dict(img=_noise(rng, segm.shape, 3), segm=segm, labels=labels, padding=1, use_mask=False, bg_color=None, allow_rotate=True)


def _large(seed):
    """130 x 70: the object spans more than one tile of every kernel in both directions"""
    rng = np.random.RandomState(seed)
    segm = np.zeros((130, 70), dtype=np.int32)
    _paint(segm, 1, 64 + rng.uniform(-2, 2), 35 + rng.uniform(-2, 2), 55, 24, rng.uniform(0.2, 0.6))
    return dict(img=_noise(rng, segm.shape, 3), segm=segm, labels=[1], padding=4, use_mask=True, bg_color=None, allow_rotate=True)


#: name -> (kind, builder)
CASES = {
    'doctest_u8': ('fixed', _doctest({}, np.uint8)),
    'doctest_u8_mask': ('fixed', _doctest({'use_mask': True, 'allow_rotate': False}, np.uint8)),
    'rgb_p0': ('seeded', _ellipses(3, 0, False)),
    'rgb_p4_mask': ('seeded', _ellipses(3, 4, True)),
    'gray_p0_mask': ('seeded', _ellipses(0, 0, True)),
    'gray_p4': ('seeded', _ellipses(0, 4, False)),
    'rgba_p4_mask_bg': ('seeded', _ellipses(4, 4, True, bg_color=(1, 2, 3, 4))),
    'rgb_p60_mask': ('seeded', _ellipses(3, 60, True)),          # the crop is the whole canvas, corners outside the turned frame included
    'no_rotate': ('seeded', _ellipses(3, 4, True, allow_rotate=False)),
    'border': ('seeded', _border),
    'two_pieces': ('seeded', _two_pieces),
    'axis_aligned': ('fixed', _axis_aligned),
    'one_pixel': ('fixed', _one_pixel),
    'sparse33': ('seeded', _sparse33),
    'large': ('seeded', _large),
}

#: cases whose MASK is handed over as int64 (host statement only): the doctest's own dtypes, and a turned object under use_mask
INT_MASK_CASES = {
    'doctest_int': ('fixed', _doctest({}, np.int64)),
    'doctest_int_mask': ('fixed', _doctest({'use_mask': True, 'allow_rotate': False}, np.int64)),
    'int_mask_turned': ('seeded', _ellipses(3, 60, True)),
}


def case(name, seed):
    table = CASES if name in CASES else INT_MASK_CASES
    return table[name][1](int(seed))


def masks_of(name, inputs):
    """the masks the reference is called with, one per label: boolean, or int64 for the INT_MASK_CASES"""
    for label in inputs['labels']:
        mask = inputs['segm'] == label
        yield label, (mask.astype(np.int64) if name in INT_MASK_CASES else mask)


def load_golden():
    return np.load(GOLDEN, allow_pickle=False)


def golden_crops(golden, name, count):
    return [golden['%s_crop%d' % (name, k)] for k in range(count)]
