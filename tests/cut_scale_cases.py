"""Inputs of the cut-and-scale tests (tests/test_cut_scale_reference_host.py, tests/test_gpu_cut_scale.py) and of their golden
generator (tests/golden/make_golden_cut_scale.py).  Everything is generated from seeds with numpy's legacy ``RandomState``; the
golden file pins the CRC of every input."""
import zlib

import numpy as np

#: resize cases against scikit-image 0.18.3: name -> (H, W, channels (0: no channel axis), h, w)
RESIZE_CASES = {
    'shrink_rgb': (57, 83, 3, 20, 31),
    'shrink_gray': (64, 48, 0, 21, 17),
    'shrink_c1': (45, 70, 1, 15, 20),
    'shrink_strong_rgb': (150, 120, 3, 13, 11),
    'enlarge_rgb': (17, 23, 3, 40, 52),
    'enlarge_gray': (12, 9, 0, 30, 31),
    'mixed_rgb': (60, 20, 3, 25, 45),
    'mixed_gray': (15, 66, 0, 33, 20),
    'same_rgb': (40, 40, 3, 40, 40),
    'loses_one_gray': (64, 48, 0, 21, 17),
}
#: a given background value: 62 comes out of this case's blur as 61 (the fp64 sum of 62 times the weights ends below 62)
BACKGROUNDS = {'loses_one_gray': 62}
#: the cases whose exported bytes the reference itself does not reproduce (ISSUE: every stretched value sits on an integer)
SAME_SIZE_CASES = ('same_rgb', )

#: full chain cases against the reference's own extract_ellipse_object: name -> (H, W, channels, ellipses, norm_size)
#: ellipse rows are xc, yc, a, b, theta: centre on the first and second image axis, the two radii, the angle
CHAIN_CASES = {
    'chain_rgb': (96, 128, 3, [(40.3, 50.8, 30.2, 17.9, 0.31), (55.1, 80.2, 25.7, 14.2, -0.83), (50.6, 66.0, 12.4, 21.3, 1.93)], (16, 27)),
    'chain_gray': (80, 100, 0, [(33.9, 41.2, 22.5, 13.1, 0.57), (47.0, 63.4, 18.8, 9.6, 2.41)], (30, 48)),
    'chain_border': (96, 128, 3, [(14.2, 31.5, 27.4, 15.3, 0.44), (70.2, 110.9, 31.0, 12.8, -0.37)], (14, 28)),
}


def crc(arr):
    return zlib.crc32(np.ascontiguousarray(arr).tobytes())


def _seed(name):
    return zlib.crc32(name.encode('ascii')) % (2 ** 31)


def textured_image(name, height, width, channels):
    """a textured ellipse on a constant background, uint8 [H, W] (channels 0) or [H, W, channels]"""
    rng = np.random.RandomState(_seed(name))
    planes = max(channels, 1)
    rows, cols = np.mgrid[0:height, 0:width].astype(np.float64)
    inside = ((rows - height / 2.) / (0.45 * height)) ** 2 + ((cols - width / 2.) / (0.4 * width)) ** 2 < 1
    img = np.empty((height, width, planes), dtype=np.uint8)
    for ch in range(planes):
        wave = 120 + 70 * np.sin(rows / (2.5 + ch)) * np.cos(cols / (3.5 - 0.5 * ch)) + rng.randint(-40, 41, size=(height, width))
        background = BACKGROUNDS.get(name, rng.randint(5, 60))
        img[:, :, ch] = np.where(inside, np.clip(wave, 0, 255), background).astype(np.uint8)
    return img if channels else img[:, :, 0]


def resize_case(name):
    height, width, channels, h, w = RESIZE_CASES[name]
    return textured_image(name, height, width, channels), (h, w)


def scene_image(name, height, width, channels):
    """an image with texture everywhere and a mostly dark border, so that the border colour differs from the eggs"""
    rng = np.random.RandomState(_seed(name))
    planes = max(channels, 1)
    rows, cols = np.mgrid[0:height, 0:width].astype(np.float64)
    img = np.empty((height, width, planes), dtype=np.uint8)
    for ch in range(planes):
        wave = 110 + 60 * np.sin(rows / (4. + ch)) * np.cos(cols / (5. - ch)) + rng.randint(-50, 51, size=(height, width))
        img[:, :, ch] = np.clip(wave, 0, 255).astype(np.uint8)
        img[:2, :, ch] = img[-2:, :, ch] = 10 + ch
    return img if channels else img[:, :, 0]


def chain_case(name):
    height, width, channels, ellipses, norm_size = CHAIN_CASES[name]
    return scene_image(name, height, width, channels), [tuple(ell) for ell in ellipses], norm_size
