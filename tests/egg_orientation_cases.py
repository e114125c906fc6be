"""Case stacks of the egg orientation tests (tests/test_egg_orientation_reference_host.py, tests/test_gpu_egg_orientation.py) and
of the generator tests/golden/make_egg_orientation_golden.py.  Seeded and small: the largest stack holds about 4 MB.

A case is ``(images, template)``: a list of uint8 arrays [h_i, w_i, C] and a given template [h, w], or None for the median of the
stack.  The cases cover the counter width and even / odd N of the median (N = 1, 2, 3, 4, 255, 256, 257, 65 535), equal planes,
only 0 and 255, three grey levels (many ties), pixel counts around a wave and beyond a workgroup with an odd count for the turn
(1, 63, 64, 65, 257, 1025), widths 1 to 4 (a third of 0 and of 1 columns), one row, 1, 3 and 4 channels, ragged sizes, a ramp
stack with half of the images turned, point-symmetric images (the exact tie), constant images and a constant template (deviation
0), images whose non-minimum pixels are all equal, a given template with .5 values and one that is no half-integer."""
import os
import zlib

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'egg_orientation.npz')


def _rng(name):
    return np.random.RandomState(zlib.crc32(name.encode()) & 0x7fffffff)


def _random_stack(name, n, h, w, c=3):
    rng = _rng(name)
    return [rng.randint(0, 256, (h, w, c)).astype(np.uint8) for _ in range(n)], None


def _count_case(n):
    def make():
        if n < 1000:
            return _random_stack('n%d' % n, n, 8, 8)
        # 61 distinct planes in turn; pixel (0, 0) holds one value in all of them: one counter reaches N
        rng = _rng('n%d' % n)
        base = rng.randint(0, 256, (61, 8, 8, 1)).astype(np.uint8)
        base[:, 0, 0] = 200
        base[:, 0, 1] = np.arange(61)[:, None] % 2 * 255
        return [base[i % 61] for i in range(n)], None
    return make


def _size_case(h, w, n=9, c=3):
    return lambda: _random_stack('size_%dx%d' % (h, w), n, h, w, c)


def equal_planes():
    img = _rng('equal_planes').randint(0, 256, (9, 12, 3)).astype(np.uint8)
    return [img.copy() for _ in range(5)], None


def two_values():
    rng = _rng('two_values')
    return [(rng.randint(0, 2, (10, 13, 3)) * 255).astype(np.uint8) for _ in range(7)], None


def three_levels():
    rng = _rng('three_levels')
    return [(rng.randint(1, 4, (6, 7, 3)) * 60).astype(np.uint8) for _ in range(24)], None


def ragged():
    rng = _rng('ragged')
    sizes = [(14, 19), (12, 22), (15, 17), (12, 17), (20, 20), (13, 18)]
    return [rng.randint(0, 256, (h, w, 3)).astype(np.uint8) for h, w in sizes], None


def ramp_half_turned():
    """bright on the right, dark on the left, with noise; every second image is turned: 6 of 13, so that the median keeps the
    orientation of the other 7"""
    rng = _rng('ramp_half_turned')
    ramp = np.linspace(20, 220, 24)[None, :, None] + np.linspace(0, 20, 16)[:, None, None]
    images = []
    for i in range(13):
        img = np.clip(ramp + rng.randint(-15, 16, (16, 24, 3)), 0, 255).astype(np.uint8)
        images.append(np.ascontiguousarray(img[::-1, ::-1]) if i % 2 else img)
    return images, None


def _symmetric(rng, h, w, c=3):
    img = rng.randint(0, 256, (h, w, c)).astype(np.uint8)
    flat = img.reshape(h * w, c)
    half = (h * w) // 2
    flat[h * w - half:] = flat[:half][::-1]
    return flat.reshape(h, w, c)


def point_symmetric():
    """images 3 and 11 of 20 equal their own turn: P == Pf exactly"""
    rng = _rng('point_symmetric')
    images = [rng.randint(0, 256, (9, 11, 3)).astype(np.uint8) for _ in range(20)]
    images[3], images[11] = _symmetric(rng, 9, 11), _symmetric(rng, 9, 11)
    return images, None


def constant_image():
    """images 2 and 9 of 20 are constant: deviation 0, and no pixel above the minimum"""
    rng = _rng('constant_image')
    images = [rng.randint(0, 256, (8, 10, 3)).astype(np.uint8) for _ in range(20)]
    images[2], images[9] = np.full((8, 10, 3), 77, dtype=np.uint8), np.zeros((8, 10, 3), dtype=np.uint8)
    return images, None


def constant_template():
    images, _ = _random_stack('constant_template', 5, 7, 9)
    return images, np.full((7, 9), 100.)


def flat_above_minimum():
    """two values per image: the non-minimum pixels equal their mean, g is all False"""
    rng = _rng('flat_above_minimum')
    images = []
    for i in range(10):
        low, high = 10 + i, 100 + 7 * i
        images.append(np.where(rng.rand(8, 12, 1) < 0.4, low, high).astype(np.uint8).repeat(3, axis=2))
    return images, None


def given_half_template():
    images, _ = _random_stack('given_half_template', 8, 10, 12)
    other, _ = _random_stack('given_half_template_source', 6, 10, 12)
    template = np.median([img[:, :, 0] for img in other], axis=0)
    assert np.any(template != np.floor(template))
    return images, template


def given_other_template():
    """a mean, not a median: 2 * template is no whole number, the host statements run"""
    images, _ = _random_stack('given_other_template', 8, 10, 12)
    return images, np.mean([img[:, :, 0] for img in images[:3]], axis=0)


CASES = {
    'n1': _count_case(1), 'n2': _count_case(2), 'n3': _count_case(3), 'n4': _count_case(4), 'n255': _count_case(255),
    'n256': _count_case(256), 'n257': _count_case(257), 'n65535': _count_case(65535),
    'equal_planes': equal_planes, 'two_values': two_values, 'three_levels': three_levels,
    'px1': _size_case(1, 1), 'px63': _size_case(7, 9), 'px64': _size_case(8, 8), 'px65': _size_case(5, 13),
    'px257_w1': _size_case(257, 1), 'px1025': _size_case(25, 41),
    'w2': _size_case(6, 2), 'w3': _size_case(6, 3), 'w4': _size_case(6, 4), 'h1': _size_case(1, 30),
    'c1': _size_case(9, 10, c=1), 'c4': _size_case(9, 11, c=4),
    'ragged': ragged, 'ramp_half_turned': ramp_half_turned, 'point_symmetric': point_symmetric, 'constant_image': constant_image,
    'constant_template': constant_template, 'flat_above_minimum': flat_above_minimum, 'given_half_template': given_half_template,
    'given_other_template': given_other_template,
}
#: the case whose template the device does not take
HOST_ONLY = ('given_other_template', )

_MADE = {}


def case(name):
    """``(images, template)`` of a case, built once; nobody writes into them"""
    if name not in _MADE:
        images, template = CASES[name]()
        for img in images:
            img.setflags(write=False)
        _MADE[name] = images, template
    return _MADE[name]


def cropped(name):
    """``(stack uint8 [N, h, w, C], template or None)``: the images of a case cropped as the reference crops them -- to the given
    template, else to the per-axis minimum of the sizes"""
    images, template = case(name)
    h, w = template.shape if template is not None else np.min([img.shape[:2] for img in images], axis=0)
    return np.stack([img[:h, :w] for img in images]), template


def crc(name):
    images, template = case(name)
    value = 0
    for img in images:
        value = zlib.crc32(np.ascontiguousarray(img).tobytes(), zlib.crc32(repr(img.shape).encode(), value))
    if template is not None:
        value = zlib.crc32(np.ascontiguousarray(template, dtype=np.float64).tobytes(), value)
    return value & 0xffffffff


def load_golden():
    with np.load(GOLDEN) as data:
        return {key: data[key] for key in data.files}


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
