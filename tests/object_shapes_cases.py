"""Seeded annotated maps for ``compute_object_shapes`` (tests/golden/make_golden_object_shapes.py records the reference's answers
on them, tests/test_object_shapes_reference_host.py compares) and the ray tables the model functions are recorded on.  Small on
purpose: the reference masks the whole map once per object."""
import numpy as np

#: name -> (height, width, ray_step)
CASES = {
    'binary': (48, 56, 45),           # a 0 / 1 map: the objects are the components of ndimage.label
    'binary_float': (40, 44, 30),     # the same kind as float64 with the values 0. and 3.
    'labels': (52, 60, 20),           # one value per object, 0 behind them
    'border': (44, 50, 15),           # objects cut by the border of the map: rays of -1
    'offset': (40, 48, 40),           # the values -3 (the smallest: no object), 5 and 1000
    'pieces': (56, 64, 24),           # an object of two far pieces, its centre between them
}

#: the ray lists of the reference's doctests (imsegm/region_growing.py:372-373)
DOCTEST_RAYS = [[9, 4, 9], [4, 9, 7], [9, 7, 11], [10, 8, 10], [9, 11, 8], [4, 8, 5], [8, 10, 6], [9, 7, 11]]


def _disc(shape, centre, radii):
    rows, cols = np.indices(shape)
    return ((rows - centre[0]) / float(radii[0]))**2 + ((cols - centre[1]) / float(radii[1]))**2 <= 1.


def case(name, seed):
    """(map, ray_step) of a case"""
    height, width, ray_step = CASES[name]
    rng = np.random.RandomState(seed)
    shape = (height, width)
    img = np.zeros(shape, dtype=np.int64)

    def blob():
        radii = rng.randint(4, 9, 2)
        margin = radii + 2
        centre = [rng.randint(margin[0], height - margin[0]), rng.randint(margin[1], width - margin[1])]
        return _disc(shape, centre, radii)

    if name in ('binary', 'binary_float'):
        for _ in range(4):
            img[blob()] = 1
        return (img * 3.) if name == 'binary_float' else img, ray_step
    if name == 'labels':
        for value in (1, 2, 4, 7):
            img[blob()] = value
    elif name == 'border':
        spots = [(0, rng.randint(8, width - 8)), (height - 1, rng.randint(8, width - 8)), (rng.randint(8, height - 8), 0),
                 (rng.randint(8, height - 8), width - 1)]
        for value, spot in enumerate(spots, 1):
            img[_disc(shape, spot, rng.randint(4, 8, 2))] = value
        img[blob()] = 6
    elif name == 'offset':
        img[:] = -3
        img[blob()] = 5
        img[blob()] = 1000
    elif name == 'pieces':
        img[_disc(shape, (12, 14), (6, 7))] = 2
        img[_disc(shape, (44, 50), (6, 5))] = 2
        img[blob()] = 1
        img[blob()] = 3
    return img, ray_step


def ray_table(seed, count=24, angles=6):
    """integer ray lengths of ``count`` objects around two shapes"""
    rng = np.random.RandomState(100 + seed)
    base = np.array([rng.randint(6, 20, angles), rng.randint(10, 30, angles)])
    return (base[rng.randint(0, 2, count)] + rng.randint(-2, 3, (count, angles))).tolist()


def cumulative_inputs(seed):
    """(means, stds, weights, max_dist) for ``compute_cumulative_distrib``"""
    rng = np.random.RandomState(200 + seed)
    means, stds = rng.uniform(5, 25, (3, 5)), rng.uniform(0.5, 4, (3, 5))
    weights = rng.dirichlet(np.ones(3))
    return means, stds, weights, float(np.max(means + 2 * stds))


#: maps wider than one workgroup of 256 pixels, so that a row is more than one chunk of the run labelling
SEAM_SHAPES = ((9, 257), (12, 300))


def seam_map(shape, multi):
    """three objects around the seam between the pixels 255 and 256 of a row: a run across it, a U whose two bars (columns 252 and
    256) meet only in its bottom row -- the union across the seam closes last -- and a single pixel at column 256; one value
    (``multi`` False) or the values 2, 3, 5"""
    height, width = shape
    img = np.zeros(shape, dtype=np.int32)
    img[0, 240:min(width, 290)] = 2
    img[2:6, 252] = 3
    img[2:6, 256] = 3
    img[5, 252:257] = 3
    img[7, 256] = 5
    return img if multi else (img != 0).astype(np.int32)
