"""Plain-numpy statement of the centre-candidate point descriptors, written from their definitions, and the cases the tests of
``pyimsegm_amd.descriptors.compute_label_histograms_positions`` / ``compute_ray_features_positions`` share.

Definitions:

* disc of radius r: the pixels (dy, dx) of the (2r+1) x (2r+1) grid with dy^2 + dx^2 <= r^2;
* a box of b pixels centred at position p covers [p - floor(b / 2), p + ceil(b / 2)), clipped to [0, size);
* the label histogram under an element counts, per label 0 <= l < nb_labels, the window's pixels with that label where the
  element is 1; the size of the element is the number of its ones inside the map, whatever the labels;
* ring d = (hist_d - hist_{d-1}) / (size_d - size_{d-1}), with hist_{-1} = 0 and size_{-1} = 0; a size that does not grow and a
  count that shrinks are errors;
* the probability variant sums the layers' values instead of counting (here in ``np.longdouble``, with the sum of magnitudes);
* smoothing along the angle: correlation with the normalised Gaussian exp(-x^2 / (2 sigma^2)), |x| <= int(4 sigma + 0.5), on
  the line continued by reflection (d c b a | a b c d | d c b a), float64, centre tap first, then the pairs from the farthest to
  the nearest, rounded to float32.
"""
import numpy as np

# ---- recorded results of the reference's doctests (imsegm/descriptors.py, scikit-image 0.18.3) -----------------------------
DOCTEST_RADII = [1, 2, 4]
DOCTEST_POINTS = [[3, 3], [4, 4], [2, 7], [6, 6]]
DOCTEST_LABEL_TABLE = np.array([[0., 0.8, 0.2, 0.12, 0.62, 0.25, 0.44, 0.41, 0.15],
                                [0., 0.2, 0.8, 0., 0.62, 0.38, 0.22, 0.75, 0.03],
                                [0.2, 0.8, 0., 0.5, 0.5, 0., 0.46, 0.33, 0.21],
                                [0., 0.8, 0.2, 0.12, 0.62, 0.25, 0.44, 0.41, 0.15]])
DOCTEST_LAYER_TABLE = np.array([[1., 0.2, 1., 0.25, 1., 0.15],
                                [1., 0.8, 1., 0.38, 1., 0.03],
                                [1., 0., 1., 0., 1., 0.21],
                                [1., 0.2, 1., 0.25, 1., 0.15]])
DOCTEST_NAMES = ['hist-d_1-lb_0', 'hist-d_1-lb_1', 'hist-d_1-lb_2', 'hist-d_2-lb_0', 'hist-d_2-lb_1', 'hist-d_2-lb_2',
                 'hist-d_4-lb_0', 'hist-d_4-lb_1', 'hist-d_4-lb_2']
SHIFT_VECTOR = np.array([43, 46, 44, 39, 28, 18, 12, 10, 9, 12, 22, 28])
SHIFT_RESULT = np.array([46, 44, 39, 28, 18, 12, 10, 9, 12, 22, 28, 43])
DEFAULT_RADII = (10, 20, 30, 40, 50)


def doctest_label_map():
    segm = np.zeros((10, 10), dtype=int)
    segm[1:9, 2:8] = 1
    segm[3:7, 4:6] = 2
    return segm


def doctest_layers():
    segm = np.zeros((10, 10, 2), dtype=int)
    segm[3:7, 4:6, 1] = 1
    segm[:, :, 0] = 1 - segm[:, :, 0]
    return segm


# ---- the definitions ---------------------------------------------------------------------------------------------------------
def disc(radius):
    grid = np.arange(-radius, radius + 1)
    return (grid[:, None] ** 2 + grid[None, :] ** 2 <= radius ** 2).astype(np.uint8)


def clipped(segm, element, position):
    """the part of ``segm`` (first two axes) under ``element`` centred at ``position`` and the matching part of the element"""
    window, part = [], []
    for size, box, pos in zip(segm.shape[:2], element.shape, position):
        first = int(pos) - box // 2
        lo, hi = max(first, 0), min(first + box, size)
        window.append(slice(lo, hi))
        part.append(slice(lo - first, hi - first))
    return segm[tuple(window)], element[tuple(part)]


def label_counts(segm, position, element, nb_labels):
    window, part = clipped(segm, element, position)
    return np.array([np.count_nonzero((window == lb) & (part == 1)) for lb in range(nb_labels)], dtype=float), float(part.sum())


def layer_sums(segm, position, element):
    """(long-double sums per layer, sums of magnitudes per layer, pixels under the element)"""
    window, part = clipped(segm, element, position)
    values = window[part == 1].astype(np.longdouble)                     # n x C
    return values.sum(axis=0), np.abs(values).sum(axis=0), int(part.sum())


def rings(hists, sizes):
    """one position: hists D x L, sizes D -> the D * L ring values"""
    out, hist_last, size_last = [], np.zeros(len(hists[0])), 0.
    for hist, size in zip(hists, sizes):
        if size - size_last <= 0:
            raise ValueError('norm or element should be positive')
        if not np.all(hist >= hist_last):
            raise ValueError('outer elem should have more labels %r then the inter %r' % (hist.tolist(), hist_last.tolist()))
        out += ((hist - hist_last) / float(size - size_last)).tolist()
        hist_last, size_last = hist, size
    return out


def label_ring_table(segm, positions, radii, nb_labels):
    table = []
    for pos in positions:
        per_disc = [label_counts(segm, pos, disc(r), nb_labels) for r in radii]
        table.append(rings([h for h, _ in per_disc], [s for _, s in per_disc]))
    return np.array(table, dtype=float).reshape(len(positions), len(radii) * nb_labels)


def layer_ring_table(segm, positions, radii):
    table = []
    for pos in positions:
        per_disc = [layer_sums(segm, pos, disc(r)) for r in radii]
        table.append(rings([np.asarray(h, dtype=float) for h, _, _ in per_disc], [float(n) for _, _, n in per_disc]))
    return np.array(table, dtype=float).reshape(len(positions), len(radii) * segm.shape[2])


def ring_names(radii, nb_labels):
    return ['hist-d_%i-lb_%i' % (r, lb) for r in radii for lb in range(nb_labels)]


def ray_names(border_labels, angle_step, n_angles):
    return ['ray-lb_%s-agl_%i' % (''.join(str(lb) for lb in border_labels), int(angle))
            for angle in np.linspace(0, 360 - angle_step, n_angles)]


def gaussian_half_kernel(sigma):
    radius = int(4 * sigma + 0.5)
    x = np.arange(-radius, radius + 1)
    weights = np.exp(-0.5 / (sigma * sigma) * x ** 2)
    weights = weights / weights.sum()
    return weights[radius:]


def smooth_along_angle(row, sigma):
    """the smoothing statement of the module docstring on one float32 row"""
    row = np.asarray(row, dtype=np.float32)
    taps, n = gaussian_half_kernel(sigma), len(row)

    def at(i):
        m = i % (2 * n)
        return np.float64(row[m if m < n else 2 * n - 1 - m])

    out = np.empty(n, dtype=np.float32)
    for i in range(n):
        total = at(i) * taps[0]
        for j in range(len(taps) - 1, 0, -1):
            total += (at(i - j) + at(i + j)) * taps[j]
        out[i] = np.float32(total)
    return out


# ---- cases -------------------------------------------------------------------------------------------------------------------
def random_label_map(shape=(97, 131), nb_labels=3, seed=7):
    """blocky random labels (patches of 6 x 6), so that rings differ in content"""
    rng = np.random.RandomState(seed)
    coarse = rng.randint(0, nb_labels, (shape[0] // 6 + 1, shape[1] // 6 + 1))
    return np.kron(coarse, np.ones((6, 6), dtype=int))[:shape[0], :shape[1]]


def random_positions(shape, count, seed=11):
    rng = np.random.RandomState(seed)
    corners = [[0, 0], [0, shape[1] - 1], [shape[0] - 1, 0], [shape[0] - 1, shape[1] - 1]]
    inner = np.stack([rng.randint(0, shape[0], count - 4), rng.randint(0, shape[1], count - 4)], axis=1).tolist()
    return corners + inner


def label_ring_cases():
    """(name, segm, positions, radii, nb_labels)"""
    big = random_label_map()
    odd = random_label_map((23, 31), 3, seed=3).astype(np.int64)
    odd[::5, ::7] = -1
    odd[2::9, 1::4] = 3                                  # = nb_labels: counts for the size only
    row, column = random_label_map((1, 40), 3, seed=5), random_label_map((40, 1), 3, seed=6)
    small_positions = random_positions((23, 31), 12, seed=2)
    return [
        ('doctest', doctest_label_map(), DOCTEST_POINTS, DOCTEST_RADII, 3),
        ('random 97x131', big, random_positions(big.shape, 300), list(DEFAULT_RADII), 3),
        ('whole 10x10 under radius 50', doctest_label_map(), [[0, 0], [9, 9], [4, 5], [0, 9], [9, 0]], [2, 5, 50], 3),
        # every default radius covers the whole 10 x 10 map from its centre: the second disc adds nothing, which is an error
        ('10x10 under the default radii: error', doctest_label_map(), [[0, 0], [4, 5]], list(DEFAULT_RADII), 3),
        ('1x40', row, [[0, 0], [0, 39], [0, 17]], [1, 3, 10, 50], 3),
        ('40x1', column, [[0, 0], [39, 0], [22, 0]], [1, 3, 10, 50], 3),
        ('labels -1 and nb_labels', odd, small_positions, [1, 2, 4, 9], 3),
        # 5 radii: (nb_labels + 1) * 5 = 30 bins is the last that fits the 32 LDS columns of a lane, 35 composes per radius
        ('5 labels: device bins 30', random_label_map((23, 31), 5, seed=8), small_positions, [1, 2, 4, 9, 15], 5),
        ('6 labels: composed, bins 35', random_label_map((23, 31), 6, seed=9), small_positions, [1, 2, 4, 9, 15], 6),
        ('nb_labels above the labels of the map', odd.clip(0, 2), small_positions, [2, 5], 7),
    ]


def layer_ring_cases():
    """(name, layers, positions, radii)"""
    cases = []
    for channels, seed in ((2, 21), (5, 22)):
        rng = np.random.RandomState(seed)
        layers = rng.random_sample((97, 131, channels))
        layers /= layers.sum(axis=2, keepdims=True)
        cases.append(('random 97x131x%d' % channels, layers, random_positions((97, 131), 100, seed=seed), list(DEFAULT_RADII)))
    rng = np.random.RandomState(23)
    cases.append(('signed 20x33x2', rng.standard_normal((20, 33, 2)) * 1e3, random_positions((20, 33), 10, seed=23), [1, 2, 4]))
    return cases


def ray_map():
    """label 0 outside, a disc of label 1 with an off-centre disc of label 2 inside, and a notch of label 3"""
    yy, xx = np.mgrid[:61, :83]
    segm = np.zeros((61, 83), dtype=int)
    segm[(yy - 30) ** 2 + (xx - 40) ** 2 <= 24 ** 2] = 1
    segm[(yy - 35) ** 2 + (xx - 33) ** 2 <= 8 ** 2] = 2
    segm[28:33, 50:70] = 3
    return segm


#: inside label 1, inside label 2, on the border pixels of the discs, at the rim and the corners of the map
RAY_POSITIONS = [(30, 40), (35, 33), (30, 16), (30, 17), (35, 41), (6, 40), (0, 0), (60, 82), (0, 41), (30, 82), (30, 60), (45, 50)]
RAY_BORDER_SETS = ([0], [1, 2], [7])
