"""Shared inputs of the object-cut tests (``object_segmentation_graphcut_pixels`` / ``_slic``): the reference's doctest vectors --
the only ones from the real gco --, seeded cases whose reference results are in tests/golden/object_cut.npz (written by
tests/golden/make_golden_object_cut.py), numpy stand-ins for the device pieces of the superpixel variant, and pyGCO's grid in
numpy."""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, 'golden', 'object_cut.npz')

# ---- imsegm/region_growing.py:182-200
DOCTEST_SEGM = np.array([[0] * 10, [1] * 5 + [0] * 5, [1] * 4 + [0] * 6, [0] * 6 + [1] * 4, [0] * 5 + [1] * 5, [0] * 10])
DOCTEST_CENTRES = [(1, 2), (4, 8)]
DOCTEST_PIXELS = [
    (dict(gc_regul=0., coef_shape=0.5),
     [[0, 0, 0, 0, 0, 0, 0, 0, 0, 0], [2, 2, 1, 2, 2, 0, 0, 0, 0, 0], [2, 2, 2, 2, 0, 0, 0, 0, 0, 0], [0, 0, 0, 0, 0, 0, 2, 2, 2, 2],
      [0, 0, 0, 0, 0, 2, 2, 2, 2, 2], [0, 0, 0, 0, 0, 0, 0, 0, 0, 0]]),
    (dict(gc_regul=.5, seed_size=1),
     [[0, 0, 0, 0, 0, 0, 0, 0, 0, 0], [1, 1, 1, 1, 1, 0, 0, 0, 0, 0], [1, 1, 1, 1, 0, 0, 0, 0, 0, 0], [0, 0, 0, 0, 0, 0, 2, 2, 2, 2],
      [0, 0, 0, 0, 0, 2, 2, 2, 2, 2], [0, 0, 0, 0, 0, 0, 0, 0, 0, 0]]),
]
# ---- imsegm/region_growing.py:70-76
DOCTEST_SLIC = np.array([[0] * 3 + [1] * 3 + [2] * 3 + [3] * 3 + [4] * 3, [5] * 3 + [6] * 3 + [7] * 3 + [8] * 3 + [9] * 3])
DOCTEST_SLIC_SEGM = np.array([[0] * 15, [1] * 12 + [0] * 3])
DOCTEST_SLIC_CENTRES = [(1, 7)]
DOCTEST_SLIC_RUNS = [
    (dict(gc_regul=0., edge_coef=1., coef_shape=1.), [0, 0, 0, 0, 0, 1, 1, 1, 1, 0]),
    (dict(gc_regul=1., edge_coef=1.), [0, 0, 0, 0, 0, 1, 1, 1, 1, 0]),
]

#: name -> (height, width, number of centres, keyword arguments, corner); the sizes are those at which the device takes another
#: path: one workgroup with everything in LDS (33 x 47), just over the 8 192 sites beyond which the whole device cuts (90 x 93), a
#: grid without vertical or without horizontal edges, and as many labels as the cut takes
PIXEL_CASES = {
    'p33_seed0': (33, 47, 3, dict(gc_regul=1., seed_size=0), False),
    'p33_seed2': (33, 47, 3, dict(gc_regul=1., seed_size=2), False),
    'p33_shape0_corner': (33, 47, 3, dict(gc_regul=0.5, seed_size=0, coef_shape=0.), True),
    'p33_shape_corner': (33, 47, 3, dict(gc_regul=0.5, seed_size=0, coef_shape=0.5, shape_mean_std=(30., 15.)), True),
    'p90': (90, 93, 4, dict(gc_regul=2., seed_size=3, coef_shape=0.1, shape_mean_std=(20., 6.)), False),
    'row': (1, 40, 2, dict(gc_regul=0.3, coef_shape=0.2, shape_mean_std=(6., 2.)), False),
    'col': (40, 1, 2, dict(gc_regul=0.3, coef_shape=0.2, shape_mean_std=(6., 2.)), False),
    'many': (20, 21, 63, dict(gc_regul=0.01), False),
}
LABELS_FG_PROB = (0.1, 0.9, 0.7)
#: name -> keyword arguments of the 64 x 96 superpixel case
SLIC_CASES = {
    'model': dict(gc_regul=1., edge_coef=0.5, edge_type='model', coef_shape=0.2, shape_mean_std=(14., 5.)),
    'const': dict(gc_regul=0.5, edge_coef=1., edge_type='', coef_shape=0.2, shape_mean_std=(14., 5.)),
    'const_neighbours': dict(gc_regul=0.5, edge_coef=2., edge_type='', coef_shape=0.2, shape_mean_std=(14., 5.), add_neighbours=True),
}


def pixel_case(name, seed):
    """(segm, centres, keyword arguments): blobs of the classes 1 and 2 around the centres on class 0, with noise"""
    height, width, n_centres, kwargs, corner = PIXEL_CASES[name]
    rng = np.random.RandomState(seed)
    margin = min(3, (height - 1) // 2), min(3, (width - 1) // 2)
    cells = rng.permutation((height - 2 * margin[0]) * (width - 2 * margin[1]))[:n_centres]
    centres = [(margin[0] + int(c) // (width - 2 * margin[1]), margin[1] + int(c) % (width - 2 * margin[1])) for c in cells]
    if corner:
        centres[0] = (0, 0)
    rows, cols = np.indices((height, width))
    segm = np.zeros((height, width), dtype=int)
    radius = 1.5 if n_centres > 8 else max(2., min(height, width, 40) / 4.)
    for i, (r, c) in enumerate(centres):
        segm[(rows - r)**2 + (cols - c)**2 <= radius**2] = 1 + i % 2
    noise = rng.rand(height, width) < 0.08
    segm[noise] = rng.randint(0, 3, int(noise.sum()))
    return segm, centres, dict(kwargs, labels_fg_prob=LABELS_FG_PROB)


def slic_case(seed):
    """(slic, segm, centres) of the 64 x 96 case: 8 x 8 blocks with ragged borders, two blobs"""
    rng = np.random.RandomState(seed)
    height, width = 64, 96
    rows, cols = np.indices((height, width))
    shift_r, shift_c = rng.randint(-2, 3, (2, height, width))
    slic = (np.clip(rows + shift_r * (rng.rand(height, width) < 0.3), 0, height - 1) // 8) * (width // 8) \
        + np.clip(cols + shift_c * (rng.rand(height, width) < 0.3), 0, width - 1) // 8
    centres = [(20 + int(rng.randint(-3, 4)), 28 + int(rng.randint(-3, 4))), (40 + int(rng.randint(-3, 4)), 70 + int(rng.randint(-3, 4)))]
    segm = np.zeros((height, width), dtype=int)
    for i, (r, c) in enumerate(centres):
        segm[(rows - r)**2 + (cols - c)**2 <= 14**2] = 1 + i
    noise = rng.rand(height, width) < 0.05
    segm[noise] = rng.randint(0, 3, int(noise.sum()))
    return slic, segm, centres


def load_fixture():
    with np.load(FIXTURE) as data:
        return {key: data[key] for key in data.files}


# ---- numpy stand-ins of the device pieces the superpixel variant is composed of (CPU tests)
def label_classes(slic, segm):
    """argmax of ``histogram_regions_labels_norm``"""
    counts = np.zeros((int(slic.max()) + 1, int(segm.max()) + 1))
    np.add.at(counts, (slic.ravel(), segm.ravel()), 1)
    return np.argmax(counts / np.maximum(counts.sum(axis=1, keepdims=True), 1), axis=1)


def superpixel_centres(slic):
    rows, cols = np.indices(slic.shape)
    count = np.bincount(slic.ravel())
    return np.stack([np.bincount(slic.ravel(), rows.ravel()) / count, np.bincount(slic.ravel(), cols.ravel()) / count], axis=1)


def adjacency_edges(slic):
    """edges a < b of the 4-connected region adjacency graph, ordered by (b, a)"""
    pairs = np.vstack([np.stack([slic[:, :-1].ravel(), slic[:, 1:].ravel()], axis=1),
                       np.stack([slic[:-1, :].ravel(), slic[1:, :].ravel()], axis=1)])
    pairs = np.sort(pairs[pairs[:, 0] != pairs[:, 1]], axis=1)
    n = int(slic.max()) + 1
    codes = np.unique(pairs[:, 0] + n * pairs[:, 1].astype(np.int64))
    return np.stack([codes % n, codes // n], axis=1).astype(np.int32)


# ---- pyGCO's grid
def grid_edges(height, width):
    """edges and weights order of ``gco.cut_grid_graph``: all vertical edges row-major, then all horizontal ones"""
    index = np.arange(height * width, dtype=np.int32).reshape(height, width)
    return np.concatenate([np.stack([index[:-1].ravel(), index[1:].ravel()], axis=1),
                           np.stack([index[:, :-1].ravel(), index[:, 1:].ravel()], axis=1)], axis=0)


def arcs_by_loop(edges, n_sites):
    """(arc_start, arc_to, arc_rev, edge_arc) as the host loop of ``imsegm_cut_general_graph`` builds them"""
    arc_start = np.zeros(n_sites + 1, dtype=np.int64)
    for a, b in edges:
        arc_start[a + 1] += 1
        arc_start[b + 1] += 1
    arc_start = np.cumsum(arc_start)
    fill = arc_start[:-1].copy()
    arc_to, arc_rev = np.zeros(2 * len(edges), dtype=np.int64), np.zeros(2 * len(edges), dtype=np.int64)
    edge_arc = np.zeros((len(edges), 2), dtype=np.int64)
    for j, (a, b) in enumerate(edges):
        ia, ib = fill[a], fill[b]
        fill[a] += 1
        fill[b] += 1
        arc_to[ia], arc_to[ib], arc_rev[ia], arc_rev[ib] = b, a, ib, ia
        edge_arc[j] = ia, ib
    return arc_start, arc_to, arc_rev, edge_arc
