"""Shared by tests/test_graph_reference_host.py and tests/test_gpu_graph.py: a plain numpy statement of the region adjacency graph
and the superpixel centres of a label map (``make_graph_segm_connect_grid2d_conn4`` / ``..._grid3d_conn6`` and
``superpixel_centers`` of the reference), and the label maps the adjacency kernels are held to.  numpy only; the project is not
imported here.

Reference.  Edges: along every axis the pairs of unequal neighbours, ``min + K * max`` through ``np.unique`` -- rows ``[a, b]``,
a < b, sorted by (b, a).  Centres: int64 coordinate sums and counts per label (``np.add.at``), ``sum.astype(float64) / count``;
labels without pixels get -1 in every coordinate.  Sums and counts stay far below 2^53, so both sides divide the same two exact
numbers: every comparison is ``np.array_equal``, there is no tolerance.

Cases.  SLIC output is compact, planar, a dozen labels per tile; these maps are what it never is.  The 2-D kernel
(csrc/graph.hip ``k_adjacency_centres``) covers 64 x 16 pixels per workgroup and 64 x 4 per wave, the 3-D kernel
(csrc/volume_graph.hip ``k_vol_adjacency_runs``) 64 x 16 x 8 voxels per workgroup; both find the runs of equal labels of a 64-pixel
row with one ballot and add their sums in a 64-slot LDS hash table per workgroup.  Hence: salt (more than 64 labels in a tile:
the global-atomics branch; far more neighbour pairs than the first edge capacity of ``graph()``), runs of one pixel and of exactly
64, borders on the wave (x = 63 / 64 / 65), row-block (y = 3 / 4 / 5, 15 / 16 / 17) and slice-group (z = 7 / 8, 15 / 16) seams,
label counts around the 32-bit words of the bitmap, id ranges with holes and with absent labels behind the last one, rows and
slices that are constant next to rows and slices that are salt (the 3-D kernel reports a pair across y or z only where either
label changes along x), hub labels with 31 .. 300 neighbours (the neighbour table's rows are widened 32 -> 64 -> ... until they
fit, and hold colliding hashes), and shapes of one pixel, one row, one column.  No case exceeds 2^17 elements.

``CASES_2D`` / ``CASES_3D``: lists of ``(id, make)``, ``make()`` -> int32 map.  ``N_LABELS``: the cases installed with more labels
than ``max + 1``.  ``SALT_TILES``, ``RETRY``, ``HUBS``, ``SEAMS``: what the host test asserts about the cases themselves."""
import numpy as np

SEED = 20261020
TILE_2D = (16, 64)
TILE_3D = (8, 16, 64)


def graph_reference(labels, n_labels=None):
    """(edges int64 E x 2 sorted by (b, a); centres float64 K x ndim; present bool K) of a 2-D or 3-D label map"""
    labels = np.asarray(labels).astype(np.int64)
    n_labels = int(labels.max()) + 1 if n_labels is None else int(n_labels)
    keys = []
    for axis in range(labels.ndim):
        first = np.take(labels, np.arange(labels.shape[axis] - 1), axis=axis).ravel()
        second = np.take(labels, np.arange(1, labels.shape[axis]), axis=axis).ravel()
        differ = first != second
        keys.append(np.minimum(first, second)[differ] + n_labels * np.maximum(first, second)[differ])
    keys = np.unique(np.concatenate(keys))
    edges = np.stack([keys % n_labels, keys // n_labels], axis=1).astype(np.int64)
    counts = np.zeros(n_labels, dtype=np.int64)
    np.add.at(counts, labels.ravel(), 1)
    sums = np.zeros((n_labels, labels.ndim), dtype=np.int64)
    for axis, coords in enumerate(np.indices(labels.shape)):
        np.add.at(sums[:, axis], labels.ravel(), coords.ravel().astype(np.int64))
    present = counts > 0
    centres = np.full((n_labels, labels.ndim), -1.0, dtype=np.float64)
    centres[present] = sums[present].astype(np.float64) / counts[present, np.newaxis]
    return edges, centres, present


def max_degree(edges, n_labels):
    """the largest number of neighbours of a label"""
    if not len(edges):
        return 0
    return int(np.bincount(np.asarray(edges).ravel(), minlength=n_labels).max())


def distinct_per_tile(labels, tile):
    """number of distinct labels in every tile of the grid the kernels lay over the map"""
    labels = np.asarray(labels)
    steps = [range(0, extent, step) for extent, step in zip(labels.shape, tile)]
    grid = np.meshgrid(*steps, indexing='ij')
    out = []
    for corner in zip(*[g.ravel() for g in grid]):
        window = tuple(slice(c, c + step) for c, step in zip(corner, tile))
        out.append(len(np.unique(labels[window])))
    return out


def has_border(labels, axis, coordinate):
    """a label changes between ``coordinate - 1`` and ``coordinate`` along ``axis``"""
    labels = np.asarray(labels)
    return bool((np.take(labels, coordinate - 1, axis=axis) != np.take(labels, coordinate, axis=axis)).any())


def _rng(*key):
    return np.random.default_rng([SEED] + [int(k) for k in key])


def salt(shape, n_labels, seed=0, first=0):
    """an independent random label ``first .. first + n_labels - 1`` per pixel; the largest label is present"""
    out = _rng(seed, n_labels, *shape).integers(0, n_labels, shape)
    out.flat[0] = n_labels - 1
    return (out + first).astype(np.int32)


def _i32(labels):
    return np.ascontiguousarray(labels, dtype=np.int32)


def _case(cases, name, call, *args, **kwargs):
    cases.append((name, lambda: call(*args, **kwargs)))


def word_blocks(shape, n_labels, scale=1):
    """blocks of two pixels along x numbered modulo ``n_labels`` (so that the last label meets label 0), shifted by about a third
    of the range every third row and by about a half every slice; ``scale`` 3 leaves two ids out of three unused"""
    coords = np.indices(shape)
    x, y = coords[-1], coords[-2]
    z = coords[0] if len(shape) == 3 else 0
    return _i32((x // 2 + (y // 3) * (n_labels // 3) + z * (n_labels // 2 + 1)) % n_labels * scale)


def hub(n_neighbours, shape=(6, 30, 80)):
    """runs of 8 voxels numbered modulo N and one slab between them that touches them all; the slab's id is in the middle of the
    range, so it has neighbours of smaller and of larger number: exactly N"""
    out = (np.arange(int(np.prod(shape))).reshape(shape) // 8) % n_neighbours
    out += out >= n_neighbours // 2
    out[shape[0] // 2] = n_neighbours // 2
    return _i32(out)


def staircase(shape, first_border, step):
    """every row of every slice holds two labels of its own; their border moves by ``step`` from row to row and slice to slice"""
    z, y, x = np.indices(shape)
    return _i32(2 * (z * shape[1] + y) + (x >= first_border + step * (y + z)))


def _steps(coords, borders):
    return np.searchsorted(np.asarray(borders), coords, side='right')


def bands(shape, x_borders=(63, 64, 65), y_borders=(15, 16, 17)):
    """the same bands in every slice: a new label at every border along x and along y"""
    _, y, x = np.indices(shape)
    return _i32(_steps(x, x_borders) + (len(x_borders) + 1) * _steps(y, y_borders))


WORD_COUNTS = (1, 2, 31, 32, 33, 63, 64, 65, 96, 97)
N_LABELS = {}                 # id -> labels the session is told of (more than max + 1: absent labels behind the last one)
SALT_TILES = {}               # id -> 'over': some tile holds more than 64 labels; 'within': none does
RETRY = []                    # ids with more edges than the first capacity of graph()
HUBS = {}                     # id -> (hub label, its number of neighbours)
SEAMS = {}                    # id -> [(axis, coordinate)]: a label changes between coordinate - 1 and coordinate


def _cases_2d():
    cases = []
    for n_labels in (64, 65, 200):
        for shape in ((16, 64), (17, 65), (33, 130)):
            name = 'salt_%dx%d_K%d' % (shape + (n_labels, ))
            _case(cases, name, salt, shape, n_labels)
            SALT_TILES[name] = 'within' if n_labels <= 64 else 'over'
    RETRY.append('salt_33x130_K200')
    for n_labels in (2, 7, 64, 65):                                    # runs of one pixel, a pair across lane 63 -> lane 0
        name = 'vstripes_K%d' % n_labels
        _case(cases, name, lambda k: _i32(np.indices((6, 130))[1] % k), n_labels)
        SEAMS[name] = [(1, 64)]
    for border in (63, 64, 65):
        name = 'vband_x%d' % border
        _case(cases, name, lambda b: _i32(np.indices((5, 130))[1] >= b), border)
        SEAMS[name] = [(1, border)]
    _case(cases, 'vbands_x63_64_65', lambda: _i32(_steps(np.indices((5, 130))[1], (63, 64, 65))))
    SEAMS['vbands_x63_64_65'] = [(1, 63), (1, 64), (1, 65)]
    for width in (1, 63, 64, 65, 127, 128, 129):                       # a run of exactly 64, a run cut at the wave's edge, < 64 lanes
        _case(cases, 'rows_W%d' % width, lambda w: _i32(np.indices((5, w))[0]), width)
    for height in (1, 3, 4, 5, 15, 16, 17, 33):
        name = 'hstripes_H%d' % height
        _case(cases, name, lambda h: _i32(np.indices((h, 70))[0] % 3), height)
        SEAMS[name] = [(0, y) for y in (3, 4, 5, 15, 16, 17) if y < height]
    for border in (3, 4, 5, 15, 16, 17):
        name = 'hband_y%d' % border
        _case(cases, name, lambda b: _i32(np.indices((33, 70))[0] >= b), border)
        SEAMS[name] = [(0, border)]

    def const_and_salt(shape, parity):
        out = salt(shape, 50, seed=parity, first=shape[0])
        rows = np.arange(shape[0])
        out[rows % 2 == parity] = rows[rows % 2 == parity, np.newaxis]
        return out

    _case(cases, 'const_over_salt', const_and_salt, (6, 130), 0)      # row 0 a single label, row 1 salt, ...
    _case(cases, 'salt_over_const', const_and_salt, (6, 130), 1)
    _case(cases, 'diagonal_down', lambda: _i32(np.indices((20, 130)).sum(axis=0) // 3))
    _case(cases, 'diagonal_up', lambda: _i32((np.indices((20, 130))[1] - np.indices((20, 130))[0]) // 3 + 7))
    _case(cases, 'checker_1', lambda: _i32(np.indices((17, 130)).sum(axis=0) % 2))
    _case(cases, 'checker_2', lambda: _i32((np.indices((17, 130)) // 2).sum(axis=0) % 2))
    for n_labels in WORD_COUNTS:
        shape = (6, 2 * n_labels + 3)
        _case(cases, 'words_K%d' % n_labels, word_blocks, shape, n_labels)
        _case(cases, 'words_K%d_holes' % n_labels, word_blocks, shape, n_labels, 3)
        _case(cases, 'words_K%d_trailing' % n_labels, word_blocks, shape, n_labels)
        N_LABELS['words_K%d_trailing' % n_labels] = n_labels + 40
    for shape in ((1, 1), (1, 300), (300, 1), (4, 4)):
        _case(cases, 'tiny_%dx%d' % shape, salt, shape, 5)
    return cases


def _cases_3d():
    cases = []
    for n_labels in (65, 300):
        for shape in ((1, 16, 64), (2, 17, 65), (9, 20, 70)):
            name = 'salt_%dx%dx%d_K%d' % (shape + (n_labels, ))
            _case(cases, name, salt, shape, n_labels)
            SALT_TILES[name] = 'over'
    RETRY.append('salt_9x20x70_K300')
    for n_labels in (2, 3, 9):                                         # the seams between workgroups, the last turns of the pipeline
        for depth in (1, 2, 7, 8, 9, 15, 16, 17):
            name = 'slabs_K%d_D%d' % (n_labels, depth)
            _case(cases, name, lambda k, d: _i32(np.indices((d, 6, 70))[0] % k), n_labels, depth)
            SEAMS[name] = [(0, z) for z in (7, 8, 15, 16) if z < depth]
    _case(cases, 'slab_bands_z8_16', lambda: _i32(np.indices((17, 6, 70))[0] // 8))
    SEAMS['slab_bands_z8_16'] = [(0, 8), (0, 16)]

    def columns(depth, other=None):
        out = np.repeat(salt((1, 6, 70), 50), depth, axis=0)
        if other is not None:
            out[other] = salt((6, 70), 50, seed=1)
        return out

    _case(cases, 'columns', columns, 17)
    for other in (0, 8, 16):
        name = 'columns_but_z%d' % other
        _case(cases, name, columns, 17, other)
        SEAMS[name] = [(0, z) for z in (other, other + 1) if 0 < z < 17]

    def const_and_salt(shape, axis, parity):
        out = salt(shape, 50, seed=10 * axis + parity, first=shape[axis])
        index = np.arange(shape[axis])
        chosen = index % 2 == parity
        if axis == 0:
            out[chosen] = index[chosen, np.newaxis, np.newaxis]
        else:
            out[:, chosen] = index[chosen, np.newaxis]
        return out

    _case(cases, 'const_slice_then_salt', const_and_salt, (4, 6, 130), 0, 0)
    _case(cases, 'salt_slice_then_const', const_and_salt, (4, 6, 130), 0, 1)
    _case(cases, 'const_row_then_salt', const_and_salt, (3, 6, 130), 1, 0)
    _case(cases, 'salt_row_then_const', const_and_salt, (3, 6, 130), 1, 1)
    _case(cases, 'diagonal', lambda: _i32(np.indices((5, 9, 130)).sum(axis=0) // 3))
    for name, border, step in (('stair_same_x', 40, 0), ('stair_next_x', 40, 1), ('stair_same_x64', 64, 0), ('stair_over_x64', 60, 1)):
        _case(cases, name, staircase, (3, 6, 130), border, step)
    SEAMS['stair_same_x64'] = [(2, 64)]
    SEAMS['stair_over_x64'] = [(2, 64)]
    for width in (63, 64, 65, 129):
        name = 'bands_W%d' % width
        _case(cases, name, bands, (3, 20, width))
        SEAMS[name] = [(1, 15), (1, 16), (1, 17)] + [(2, x) for x in (63, 64, 65) if x < width]
    for n_neighbours in (31, 32, 33, 64, 65, 150, 300):
        name = 'hub_N%d' % n_neighbours
        _case(cases, name, hub, n_neighbours)
        HUBS[name] = (n_neighbours // 2, n_neighbours)
    for n_labels in WORD_COUNTS:
        shape = (3, 4, 2 * n_labels + 3)
        _case(cases, 'words3_K%d' % n_labels, word_blocks, shape, n_labels)
        _case(cases, 'words3_K%d_holes' % n_labels, word_blocks, shape, n_labels, 3)
        _case(cases, 'words3_K%d_trailing' % n_labels, word_blocks, shape, n_labels)
        N_LABELS['words3_K%d_trailing' % n_labels] = n_labels + 40
    return cases


CASES_2D = _cases_2d()
CASES_3D = _cases_3d()
IDS_2D = [name for name, _ in CASES_2D]
IDS_3D = [name for name, _ in CASES_3D]


def first_capacity(n_labels, ndim):
    """the edge capacity of the first attempt of ``Image2D.graph`` / ``Volume3D.graph``"""
    return max(64, (4 if ndim == 2 else 8) * n_labels)
