"""Shared by tests/test_boundary3d_reference_host.py and tests/test_gpu_boundary3d.py: seeded 3-D label maps and the definitions
behind ``pyimsegm_amd.labeling.compute_boundary_distances`` on volumes, in numpy / scipy and written independently of the package.

Definitions.  The thick boundary mask is ``grey_dilation != grey_erosion`` with ``generate_binary_structure(3, 1)`` (what
scikit-image's ``find_boundaries(mode='thick')`` evaluates); distances are ``scipy.ndimage.distance_transform_edt`` of the
complement; points are ``np.argwhere`` (raster order).  ``edt_brute`` is the square root of the brute-force integer minimum over
the set voxels (for a mask without one: the distance to (-1, 0, 0), which is scipy's answer), the host test shows that scipy equals
it bit for bit on the small maps.  Every result is exact -- integers up to one correctly rounded square root -- so all comparisons
are ``same``: ``np.array_equal`` with dtype and shape.  No expected number comes from the device code.

Maps (all int64, read-only, built once).

* Extents at the kernels' edges: x in 1, 63, 64, 65, 255, 256, 257, 513 at depth 3 and height 5 (the 64-lane wave, the 256-voxel
  tile ``EDT_B`` and the 256-offset round ``EDT_T`` of the row pass), the same on y, depths 1, 2, 3, 17 and the shapes 1 x 1 x 1,
  1 x 1 x 7, 1 x 7 x 1, 7 x 1 x 1.  Each extent comes as a random 2-label map and as a sparse one (a handful of odd voxels: long
  searches on every axis).
* A constant map (empty mask: scipy's (-1, 0, 0) answer); one odd voxel in the far corner of 9 x 40 x 300 (the longest search on
  all three axes); set voxels in the middle of the depth only, first slices only, last slices only.  The thick boundary of a label
  change always marks both sides, so in a volume deeper than one slice an odd voxel of slice z sets voxels of slices z - 1 .. z + 1:
  three neighbouring slices (two at either end of the depth) are the narrowest band there is, every other slice is empty.
* Random maps of 2 and 5 labels, a blocky supervoxel-like map and a shifted copy of it.
* Long rows, 1 x 1 x 65535 and 2 x 1 x 65535 with one odd voxel at x = 0 (set voxels at x = 0 and 1): squared distances up to 65533^2 =
  4 294 574 089, next to the 32-bit cap.
* Compaction: reference maps with a stated number of boundary voxels around the chunk the compaction kernels count by (read from
  csrc/boundary.hip by ``compaction_chunk``): none, two (the fewest a thick boundary can have), one chunk, one chunk and one more,
  two chunks, every voxel.  The counts are literals (``COMPACTION_COUNTS``), the host test checks them on the generated maps."""
import functools
import os
import re

import numpy as np
from scipy import ndimage

SEED = 20261021
EDGE_EXTENTS = (1, 63, 64, 65, 255, 256, 257, 513)
DEPTHS = (1, 2, 3, 17)
TINY_SHAPES = ((1, 1, 1), (1, 1, 7), (1, 7, 1), (7, 1, 1))
BOUNDARY_HIP = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'pyimsegm_amd', 'csrc', 'boundary.hip')
#: boundary voxels of the compaction references; CHUNK = 2048 voxels per workgroup of k_compact_count (``compaction_chunk``)
COMPACTION_COUNTS = {'none': 0, 'two': 2, 'one_chunk': 2048, 'one_chunk_and_one': 2049, 'two_chunks': 4096, 'every_voxel': 3168}
#: the largest number of (voxel, set voxel) pairs ``edt_brute`` is asked for
BRUTE_PAIRS = 3 * 10**7


def _rng(*key):
    return np.random.default_rng([SEED] + [int(k) for k in key])


def compaction_chunk():
    """CP_CHUNK of csrc/boundary.hip: the voxels one workgroup of the compaction kernels owns"""
    text = open(BOUNDARY_HIP).read()
    found = re.search(r'constexpr int CP_ITEMS = (\d+), CP_CHUNK = (\d+) \* CP_ITEMS;', text)
    return int(found.group(1)) * int(found.group(2))


# ---- label maps ---------------------------------------------------------------------------------------------------------------
def random_map(shape, n_labels, seed=0):
    return _rng(seed, n_labels, *shape).integers(0, n_labels, shape).astype(np.int64)


def sparse_map(shape, n_odd=4, seed=0):
    """zeros with ``n_odd`` voxels (fewer in a tiny volume) of label 1 at seeded places"""
    seg = np.zeros(shape, dtype=np.int64)
    rng = _rng(seed, 77, *shape)
    for _ in range(min(n_odd, max(1, seg.size // 4))):
        seg[tuple(int(rng.integers(0, extent)) for extent in shape)] = 1
    return seg


def block_map(shape, step=(4, 9, 11)):
    """boxes of ``step`` voxels numbered in raster order"""
    z, y, x = np.indices(shape)
    per_row, per_slice = -(-shape[2] // step[2]), -(-shape[1] // step[1]) * -(-shape[2] // step[2])
    return ((z // step[0]) * per_slice + (y // step[1]) * per_row + x // step[2]).astype(np.int64)


def _line_with(count, length):
    """1 x 1 x length labels whose thick boundary is exactly the first ``count`` voxels (count 0 or >= 2): they alternate, the rest
    keeps the last of them"""
    line = np.zeros(length, dtype=np.int64)
    line[:count] = np.arange(count) % 2
    line[count:] = line[count - 1] if count else 0
    return line.reshape(1, 1, length)


@functools.lru_cache(maxsize=None)
def maps():
    """name -> label map (int64, read-only)"""
    out = {}
    shapes = [(3, 5, x) for x in EDGE_EXTENTS] + [(3, y, 5) for y in EDGE_EXTENTS if y != 5] + [(d, 9, 70) for d in DEPTHS]
    for shape in shapes + list(TINY_SHAPES):
        out['rand_%dx%dx%d_L2' % shape] = random_map(shape, 2)
        out['sparse_%dx%dx%d' % shape] = sparse_map(shape)
    out['constant_4x6x70'] = np.full((4, 6, 70), 3, dtype=np.int64)
    out['rand_4x6x70_L2'] = random_map((4, 6, 70), 2)
    far = np.zeros((9, 40, 300), dtype=np.int64)
    far[8, 39, 299] = 1                                 # thick boundary: the corner voxel and its three neighbours
    out['far_corner_9x40x300'] = far
    middle = np.zeros((9, 12, 70), dtype=np.int64)
    middle[4, 2, 3] = middle[4, 9, 66] = middle[4, 5, 30] = 1     # set voxels in slices 3, 4, 5; slices 0-2 and 6-8 are empty
    out['middle_slices_9x12x70'] = middle
    first, last = np.zeros((9, 12, 70), dtype=np.int64), np.zeros((9, 12, 70), dtype=np.int64)
    first[0, 3, 60] = first[0, 10, 2] = 1               # set voxels in slices 0 and 1
    last[8, 3, 60] = last[8, 10, 2] = 1                 # set voxels in slices 7 and 8
    out['first_slices_9x12x70'], out['last_slices_9x12x70'] = first, last
    for count in (2, 5):
        out['rand_5x33x65_L%d' % count] = random_map((5, 33, 65), count)
        out['rand_17x65x257_L%d' % count] = random_map((17, 65, 257), count)
    out['rand_5x6x7_L3'] = random_map((5, 6, 7), 3)
    out['blocks_12x40x48'] = block_map((12, 40, 48))
    out['blocks_shifted_12x40x48'] = np.roll(out['blocks_12x40x48'], (1, 2, 3), axis=(0, 1, 2))
    for depth in (1, 2):
        row = np.zeros((depth, 1, 65535), dtype=np.int64)
        row[0, 0, 0] = 1
        out['long_row_%dx1x65535' % depth] = row
    chunk = compaction_chunk()
    for key, count in COMPACTION_COUNTS.items():
        name = 'points_%s_%d_chunk_%d' % (key, count, chunk)
        if key == 'every_voxel':
            z, y, x = np.indices((4, 24, 33))
            out[name] = ((z + y + x) % 2).astype(np.int64)
        else:
            out[name] = _line_with(count, 4500)
    out['other_1x1x4500'] = sparse_map((1, 1, 4500), 3, seed=5)
    out['other_4x24x33'] = sparse_map((4, 24, 33), 3, seed=5)
    for seg in out.values():
        seg.setflags(write=False)
    return out


def compaction_name(key):
    return 'points_%s_%d_chunk_%d' % (key, COMPACTION_COUNTS[key], compaction_chunk())


def pair_cases():
    """(reference map, other map) of one shape: every map against itself, plus the pairs that differ -- a reference with
    boundaries against a map without (scipy's answer for the empty mask at the points) and the other way round (0 points), random
    against random, blocks against their shifted copy, the compaction references against a sparse map"""
    names = [name for name in maps() if not name.startswith(('points_', 'other_'))]
    pairs = [(name, name) for name in names]
    pairs += [('rand_5x33x65_L5', 'rand_5x33x65_L2'), ('rand_5x33x65_L2', 'rand_5x33x65_L5'), ('rand_17x65x257_L5', 'rand_17x65x257_L2'),
              ('blocks_12x40x48', 'blocks_shifted_12x40x48'), ('blocks_shifted_12x40x48', 'blocks_12x40x48'),
              ('middle_slices_9x12x70', 'first_slices_9x12x70'), ('first_slices_9x12x70', 'last_slices_9x12x70'),
              ('last_slices_9x12x70', 'middle_slices_9x12x70'), ('rand_3x5x257_L2', 'sparse_3x5x257'), ('sparse_3x5x513', 'rand_3x5x513_L2'),
              ('rand_4x6x70_L2', 'constant_4x6x70'), ('constant_4x6x70', 'rand_4x6x70_L2')]
    for key in COMPACTION_COUNTS:
        pairs.append((compaction_name(key), 'other_4x24x33' if key == 'every_voxel' else 'other_1x1x4500'))
    return pairs


def small_pair_cases():
    """the pairs of at most 30 000 voxels: what the host statement of the package is held to on every run"""
    return [(a, b) for a, b in pair_cases() if maps()[a].size <= 30000]


# ---- the definitions in numpy / scipy -----------------------------------------------------------------------------------------
def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)


def thick(seg):
    """boolean mask: a neighbour along z, y or x inside the volume carries another label"""
    cross = ndimage.generate_binary_structure(3, 1)
    return ndimage.grey_dilation(seg, footprint=cross) != ndimage.grey_erosion(seg, footprint=cross)


def thick_shifted(seg):
    """the same by shifted comparisons (no morphology, no border mode)"""
    seg = np.asarray(seg)
    mask = np.zeros(seg.shape, dtype=bool)
    for axis in range(3):
        a, b = np.swapaxes(seg, 0, axis), np.swapaxes(mask, 0, axis)
        differs = a[1:] != a[:-1]
        b[1:] |= differs
        b[:-1] |= differs
    return mask


@functools.lru_cache(maxsize=None)
def _edt_of(name):
    dist = ndimage.distance_transform_edt(~thick(maps()[name]))
    dist.setflags(write=False)
    return dist


def edt(mask):
    """float64 distance of every voxel to the nearest set voxel of ``mask``"""
    return ndimage.distance_transform_edt(~np.asarray(mask, dtype=bool))


def distance_map(name):
    """``edt(thick(maps()[name]))``, computed once per map"""
    return _edt_of(name)


def brute_fits(mask):
    return mask.size * max(1, int(np.count_nonzero(mask))) <= BRUTE_PAIRS


def edt_brute(mask):
    """square root of the brute-force integer minimum; a mask without a set voxel: the distance to (-1, 0, 0)"""
    mask = np.asarray(mask, dtype=bool)
    where = np.argwhere(mask).astype(np.int64)
    if not len(where):
        where = np.array([[-1, 0, 0]], dtype=np.int64)
    voxels = np.indices(mask.shape).reshape(3, -1).T.astype(np.int64)
    best = np.full(len(voxels), np.iinfo(np.int64).max, dtype=np.int64)
    for start in range(0, len(where), 32):
        part = where[start:start + 32]
        d2 = ((voxels[:, None, :] - part[None, :, :])**2).sum(axis=2)
        best = np.minimum(best, d2.min(axis=1))
    return np.sqrt(best.astype(np.float64)).reshape(mask.shape)


def boundary_distances(ref_name, name):
    """(points int64 n x 3 in raster order, distances float64 n) of the thick boundary of the reference map to that of the other"""
    on_ref = thick(maps()[ref_name])
    return np.argwhere(on_ref).astype(np.int64), distance_map(name)[on_ref]
