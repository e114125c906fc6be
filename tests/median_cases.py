"""Shared by tests/test_median_reference_host.py and tests/test_gpu_median_reference.py: the cases and the references of the per-label
'median' and 'meanGrad' statistics (csrc/median.hip through ``Image2D`` / ``Volume3D`` ``.median()``, ``.mean_gradient()``,
``.response_median()``, ``.response_mean_gradient()``).

References.  The operations are exact, so numpy itself is the reference: ``np.median`` of the values of every label and channel in
the image's dtype (bit for bit), ``np.sum(np.gradient(plane), axis=0)`` stored in the image's dtype (per pixel).  The one inexact
step, the segmented mean of the gradient image, is held to a ``numpy.longdouble`` sum of the float32-cast values within
``1e-12 |ref| + B``, B the fixed-point bound of csrc/stats.hip as tests/test_gpu_stats.py computes it.  No expected number comes
from the device code.

Models.  ``model_median`` / ``model_gradient`` restate the device's evaluation in numpy (order keys, two stable sorts, scan, pick; the
kernel's index arithmetic over the flat array) with ONE defect or none: tests/test_median_reference_host.py shows on the CPU that
the cases see every defect."""
import functools

import numpy as np

from test_gpu_stats import fixed_point_bound

LD = np.longdouble
SEED = 20261018
RTOL = 1e-12

DTYPES = {'u8': np.uint8, 'f32': np.float32, 'f64': np.float64}


def _rng(*key):
    return np.random.default_rng([SEED] + [int(k) for k in key])


# ---- values and label maps ---------------------------------------------------------------------------------------------------
def values(shape, dtype, seed):
    """uint8: 0 .. 255 (256 distinct keys, long runs of equal keys); floats: signed, half of them on a grid of 1 / 4 (ties)"""
    rng = _rng(seed, *shape)
    if dtype == 'u8':
        return rng.integers(0, 256, shape).astype(np.uint8)
    v = rng.standard_normal(shape) * 3
    grid = rng.random(shape) < 0.5
    v[grid] = np.round(v[grid] * 4) / 4
    return v.astype(DTYPES[dtype])


def block_labels(shape, seed, steps=(2, 23, 23)):
    """blocks of 23 x 23 pixels (2 slices in z), one pixel in ten moved to a random label, label 2 left empty, odd and even
    counts; -> (map, n_labels)"""
    rng = _rng(seed, *shape)
    steps = steps[-len(shape):]
    grid = tuple(-(-n // s) for n, s in zip(shape, steps))
    seg = np.ravel_multi_index(tuple(g // s for g, s in zip(np.indices(shape), steps)), grid)
    moved = rng.random(shape) < 0.1
    seg[moved] = rng.integers(0, seg.max() + 1, int(moved.sum()))
    seg[seg >= 2] += 1
    counts = np.bincount(seg.ravel())
    if len(set(counts[counts > 0] % 2)) == 1:            # (a handful of labels, all odd or all even: one pixel changes two of them)
        seg.flat[np.flatnonzero(seg.ravel() == 0)[0]] = 1
    return seg.astype(np.int32), int(seg.max()) + 1


def spread_labels(shape, n_labels, seed):
    """permutation(arange(n)) % n_labels: the largest label is present, the counts are n // n_labels or one more"""
    n = int(np.prod(shape))
    return (_rng(seed, n_labels).permutation(n) % n_labels).astype(np.int32).reshape(shape)


def identity_labels(shape):
    return np.arange(int(np.prod(shape)), dtype=np.int32).reshape(shape)


def special_values(dtype, count, seed, infinities=False):
    """+-0, +- the smallest denormal, the smallest normal, the largest finite, +-1 and its two neighbours, then random finite bit
    patterns of both signs (``infinities``: +-inf among them)"""
    ft = DTYPES[dtype]
    fi = np.finfo(ft)
    one = ft(1)
    head = [0.0, fi.smallest_subnormal, fi.tiny, fi.max, one, np.nextafter(one, ft(2)), np.nextafter(one, ft(0))]
    head = np.array(head + [-v for v in head], dtype=ft)
    assert np.signbit(head[7]) and head[7] == 0
    if infinities:
        head = np.concatenate([head, np.array([np.inf, -np.inf], dtype=ft)])
    rng = _rng(seed, count)
    it = np.uint64 if ft is np.float64 else np.uint32
    bits = rng.integers(0, np.iinfo(it).max, count, dtype=it, endpoint=True)
    rnd = bits.view(ft).copy()
    bad = ~np.isfinite(rnd)                             # an exponent of all ones: +-1.5 instead
    rnd[bad] = np.where(np.signbit(rnd[bad]), ft(-1.5), ft(1.5))
    out = np.concatenate([head, rnd])[:count] if count >= len(head) else head[:count]
    return _rng(seed, 1).permutation(out)


def crafted(dtype, shape, seed):
    """one image / volume whose labels are scattered over the pixels: segments of 1, 2, 3, 4, 255, 256 and 257 pixels, an all-equal
    segment, all -0 / all +0 / mixed zeros (floats), segments that straddle zero, the float32 pairs whose float32 mean rounds or
    overflows (float64: the overflowing pair of the largest finite), the uint8 pairs (254, 255) and (0, 255); the rest is one
    filler label.  -> (array [n, C] flattened back to ``shape`` (+ (3, )), label map, n_labels, names of the segments)"""
    ft = DTYPES[dtype]
    rng = _rng(seed, *shape)
    volume = len(shape) == 3
    n, chans = int(np.prod(shape)), 1 if volume else 3
    segs, names = [], []

    def add(name, columns):
        columns = [np.asarray(col, dtype=ft) for col in columns]
        assert len(columns) in (1, 3) and all(len(col) == len(columns[0]) for col in columns)
        segs.append(np.stack([columns[c % len(columns)] for c in range(chans)], axis=1))
        names.append(name)

    for size in (1, 2, 3, 4, 255, 256, 257):
        add('size%d' % size, [values((size, ), dtype, seed * 1000 + size * 3 + c) for c in range(3)])
    if dtype == 'u8':
        add('equal', [[77] * 10])
        add('pair-254-255', [[0, 254, 255, 255], [3, 254, 255, 255], [254, 254, 255, 255]])
        add('pair-0-255', [[0, 0, 255, 255], [0, 0, 255, 255, ][::-1], [255, 0, 255, 0]])
    else:
        add('equal', [[0.75] * 10])
        add('neg-zeros', [[-0.0] * 5])
        add('pos-zeros', [[0.0] * 6])
        add('mixed-zeros', [[0.0, -0.0, -0.0, 0.0]])
        add('straddle-even', [[-2, -1, 1, 2], [-2, -1e-300 if dtype == 'f64' else -1e-40, 3, 4], [-1, -0.0, 0.0, 5]])
        add('straddle-odd', [[-1, 0, 1], [-1, -0.0, 1], [-3, -2, 1]])
        big = np.finfo(ft).max
        add('pair-overflow', [[1, big, big, big], [-1, -big, -big, -big], [0, 3e38 if dtype == 'f32' else 1.7e308] * 2])
        if dtype == 'f32':
            a = np.nextafter(np.float32(1), np.float32(2))
            b = np.nextafter(a, np.float32(2))
            assert np.float64((a + b) / np.float32(2)) != (np.float64(a) + np.float64(b)) / 2
            add('pair-adjacent', [[-5, a, b, 7], [-5, -b, -a, 7], [a, b, a, b]])
            add('pair-3e38', [[1, 3e38, 3e38, 3.1e38]])
    used = sum(len(s) for s in segs)
    assert used < n
    add('filler', [values((n - used, ), dtype, seed * 1000 + 999 + c) for c in range(3)])
    lab = np.concatenate([np.full(len(s), k) for k, s in enumerate(segs)])
    where = rng.permutation(n)
    arr = np.empty((n, chans), dtype=ft)
    seg = np.empty(n, dtype=np.int32)
    arr[where] = np.concatenate(segs)
    seg[where] = lab
    return arr.reshape(shape if volume else shape + (3, )), seg.reshape(shape), len(segs), names


# ---- the median cases --------------------------------------------------------------------------------------------------------
#: element counts on both sides of the two thresholds of rocPRIM's radix sort (see tests/test_gpu_median_reference.py)
REGIME_SMALL = [('regime-%dx%d-%s' % (h, w, d), (h, w), d) for h, w in ((32, 32), (25, 41)) for d in ('u8', 'f32', 'f64')]
REGIME_LARGE = [('regime-%dx%d-%s' % (h, w, d), (h, w), d) for h, w in ((1024, 1024), (1024, 1025)) for d in ('u8', 'f64')]
REGIME_LARGE.append(('regime-5x512x410-f32', (5, 512, 410), 'f32'))
LABEL_COUNTS = (1, 2, 3, 4, 255, 256, 257, 65536, 65537)
LABEL_SHAPE = (300, 300)
IDENTITY_SHAPES = [(48, 64), (2, 40, 48)]
CRAFTED = [('crafted-u8', 'u8', (29, 31)), ('crafted-f32', 'f32', (29, 31)), ('crafted-f64', 'f64', (29, 31)),
           ('crafted-vol-f32', 'f32', (2, 15, 30)), ('crafted-vol-f64', 'f64', (2, 15, 30))]


def _full(shape, dtype, seed):
    return values(shape if len(shape) == 3 else shape + (3, ), dtype, seed)


@functools.lru_cache(maxsize=None)
def median_case(name):
    """-> (array, label map, n_labels); the arrays are shared between the tests and read-only"""
    out = None
    for seed, (nm, shape, dtype) in enumerate(REGIME_SMALL + REGIME_LARGE):
        if nm == name:
            out = (_full(shape, dtype, 10 + seed), ) + block_labels(shape, 10 + seed)
    if name.startswith('labels-K'):
        k = int(name[len('labels-K'):])
        out = (_full(LABEL_SHAPE, 'f64', 40), spread_labels(LABEL_SHAPE, k, 41), k)
    elif name == 'labels-trailing':                      # n_labels = max + 1 + 70: the trailing labels have no pixel
        out = (_full(LABEL_SHAPE, 'f64', 40), spread_labels(LABEL_SHAPE, 257, 41), 257 + 70)
    elif name == 'labels-identity':                      # K = n: every pixel is its own label
        out = (_full((48, 64), 'f64', 42), identity_labels((48, 64)), 48 * 64)
    elif name == 'labels-one-big':                       # one label holds every pixel but one: one atomic counter takes them all
        seg = np.zeros(LABEL_SHAPE, dtype=np.int32)
        seg[123, 45] = 1
        out = (_full(LABEL_SHAPE, 'f64', 40), seg, 2)
    elif name.startswith('values-'):                     # values-[inf-]<dtype>-<image|volume>: identity labels
        parts = name.split('-')
        shape = IDENTITY_SHAPES[parts[-1] == 'volume']
        full = shape if len(shape) == 3 else shape + (3, )
        vals = special_values(parts[-2], int(np.prod(full)), 50 + len(name), infinities='inf' in parts)
        out = (vals.reshape(full), identity_labels(shape), int(np.prod(shape)))
    for nm, dtype, shape in CRAFTED:
        if nm == name:
            out = crafted(dtype, shape, 60)[:3]
    if name == 'relabel-first':                          # the session test: a second map with other counts and another n_labels
        out = (_full((25, 41), 'f64', 70), ) + block_labels((25, 41), 70, steps=(2, 7, 9))
    elif name == 'relabel-second':
        out = (_full((25, 41), 'f64', 70), spread_labels((25, 41), 13, 71), 13)
    if out is None:
        raise KeyError(name)
    for a in out[:2]:
        a.setflags(write=False)
    return out


VALUE_CASES = ['values-%s-%s' % (d, k) for d in ('f64', 'f32') for k in ('image', 'volume')]
INF_CASES = ['values-inf-%s-%s' % (d, k) for d in ('f64', 'f32') for k in ('image', 'volume')]
LABEL_CASES = ['labels-K%d' % k for k in LABEL_COUNTS] + ['labels-trailing', 'labels-identity', 'labels-one-big']
SMALL_MEDIAN_CASES = ([c[0] for c in REGIME_SMALL] + LABEL_CASES + VALUE_CASES + INF_CASES + [c[0] for c in CRAFTED]
                      + ['relabel-first', 'relabel-second'])
LARGE_MEDIAN_CASES = [c[0] for c in REGIME_LARGE]


# ---- the median reference ----------------------------------------------------------------------------------------------------
def _columns(arr, seg):
    arr, seg = np.asarray(arr), np.asarray(seg)
    return arr.reshape(seg.size, -1), seg.ravel()


def median_loop(arr, seg, n_labels):
    """np.median of the values of each label and channel, taken in the image's dtype, widened to float64; NaN without pixels"""
    cols, flat = _columns(arr, seg)
    order = np.argsort(flat, kind='stable')
    counts = np.bincount(flat, minlength=n_labels)
    ends = np.cumsum(counts)
    out = np.full((n_labels, cols.shape[1]), np.nan)
    with np.errstate(over='ignore', invalid='ignore'):
        for k in np.flatnonzero(counts):
            members = cols[order[ends[k] - counts[k]:ends[k]]]
            for c in range(cols.shape[1]):
                out[k, c] = np.median(members[:, c])
    return out if np.ndim(arr) > np.ndim(seg) else out[:, 0]


def median_vectorised(arr, seg, n_labels):
    """the same by one ``np.lexsort`` per channel: the two middle elements and their mean in the image's dtype (uint8: float64)"""
    cols, flat = _columns(arr, seg)
    work = np.float32 if cols.dtype == np.float32 else np.float64
    counts = np.bincount(flat, minlength=n_labels)
    first = np.cumsum(counts) - counts
    some = counts > 0
    out = np.full((n_labels, cols.shape[1]), np.nan)
    with np.errstate(over='ignore', invalid='ignore'):
        for c in range(cols.shape[1]):
            ranked = cols[:, c][np.lexsort((cols[:, c], flat))].astype(work)
            lo, hi = ranked[first[some] + (counts[some] - 1) // 2], ranked[first[some] + counts[some] // 2]
            # np.mean itself, so that whatever it does to a pair or a single value is done here (it sums from +0.0: -0.0 -> +0.0)
            out[some, c] = np.where(counts[some] % 2 == 1, np.mean(lo[:, None], axis=1), np.mean(np.stack([lo, hi], axis=1), axis=1))
    return out if np.ndim(arr) > np.ndim(seg) else out[:, 0]


def mixed_zero_segments(arr, seg, n_labels):
    """[label, channel]: the segment holds zeros of both signs -- numpy's partition does not define which one a median of 0 is"""
    cols, flat = _columns(arr, seg)
    if cols.dtype == np.uint8:
        mixed = np.zeros((n_labels, cols.shape[1]), dtype=bool)
    else:
        zero, neg = cols == 0, np.signbit(cols)
        mixed = np.stack([(np.bincount(flat, zero[:, c] & neg[:, c], n_labels) > 0) & (np.bincount(flat, zero[:, c] & ~neg[:, c], n_labels) > 0)
                          for c in range(cols.shape[1])], axis=1)
    return mixed if np.ndim(arr) > np.ndim(seg) else mixed[:, 0]


def median_mismatches(got, ref, mixed_zero=None):
    """indices at which ``got`` is not ``ref`` bit for bit: NaN positions first, then the int64 views everywhere else; the sign of a
    zero counts only where the segment has zeros of one sign"""
    got, ref = np.ascontiguousarray(got, dtype=np.float64), np.ascontiguousarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    nan_got, nan_ref = np.isnan(got), np.isnan(ref)
    differ = got.view(np.int64) != ref.view(np.int64)
    if mixed_zero is not None:
        differ &= ~(mixed_zero & (got == 0) & (ref == 0))
    return np.argwhere((nan_got != nan_ref) | (differ & ~nan_got & ~nan_ref))


def describe(bad, got, ref):
    i = tuple(bad[0])
    return '%d entries differ, first %r: got %r, numpy %r' % (len(bad), i, np.asarray(got)[i], np.asarray(ref)[i])


# ---- the gradient reference --------------------------------------------------------------------------------------------------
def as_planes(arr, volume):
    """[planes][H][W] view: the slices of a volume, the channels of an image"""
    return np.asarray(arr) if volume else np.moveaxis(np.asarray(arr), -1, 0)


def gradient_image(arr, volume):
    """per plane np.sum(np.gradient(plane), axis=0) stored into an array of the image's dtype, as the reference's descriptors do"""
    arr = np.asarray(arr)
    out = np.zeros_like(arr)
    with np.errstate(invalid='ignore'):
        if volume:
            for z, plane in enumerate(arr):
                out[z] = np.sum(np.gradient(plane), axis=0)
        else:
            for c in range(arr.shape[-1]):
                out[..., c] = np.sum(np.gradient(arr[..., c]), axis=0)
    return out


def gradient_sums(arr, volume):
    """the float64 sums before they are stored (uint8 images)"""
    planes = as_planes(arr, volume).astype(np.float64)
    sums = np.stack([np.sum(np.gradient(p), axis=0) for p in planes])
    return sums if volume else np.moveaxis(sums, 0, -1)


def uint8_by_rule(sums):
    """the stored uint8 value by rule: the float64 sum truncated towards zero, then modulo 256"""
    return (np.trunc(sums).astype(np.int64) % 256).astype(np.uint8)


def gradient_mean_reference(grad, seg, n_labels):
    """(mean in longdouble [K(, C)], counts): the float32-cast gradient values summed in longdouble per label; 0 without pixels"""
    cols, flat = _columns(grad, seg)
    cols = cols.astype(np.float32).astype(LD)
    counts = np.bincount(flat, minlength=n_labels)
    order = np.argsort(flat, kind='stable')
    some = np.flatnonzero(counts)
    starts = (np.cumsum(counts) - counts)[some]
    mean = np.zeros((n_labels, cols.shape[1]), dtype=LD)
    mean[some] = np.add.reduceat(cols[order], starts, axis=0) / counts[some, None].astype(LD)
    return (mean if np.ndim(grad) > np.ndim(seg) else mean[:, 0]), counts


def gradient_bound(n_pixels, maxabs):
    """B of the segmented mean (csrc/stats.hip), n the pixel count of the whole image or volume; maxabs as the library takes it:
    255 for uint8, the largest magnitude of the gradient image for float images, 4 mul on the response path"""
    return fixed_point_bound(n_pixels, maxabs)[0]


def image_maxabs(grad):
    grad = np.asarray(grad)
    return 255.0 if grad.dtype == np.uint8 else float(np.abs(grad.astype(np.float64)).max())


def mean_deviation(got, ref, counts, bound):
    """(worst |got - ref| / (1e-12 |ref| + B), indices outside the tolerance, labels without pixels that are not exactly 0)"""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    err = np.abs(got.astype(LD) - ref)
    tol = LD(RTOL) * np.abs(ref) + LD(bound)
    empty = counts == 0
    return float((err / tol).max()), np.argwhere(~(err <= tol)), np.argwhere(got[empty] != 0)


def gradient_pattern(shape, dtype, seed):
    """image H x W x 3 / volume D x H x W for the per-pixel test.  Floats: one pattern, the channels at 1, 1e3 and 1e-3 times it
    (the slices at 1, 1e3, 1e-3, 30).  uint8: one pattern of {0, 1, 254, 255} (differences of 0, +-1 and +-253 .. +-255: sums of
    +-0.5, +-127.5, +-255.5 on the interior and the edges) whose first and last corner give +-510 in the first channel / slice,
    with 1, 40 and 200 added modulo 256 (slices: 1, 40, 200, 90)"""
    volume = len(shape) == 3
    h, w = shape[-2:]
    rng = _rng(seed, *shape)
    planes = shape[0] if volume else 3
    if dtype == 'u8':
        pat = rng.choice(np.array([0, 1, 254, 255]), (h, w))
        pat[0, 0] = pat[-1, -1] = 255
        pat[0, 1] = pat[1, 0] = pat[-1, -2] = pat[-2, -1] = 254
        out = np.stack([(pat + (1, 40, 200, 90)[p % 4]) % 256 for p in range(planes)]).astype(np.uint8)
    else:
        pat = rng.standard_normal((h, w))
        out = np.stack([pat * (1.0, 1e3, 1e-3, 30.0)[p % 4] for p in range(planes)]).astype(DTYPES[dtype])
    return np.ascontiguousarray(out if volume else np.moveaxis(out, 0, -1))


PIXEL_IMAGE_SHAPES = [(2, 2), (2, 3), (3, 2), (2, 257), (257, 2), (17, 19)]
PIXEL_VOLUME_SHAPES = [(3, 2, 2), (4, 9, 11), (1, 9, 11)]
#: sums a uint8 pattern must produce so that both the truncation and the wrap of the cast are exercised
UINT8_SUMS = (0.5, -0.5, 127.5, -127.5, 255.5, -255.5, 510.0, -510.0)
MEAN_CASES = [((67, 93), d) for d in ('u8', 'f32', 'f64')] + [((5, 31, 40), d) for d in ('u8', 'f32', 'f64')]
MEAN_LARGE = ((1024, 1025), 'f32')


@functools.lru_cache(maxsize=None)
def mean_case(shape, dtype):
    """(array, label map, n_labels) of the per-label gradient mean: noise on blocks of 9 x 13 (23 x 23 at the large size)"""
    big = int(np.prod(shape)) > 100000
    arr = values(shape if len(shape) == 3 else shape + (3, ), dtype, 80)
    if dtype != 'u8':
        arr = (arr * arr.dtype.type(40)).astype(arr.dtype)
    seg, nb = block_labels(shape, 81, steps=(2, 23, 23) if big else (2, 9, 13))
    arr.setflags(write=False)
    seg.setflags(write=False)
    return arr, seg, nb


# ---- the response path -------------------------------------------------------------------------------------------------------
def response_references(resp, seg, n_labels, mul, div, volume):
    """from the response planes ([3][H][W]; a volume: [D][H][W]): numpy's median of (resp * mul) / div per label (and channel), the
    longdouble mean of the gradient of the normalised planes (each plane differenced on its own), its counts, and B from 4 mul"""
    with np.errstate(over='ignore', invalid='ignore'):
        v = (np.asarray(resp, dtype=np.float64) * mul) / div
    arr = v if volume else np.ascontiguousarray(np.moveaxis(v, 0, -1))
    median = median_vectorised(arr, seg, n_labels)
    mixed = mixed_zero_segments(arr, seg, n_labels)
    mean, counts = gradient_mean_reference(gradient_image(arr, volume), seg, n_labels)
    return median, mixed, mean, counts, gradient_bound(seg.size, 4.0 * mul)


# ---- numpy models of the device's evaluation, with one defect or none ---------------------------------------------------------
SIGN = np.uint64(1) << np.uint64(63)
MEDIAN_DEFECTS = ('sign', 'label16', 'unstable', 'inclusive', 'upper', 'f32-in-f64', 'stale-counts', 'neg-zero')
GRADIENT_DEFECTS = ('end-y0', 'end-y1', 'end-x0', 'end-x1', 'next-row', 'next-plane', 'u8-saturate', 'u8-floor')


def order_key(v, defect=None):
    b = np.ascontiguousarray(v, dtype=np.float64).view(np.uint64)
    if defect == 'sign':                                 # negative keys not inverted: they rank below the others, backwards
        return b ^ SIGN
    return np.where(b & SIGN != 0, ~b, b | SIGN)


def key_value(k, defect=None):
    if defect == 'sign':
        return (k ^ SIGN).view(np.float64)
    return np.where(k & SIGN != 0, k & ~SIGN, ~k).view(np.float64)


def model_median(arr, seg, n_labels, norm=None, defect=None, previous=None):
    """csrc/median.hip in numpy: order keys of the values widened to float64, a stable sort by key, a stable sort by the low
    ``label_bits`` bits of the label, the exclusive scan of the counts, the pick of the middle one or two and their mean summed from +0.0 as np.mean does
    (``norm``: (mul, div) applied to the picked values).  ``previous``: the label map of an earlier call on the session ('stale-counts')"""
    cols, flat = _columns(arr, seg)
    K = int(n_labels)
    f32 = cols.dtype == np.float32
    lab = np.where((flat < 0) | (flat >= K), K, flat).astype(np.int64)
    label_bits = 1
    while (1 << label_bits) <= K:
        label_bits += 1
    if defect == 'label16':
        label_bits = min(label_bits, 16)
    counts = np.bincount(lab, minlength=K + 1)[:K]
    if defect == 'stale-counts':
        counts = np.bincount(np.asarray(previous).ravel(), minlength=K)[:K]
    offsets = np.cumsum(counts) if defect == 'inclusive' else np.cumsum(counts) - counts
    zero = -0.0 if defect == 'neg-zero' else 0.0         # the sum np.mean starts from (-0.0: the picked element as it is)
    n = flat.size
    out = np.full((K, cols.shape[1]), np.nan)
    with np.errstate(over='ignore', invalid='ignore'):
        for c in range(cols.shape[1]):
            key_a = order_key(cols[:, c].astype(np.float64), defect)
            by_value = np.argsort(key_a, kind='stable')
            key_b, lab_b = key_a[by_value], lab[by_value]
            if defect == 'unstable':                     # the labels sorted from the unsorted keys
                key_b, lab_b = key_a, lab
            ranked = key_b[np.argsort(lab_b & ((1 << label_bits) - 1), kind='stable')]
            some = counts > 0
            mid = offsets[some] + counts[some] // 2
            a = key_value(ranked[np.minimum(mid - 1 + counts[some] % 2, n - 1)], defect)
            b = key_value(ranked[np.minimum(mid, n - 1)], defect)
            if norm is not None:
                a, b = (a * norm[0]) / norm[1], (b * norm[0]) / norm[1]
            if defect == 'upper':
                m = b
            elif f32 and defect != 'f32-in-f64':
                m = (((np.float32(zero) + a.astype(np.float32)) + b.astype(np.float32)) / np.float32(2)).astype(np.float64)
            else:
                m = ((zero + a) + b) / 2.0
            out[some, c] = np.where(counts[some] % 2 == 1, zero + b, m)
    return out if np.ndim(arr) > np.ndim(seg) else out[:, 0]


def model_gradient(src, S, H, W, C, norm=None, defect=None):
    """k_gradient_image over the flat array ([S][H][W][C]; C = 3, S = 1: an interleaved image; C = 1: the slices of a volume or the
    planes of a response), one element per thread; reads past the array (defects only) are clamped to it"""
    src = np.ascontiguousarray(src)
    dtype = src.dtype
    flat = src.ravel()
    F = np.float32 if dtype == np.float32 else np.float64
    total = S * H * W * C
    assert flat.size == total
    i = np.arange(total)
    px = i // C
    x, y = px % W, (px // W) % H
    row, col = W * C, C

    def ld(j):
        v = flat[np.clip(j, 0, total - 1)]
        if norm is not None:
            return ((v.astype(np.float64) * norm[0]) / norm[1]).astype(F)
        return v.astype(F)

    def along(pos, last, step, name, spill):
        if last == 0:
            raise ValueError('Shape of array too small to calculate a numerical gradient')
        first_div = F(2) if defect == name + '0' else F(1)
        last_div = F(2) if defect == name + '1' else F(1)
        centre = (ld(i + step) - ld(i - step)) / F(2)
        g = np.where(pos == 0, (ld(i + step) - ld(i)) / first_div, centre)
        if defect != spill:                              # (spill: the last element takes the interior branch and reads past its line)
            g = np.where(pos == last, (ld(i) - ld(i - step)) / last_div, g)
        return g.astype(F)

    with np.errstate(invalid='ignore', over='ignore'):
        g = along(y, H - 1, row, 'end-y', 'next-plane') + along(x, W - 1, col, 'end-x', 'next-row')
        if dtype == np.uint8:
            if defect == 'u8-saturate':
                out = np.trunc(np.clip(g, 0, 255)).astype(np.uint8)
            elif defect == 'u8-floor':
                out = (np.floor(g).astype(np.int64) % 256).astype(np.uint8)
            else:
                out = (np.trunc(g).astype(np.int64) % 256).astype(np.uint8)
        else:
            out = g.astype(dtype)
    return out.reshape(src.shape)


def model_gradient_of(arr, volume, norm=None, defect=None):
    """``model_gradient`` of an H x W x 3 image or a D x H x W volume (``norm``: planes [P][H][W] of a response)"""
    arr = np.asarray(arr)
    if volume or norm is not None:
        return model_gradient(arr, arr.shape[0], arr.shape[1], arr.shape[2], 1, norm, defect)
    return model_gradient(arr, 1, arr.shape[0], arr.shape[1], 3, norm, defect)


def model_mean(grad, seg, n_labels):
    """the segmented mean of the float32-staged values in float64 (what the device computes up to its fixed-point grid)"""
    cols, flat = _columns(grad, seg)
    cols = cols.astype(np.float32).astype(np.float64)
    counts = np.bincount(flat, minlength=n_labels)
    sums = np.stack([np.bincount(flat, cols[:, c], n_labels) for c in range(cols.shape[1])], axis=1)
    mean = np.where(counts[:, None] > 0, sums / np.maximum(counts, 1)[:, None], 0.0)
    return mean if np.ndim(grad) > np.ndim(seg) else mean[:, 0]
