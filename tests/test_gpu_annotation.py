"""The annotation calls on the device (csrc/annotation.hip) against the host statements of pyimsegm_amd/annotation.py, byte for byte;
the nearest-valid transform against ``nearest_valid_host``, the brute-force statement of its tie rule.  Every call is made twice.
Refusals are ordinary error returns, checked on the host before any launch or read from a flag before the download."""
import os

import numpy as np
import pytest

import annotation_cases as cases

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope='module')
def hip():
    from pyimsegm_amd import _hip
    return _hip


@pytest.fixture(scope='module')
def ann():
    from pyimsegm_amd import annotation
    return annotation


@pytest.fixture(scope='module')
def golden():
    return dict(np.load(os.path.join(HERE, 'golden', 'annotation.npz')))


def twice(call):
    first, second = call(), call()
    if isinstance(first, tuple):
        assert all(np.array_equal(a, b) for a, b in zip(first, second))
    elif isinstance(first, np.ndarray):
        assert np.array_equal(first, second) and first.dtype == second.dtype
    else:
        assert first == second
    return first


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)


def random_table(rng, count):
    """`count` distinct colours, the first ones with components 0 and 255"""
    keys = rng.choice(1 << 24, size=count, replace=False)
    keys[:min(count, 2)] = [0xff00ff, 0x000000][:min(count, 2)]
    keys = list(dict.fromkeys(int(k) for k in keys))
    return [(k >> 16, (k >> 8) & 255, k & 255) for k in keys]


# ---------------------------------------------------------------------------------------------------
# match and paint: the 4-pixel load and its tail, table sizes, ties, duplicates, no uint8 wrap
# ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('n_pixels', [1, 3, 4, 5, 255, 256, 257])
@pytest.mark.parametrize('n_colors', [1, 256])
def test_match_and_paint_sizes(hip, ann, n_pixels, n_colors):
    rng = np.random.RandomState(n_pixels * 7 + n_colors)
    colors = random_table(rng, n_colors)
    assert len(colors) == n_colors                     # (no colour of the draw fell on one of the two fixed ones)
    table = np.array(colors, dtype=np.uint8)
    picks = rng.randint(0, len(colors), n_pixels)
    image = table[picks].reshape(1, n_pixels, 3).copy()
    noisy = image.copy()
    noisy[0, ::3] = rng.randint(0, 256, (len(range(0, n_pixels, 3)), 3))
    labels = rng.permutation(1000)[:len(colors)].astype(np.int32)
    # exact
    found, missed = twice(lambda: hip.annot_match(noisy, table, labels))
    expected, converted = ann.colors_to_labels_host(noisy, colors, labels)
    unmatched = ~(noisy[:, :, None, :] == table[None, None]).all(axis=3).any(axis=2)
    assert missed == int(unmatched.sum()) == n_pixels - converted
    assert found.dtype == np.int32 and np.array_equal(found[~unmatched], expected[~unmatched]) and (found[unmatched] == -1).all()
    # nearest, index and colour
    index = twice(lambda: hip.annot_match(noisy, table, mode=hip.ANNOT_MATCH_NEAREST))
    assert np.array_equal(index.ravel(), ann.nearest_color_index_host(noisy, colors))
    colour = twice(lambda: hip.annot_match(noisy, table, mode=hip.ANNOT_MATCH_NEAREST_COLOR))
    assert colour.dtype == np.uint8 and np.array_equal(colour, table[index])
    # paint, with a negative first label
    segm = (picks - 7).astype(np.int32).reshape(1, n_pixels)
    painted = twice(lambda: hip.annot_paint(segm, -7, table))
    assert painted.dtype == np.uint8 and np.array_equal(painted, ann.labels_to_colors_host(segm, -7, table))
    # the public functions
    assert same(twice(lambda: ann.image_color_2_labels(noisy, colors, on='device')), ann.image_color_2_labels(noisy, colors, on='host'))
    assert same(twice(lambda: ann.quantize_image_nearest_color(noisy, colors, on='device')),
                ann.quantize_image_nearest_color(noisy, colors, on='host'))
    lut = {int(i) - 7: clr for i, clr in enumerate(colors)}
    assert same(twice(lambda: ann.convert_img_labels_to_colors(segm, lut, on='device')), ann.convert_img_labels_to_colors(segm, lut, on='host'))
    lut = {int(i) + 3: clr for i, clr in enumerate(colors)}
    assert same(twice(lambda: ann.convert_img_colors_to_labels(image, lut, on='device')), ann.convert_img_colors_to_labels(image, lut, on='host'))
    if unmatched.any():
        with pytest.raises(ValueError):
            ann.convert_img_colors_to_labels(noisy, lut, on='device')


def test_match_ties_duplicates_and_extremes(hip, ann):
    # (10, 10, 10) is 3 away from both of the first two colours: the first wins; 0 against 255: the distance is 765, not 765 mod 256
    colors = [(10, 10, 13), (13, 10, 10), (0, 0, 0), (255, 255, 255), (13, 10, 10), (0, 1, 0)]
    table = np.array(colors, dtype=np.uint8)
    image = np.array([[(10, 10, 10), (255, 255, 255), (0, 0, 0), (13, 10, 10), (254, 255, 255), (1, 0, 0), (13, 10, 11)]], dtype=np.uint8)
    index = twice(lambda: hip.annot_match(image, table, mode=hip.ANNOT_MATCH_NEAREST))
    assert index.tolist() == [[0, 3, 2, 1, 3, 2, 1]]
    assert np.array_equal(index.ravel(), ann.nearest_color_index_host(image, colors))
    # black is 765 from white and 6 from (2, 2, 2); with differences that wrap in uint8 white would be 3 away
    black = np.zeros((1, 5, 3), dtype=np.uint8)
    assert twice(lambda: hip.annot_match(black, np.array([(255, 255, 255), (2, 2, 2)], dtype=np.uint8), mode=hip.ANNOT_MATCH_NEAREST)).tolist() == [[1] * 5]
    # a duplicated colour: the last entry's label
    found, missed = twice(lambda: hip.annot_match(image, table, np.arange(10, 16, dtype=np.int32)))
    assert found.tolist() == [[-1, 13, 12, 14, -1, -1, -1]] and missed == 4
    expected, _ = ann.colors_to_labels_host(image, colors, range(10, 16))
    assert np.array_equal(found[found >= 0], expected[found >= 0])
    with pytest.raises(hip.HipError):
        hip.annot_match(image, table, np.array([0, 1, -1, 2, 3, 4], dtype=np.int32))


def test_paint_refuses_a_label_without_a_colour(hip, ann):
    table = np.array([(1, 2, 3), (4, 5, 6), (7, 8, 9)], dtype=np.uint8)
    for segm, present in ((np.array([[0, 1, 2, 3, 0]], dtype=np.int32), None), (np.array([[0, 1, 2, -1, 0]], dtype=np.int32), None),
                          (np.array([[0, 1, 2, 1, 0]], dtype=np.int32), [1, 0, 1])):
        out = np.full(segm.shape + (3, ), 77, dtype=np.uint8)
        for _ in range(2):
            with pytest.raises(hip.HipError):
                hip.annot_paint(segm, 0, table, present, out=out)
            assert (out == 77).all()
    assert hip.annot_paint(np.array([[0, 2, 2]], dtype=np.int32), 0, table, [1, 0, 1]).tolist() == [[[1, 2, 3], [7, 8, 9], [7, 8, 9]]]
    with pytest.raises(ValueError):
        ann.convert_img_labels_to_colors(np.array([[0, 1, 2]]), {0: (1, 2, 3), 2: (7, 8, 9)}, on='device')
    # a gap in the label range that the map does not use
    lut = {0: (1, 2, 3), 2: (7, 8, 9)}
    assert same(ann.convert_img_labels_to_colors(np.array([[0, 2, 2]]), lut, on='device'),
                ann.convert_img_labels_to_colors(np.array([[0, 2, 2]]), lut, on='host'))


# ---------------------------------------------------------------------------------------------------
# histogram
# ---------------------------------------------------------------------------------------------------

def test_hist_one_colour_heaviest_contention(hip, ann):
    image = np.empty((300, 300, 3), dtype=np.uint8)
    image[...] = (9, 200, 31)
    keys, counts = twice(lambda: hip.annot_color_hist(image))
    assert keys.tolist() == [(9 << 16) | (200 << 8) | 31] and counts.tolist() == [90000]
    assert twice(lambda: np.array(ann.unique_image_colors(image, on='device'))).tolist() == [[9, 200, 31]]


def test_hist_all_distinct_and_extreme_keys(hip, ann):
    rng = np.random.RandomState(4)
    keys_in = np.concatenate([[0x000000, 0xffffff], 1 + rng.choice((1 << 24) - 2, size=64 * 64 - 2, replace=False)])[rng.permutation(64 * 64)]
    image = np.stack([keys_in >> 16, (keys_in >> 8) & 255, keys_in & 255], axis=1).astype(np.uint8).reshape(64, 64, 3)
    ref_keys, ref_counts = ann.color_counts_host(image)
    for capacity in (None, 4096):                      # (room for one colour per pixel; exactly as many as there are)
        keys, counts = twice(lambda: hip.annot_color_hist(image, capacity=capacity))
        assert keys.dtype == np.uint32 and np.array_equal(keys, ref_keys) and np.array_equal(counts, ref_counts)
        assert keys[0] == 0 and keys[-1] == 0xffffff and len(keys) == 64 * 64 and (counts == 1).all()
    for _ in range(2):                                 # (one colour too many for the arrays: an error, and the next call is sound)
        with pytest.raises(ValueError):
            hip.annot_color_hist(image, capacity=4095)
    assert np.array_equal(hip.annot_color_hist(image)[0], ref_keys)
    assert twice(lambda: ann.unique_image_colors(image, on='device')) == ann.unique_image_colors(image, on='host')


@pytest.mark.parametrize('shape', [(1, 1), (1, 3), (1, 5), (7, 37), (64, 65)])
def test_hist_runs_and_tails(hip, ann, shape):
    # runs of every length from 1 on, a pixel count that is no multiple of 4 and of 64, runs that cross lanes and waves
    rng = np.random.RandomState(shape[0] * 100 + shape[1])
    n = shape[0] * shape[1]
    lengths = rng.randint(1, 40, n)
    picks = np.repeat(rng.randint(0, 5, n), lengths)[:n]
    table = np.array([(0, 0, 0), (255, 255, 255), (1, 0, 0), (0, 0, 1), (0, 1, 0)], dtype=np.uint8)
    image = table[picks].reshape(shape + (3, ))
    keys, counts = twice(lambda: hip.annot_color_hist(image))
    ref_keys, ref_counts = ann.color_counts_host(image)
    assert np.array_equal(keys, ref_keys) and np.array_equal(counts, ref_counts)


def test_frequent_colours_threshold_at_a_count(ann):
    image, _, _, _ = cases.painted('small_default4')
    host = ann.image_frequent_colors(image, on='host')
    assert ann.image_frequent_colors(image, on='device') == host and ann.image_frequent_colors(image, on='device') == host
    count = sorted(host.values())[len(host) // 2]
    at = float(count) / float(image.shape[0] * image.shape[1])
    found = ann.image_frequent_colors(image, at, on='device')
    assert found == ann.image_frequent_colors(image, at, on='host') and count in found.values()
    assert all(type(v) is int for k in found for v in k + (found[k], ))


# ---------------------------------------------------------------------------------------------------
# nearest valid pixel
# ---------------------------------------------------------------------------------------------------

def check_nearest(hip, ann, labels):
    labels = np.ascontiguousarray(labels, dtype=np.int32)
    result = twice(lambda: hip.annot_nearest_valid(labels))
    expected = ann.nearest_valid_host(labels, labels != -1, rows_per_chunk=max(1, (1 << 22) // max(1, labels.shape[1] * int((labels != -1).sum()))))
    assert result.dtype == np.int32 and np.array_equal(result, expected)
    return result


@pytest.mark.parametrize('height', [1, 2, 5])
@pytest.mark.parametrize('width', [1, 63, 64, 65, 255, 256, 257])
def test_nearest_valid_sizes(hip, ann, height, width):
    rng = np.random.RandomState(height * 1000 + width)
    labels = rng.randint(0, 6, (height, width))
    labels[rng.rand(height, width) < 0.8] = -1
    labels[rng.randint(height), rng.randint(width)] = 3
    check_nearest(hip, ann, labels)


def test_nearest_valid_long_search_from_a_corner(hip, ann):
    for corner in ((0, 0), (7, 699), (0, 699), (7, 0)):
        labels = np.full((8, 700), -1)
        labels[corner] = 5
        assert (check_nearest(hip, ann, labels) == 5).all()


def test_nearest_valid_four_way_ties(hip, ann):
    for shape in ((9, 9), (5, 257), (8, 64)):
        labels = np.full(shape, -1)
        labels[0, 0], labels[0, -1], labels[-1, 0], labels[-1, -1] = 1, 2, 3, 4
        result = check_nearest(hip, ann, labels)
        if shape == (9, 9):
            assert result[4, 4] == 1 and result[0, 4] == 1 and result[4, 0] == 1 and result[4, 8] == 2 and result[8, 4] == 3


def test_nearest_valid_checkerboard_identity_and_other_labels(hip, ann):
    yy, xx = np.mgrid[0:21, 0:67]
    board = np.where((yy + xx) % 2 == 0, 1 + (yy // 2 + xx // 2) % 2, -1)
    check_nearest(hip, ann, board)
    full = np.random.RandomState(2).randint(-5, 5, (13, 70))
    full[full == -1] = -2                              # (every value but -1 is a label: negative ones too)
    assert np.array_equal(check_nearest(hip, ann, full), full)
    sparse = np.where(np.random.RandomState(3).rand(13, 70) < 0.1, full, -1)
    sparse[4, 4] = -7
    check_nearest(hip, ann, sparse)


def test_nearest_valid_refuses_a_map_without_a_valid_pixel(hip, ann):
    labels = np.full((6, 70), -1, dtype=np.int32)
    out = np.full((6, 70), 55, dtype=np.int32)
    for _ in range(2):
        with pytest.raises(hip.HipError):
            hip.annot_nearest_valid(labels, out=out)
        assert (out == 55).all()
    # the public functions do what their host statements do: NaN everywhere, and an index no colour table has
    nans = np.full((4, 5), np.nan)
    assert np.isnan(ann.image_inpaint_pixels(nans, ~np.isnan(nans), on='device')).all()
    with pytest.raises(IndexError), np.errstate(invalid='ignore'):
        ann.quantize_image_nearest_pixel(np.full((4, 5, 3), 7, dtype=np.uint8), [(0, 0, 0), (1, 1, 1)], on='device')


@pytest.mark.parametrize('name', sorted(cases.PAINTED))
def test_seeded_cases_and_the_composition(hip, ann, golden, name):
    image, colors, segm, kept = cases.painted(name)
    ambiguous = cases.ambiguous_mask(segm, kept)
    assert ambiguous.mean() <= cases.AMBIGUOUS_CAP
    labels = np.where(kept, segm, -1)
    check_nearest(hip, ann, labels)
    floats = np.where(kept, segm, np.nan)
    inpainted = twice(lambda: ann.image_inpaint_pixels(floats, kept, on='device'))
    assert same(inpainted, ann.nearest_valid_host(floats, kept))
    assert np.array_equal(inpainted[~ambiguous], golden[name + '_inpaint'][~ambiguous])
    # the composition: the recorded reference outside the ambiguous mask, its own host composition everywhere
    quantized = twice(lambda: ann.quantize_image_nearest_pixel(image, colors, on='device'))
    recorded = golden[name + '_nearest_pixel']
    assert quantized.dtype == recorded.dtype and np.array_equal(quantized[~ambiguous], recorded[~ambiguous])
    exact = ann.exact_color_index_host(image, colors)
    composed = np.asarray(colors)[ann.nearest_valid_host(exact, ~np.isnan(exact)).astype(int)]
    assert same(quantized, composed)
    raw = twice(lambda: hip.annot_quantize_nearest_pixel(image, np.array(colors, dtype=np.uint8)))
    assert raw.dtype == np.uint8 and np.array_equal(raw, composed)
    # the other public functions on the same image
    assert same(twice(lambda: ann.image_color_2_labels(image, on='device')), ann.image_color_2_labels(image, on='host'))
    clean, lut, _ = cases.clean(name)
    assert same(twice(lambda: ann.convert_img_colors_to_labels(clean, lut, on='device')), golden[name + '_to_labels'])
    assert same(twice(lambda: ann.convert_img_labels_to_colors(segm, lut, on='device')), golden[name + '_to_colors'])


# ---------------------------------------------------------------------------------------------------
# calls the device does not take: the host statement's result with on=None
# ---------------------------------------------------------------------------------------------------

def test_calls_the_device_does_not_take(hip, ann, monkeypatch):
    def no_device_call(*args, **kwargs):
        raise AssertionError('the device was asked')
    for name in ('annot_match', 'annot_paint', 'annot_color_hist', 'annot_nearest_valid', 'annot_quantize_nearest_pixel'):
        monkeypatch.setattr(hip, name, no_device_call)
    monkeypatch.setattr(ann, 'HOST_BY_DEFAULT', frozenset())
    # float images (the reference's own doctest)
    np.random.seed(0)
    seg = np.random.randint(0, 2, (5, 7))
    img = np.array([(0.2, 0.2, 0.2), (0.9, 0.9, 0.9)])[seg]
    lut = {0: (0.2, 0.2, 0.2), 1: (0.9, 0.9, 0.9)}
    assert same(ann.convert_img_colors_to_labels(img, lut), seg)
    assert same(ann.convert_img_labels_to_colors(seg, lut), img)
    assert same(ann.quantize_image_nearest_color(img, list(lut.values())), img)
    assert same(ann.quantize_image_nearest_pixel(img, list(lut.values())), img)
    # 257 colours
    rng = np.random.RandomState(1)
    colors = random_table(rng, 257)
    image = np.array(colors, dtype=np.uint8)[rng.randint(0, 257, (6, 9))]
    assert same(ann.image_color_2_labels(image, colors), ann.image_color_2_labels(image, colors, on='host'))
    assert same(ann.quantize_image_nearest_pixel(image, colors), ann.quantize_image_nearest_pixel(image, colors, on='host'))
    lut = dict(enumerate(colors))
    assert same(ann.convert_img_colors_to_labels(image, lut), ann.convert_img_colors_to_labels(image, lut, on='host'))
    # a component of 300
    odd = [(0, 0, 0), (300, 0, 0)]
    assert same(ann.image_color_2_labels(image, odd), ann.image_color_2_labels(image, odd, on='host'))
    assert same(ann.quantize_image_nearest_color(image.astype(np.int64), odd), ann.quantize_image_nearest_color(image.astype(np.int64), odd, on='host'))
    wide = image.astype(np.int64) + 100
    assert ann.image_color_2_labels(wide, colors[:5]).tolist() == ann.image_color_2_labels(wide, colors[:5], on='host').tolist()
    # a 2-D image
    gray = rng.randint(0, 3, (6, 9)).astype(np.uint8)
    assert ann.unique_image_colors(gray) == ann.unique_image_colors(gray, on='host') == [(0, 0, 0), (1, 1, 1), (2, 2, 2)]
    assert ann.image_frequent_colors(gray) == ann.image_frequent_colors(gray, on='host')
    # labels the exact match does not take
    assert same(ann.convert_img_colors_to_labels_reverted(image[:1, :1], {colors[0]: -1, tuple(image[0, 0]): -4}),
                np.array([[-4]]))
    with pytest.raises(ValueError):
        ann.image_color_2_labels(image, colors, on='nowhere')


def test_integer_images_of_other_dtypes_go_to_the_device(ann):
    image, colors, _, _ = cases.painted('small_default4')
    wide = image.astype(np.int64)
    assert same(ann.quantize_image_nearest_color(wide, colors, on='device'), ann.quantize_image_nearest_color(wide, colors, on='host'))
    assert same(ann.image_color_2_labels(wide, colors, on='device'), ann.image_color_2_labels(wide, colors, on='host'))
