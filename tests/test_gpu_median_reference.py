"""The per-label 'median' and 'meanGrad' statistics of the device (csrc/median.hip through ``Image2D`` / ``Volume3D``) against numpy at
their sort and plane edges; cases and references in tests/median_cases.py, shown able to catch a defect by
tests/test_median_reference_host.py.

Medians are compared bit for bit with ``np.median`` in the image's dtype.  The gradient image is read per pixel through identity
labels (the mean of one value is float32 of that value); label means are held to the 80-bit sum within 1e-12 |ref| + B, B the
fixed-point bound of csrc/stats.hip.

Sort routes.  ``launch_segment_median`` sorts with ``hipcub::DeviceRadixSort::SortPairs``; rocPRIM
(``rocprim/device/device_radix_sort.hpp``, limits in ``rocprim/device/device_radix_sort_config.hpp``) sorts up to 1024 elements in
one block, up to 1024 * 1024 by its merge sort and anything larger by onesweep.  32 x 32 and 25 x 41 lie on the two sides of the
first limit, 1024 x 1024 and 1024 x 1025 (and the 5 x 512 x 410 volume) on the two sides of the second.  Nothing here asserts
which route ran."""
import numpy as np
import pytest

import median_cases as M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def hip():
    from pyimsegm_amd import _hip
    _hip.default_context()
    return _hip


def session(hip, arr, seg, n_labels):
    volume = np.ndim(arr) == np.ndim(seg)
    return (hip.Volume3D if volume else hip.Image2D)(*seg.shape).upload(arr).set_labels(seg, n_labels)


def device_median(hip, arr, seg, n_labels):
    sess = session(hip, arr, seg, n_labels)
    try:
        return sess.median()
    finally:
        sess.close()


def device_mean_gradient(hip, arr, seg, n_labels):
    sess = session(hip, arr, seg, n_labels)
    try:
        return sess.mean_gradient()
    finally:
        sess.close()


def check_median(hip, name):
    arr, seg, nb = M.median_case(name)
    got = device_median(hip, arr, seg, nb)
    ref = M.median_vectorised(arr, seg, nb)
    bad = M.median_mismatches(got, ref, M.mixed_zero_segments(arr, seg, nb))
    assert bad.size == 0, '%s: %s' % (name, M.describe(bad, got, ref))
    return got, np.bincount(seg.ravel(), minlength=nb)


# ---- median ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', [c[0] for c in M.REGIME_SMALL + M.REGIME_LARGE])
def test_median_on_both_sides_of_the_sort_thresholds(hip, name):
    got, counts = check_median(hip, name)
    assert counts[2] == 0 and np.all(np.isnan(got[2])) and np.any(counts % 2 == 1) and np.any(counts[counts > 0] % 2 == 0)


@pytest.mark.parametrize('name', M.LABEL_CASES)
def test_median_at_the_edges_of_the_label_bits(hip, name):
    got, counts = check_median(hip, name)
    if name == 'labels-trailing':
        assert np.all(np.isnan(got[-70:])) and not np.any(np.isnan(got[:-70]))
    elif name == 'labels-one-big':
        assert counts.tolist() == [M.LABEL_SHAPE[0] * M.LABEL_SHAPE[1] - 1, 1]
    else:
        assert counts.min() >= 1 and counts[-1] >= 1


@pytest.mark.parametrize('name', M.VALUE_CASES)
def test_key_round_trip_of_every_kind_of_value(hip, name):
    """identity labels: the median is the value itself (the sign of a zero apart: np.mean sums from +0.0)"""
    arr, seg, nb = M.median_case(name)
    got, _ = check_median(hip, name)
    flat = arr.reshape(nb, -1).astype(np.float64).reshape(got.shape)
    assert np.array_equal(got, flat) and not np.any(np.signbit(got[got == 0]))


@pytest.mark.parametrize('name', M.INF_CASES)
def test_key_round_trip_of_infinities(hip, name):
    arr, _, _ = M.median_case(name)
    got, _ = check_median(hip, name)
    assert np.isinf(got).sum() == np.isinf(arr).sum() >= 2


@pytest.mark.parametrize('name', [c[0] for c in M.CRAFTED])
def test_median_of_crafted_segments(hip, name):
    check_median(hip, name)


def test_session_state_does_not_leak_between_calls(hip):
    arr, first, nb_first = M.median_case('relabel-first')
    _, second, nb_second = M.median_case('relabel-second')
    other = M.values(arr.shape, 'f64', 72)
    fresh = {}
    for key, (a, s, k) in {'first': (arr, first, nb_first), 'second': (arr, second, nb_second), 'other': (other, second, nb_second)}.items():
        fresh[key] = (device_median(hip, a, s, k), device_mean_gradient(hip, a, s, k))
    assert np.bincount(first.ravel()).tolist() != np.bincount(second.ravel()).tolist() and nb_first != nb_second
    for order in ('median-first', 'gradient-first'):
        sess = session(hip, arr, first, nb_first)
        try:
            assert np.array_equal(sess.median(), fresh['first'][0], equal_nan=True)
            sess.set_labels(second, nb_second)
            assert np.array_equal(sess.median(), fresh['second'][0], equal_nan=True)
            sess.upload(other)
            if order == 'median-first':
                got = (sess.median(), sess.mean_gradient())
            else:
                got = (sess.mean_gradient(), sess.median())[::-1]
            assert np.array_equal(got[0], fresh['other'][0], equal_nan=True), order
            assert np.array_equal(got[1], fresh['other'][1]), order
        finally:
            sess.close()
    ref = M.median_vectorised(other, second, nb_second)
    assert M.median_mismatches(fresh['other'][0], ref, M.mixed_zero_segments(other, second, nb_second)).size == 0


# ---- gradient image per pixel ------------------------------------------------------------------------------------------------
def check_mean(got, grad, seg, n_labels, maxabs, what):
    ref, counts = M.gradient_mean_reference(grad, seg, n_labels)
    worst, outside, nonzero = M.mean_deviation(got, ref, counts, M.gradient_bound(seg.size, maxabs))
    print('%s: worst deviation %.3g of the tolerance' % (what, worst))
    assert outside.size == 0, '%s: %d entries outside, first %r, worst %.3g x the tolerance' % (what, len(outside), tuple(outside[0]), worst)
    assert nonzero.size == 0, '%s: a label without pixels is not 0' % what
    return counts


@pytest.mark.parametrize('dtype', ['u8', 'f32', 'f64'])
@pytest.mark.parametrize('shape', M.PIXEL_IMAGE_SHAPES + M.PIXEL_VOLUME_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_gradient_image_per_pixel(hip, shape, dtype):
    volume = len(shape) == 3
    arr = M.gradient_pattern(shape, dtype, 7)
    seg = M.identity_labels(shape)
    expected = M.gradient_image(arr, volume)
    got = device_mean_gradient(hip, arr, seg, seg.size)
    check_mean(got, expected, seg, seg.size, M.image_maxabs(expected), '%r %s' % (shape, dtype))
    if dtype == 'u8':
        sums = M.gradient_sums(arr, volume)
        assert np.array_equal(expected, M.uint8_by_rule(sums))
        assert np.array_equal(got, expected.reshape(got.shape).astype(np.float64))        # integers: exact
        if shape == (17, 19):
            for s in M.UINT8_SUMS:
                assert np.any(sums == s), s


@pytest.mark.parametrize('volume', [False, True], ids=['image', 'volume'])
def test_planes_of_one_row_or_column_are_refused(hip, volume):
    for h, w in ((1, 9), (9, 1)):
        shape = (2, h, w) if volume else (h, w)
        arr = M.gradient_pattern((2, 9, 9), 'f64', 7)[:, :h, :w] if volume else np.zeros((h, w, 3))
        sess = session(hip, np.ascontiguousarray(arr), M.identity_labels(shape), h * w * (2 if volume else 1))
        try:
            with pytest.raises(hip.HipError, match='Shape of array too small to calculate a numerical gradient'):
                sess.mean_gradient()
        finally:
            sess.close()


# ---- gradient mean per label -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape,dtype', M.MEAN_CASES + [M.MEAN_LARGE], ids=lambda v: v if isinstance(v, str) else 'x'.join(map(str, v)))
def test_gradient_mean_per_label(hip, shape, dtype):
    volume = len(shape) == 3
    arr, seg, nb = M.mean_case(shape, dtype)
    grad = M.gradient_image(arr, volume)
    got = device_mean_gradient(hip, arr, seg, nb)
    counts = check_mean(got, grad, seg, nb, M.image_maxabs(grad), '%r %s' % (shape, dtype))
    assert counts[2] == 0
    if dtype == 'u8':
        cols = grad.reshape(seg.size, -1)
        sums = np.stack([np.bincount(seg.ravel(), cols[:, c], nb) for c in range(cols.shape[1])], axis=1)
        exact = np.where(counts[:, None] > 0, sums.astype(np.float64) / np.maximum(counts, 1)[:, None], 0)
        assert np.array_equal(got, exact.reshape(got.shape))


# ---- the response path -------------------------------------------------------------------------------------------------------
def _response_session(hip, shape):
    volume = len(shape) == 3
    rng = np.random.default_rng([M.SEED, 95] + list(shape))
    data = rng.random(shape if volume else shape + (3, ))
    seg, nb = M.block_labels(shape, 96, steps=(2, 23, 23) if np.prod(shape) > 100000 else (2, 9, 13))
    return (hip.Volume3D if volume else hip.Image2D)(*shape).upload(data).set_labels(seg, nb).lm_prepare(150.), seg, nb, volume


def _check_response(sess, resp, seg, nb, volume, mul, div, what):
    median, mixed, mean, counts, bound = M.response_references(resp, seg, nb, mul, div, volume)
    got = sess.response_median(mul, div)
    bad = M.median_mismatches(got, median, mixed)
    assert bad.size == 0, '%s median: %s' % (what, M.describe(bad, got, median))
    assert counts[2] == 0 and np.all(np.isnan(got[2]))
    grad = sess.response_mean_gradient(mul, div)
    worst, outside, nonzero = M.mean_deviation(grad, mean, counts, bound)
    print('%s: gradient mean, worst deviation %.3g of the tolerance' % (what, worst))
    assert outside.size == 0, '%s gradient mean: %d outside, worst %.3g x the tolerance' % (what, len(outside), worst)
    assert nonzero.size == 0
    return got, grad


@pytest.mark.parametrize('shape', [(57, 70), (3, 38, 45), (1024, 1025)], ids=lambda s: 'x'.join(map(str, s)))
def test_response_median_and_mean_gradient(hip, shape):
    from pyimsegm_amd import descriptors as D
    filters, _ = D._select_bank('short')
    large = int(np.prod(shape)) > 100000
    sess, seg, nb, volume = _response_session(hip, shape)
    try:
        for index in ((2, ) if large else (0, 2, 4)):
            norm = sess.lm_battery(filters[index], D.MAX_SIGNAL_RESPONSE)
            assert 0 < norm < np.inf
            resp = sess.get_response()
            what = '%r battery %d' % (shape, index)
            _check_response(sess, resp, seg, nb, volume, np.log(1 + norm) / 0.03, norm, what)
            if large:
                continue
            med, grad = _check_response(sess, resp, seg, nb, volume, 0.0, norm, what + ' mul = 0')
            assert not np.any(np.nan_to_num(med)) and not np.any(grad)
            # the largest |v| / mul the precondition allows: div = max |response|
            _check_response(sess, resp, seg, nb, volume, 2.0 ** 40, float(np.abs(resp).max()), what + ' mul = 2^40')
    finally:
        sess.close()
