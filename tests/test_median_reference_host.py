"""The cases of tests/median_cases.py can catch a subtly wrong median or gradient kernel, shown on the CPU from numpy alone -- before
any GPU sees them: the vectorised median reference equals the per-label ``np.median`` loop; the uint8 cast rule is numpy's cast
here; and a numpy restatement of the device's evaluation with ONE defect leaves the comparison on the cases meant for that defect,
while the same restatement without a defect stays inside on every case.

Measured here (numpy 2.2).  A median defect shows as a bit difference (labels that differ / labels of the case, fewest .. most over
the cases listed in MEDIAN_DEFECT_CASES):
  negative keys not inverted 2/17 .. 3/3; label sort cut to 16 bits 65537/65537; second sort not stable 4/5 .. 255/255; inclusive scan
  4/5 .. 256/256; upper middle element alone 1/5 .. 24464/65536; float32 pair averaged in float64 6/17; counts of the first channel
  reused after a change of label map 13/13; the picked -0.0 returned as it is (np.mean sums from +0.0) 1/17 .. 3/15.
A gradient defect deviates by a multiple of the tolerance 1e-12 |ref| + B (smallest .. largest over the cases it applies to):
  an end as interior 1e+11 .. 8e+22 (each of the four ends); right neighbour from the next row 4e+11 .. 8e+22; lower neighbour from
  the next plane 6e+12 .. 6e+22; uint8 saturated 1e+12 .. 8e+22; uint8 floored 8e+22."""
import numpy as np
import pytest

import median_cases as M

MARGIN = 100

#: the cases meant for each median defect
MEDIAN_DEFECT_CASES = {
    'sign': ['regime-32x32-f64', 'regime-25x41-f32', 'crafted-f64', 'crafted-vol-f32', 'labels-K3'],
    'label16': ['labels-K65537'],
    'unstable': ['regime-32x32-u8', 'regime-25x41-f64', 'crafted-u8', 'labels-K255'],
    'inclusive': ['regime-32x32-f32', 'crafted-f32', 'labels-K1', 'labels-K256', 'labels-K65536', 'labels-identity'],
    'upper': ['regime-25x41-u8', 'crafted-u8', 'crafted-f64', 'labels-K65536'],
    'f32-in-f64': ['crafted-f32'],
    'neg-zero': ['crafted-f32', 'crafted-f64', 'crafted-vol-f32', 'labels-K255'],       # (-0.0 from the grid of quarters)
}
assert set(MEDIAN_DEFECT_CASES) | {'stale-counts'} == set(M.MEDIAN_DEFECTS)


def _reference(name):
    arr, seg, nb = M.median_case(name)
    return M.median_vectorised(arr, seg, nb), M.mixed_zero_segments(arr, seg, nb)


@pytest.mark.parametrize('name', M.SMALL_MEDIAN_CASES)
def test_vectorised_median_equals_the_np_median_loop_and_the_model(name):
    arr, seg, nb = M.median_case(name)
    ref, mixed = _reference(name)
    loop = M.median_loop(arr, seg, nb)
    bad = M.median_mismatches(ref, loop, mixed)
    assert bad.size == 0, M.describe(bad, ref, loop)
    counts = np.bincount(seg.ravel(), minlength=nb)
    assert np.array_equal(np.isnan(ref).reshape(nb, -1).all(axis=1), counts == 0)
    got = M.model_median(arr, seg, nb)
    bad = M.median_mismatches(got, ref, mixed)
    assert bad.size == 0, M.describe(bad, got, ref)


def test_block_label_cases_have_odd_even_and_empty_labels():
    for name, _, _ in M.REGIME_SMALL:
        _, seg, nb = M.median_case(name)
        counts = np.bincount(seg.ravel(), minlength=nb)
        assert counts[2] == 0 and np.any(counts % 2 == 1) and np.any(counts[counts > 0] % 2 == 0)
    _, seg, nb = M.median_case('labels-K65537')
    assert set(np.bincount(seg.ravel(), minlength=nb)) == {1, 2} and seg.max() == 65536
    _, seg, nb = M.median_case('labels-trailing')
    assert nb == seg.max() + 1 + 70


def test_crafted_segments_are_what_they_claim():
    arr, seg, nb, names = M.crafted('f32', (29, 31), 60)
    ref = M.median_vectorised(arr, seg, nb)
    k = names.index('pair-adjacent')
    a = np.nextafter(np.float32(1), np.float32(2))
    b = np.nextafter(a, np.float32(2))
    assert ref[k, 0] == np.float64(b) and ref[k, 0] != (np.float64(a) + np.float64(b)) / 2      # the float32 mean rounds
    assert ref[names.index('pair-3e38'), 0] == np.inf                                            # numpy's float32 mean overflows
    # np.mean sums from +0.0, so numpy's median of a segment of -0.0 alone is +0.0: a pick that returns the element itself shows
    assert not np.signbit(np.median(np.full(5, -0.0, dtype=np.float32))) and not np.signbit(np.median(np.full(4, -0.0)))
    assert not np.signbit(ref[names.index('neg-zeros'), 0]) and not np.signbit(ref[names.index('pos-zeros'), 0])
    assert [int((seg == names.index('size%d' % s)).sum()) for s in (1, 2, 3, 4, 255, 256, 257)] == [1, 2, 3, 4, 255, 256, 257]
    arr, seg, nb, names = M.crafted('u8', (29, 31), 60)
    ref = M.median_vectorised(arr, seg, nb)
    assert ref[names.index('pair-254-255'), 0] == 254.5 and ref[names.index('pair-0-255'), 0] == 127.5
    arr, seg, nb, names = M.crafted('f64', (29, 31), 60)
    assert M.median_vectorised(arr, seg, nb)[names.index('pair-overflow'), 0] == np.inf


def test_special_values_hold_every_edge():
    for dtype in ('f32', 'f64'):
        fi = np.finfo(M.DTYPES[dtype])
        v = M.median_case('values-%s-image' % dtype)[0].ravel()
        assert np.all(np.isfinite(v))
        for edge in (fi.smallest_subnormal, fi.tiny, fi.max, 1.0, np.nextafter(fi.dtype.type(1), fi.dtype.type(2))):
            assert np.any(v == edge) and np.any(v == -edge)
        assert np.any((v == 0) & np.signbit(v)) and np.any((v == 0) & ~np.signbit(v))
        assert np.any(np.isinf(M.median_case('values-inf-%s-image' % dtype)[0]))


@pytest.mark.parametrize('defect', sorted(MEDIAN_DEFECT_CASES))
def test_every_median_defect_shows_as_a_bit_difference(defect):
    for name in MEDIAN_DEFECT_CASES[defect]:
        arr, seg, nb = M.median_case(name)
        ref, mixed = _reference(name)
        bad = M.median_mismatches(M.model_median(arr, seg, nb, defect=defect), ref, mixed)
        labels = len(set(int(b[0]) for b in bad))
        print('%-12s %-20s %d of %d labels differ' % (defect, name, labels, nb))
        assert labels >= 1, (defect, name)


def test_stale_counts_after_a_change_of_label_map_show():
    arr, first, _ = M.median_case('relabel-first')
    _, second, nb = M.median_case('relabel-second')
    ref, mixed = _reference('relabel-second')
    bad = M.median_mismatches(M.model_median(arr, second, nb, defect='stale-counts', previous=first), ref, mixed)
    labels = len(set(int(b[0]) for b in bad))
    print('stale-counts %d of %d labels differ' % (labels, nb))
    assert labels >= 1


def test_normalised_median_model_equals_numpy_on_the_normalised_values():
    """the response path ranks the raw values and normalises the picked ones: the same as numpy's median of (v * mul) / div"""
    rng = np.random.default_rng(5)
    seg, nb = M.block_labels((57, 70), 90, steps=(2, 9, 13))
    resp = rng.standard_normal((3, 57, 70)) * 17
    for mul, div in ((np.log(1 + 340.) / 0.03, 340.), (0.0, 340.), (2.0 ** 40, float(np.abs(resp).max()))):
        median, mixed, mean, counts, bound = M.response_references(resp, seg, nb, mul, div, False)
        got = M.model_median(np.moveaxis(resp, 0, -1), seg, nb, norm=(mul, div))
        bad = M.median_mismatches(got, median, mixed)
        assert bad.size == 0, M.describe(bad, got, median)
        grad = M.model_gradient_of(resp, False, norm=(mul, div))
        assert np.abs(grad).max() <= 4 * mul                              # the bound the fixed-point scale is taken from
        worst, outside, nonzero = M.mean_deviation(M.model_mean(np.moveaxis(grad, 0, -1), seg, nb), mean, counts, bound)
        assert outside.size == 0 and nonzero.size == 0, (mul, worst)


# ---- gradient ----------------------------------------------------------------------------------------------------------------
def _pixel_cases():
    return [(s, d) for s in M.PIXEL_IMAGE_SHAPES + M.PIXEL_VOLUME_SHAPES for d in ('u8', 'f32', 'f64')]


def _applies(defect, shape, dtype):
    if defect in ('u8-saturate', 'u8-floor'):
        return dtype == 'u8' and shape[-2:] not in ((2, 2), (2, 3), (3, 2))    # (no half and no wrap below 0 on so few pixels)
    if defect == 'next-plane':
        return len(shape) == 3 and shape[0] > 1
    return True


def _per_pixel(arr, volume, grad):
    """(got, ref, counts, bound) of the per-pixel comparison: identity labels, so the mean is float32 of every gradient value"""
    seg = M.identity_labels(arr.shape[:3] if volume else arr.shape[:2])
    expected = M.gradient_image(arr, volume)
    ref, counts = M.gradient_mean_reference(expected, seg, seg.size)
    return M.model_mean(grad, seg, seg.size), ref, counts, M.gradient_bound(seg.size, M.image_maxabs(expected))


@pytest.mark.parametrize('shape,dtype', _pixel_cases())
def test_gradient_model_equals_np_gradient_per_pixel(shape, dtype):
    volume = len(shape) == 3
    arr = M.gradient_pattern(shape, dtype, 7)
    expected = M.gradient_image(arr, volume)
    model = M.model_gradient_of(arr, volume)
    assert model.dtype == expected.dtype and np.array_equal(model.view(np.uint8), expected.view(np.uint8))
    worst, outside, nonzero = M.mean_deviation(*_per_pixel(arr, volume, model))
    assert outside.size == 0 and nonzero.size == 0, worst


@pytest.mark.parametrize('shape', M.PIXEL_IMAGE_SHAPES + M.PIXEL_VOLUME_SHAPES)
def test_uint8_cast_rule_is_the_cast_of_this_numpy(shape):
    """truncation towards zero, then modulo 256: a numpy that casts otherwise shows here, not as a GPU failure"""
    volume = len(shape) == 3
    arr = M.gradient_pattern(shape, 'u8', 7)
    sums = M.gradient_sums(arr, volume)
    assert np.array_equal(M.gradient_image(arr, volume), M.uint8_by_rule(sums))
    if shape == (17, 19):
        for s in M.UINT8_SUMS:
            assert np.any(sums == s), s
    else:
        assert sums.min() < 0 and sums.max() > 255 or min(shape[-2:]) == 2


@pytest.mark.parametrize('defect', M.GRADIENT_DEFECTS)
def test_every_gradient_defect_leaves_the_tolerance(defect):
    ratios = []
    for shape, dtype in _pixel_cases():
        if not _applies(defect, shape, dtype):
            continue
        volume = len(shape) == 3
        arr = M.gradient_pattern(shape, dtype, 7)
        worst, outside, _ = M.mean_deviation(*_per_pixel(arr, volume, M.model_gradient_of(arr, volume, defect=defect)))
        ratios.append(worst)
        assert worst > MARGIN and outside.size, (defect, shape, dtype, worst)
    rng = np.random.default_rng(6)                                        # the planes of a response: normalised on load
    resp, seg = rng.standard_normal((3, 9, 11)) * 17, M.identity_labels((9, 11))
    if not defect.startswith('u8'):
        mul, div = 190.0, 340.0
        _, _, mean, counts, bound = M.response_references(resp, seg, seg.size, mul, div, False)
        grad = np.moveaxis(M.model_gradient_of(resp, False, norm=(mul, div), defect=defect), 0, -1)
        worst, outside, _ = M.mean_deviation(M.model_mean(grad, seg, seg.size), mean, counts, bound)
        ratios.append(worst)
        assert worst > MARGIN and outside.size, (defect, 'response', worst)
    print('%-12s %.0e .. %.0e x the tolerance over %d cases' % (defect, min(ratios), max(ratios), len(ratios)))


@pytest.mark.parametrize('shape,dtype', M.MEAN_CASES)
def test_gradient_mean_model_stays_inside_the_bound(shape, dtype):
    volume = len(shape) == 3
    arr, seg, nb = M.mean_case(shape, dtype)
    grad = M.gradient_image(arr, volume)
    ref, counts = M.gradient_mean_reference(grad, seg, nb)
    got = M.model_mean(M.model_gradient_of(arr, volume), seg, nb)
    worst, outside, nonzero = M.mean_deviation(got, ref, counts, M.gradient_bound(seg.size, M.image_maxabs(grad)))
    assert outside.size == 0 and nonzero.size == 0 and counts[2] == 0, worst
    if dtype == 'u8':
        sums = np.stack([np.bincount(seg.ravel(), grad.reshape(seg.size, -1)[:, c], nb) for c in range(grad.size // seg.size)], axis=1)
        exact = np.where(counts[:, None] > 0, sums.astype(np.float64) / np.maximum(counts, 1)[:, None], 0).reshape(got.shape)
        assert np.array_equal(got, exact)


def test_planes_without_a_second_row_or_column_are_refused():
    for shape in ((1, 9, 3), (9, 1, 3)):
        with pytest.raises(ValueError, match='Shape of array too small'):
            np.gradient(np.zeros(shape[:2]))
        with pytest.raises(ValueError, match='Shape of array too small'):
            M.model_gradient_of(np.zeros(shape), False)


# ---- the host route of the dtypes the device does not keep -------------------------------------------------------------------
@pytest.mark.parametrize('dtype,shape', [(np.int16, (37, 41)), (np.uint16, (37, 41)), (np.int32, (37, 41)), (np.int32, (3, 20, 23))])
def test_channel_medians_equal_np_median_per_label(dtype, shape):
    from pyimsegm_amd import descriptors as D
    rng = np.random.default_rng(8)
    volume = len(shape) == 3
    info = np.iinfo(dtype)
    arr = rng.integers(info.min, info.max, shape if volume else shape + (3, ), dtype=dtype, endpoint=True)
    seg, nb = M.block_labels(shape, 91, steps=(2, 7, 9))
    counts = np.bincount(seg.ravel(), minlength=nb)
    assert counts[2] == 0 and np.any(counts % 2 == 1) and np.any(counts[counts > 0] % 2 == 0)
    got = D._channel_medians(arr, seg)
    ref = M.median_loop(arr, seg, nb)
    assert got.shape == ref.shape and np.all(np.isnan(got[2]))
    bad = M.median_mismatches(got, ref)
    assert bad.size == 0, M.describe(bad, got, ref)
