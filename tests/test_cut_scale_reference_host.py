"""The host statements of pyimsegm_amd/ellipse_cut_scale.py against scikit-image 0.18.3 and the reference's own
``extract_ellipse_object`` (tests/golden/cut_scale.npz, written by tests/golden/make_golden_cut_scale.py); no device.

* the blur equals what scikit-image's ``resize`` got back from ``ndi.gaussian_filter`` byte for byte;
* the float result differs from scikit-image's by at most 16 times the difference the generator recorded (``max_float_diff`` of
  the golden file, see tests/golden/README_cut_scale.md) -- the bound comes from the golden, not from the code under test;
* every exported byte equals the golden's, with one excuse: a pixel may differ by exactly 1 where the golden's own stretched float
  value lies within 1e-9 of an integer (there the truncation is decided by the last bits of scikit-image's least-squares scale
  factors); on every re-scaling case at most 1 % of the pixels may use the excuse.  The same-size case is held to the float bound
  and the by-one rule only: every stretched value sits on an integer there and the reference's own bytes are not reproducible;
* ``extract_ellipse_objects_host`` against the full-chain cases by the same rules;
* the small helpers."""
import os

import numpy as np
import pytest

import cut_scale_cases as C

from pyimsegm_amd import ellipse_cut_scale as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEAR_INTEGER = 1e-9
EXCUSED_SHARE = 0.01


@pytest.fixture(scope='module')
def golden():
    return np.load(os.path.join(ROOT, 'tests', 'golden', 'cut_scale.npz'))


@pytest.fixture(autouse=True)
def on_host(monkeypatch):
    monkeypatch.setenv('IMSEGM_CUT_SCALE_ON', 'host')


def float_bound(golden):
    recorded = float(golden['max_float_diff'])
    assert 0 < recorded < 1e-12, 'the recorded difference is of the order of 1e-14'
    return 16 * recorded


def check_exported(mine, resized, exported, rescaled):
    """the by-one rule on the golden's own stretched values; returns the number of excused pixels"""
    assert mine.dtype == np.uint8 and mine.shape == exported.shape
    stretched = resized / float(resized.max()) * 255
    near = np.abs(stretched - np.rint(stretched)) <= NEAR_INTEGER
    delta = np.abs(mine.astype(np.int16) - exported.astype(np.int16))
    print('bytes differing: %d of %d, near an integer: %d' % ((delta > 0).sum(), delta.size, near.sum()))
    assert delta.max() <= 1
    assert not np.any((delta == 1) & ~near), 'a byte differs where the stretched value is not next to an integer'
    excused = int((delta == 1).sum())
    if rescaled:
        assert excused <= EXCUSED_SHARE * delta.size
    return excused


@pytest.mark.parametrize('name', list(C.RESIZE_CASES) + list(C.CHAIN_CASES))
def test_inputs_are_the_ones_the_fixture_was_written_for(golden, name):
    img = C.resize_case(name)[0] if name in C.RESIZE_CASES else C.chain_case(name)[0]
    assert int(golden[name + '_crc']) == C.crc(img)


@pytest.mark.parametrize('name', list(C.RESIZE_CASES))
def test_blur_equals_scikit_image_byte_for_byte(golden, name):
    img, shape = C.resize_case(name)
    blurred = E.blur_image_host(img, shape)
    assert blurred.dtype == np.uint8 and np.array_equal(blurred, golden[name + '_blurred'])


def test_the_blur_cases_shrink_enlarge_and_truncate(golden):
    """what the cases have to contain to mean anything: a blurred axis and an untouched one, and a constant area that lost one"""
    from scipy import ndimage
    lost = 0
    for name in C.RESIZE_CASES:
        img, shape = C.resize_case(name)
        blurred = golden[name + '_blurred'].reshape(img.shape[0], img.shape[1], -1)
        source = img.reshape(blurred.shape)
        reach = [2 * E.blur_taps(sigma)[0] + 1 for sigma in E._blur_sigmas(img.shape, shape)] + [1]
        constant = ndimage.maximum_filter(source, size=reach, mode='mirror') == ndimage.minimum_filter(source, size=reach, mode='mirror')
        assert np.all(source[constant].astype(int) - blurred[constant] <= 1) and np.all(blurred[constant] <= source[constant])
        lost += int((blurred[constant] == source[constant].astype(int) - 1).sum())
    assert lost, 'no case shows the v - 1 of the integer-typed blur'
    assert np.array_equal(golden['enlarge_rgb_blurred'], C.resize_case('enlarge_rgb')[0])


@pytest.mark.parametrize('name', list(C.RESIZE_CASES))
def test_resize_is_within_the_recorded_bound_of_scikit_image(golden, name):
    img, shape = C.resize_case(name)
    mine = E.resize_image_host(img, shape)
    assert mine.dtype == np.float64 and mine.shape == golden[name + '_resized'].shape
    diff = float(np.abs(mine - golden[name + '_resized']).max())
    print(name, 'largest difference %.3e, bound %.3e' % (diff, float_bound(golden)))
    assert diff <= float_bound(golden)


@pytest.mark.parametrize('name', list(C.RESIZE_CASES))
def test_exported_bytes_equal_the_reference(golden, name):
    img, shape = C.resize_case(name)
    mine = E.export_image_array(E.resize_image_host(img, shape))
    check_exported(mine, golden[name + '_resized'], golden[name + '_exported'], name not in C.SAME_SIZE_CASES)


@pytest.mark.parametrize('name', list(C.CHAIN_CASES))
def test_full_chain_equals_the_reference(golden, name):
    img, ellipses, norm_size = C.chain_case(name)
    floats = E.extract_ellipse_objects_host(img, ellipses, norm_size, as_uint8=False)
    stack = E.extract_ellipse_objects_host(img, ellipses, norm_size)
    assert floats.dtype == np.float64 and stack.dtype == np.uint8
    assert stack.shape == (len(ellipses), ) + tuple(norm_size) + img.shape[2:] == floats.shape
    for k in range(len(ellipses)):
        resized = golden['%s_resized%d' % (name, k)]
        assert float(np.abs(floats[k] - resized).max()) <= float_bound(golden)
        check_exported(stack[k], resized, golden['%s_exported%d' % (name, k)], True)
    assert np.array_equal(E.extract_ellipse_objects(img, ellipses, norm_size), stack)


def test_resize_images_stacks_the_host_statement():
    images = [C.resize_case(name)[0] for name in ('shrink_rgb', 'enlarge_rgb', 'mixed_rgb')]
    stack = E.resize_images(images, (11, 14))
    assert stack.shape == (3, 11, 14, 3) and stack.dtype == np.float64
    for img, out in zip(images, stack):
        assert np.array_equal(out, E.resize_image_host(img, (11, 14)))
    grey = E.resize_images([C.resize_case('shrink_gray')[0]], (5, 1), as_uint8=True)
    assert grey.shape == (1, 5, 1) and grey.dtype == np.uint8
    with pytest.raises(ValueError):
        E.resize_images([images[0], C.resize_case('shrink_gray')[0]], (4, 4))
    with pytest.raises(ValueError):
        E.resize_image_host(images[0].astype(np.float64), (4, 4))


def test_edges_of_the_definition():
    """1 x 1 output reads the centre; an axis of length 1 reads its single pixel; a radius above the axis reflects repeatedly"""
    img = np.arange(30, dtype=np.uint8).reshape(5, 6) * 8
    one = E.resize_image_host(img, (1, 1))
    blurred = E.blur_image_host(img, (1, 1)) * (1. / 255)
    assert one.shape == (1, 1) and one[0, 0] == 0.5 * (blurred[2, 2] + blurred[2, 3])
    line = E.resize_image_host(np.array([[10, 200, 30]], dtype=np.uint8), (4, 7))
    assert line.shape == (4, 7) and np.array_equal(line[0], line[3])
    narrow = C.textured_image('narrow', 40, 2, 3)
    assert E.resize_image_host(narrow, (40, 2)).shape == (40, 2, 3)
    radius, taps = E.blur_taps((74. / 2 - 1) / 2)
    assert radius == 72 and len(taps) == 73 and E.blur_taps(0.)[0] == 0


def test_stage_norm_size():
    rows = [(50, 60, 30.5, 20, 0.), (10, 10, 40, 25.8, 1.), (30, 30, 33, 21, 2.), (1, 1, 36.9, 28, 0.)]
    assert E.stage_norm_size(rows) == (int(np.median([20, 25.8, 21, 28])), int(np.median([30.5, 40, 33, 36.9]))) == (23, 34)
    assert E.stage_norm_size(rows, np.max) == (28, 40)
    assert E.COLUMNS_ELLIPSE == ['ellipse_xc', 'ellipse_yc', 'ellipse_a', 'ellipse_b', 'ellipse_theta']


def test_export_image_array():
    zeros = E.export_image_array(np.zeros((3, 4, 3)))
    assert zeros.dtype == np.uint8 and not zeros.any()
    img = np.array([[0.2, 0.4], [0.1, 0.3]])
    assert np.array_equal(E.export_image_array(img), (img / 0.4 * 255).astype(np.uint8))
    assert np.array_equal(E.export_image_array(img, stretch_range=False), np.zeros((2, 2), dtype=np.uint8))


def test_an_empty_mask_raises():
    img, _, norm_size = C.chain_case('chain_rgb')
    with pytest.raises(IndexError):
        E.extract_ellipse_objects_host(img, [(-400., -400., 20., 10., 0.3)], norm_size)
    with pytest.raises(IndexError):
        E.extract_ellipse_objects(img, [(40., 50., 20., 10., 0.3), (-400., -400., 20., 10., 0.3)], norm_size)
    assert E.extract_ellipse_objects(img, [], norm_size).shape == (0, ) + tuple(norm_size) + (3, )
