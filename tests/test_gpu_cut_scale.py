"""``imsegm_resize_crops`` / ``imsegm_ellipse_cut_scale`` (csrc/resize.hip, the ellipse masks of csrc/cut_objects.hip) behind
pyimsegm_amd/ellipse_cut_scale.py: the device equals the host statements ``resize_image_host``, ``export_image_array`` and
``extract_ellipse_objects_host`` byte for byte -- the bits of the float64 result and the uint8 stack

* on resize cases at every edge of the kernels: shrinking and enlarging on both axes and on one each, the same size, outputs of
  1 x 1 and 1 x 4, a crop of width 2 under a radius of 18 (several reflections), axes of length 1, output widths 63, 64 and 65,
  1, 3 and 4 channels, 1, 2 and 65 crops of unequal sizes in one call, a constant crop that loses one, an all-zero crop;
* through ``extract_ellipse_objects`` on a 96 x 128 RGB image with 1, 3 and 12 ellipses, two of which overlap, one clipped by the
  image border and one turned by 90 degrees, and ``swap_orientations`` takes the stack;
* a second time on a context whose scratch a larger call has used;
* and what the caps exclude returns None from ``_hip`` and the host result from the public functions."""
import numpy as np
import pytest

import cut_scale_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def hip():
    from pyimsegm_amd import _hip
    _hip.default_context()
    return _hip


@pytest.fixture(scope='module')
def ecs():
    from pyimsegm_amd import ellipse_cut_scale
    return ellipse_cut_scale


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def ragged(count, channels, seed, largest=40):
    """``count`` crops of unequal sizes, some of them a single row or column"""
    rng = np.random.RandomState(seed)
    crops = []
    for k in range(count):
        h, w = (1 + k % 3, rng.randint(1, largest)) if k % 7 == 3 else (rng.randint(1, largest), rng.randint(1, largest))
        crops.append(rng.randint(0, 256, size=(h, w, channels)).astype(np.uint8))
    return crops


def _cases():
    img = C.textured_image
    return {
        'shrink_both': ([img('a', 57, 83, 3)], (20, 31)),
        'shrink_strong': ([img('b', 150, 120, 3)], (13, 11)),
        'enlarge_both': ([img('c', 17, 23, 3)], (40, 52)),
        'shrink_rows_enlarge_columns': ([img('d', 60, 20, 3)], (25, 45)),
        'enlarge_rows_shrink_columns': ([img('e', 15, 66, 1)], (33, 20)),
        'same_size': ([img('f', 40, 40, 3)], (40, 40)),
        'output_1x1': ([img('g', 15, 22, 3), img('g2', 8, 9, 3)], (1, 1)),
        'output_1x4': ([img('h', 15, 22, 1)], (1, 4)),
        'row_of_pixels': ([img('i', 1, 30, 3)], (4, 7)),
        'column_of_pixels': ([img('j', 30, 1, 1), img('j2', 1, 1, 1)], (7, 3)),
        'width_63': ([img('k', 20, 100, 1)], (5, 63)),
        'width_64': ([img('k', 20, 100, 1)], (5, 64)),
        'width_65': ([img('k', 20, 100, 1)], (5, 65)),
        'four_channels': ([img('l', 33, 47, 4)], (12, 17)),
        'tiles_beyond_one': ([img('m', 37, 150, 3)], (16, 70)),
        'two_crops': ([img('n', 57, 83, 3), img('o', 9, 31, 3)], (12, 18)),
        'sixty_five_crops': (ragged(65, 3, 5), (6, 9)),
        'sixty_five_grey_crops': (ragged(65, 1, 6, largest=90), (11, 4)),
        'constant_loses_one': ([np.full((64, 48, 1), 62, dtype=np.uint8)], (21, 17)),
        'all_zero': ([np.zeros((20, 30, 3), dtype=np.uint8), img('p', 12, 12, 3)], (7, 9)),
    }


CASES = _cases()
_REF = {}


def reference(ecs, name):
    """the host statements on a case, computed once: (float64 stack, uint8 stack)"""
    if name not in _REF:
        crops, shape = CASES[name]
        floats = np.stack([ecs.resize_image_host(crop, shape) for crop in crops])
        _REF[name] = floats, np.stack([ecs.export_image_array(one) for one in floats])
    return _REF[name]


@pytest.mark.parametrize('name', list(CASES))
def test_resize_crops_equals_the_host_statement(hip, ecs, name):
    crops, shape = CASES[name]
    floats, exported = reference(ecs, name)
    radii, weights = ecs._taps_of([crop.shape[:2] for crop in crops], shape)
    got = hip.resize_crops(crops, shape, radii, weights)
    assert got is not None, 'the entry refused a case inside its caps'
    assert same_bits(got[0], floats), name
    got = hip.resize_crops(crops, shape, radii, weights, want_u8=True)
    assert got[0] is None and same_bits(got[1], exported), name
    assert same_bits(ecs.resize_images(crops, shape, on='device'), floats)
    assert same_bits(ecs.resize_images(crops, shape, on='device', as_uint8=True), exported)


def test_the_cases_are_what_their_names_say(ecs):
    floats, exported = reference(ecs, 'constant_loses_one')
    assert np.all(floats == 61 * (1. / 255)) and np.all(exported == 255)
    floats, exported = reference(ecs, 'all_zero')
    assert not floats[0].any() and not exported[0].any() and exported[1].max() == 255
    assert reference(ecs, 'enlarge_both')[0].shape == (1, 40, 52, 3)
    assert max(ecs._taps_of([(150, 120)], (13, 11))[0][0]) > 16


def test_narrow_crop_under_a_wide_blur_reflects_repeatedly(hip, ecs):
    """a crop of width 2 and one of height 3 under radius 18: the caller's taps, scikit-image's ``anti_aliasing_sigma``"""
    crops = [C.textured_image('narrow', 40, 2, 3), C.textured_image('flat', 3, 37, 3), C.textured_image('dot', 1, 1, 3)]
    radius, taps = ecs.blur_taps(4.5)
    assert radius == 18
    radii = np.full((3, 2), radius, dtype=np.int32)
    weights = np.zeros((3, 2, hip.RESIZE_MAX_RADIUS + 1))
    weights[:, :, :radius + 1] = taps
    floats = np.stack([ecs.resize_image_host(crop, (9, 5), anti_aliasing_sigma=(4.5, 4.5)) for crop in crops])
    got = hip.resize_crops(crops, (9, 5), radii, weights)
    assert same_bits(got[0], floats)
    got = hip.resize_crops(crops, (9, 5), radii, weights, want_u8=True)
    assert same_bits(got[1], np.stack([ecs.export_image_array(one) for one in floats]))


def test_a_smaller_call_after_a_larger_one_on_the_same_context(hip, ecs):
    """the scratch keeps what the larger call left: ranges, maxima and crops beyond the smaller call's"""
    for name in ('sixty_five_crops', 'column_of_pixels', 'shrink_strong', 'all_zero'):
        crops, shape = CASES[name]
        floats, exported = reference(ecs, name)
        assert same_bits(ecs.resize_images(crops, shape, on='device'), floats), name
        assert same_bits(ecs.resize_images(crops, shape, on='device', as_uint8=True), exported), name


def test_outside_the_caps_the_host_statement_answers(hip, ecs):
    tall = C.textured_image('tall', 300, 6, 1)
    assert ecs._taps_of([tall.shape[:2]], (2, 6)) is None                     # radius 298
    assert same_bits(ecs.resize_images([tall], (2, 6), on='device'), ecs.resize_image_host(tall, (2, 6))[None])
    radii = np.array([[hip.RESIZE_MAX_RADIUS + 1, 0]], dtype=np.int32)
    assert hip.resize_crops([tall], (2, 6), radii, np.ones((1, 2, hip.RESIZE_MAX_RADIUS + 1))) is None
    five = np.zeros((4, 4, 5), dtype=np.uint8)
    assert ecs.resize_images([five], (2, 2), on='device').shape == (1, 2, 2, 5)
    floats = C.textured_image('tall', 20, 20, 3).astype(np.float64)
    with pytest.raises(ValueError):
        ecs.resize_images([floats], (2, 2), on='device')


# ------------------------------------------------------------------------------------------------
# the chain
# ------------------------------------------------------------------------------------------------

#: xc, yc, a, b, theta on a 96 x 128 image: [1] overlaps [0], [2] is clipped by the image border, [3] is turned by 90 degrees
ELLIPSES = [(40.3, 50.8, 30.2, 17.9, 0.31), (52.1, 62.2, 25.7, 14.2, -0.83), (8.6, 20.0, 22.4, 11.3, 0.4), (60.2, 100.7, 12.0, 20.5, np.pi / 2),
            (30.5, 90.1, 9.9, 6.2, 2.2), (70.0, 30.0, 14.0, 14.0, 0.), (48.0, 64.0, 40.8, 30.1, 1.1), (90.9, 120.2, 15.5, 8.5, -0.2),
            (20.2, 64.6, 6.0, 3.0, 0.7), (75.5, 70.5, 10.2, 18.9, -1.3), (45.0, 15.0, 20.0, 7.7, 1.57), (66.6, 55.5, 5.5, 4.4, 3.0)]
NORM_SIZE = (16, 27)
_CHAIN = {}


def chain_reference(ecs, count):
    if count not in _CHAIN:
        img = C.scene_image('chain_gpu', 96, 128, 3)
        _CHAIN[count] = img, ecs.extract_ellipse_objects_host(img, ELLIPSES[:count], NORM_SIZE, as_uint8=False), \
            ecs.extract_ellipse_objects_host(img, ELLIPSES[:count], NORM_SIZE)
    return _CHAIN[count]


@pytest.mark.parametrize('count', [1, 3, 12])
def test_chain_equals_the_host_statements(hip, ecs, count):
    img, floats, stack = chain_reference(ecs, count)
    got = ecs.extract_ellipse_objects(img, ELLIPSES[:count], NORM_SIZE, on='device')
    assert same_bits(got, stack)
    assert same_bits(ecs.extract_ellipse_objects(img, ELLIPSES[:count], NORM_SIZE, as_uint8=False, on='device'), floats)
    geometry = ecs.ellipse_geometry([ecs._int_params(ell) for ell in ELLIPSES[:count]], img.shape)
    direct = hip.ellipse_cut_scale(img, geometry[0], geometry[1], ecs._bg_color(img), NORM_SIZE, ecs._hook_geometry,
                                   ecs._hook_taps(NORM_SIZE))
    assert direct is not None and same_bits(direct, stack), 'the entry refused a case inside its caps'


def test_chain_cases_are_what_they_claim(ecs):
    img = C.scene_image('chain_gpu', 96, 128, 3)
    masks = [ecs._ellipse_mask_host(img.shape, ell) > 0 for ell in ELLIPSES]
    assert (masks[0] & masks[1]).any(), 'two ellipses overlap'
    assert masks[2][0].any(), 'one ellipse is clipped by the border'
    assert ELLIPSES[3][4] == np.pi / 2
    assert all(mask.any() for mask in masks)


def test_chain_on_a_grey_image_and_the_orientation_step_takes_the_stack(ecs):
    from pyimsegm_amd import egg_orientation
    img, _, stack = chain_reference(ecs, 12)
    oriented, flags, template = egg_orientation.swap_orientations(list(stack), on='device')
    assert len(oriented) == 12 and flags.shape == (12, ) and template.shape == NORM_SIZE
    host = egg_orientation.swap_orientations(list(stack), on='host')
    assert np.array_equal(template, host[2])
    grey = np.ascontiguousarray(img[:, :, 1])
    got = ecs.extract_ellipse_objects(grey, ELLIPSES[:3], (30, 48), on='device')
    assert got.shape == (3, 30, 48) and same_bits(got, ecs.extract_ellipse_objects_host(grey, ELLIPSES[:3], (30, 48)))


def test_chain_after_a_larger_call_on_the_same_context(ecs):
    for count in (12, 1):
        img, _, stack = chain_reference(ecs, count)
        assert same_bits(ecs.extract_ellipse_objects(img, ELLIPSES[:count], NORM_SIZE, on='device'), stack)


def test_chain_refusals(hip, ecs):
    img, _, _ = chain_reference(ecs, 1)
    with pytest.raises(IndexError):
        ecs.extract_ellipse_objects(img, [ELLIPSES[0], (-400., -400., 20., 10., 0.3)], NORM_SIZE, on='device')
    # a blur radius above the cap: the taps hook says so in the middle of the call, the host statement answers
    tiny = ecs.extract_ellipse_objects(img, ELLIPSES[:2], (1, 1), on='device')
    assert same_bits(tiny, ecs.extract_ellipse_objects_host(img, ELLIPSES[:2], (1, 1)))
    geometry = ecs.ellipse_geometry([ecs._int_params(ell) for ell in ELLIPSES[:2]], img.shape)
    assert hip.ellipse_cut_scale(img, geometry[0], geometry[1], ecs._bg_color(img), (1, 1), ecs._hook_geometry,
                                 ecs._hook_taps((1, 1))) is None
