"""The host side of pyimsegm_amd/egg_orientation.py against the reference's own statements (tests/golden/egg_orientation.npz, written
by tests/golden/make_egg_orientation_golden.py from ``experiments_ovary_detect/run_egg_swap_orientation.py``); no device.

* ``stack_median2_host`` equals twice the reference's median byte for byte;
* the integer density decision equals the reference's on every image;
* the integer correlation decision equals the reference's on every image with ``|cc - cc_swap| > 1e-12``.  Both coefficients are
  means over at most ~1e3 terms of magnitude <= 1, whose float error stays orders below that gap, while one unit of ``P - Pf`` moves
  ``cc - cc_swap`` by at least ``0.5 / (h w 127.5^2)`` > 2e-8 on these sizes: under the gap lie exactly the images with
  ``P == Pf`` and those where the reference takes its deviation-0 branch (a constant image or template: both coefficients are
  the integer 0 and the answer is "no swap" by definition, not by rounding).  Those of the second kind are held to "no swap" on
  both sides; of the others at most 10 % of the images of any case may fall under the gap -- a cap, not a measurement;
* the float statements of the module equal the reference's decisions and coefficients, and the interface behaves."""
import os

import numpy as np
import pytest

import egg_orientation_cases as C

from pyimsegm_amd import egg_orientation as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GAP = 1e-12
CASES = list(C.CASES)


@pytest.fixture(scope='module')
def golden():
    return C.load_golden()


@pytest.fixture(autouse=True)
def on_host(monkeypatch):
    monkeypatch.setenv('IMSEGM_ORIENTATION_ON', 'host')


def template2_of(golden, name):
    doubled = golden[name + '_template'] * 2
    assert name in C.HOST_ONLY or np.array_equal(doubled, np.rint(doubled))
    return doubled


@pytest.mark.parametrize('name', CASES)
def test_inputs_are_the_ones_the_fixture_was_written_for(golden, name):
    assert int(golden[name + '_crc']) == C.crc(name)
    stack, _ = C.cropped(name)
    assert stack.nbytes <= 4.5e6 and golden[name + '_template'].shape == stack.shape[1:3]


@pytest.mark.parametrize('name', [n for n in CASES if C.case(n)[1] is None])
def test_integer_median_is_twice_the_reference_median_byte_for_byte(golden, name):
    stack, _ = C.cropped(name)
    template2 = E.stack_median2_host(stack[..., 0])
    assert template2.dtype == np.uint16
    assert C.same(template2.astype(np.float64), golden[name + '_template'] * 2)
    assert C.same(E.compute_mean_image(C.case(name)[0]), golden[name + '_template'])


@pytest.mark.parametrize('name', [n for n in CASES if n not in C.HOST_ONLY])
def test_integer_decisions_equal_the_reference(golden, name):
    stack, _ = C.cropped(name)
    template2 = template2_of(golden, name).astype(np.uint16)
    sums = E.orientation_sums_host(stack[..., 0], template2)
    assert sums.dtype == np.int64 and sums.shape == (len(stack), 9)
    assert np.array_equal(E.orientation_flags_host(sums, template2, 'density'), golden[name + '_swap_density'])
    ours = E.orientation_flags_host(sums, template2, 'cc')
    cc, cc_swap = golden[name + '_cc'], golden[name + '_cc_swap']
    under = np.abs(cc - cc_swap) <= GAP
    no_deviation = (sums[:, E.SUM_MIN] == sums[:, E.SUM_MAX]) | (template2.min() == template2.max())
    tie = sums[:, E.SUM_P] == sums[:, E.SUM_PF]
    print('%s: %d of %d images under the gap, %d of them without a deviation, %d exact ties' % (
        name, under.sum(), len(under), (under & no_deviation).sum(), (tie & ~no_deviation).sum()))
    assert np.array_equal(ours[~under], golden[name + '_swap_cc'][~under])
    assert np.all(cc[no_deviation] == 0) and np.all(cc_swap[no_deviation] == 0)
    assert not ours[no_deviation].any() and not golden[name + '_swap_cc'][no_deviation].any()
    assert np.array_equal(under & ~no_deviation, tie & ~no_deviation)
    assert (under & ~no_deviation).sum() <= 0.1 * len(under)
    assert not ours[tie].any()


def test_the_exact_tie_gives_no_swap(golden):
    stack, _ = C.cropped('point_symmetric')
    template2 = template2_of(golden, 'point_symmetric').astype(np.uint16)
    sums = E.orientation_sums_host(stack[..., 0], template2)
    for i in (3, 11):
        assert np.array_equal(stack[i], stack[i, ::-1, ::-1])
        assert sums[i, E.SUM_P] == sums[i, E.SUM_PF] and sums[i, E.SUM_MIN] != sums[i, E.SUM_MAX]
    flags = E.orientation_flags_host(sums, template2, 'cc')
    assert not flags[3] and not flags[11]
    assert not golden['point_symmetric_swap_cc'][3] and not golden['point_symmetric_swap_cc'][11]


def test_cases_are_what_their_names_say(golden):
    stack, _ = C.cropped('flat_above_minimum')
    sums = E.orientation_sums_host(stack[..., 0], template2_of(golden, 'flat_above_minimum'))
    assert np.all(sums[:, E.SUM_CNT] > 0) and not sums[:, E.SUM_L].any() and not sums[:, E.SUM_R].any()
    stack, _ = C.cropped('constant_image')
    sums = E.orientation_sums_host(stack[..., 0], template2_of(golden, 'constant_image'))
    assert sums[2, E.SUM_CNT] == 0 and sums[9, E.SUM_CNT] == 0 and sums[9, E.SUM_A] == 0
    stack, _ = C.cropped('px257_w1')                    # a third of 0 columns: R is the sum of all of g, L is 0
    sums = E.orientation_sums_host(stack[..., 0], template2_of(golden, 'px257_w1'))
    assert not sums[:, E.SUM_L].any() and np.all(sums[:, E.SUM_R] > 0)
    assert np.any(golden['given_half_template_template'] % 1 == 0.5)
    assert np.any((golden['given_other_template_template'] * 2) % 1 != 0)
    assert len({img.shape for img in C.case('ragged')[0]}) > 3
    stack, _ = C.cropped('n65535')
    assert len(stack) == 65535 and np.all(stack[:, 0, 0, 0] == 200)


def test_the_swap_brings_the_turned_ramps_back(golden):
    images, _ = C.case('ramp_half_turned')
    oriented, flags, template = E.swap_orientations(images)
    assert np.array_equal(flags, np.arange(13) % 2 == 1) and np.array_equal(flags, golden['ramp_half_turned_swap_cc'])
    assert C.same(template, golden['ramp_half_turned_template'])
    for i, img in enumerate(oriented):
        assert np.array_equal(img, images[i][::-1, ::-1] if i % 2 else images[i])
        assert np.mean(img[:, 16:, 0]) > np.mean(img[:, :8, 0])             # bright on the right again


# ---- the float statements and the interface ---------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', CASES)
def test_float_statements_equal_the_reference(golden, name):
    stack, _ = C.cropped(name)
    template = golden[name + '_template']
    for i, img in enumerate(stack):
        assert E.correlation_coefficient(img[:, :, 0], template) == golden[name + '_cc'][i]
        assert E.correlation_coefficient(img[::-1, ::-1, 0], template) == golden[name + '_cc_swap'][i]
        if i >= 300:
            break
    step = max(1, len(stack) // 300)
    assert [bool(E.condition_swap_correl(img, template)) for img in stack[::step]] == list(golden[name + '_swap_cc'][::step])
    assert [E.condition_swap_density(img) for img in stack[::step]] == list(golden[name + '_swap_density'][::step])


@pytest.mark.parametrize('name', ['ragged', 'given_half_template', 'given_other_template', 'three_levels', 'c1', 'c4'])
@pytest.mark.parametrize('swap_type', ['cc', 'density'])
def test_swap_orientations_on_the_host_is_the_loop_of_single_calls(golden, name, swap_type):
    images, given = C.case(name)
    oriented, flags, template = E.swap_orientations(images, swap_type, given, on='host')
    assert flags.dtype == np.bool_ and flags.shape == (len(images), )
    assert C.same(template, golden[name + '_template'])
    assert np.array_equal(flags, golden[name + ('_swap_cc' if swap_type == 'cc' else '_swap_density')])
    for img, got, flag in zip(images, oriented, flags):
        single = E.perform_orientation_swap(img, template, swap_type)
        assert got.shape == template.shape + img.shape[2:] and np.array_equal(got, single)
        assert np.array_equal(got, img[:template.shape[0], :template.shape[1]][::-1, ::-1] if flag else img[:template.shape[0], :template.shape[1]])


def test_the_place_switch(monkeypatch):
    from pyimsegm_amd import _hip
    images, _ = C.case('px63')
    a = E.swap_orientations(images, on='host')
    monkeypatch.setenv('IMSEGM_ORIENTATION_ON', 'host')
    b = E.swap_orientations(images)
    assert np.array_equal(a[1], b[1]) and C.same(a[2], b[2]) and all(C.same(x, y) for x, y in zip(a[0], b[0]))
    monkeypatch.setenv('IMSEGM_ORIENTATION_ON', 'nowhere')
    with pytest.raises(ValueError):
        E.swap_orientations(images)
    with pytest.raises(ValueError):
        E.compute_mean_image(images)
    with pytest.raises(ValueError):
        E.compute_mean_image(images, on='gpu')
    if _hip.device_count() == 0:
        with pytest.raises(_hip.HipUnavailableError):
            E.swap_orientations(images, on='device')


def test_errors():
    images, _ = C.case('px63')
    big = np.zeros((20, 20))
    with pytest.raises(ValueError):                      # an image smaller than the template: numpy's broadcast error
        E.perform_orientation_swap(images[0], big, 'cc')
    with pytest.raises(ValueError):
        E.swap_orientations(images, 'cc', big, on='host')
    with pytest.raises(ValueError):
        E.compute_mean_image([])
    with pytest.raises(IndexError):
        E.compute_mean_image([img[:, :, 0] for img in images])             # the reference indexes a channel
    with pytest.raises(ValueError):
        E.stack_median2_host(np.zeros((3, 4, 5), dtype=np.float32))
    with pytest.raises(ValueError):
        E.orientation_sums_host(np.zeros((3, 4, 5), dtype=np.uint8), np.zeros((4, 6), dtype=np.uint16))


def test_a_template_the_device_does_not_take_is_recognised():
    assert E._template2_of(C.case('given_other_template')[1]) is None
    assert E._template2_of(np.full((3, 3), 255.5)) is None and E._template2_of(np.full((3, 3), -0.5)) is None
    assert E._template2_of(np.full((3, 3), np.nan)) is None and E._template2_of(np.zeros((3, 3, 3))) is None
    half = E._template2_of(C.case('given_half_template')[1])
    assert half.dtype == np.uint16 and np.array_equal(half, C.case('given_half_template')[1] * 2)
    assert np.array_equal(E._template2_of(np.full((2, 2), 255.)), np.full((2, 2), 510))
    assert E._device_stack([np.zeros((4, 4, 3), dtype=np.float32)], (4, 4)) is None
    assert E._device_stack([np.zeros((4, 4, 5), dtype=np.uint8)], (4, 4)) is None
    assert E._device_stack([np.zeros((4, 4, 3), dtype=np.uint8), np.zeros((4, 4, 1), dtype=np.uint8)], (4, 4)) is None
    assert E._device_stack([np.zeros((4, 4, 3), dtype=np.uint8)], (5, 4)) is None
    assert E._device_stack([np.zeros((5, 6, 3), dtype=np.uint8)] * 2, (4, 4)).shape == (2, 4, 4, 3)


def test_sources_and_entries_are_declared_and_exported():
    from pyimsegm_amd import _hip, build
    header = open(os.path.join(ROOT, 'include', 'imsegm_hip.h')).read()
    for name in ('imsegm_orient_stack', 'imsegm_stack_median_u8'):
        assert name + '(' in header and name in _hip.EXPORTED_SYMBOLS
    assert '#define IMSEGM_ORIENT_MAX_IMAGES %d' % _hip.ORIENT_MAX_IMAGES in header
    assert '#define IMSEGM_ORIENT_SUM_WORDS %d' % _hip.ORIENT_SUM_WORDS in header
    assert 'egg_orientation.hip' in build.SOURCES and 'api_egg_orientation.hip' in build.SOURCES
    assert 'egg_orientation.h' in build.HEADERS
    for name in ('egg_orientation.hip', 'api_egg_orientation.hip', 'egg_orientation.h'):
        assert os.path.isfile(os.path.join(build.CSRC, name))


def test_module_is_importable_next_to_the_alias_package():
    import imsegm  # noqa: F401  (the alias package: the stage modules; the experiment modules live in pyimsegm_amd alone)
    import pyimsegm_amd.egg_orientation as module
    for name in ('compute_mean_image', 'perform_orientation_swap', 'swap_orientations', 'correlation_coefficient',
                 'condition_swap_correl', 'condition_swap_density', 'stack_median2_host', 'orientation_sums_host'):
        assert callable(getattr(module, name)) and name in module.__all__
    assert module.IMAGE_CHANNEL == 0 and module.SWAP_CONDITION == 'cc'
