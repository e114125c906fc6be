"""``imsegm_orient_stack`` / ``imsegm_stack_median_u8`` (csrc/egg_orientation.hip) behind pyimsegm_amd/egg_orientation.py: the device
equals the integer statements ``stack_median2_host``, ``orientation_sums_host`` and ``orientation_flags_host`` and the numpy turn
byte for byte

* on every case of tests/egg_orientation_cases.py: N = 1 .. 65 535 (counter width, even / odd N), equal planes, two and three grey
  levels, pixel counts around a wave and beyond a workgroup, widths 1 to 4, one row, 1 / 3 / 4 channels, ragged sizes, exact ties,
  constant images and template, a given template with .5 values -- in both modes;
* through ``swap_orientations(on='device')`` and ``compute_mean_image(on='device')``;
* a second time on a context whose scratch a larger call has used and that was then filled with ``0x7F`` words;
* and what the caps exclude returns None from ``_hip`` and the host result from the public function."""
import numpy as np
import pytest

import egg_orientation_cases as C

pytestmark = pytest.mark.gpu

DEVICE_CASES = [name for name in C.CASES if name not in C.HOST_ONLY]
MODES = ('cc', 'density')
_REF = {}


@pytest.fixture(scope='module')
def hip():
    from pyimsegm_amd import _hip
    _hip.default_context()
    return _hip


@pytest.fixture(scope='module')
def egg():
    from pyimsegm_amd import egg_orientation
    return egg_orientation


def reference(egg, name, channel=0):
    """stack, given template2 or None, template2, sums, and per mode (flags, turned stack): the integer statements, computed once"""
    key = name, channel
    if key not in _REF:
        stack, given = C.cropped(name)
        plane = np.ascontiguousarray(stack[..., channel])
        given2 = None if given is None else egg._template2_of(given)
        template2 = egg.stack_median2_host(plane) if given is None else given2
        sums = egg.orientation_sums_host(plane, template2)
        by_mode = {}
        for mode in MODES:
            flags = egg.orientation_flags_host(sums, template2, mode)
            turned = stack.copy()
            turned[flags] = stack[flags][:, ::-1, ::-1, :]
            by_mode[mode] = flags, turned
        _REF[key] = stack, given2, template2, sums, by_mode
    return _REF[key]


@pytest.mark.parametrize('name', DEVICE_CASES)
def test_stack_median_equals_the_integer_statement(hip, egg, name):
    stack, _ = C.cropped(name)
    got = hip.stack_median(stack, 0)
    assert got is not None, 'the entry refused a case inside its caps'
    assert C.same(got, egg.stack_median2_host(np.ascontiguousarray(stack[..., 0]))), name
    assert C.same(egg.compute_mean_image(C.case(name)[0], on='device'), got / 2.)


@pytest.mark.parametrize('name', DEVICE_CASES)
@pytest.mark.parametrize('mode', MODES)
def test_orient_stack_equals_the_integer_statements(hip, egg, name, mode):
    stack, given2, template2, sums, by_mode = reference(egg, name)
    flags, turned = by_mode[mode]
    got = hip.orient_stack(stack, 0, mode, given2)
    assert got is not None, 'the entry refused a case inside its caps'
    assert C.same(got[0], template2), name
    assert C.same(got[2], sums), (name, np.argwhere(got[2] != sums)[:5])
    assert C.same(got[1], flags), name
    assert C.same(got[3], turned), name
    assert got[3] is not stack
    own = stack.copy()
    again = hip.orient_stack(own, 0, mode, given2, in_place=True)
    assert again[3] is own and C.same(own, turned)


@pytest.mark.parametrize('name', DEVICE_CASES)
@pytest.mark.parametrize('mode', MODES)
def test_swap_orientations_on_the_device_is_the_composition_of_the_integer_statements(egg, name, mode):
    stack, _, template2, _, by_mode = reference(egg, name)
    flags, turned = by_mode[mode]
    images, given = C.case(name)
    oriented, got_flags, template = egg.swap_orientations(images, mode, given, on='device')
    assert C.same(got_flags, flags)
    assert C.same(template, template2 / 2.) and template.dtype == np.float64
    assert len(oriented) == len(images) and all(C.same(a, b) for a, b in zip(oriented, turned))


def test_the_swap_brings_the_turned_ramps_back(egg):
    images, _ = C.case('ramp_half_turned')
    oriented, flags, _ = egg.swap_orientations(images, on='device')
    assert np.array_equal(flags, np.arange(13) % 2 == 1)
    assert all(np.array_equal(img, images[i][::-1, ::-1] if i % 2 else images[i]) for i, img in enumerate(oriented))


@pytest.mark.parametrize('channel', [1, 3])
def test_another_channel(hip, egg, channel):
    stack, _, template2, sums, by_mode = reference(egg, 'c4', channel)
    got = hip.orient_stack(stack, channel, 'cc')
    assert C.same(got[0], template2) and C.same(got[2], sums) and C.same(got[1], by_mode['cc'][0]) and C.same(got[3], by_mode['cc'][1])
    assert C.same(hip.stack_median(stack, channel), template2)


def test_same_bytes_on_stale_scratch(hip, egg):
    """the larger call first (the n65535 stack), then the scratch filled with ``0x7F`` words, then the same calls twice"""
    ctx = hip.Context()
    try:
        big, _ = C.cropped('n65535')
        assert hip.orient_stack(big, 0, 'cc', ctx=ctx) is not None
        assert ctx.poison(0x7F7F7F7F) > 0
        for _ in range(2):                               # poisoned, then stale data of the same entries at the same size
            for name in ('px1025', 'ragged', 'given_half_template', 'c1', 'px1'):
                stack, given2, template2, sums, by_mode = reference(egg, name)
                for mode in MODES:
                    got = hip.orient_stack(stack, 0, mode, given2, ctx=ctx)
                    assert C.same(got[0], template2) and C.same(got[2], sums), (name, mode)
                    assert C.same(got[1], by_mode[mode][0]) and C.same(got[3], by_mode[mode][1]), (name, mode)
                assert C.same(hip.stack_median(stack, 0, ctx=ctx), egg.stack_median2_host(np.ascontiguousarray(stack[..., 0])))
    finally:
        ctx.close()


def test_what_the_caps_exclude_returns_none_and_runs_the_host_statements(hip, egg, monkeypatch):
    many = np.zeros((65536, 1, 1, 1), dtype=np.uint8)
    assert hip.stack_median(many) is None and hip.orient_stack(many) is None
    wide = np.zeros((2, 3, 3, 5), dtype=np.uint8)
    assert hip.stack_median(wide) is None and hip.orient_stack(wide) is None
    large = np.zeros((1, 1 << 15, (1 << 15) + 1, 1), dtype=np.uint8)       # more than 2^30 pixels (never touched: refused first)
    assert hip.stack_median(large) is None
    del large
    heavy = np.zeros((2, 1 << 15, 1 << 15, 1), dtype=np.uint8)             # 2^31 bytes
    assert hip.stack_median(heavy) is None
    del heavy
    with pytest.raises(hip.HipError):
        hip.orient_stack(np.zeros((2, 3, 3, 1), dtype=np.uint8), template2=np.full((3, 3), 511))
    # the public function: five channels and a template that is no half-integer never reach the entry
    calls = []
    real = hip.orient_stack
    monkeypatch.setattr(hip, 'orient_stack', lambda *a, **k: calls.append(1) or real(*a, **k))
    rng = np.random.RandomState(5)
    images = [rng.randint(0, 256, (6, 9, 5)).astype(np.uint8) for _ in range(7)]
    for mode in MODES:
        a, b = egg.swap_orientations(images, mode, on='device'), egg.swap_orientations(images, mode, on='host')
        assert C.same(a[1], b[1]) and C.same(a[2], b[2]) and all(C.same(x, y) for x, y in zip(a[0], b[0]))
    images, given = C.case('given_other_template')
    a, b = egg.swap_orientations(images, 'cc', given, on='device'), egg.swap_orientations(images, 'cc', given, on='host')
    assert C.same(a[1], b[1]) and all(C.same(x, y) for x, y in zip(a[0], b[0]))
    assert not calls
    assert C.same(egg.compute_mean_image([img for img in wide], on='device'), np.zeros((3, 3)))
