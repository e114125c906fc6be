"""``imsegm_watershed`` / ``imsegm_watershed_markers`` / ``imsegm_watershed_post_morph`` (csrc/watershed.hip with the kernels of
csrc/morphology.hip, boundary.hip and center_annotation.hip) behind pyimsegm_amd/egg_segmentation.py: the device equals the host
statements byte for byte

* on every flood case of tests/watershed_cases.py: overlapping discs, a plateau, an unmarked lobe, components with and without a
  marker, a centre in a hole, a mask on all four borders, a frontier wider than a workgroup, adjacent markers, 1 and 1024 labels;
* on every clean-up case: objects at the border, overlapping closings, an object the opening removes, a box of several tiles, the
  radii 0, 1 and 64;
* end to end, on the golden cases, against the composition of the two host statements and (clean-up) scikit-image's bytes;
* on a context whose scratch holds stale data;
* and what the caps exclude takes the host path."""
import numpy as np
import pytest

import watershed_cases as C

pytestmark = pytest.mark.gpu

WORDS = (0x00000001, 0x7F7F7F7F)
_REF = {}


def cached(key, make):
    if key not in _REF:
        _REF[key] = make()
    return _REF[key]


@pytest.fixture(scope='module')
def hip():
    from pyimsegm_amd import _hip
    _hip.default_context()
    return _hip


@pytest.fixture(scope='module')
def egg():
    from pyimsegm_amd import egg_segmentation
    return egg_segmentation


@pytest.fixture(scope='module')
def golden():
    return C.load_golden()


def flood_reference(egg, name):
    def make():
        mask, markers, keys = C.FLOOD_CASES[name]()
        return mask, markers, keys, egg.watershed_markers_host(mask, markers, keys)
    return cached(('flood', name), make)


def morph_reference(egg, name):
    def make():
        segm, radius_close, radius_open = C.MORPH_CASES[name]()
        return segm, radius_close, radius_open, egg.watershed_post_morph_host(segm, radius_close, radius_open)
    return cached(('morph', name), make)


@pytest.mark.parametrize('name', list(C.FLOOD_CASES))
def test_flood_equals_the_host_definition(hip, egg, name):
    mask, markers, keys, ref = flood_reference(egg, name)
    seeds = np.flatnonzero(mask & (markers != 0))
    raw = hip.watershed_markers(mask, seeds, markers.ravel()[seeds], keys)
    assert raw is not None, 'the entry refused a case inside its caps'
    assert C.same(raw, ref), name
    assert C.same(egg.watershed_markers(mask, markers, keys, on='device'), ref), name


def test_flood_cases_are_what_their_names_say(egg):
    ref = flood_reference(egg, 'components')[3]
    assert set(np.unique(ref)) == {0, 1, 2} and not ref[45, 160]
    ref = flood_reference(egg, 'hole_with_centre')
    assert set(np.unique(ref[3])) == {0, 2} and not ref[0][50, 60]
    mask, markers, _, ref = flood_reference(egg, 'unmarked_lobe')
    assert np.array_equal(ref == 1, mask)
    assert len(np.unique(flood_reference(egg, 'strip_1024_labels')[3])) == 1025
    assert np.sum(flood_reference(egg, 'strip_1_label')[3] > 0) == 2
    mask, markers, keys, ref = flood_reference(egg, 'wide_frontier')
    replayed, longest = C.max_frontier(mask, markers, keys)
    print('wide_frontier: the longest frontier has %d pixels' % longest)
    assert C.same(replayed, ref) and longest > 2 * 1024, 'the list of a round takes more than two trips of a workgroup of 1024'


@pytest.mark.parametrize('name', list(C.MORPH_CASES))
def test_clean_up_equals_the_host_statement(hip, egg, name):
    segm, radius_close, radius_open, ref = morph_reference(egg, name)
    raw = hip.watershed_post_morph(segm, radius_close, radius_open)
    assert raw is not None, 'the entry refused a case inside its caps'
    assert C.same(raw, ref), name
    assert C.same(egg.watershed_post_morph(segm.astype(np.int64), radius_close, radius_open, on='device'), ref), name


def test_clean_up_cases_are_what_their_names_say(egg):
    segm, _, _, ref = morph_reference(egg, 'removed_by_opening')
    assert 2 in segm and set(np.unique(ref)) == {0, 1}
    segm, _, _, ref = morph_reference(egg, 'overlapping_closings')
    # both labels claim both bars of specks after their closings: the later label is painted over the earlier one
    assert np.all(ref[39:41, 32:47] == 2) and np.all(ref[36, 31:48] == 1) and np.all(ref[38:42, 75:95] == 2)


@pytest.mark.parametrize('name', list(C.GOLDEN_CASES))
@pytest.mark.parametrize('post_morph', [False, True])
def test_segment_watershed_equals_the_composition_of_the_host_statements(egg, golden, name, post_morph):
    seg, centres = C.golden_case(name)
    ref = cached(('segment', name, post_morph), lambda: egg.segment_watershed_host(seg, centres, post_morph)[0])
    segm, back, third = egg.segment_watershed(seg, centres, post_morph, on='device')
    assert back is centres and third is None
    assert C.same(segm, ref)
    assert C.same(egg.segment_watershed(seg.astype(np.int32) * 2, centres, post_morph, on='device')[0], ref)
    if post_morph:
        assert C.same(egg.watershed_post_morph(golden[name + '_flood'], on='device'), golden[name + '_clean'])


def test_empty_mask_no_centres_and_a_single_pixel(egg):
    empty = np.zeros((20, 30), dtype=bool)
    for post in (False, True):
        assert not egg.segment_watershed(empty, [(3, 3)], post, on='device')[0].any()
        assert not egg.segment_watershed(~empty, [], post, on='device')[0].any()
    one = np.ones((1, 1), dtype=bool)
    assert C.same(egg.segment_watershed(one, [(0, 0)], on='device')[0], egg.segment_watershed_host(one, [(0, 0)])[0])


def test_what_the_caps_exclude_runs_the_host_statement(hip, egg, monkeypatch):
    mask, markers, keys, ref = flood_reference(egg, 'marker_regions')
    high = np.where(markers == 7, 5000, markers)
    calls = []
    real = hip.watershed_markers
    monkeypatch.setattr(hip, 'watershed_markers', lambda *a, **k: calls.append(1) or real(*a, **k))
    assert C.same(egg.watershed_markers(mask, high, keys, on='device'), egg.watershed_markers_host(mask, high, keys))
    assert not calls
    seeds = np.flatnonzero(mask & (high != 0))
    assert real(mask, seeds, high.ravel()[seeds], keys) is None          # IMSEGM_E_OBJECT_CAPS, no error
    segm, _, _, _ = morph_reference(egg, 'missing_labels')
    assert hip.watershed_post_morph(segm, 65, 3) is None
    assert C.same(egg.watershed_post_morph(segm, 65, 3, on='device'), egg.watershed_post_morph_host(segm, 65, 3))
    assert hip.watershed_post_morph(np.where(segm == 5, 1025, segm), 2, 4) is None


@pytest.mark.parametrize('word', WORDS)
def test_same_bytes_on_stale_scratch(hip, egg, golden, monkeypatch, word):
    """the dirtier call: a larger clean-up and a larger flood on the same context; then the scratch is filled with ``word``"""
    ctx = hip.Context()
    try:
        monkeypatch.setattr(hip, 'default_context', lambda: ctx)
        segm, radius_close, radius_open, _ = morph_reference(egg, 'several_tiles')
        assert hip.watershed_post_morph(segm, radius_close, radius_open, ctx=ctx) is not None
        mask, markers, keys, ref = flood_reference(egg, 'wide_frontier')
        assert C.same(egg.watershed_markers(mask, markers, keys, on='device'), ref)
        assert ctx.poison(word) > 0
        for _ in range(2):                                   # poisoned, then stale data of the same entries at the same size
            for name in ('random_keys', 'components', 'adjacent_markers'):
                mask, markers, keys, ref = flood_reference(egg, name)
                assert C.same(egg.watershed_markers(mask, markers, keys, on='device'), ref), name
            segm, radius_close, radius_open, ref = morph_reference(egg, 'overlapping_closings')
            assert C.same(egg.watershed_post_morph(segm, radius_close, radius_open, on='device'), ref)
            seg, centres = C.golden_case('two_components')
            assert C.same(egg.segment_watershed(seg, centres, True, on='device')[0], egg.segment_watershed_host(seg, centres, True)[0])
    finally:
        ctx.close()
