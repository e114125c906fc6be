"""The host statements of pyimsegm_amd/egg_segmentation.py against scikit-image 0.18.3 (tests/golden/watershed.npz, written by
tests/golden/make_golden_watershed.py) and the interface of ``segment_watershed``; no device.

* ``watershed_post_morph_host`` on scikit-image's flood maps equals its cleaned maps byte for byte;
* ``watershed_markers_host`` -- the round definition -- equals scikit-image's flood outside a differing set whose pixels lie within
  Chebyshev distance 2 of a pixel to which scikit-image gave the definition's label, at most 1 % of the labelled pixels, and of the
  size the fixture recorded."""
import os

import numpy as np
import pytest
from scipy import ndimage

import watershed_cases as C

from pyimsegm_amd import egg_segmentation as E
from pyimsegm_amd.ellipse_fitting import fill_holes_host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def golden():
    return C.load_golden()


@pytest.fixture(autouse=True)
def on_host(monkeypatch):
    monkeypatch.setenv('IMSEGM_WATERSHED_ON', 'host')


@pytest.mark.parametrize('name', list(C.GOLDEN_CASES))
def test_inputs_are_the_ones_the_fixture_was_written_for(golden, name):
    assert int(golden[name + '_crc']) == C.crc(C.golden_case(name)[0])
    assert str(golden['skimage_version']) == '0.18.3'
    assert bool(golden[name + '_flood_sqrt'])            # -d^2 gave scikit-image the map of -d
    assert golden[name + '_flood'].shape[0] <= 192 and golden[name + '_flood'].shape[1] <= 256


@pytest.mark.parametrize('name', list(C.GOLDEN_CASES))
def test_clean_up_equals_scikit_image_byte_for_byte(golden, name):
    assert C.same(E.watershed_post_morph_host(golden[name + '_flood']), golden[name + '_clean'])
    assert C.same(E.watershed_post_morph(golden[name + '_flood']), golden[name + '_clean'])


@pytest.mark.parametrize('name', list(C.GOLDEN_CASES))
def test_round_definition_equals_scikit_image_away_from_the_ridges(golden, name):
    seg, centres = C.golden_case(name)
    theirs = golden[name + '_flood']
    ours = E.watershed_markers_host(fill_holes_host(seg > 0), C.markers_of(seg.shape, centres))
    assert ours.dtype == np.int32
    differs = ours != theirs
    labelled = int(np.sum(theirs > 0))
    print('%s: %d of %d labelled pixels differ (fixture: %d)' % (name, differs.sum(), labelled, int(golden[name + '_differs'])))
    assert np.array_equal(ours > 0, theirs > 0)
    assert int(differs.sum()) == int(golden[name + '_differs'])
    assert differs.sum() <= 0.01 * labelled
    for label in np.unique(ours[differs]):
        near = ndimage.binary_dilation(theirs == label, structure=np.ones((5, 5), dtype=bool))
        assert np.all(near[differs & (ours == label)]), label


def test_two_discs_are_split_between_their_centres(golden):
    segm = golden['two_discs_flood']
    assert segm[60, 55] == 1 and segm[60, 112] == 2 and segm[60, 20] == 1 and segm[60, 138] == 2 and segm[0, 0] == 0


# ---- the interface ---------------------------------------------------------------------------------------------------------------

def test_segment_watershed_returns_the_triple_of_the_reference(golden):
    seg, centres = C.golden_case('three_discs')
    segm, back, third = E.segment_watershed(seg, centres)
    assert back is centres and third is None
    assert segm.dtype == np.int32 and segm.shape == seg.shape
    assert C.same(segm, E.watershed_markers_host(fill_holes_host(seg), C.markers_of(seg.shape, centres)))
    cleaned = E.segment_watershed(seg, centres, post_morph=True)[0]
    assert cleaned.dtype == np.int32 and C.same(cleaned, E.watershed_post_morph_host(segm))
    assert C.same(cleaned, E.segment_watershed_host(seg, centres, True)[0])


@pytest.mark.parametrize('dtype', [np.uint8, np.int64, np.float32])
def test_bool_and_numeric_input_give_the_same_map(dtype):
    seg, centres = C.golden_case('two_components')
    wide = seg.astype(dtype) * 3
    assert C.same(E.segment_watershed(wide, centres, True)[0], E.segment_watershed(seg, centres, True)[0])


def test_a_later_centre_replaces_an_earlier_one_on_the_same_pixel(golden):
    seg, centres = C.golden_case('two_components')
    assert centres[2] == centres[3]
    segm = E.segment_watershed(seg, centres)[0]
    assert 3 not in segm and segm[55, 145] == 4
    theirs = golden['two_components_flood']
    assert 3 not in theirs and theirs[55, 145] == 4


def test_centres_are_truncated():
    seg, _ = C.golden_case('two_discs')
    a = E.segment_watershed(seg, [(60.9, 55.9), (60.2, 112.5)])[0]
    assert C.same(a, E.segment_watershed(seg, [(60, 55), (60, 112)])[0])


def test_a_centre_outside_the_mask_yields_no_label():
    seg, _ = C.golden_case('two_discs')
    segm = E.segment_watershed(seg, [(2, 2), (60, 55)])[0]
    assert set(np.unique(segm)) == {0, 2} and np.array_equal(segm > 0, seg)
    with pytest.raises(IndexError):
        E.segment_watershed(seg, [(500, 2)])


def test_empty_mask_and_no_centres():
    empty = np.zeros((20, 30), dtype=bool)
    for post in (False, True):
        segm = E.segment_watershed(empty, [(3, 3)], post)[0]
        assert segm.dtype == np.int32 and segm.shape == empty.shape and not segm.any()
        seg, _ = C.golden_case('two_discs')
        segm = E.segment_watershed(seg, [], post)[0]
        assert segm.dtype == np.int32 and segm.shape == seg.shape and not segm.any()


def test_markers_with_explicit_keys_and_the_switch(monkeypatch):
    mask, markers, keys = C.FLOOD_CASES['random_keys']()
    a = E.watershed_markers(mask, markers, keys)
    assert C.same(a, E.watershed_markers_host(mask, markers, keys))
    assert C.same(a, E.watershed_markers(mask, markers, keys, on='host'))
    assert not a[~mask].any() and np.array_equal(a[(markers != 0) & mask], markers[(markers != 0) & mask])
    monkeypatch.setenv('IMSEGM_WATERSHED_ON', 'nowhere')
    with pytest.raises(ValueError):
        E.watershed_markers(mask, markers, keys)


def test_plateau_is_split_in_the_middle():
    mask, markers, _ = C.FLOOD_CASES['plateau_bar']()
    segm = E.watershed_markers_host(mask, markers)
    assert np.array_equal(segm > 0, mask)
    assert np.all(segm[7, 6:60] == 1) and np.all(segm[7, 70:124] == 2)


def test_entries_are_declared_and_exported():
    from pyimsegm_amd import _hip
    header = open(os.path.join(ROOT, 'include', 'imsegm_hip.h')).read()
    for name in ('imsegm_watershed', 'imsegm_watershed_markers', 'imsegm_watershed_post_morph'):
        assert name + '(' in header and name in _hip.EXPORTED_SYMBOLS
    assert '#define IMSEGM_WATERSHED_MAX_LABELS %d' % _hip.WATERSHED_MAX_LABELS in header
