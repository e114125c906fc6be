"""The host statements of pyimsegm_amd/center_annotation.py, the definitions the device entries are held to:

* byte for byte the arrays the reference's ``load_correct_segm`` / ``segm_set_center_levels`` returned and wrote under scipy 1.7.1 /
  scikit-image 0.18.3 (tests/golden/center_annotation.npz, made by tests/golden/make_golden_center_annotation.py), centres to the
  last bit;
* every case of tests/center_annotation_cases.py lies on the side of its rule that it is named for;
* the public names, the place switch, the errors for bad input, the doctests."""
import doctest

import numpy as np
import pytest
from scipy import ndimage

import center_annotation_cases as C

from pyimsegm_amd import center_annotation as annot

ALL_LEVEL_CASES = list(C.LEVEL_CASES) + list(C.HOST_ONLY)


@pytest.fixture(scope='module')
def golden():
    return C.load_golden()


@pytest.mark.parametrize('name', ALL_LEVEL_CASES)
def test_levels_and_centres_equal_the_reference(golden, name):
    inputs = C.level_case(name)
    assert C.same(inputs['seg'], golden[name + '_seg'])
    got = annot.segm_center_levels(inputs['seg'], inputs['levels'], on='host')
    assert got.dtype == inputs['seg'].dtype and C.same(got.astype(np.uint8), golden[name + '_levels']), name
    assert C.same(annot.compute_eggs_center(inputs['seg'], on='host'), golden[name + '_centres']), name


@pytest.mark.parametrize('name', list(C.CORRECT_CASES) + ['sample'])
def test_correction_equals_the_reference(golden, name):
    inputs = C.correct_case(name) if name in C.CORRECT_CASES else dict(img=golden[name + '_img'], sel_radius=25, min_size=64)
    assert C.same(inputs['img'], golden[name + '_img'])
    seg, seg_lb = annot.correct_segm(inputs['img'], inputs['sel_radius'], inputs['min_size'], on='host')
    assert C.same(seg, golden[name + '_seg']) and C.same(seg_lb, golden[name + '_seg_lb'])
    level_map, centres = annot.create_annot_centers(inputs['img'], on='host', sel_radius=inputs['sel_radius'], min_size=inputs['min_size'])
    assert C.same(level_map, golden[name + '_levels']) and C.same(centres, golden[name + '_centres'])
    assert len(centres) == seg_lb.max() >= 2


def _levels_of(name, label=1):
    inputs = C.level_case(name)
    return inputs, annot.object_levels_host(inputs['seg'] == label, inputs['levels'])


def test_touching_eggs_see_each_other_as_background():
    inputs, levels = _levels_of('touching')
    seg = inputs['seg']
    assert (seg[20, 43], seg[20, 44]) == (1, 2)
    together = ndimage.distance_transform_edt(seg > 0)
    alone = ndimage.distance_transform_edt(seg == 1)
    assert alone[20, 43] == 1 and together[20, 43] > 5
    assert not levels[1][0][20, 40:44].any()


def test_the_image_border_is_no_background():
    inputs, levels = _levels_of('border')
    distance = ndimage.distance_transform_edt(inputs['seg'] == 1)
    assert (inputs['seg'][0] == 1).any() and distance[0].max() > 0.4 * distance.max() > 1      # probab > 0.4 reaches the first row
    assert levels[1][1] == (distance / distance.max() > 0.4).sum()


def test_hole_missing_label_and_row_segment():
    inputs, levels = _levels_of('hole')
    assert ndimage.label(inputs['seg'] == 0)[1] == 2 and not levels[0][0][30, 46]
    seg = C.level_case('missing_label')['seg']
    assert sorted(np.unique(seg).tolist()) == [0, 1, 3, 6] and len(annot.compute_eggs_center_host(seg)) == 3
    seg = C.level_case('row_segment')['seg']
    assert (seg[6:35] == 1).all() and seg.shape[1] > 2 * 256 + 128


def test_opening_radii_of_the_cases():
    for name, label, wanted in (('small_egg', 1, [0, 0]), ('small_egg', 3, [0, 0]), ('open1', 1, [1, 0]), ('open64', 1, [64]),
                                ('open65', 1, [65]), ('split', 1, [2, 0])):
        _, levels = _levels_of(name, label)
        assert [opening for _, _, _, opening in levels[1:]] == wanted, name
    _, levels = _levels_of('small_egg', 3)
    assert [count for _, count, _, _ in levels] == [1, 1, 1] and [radius for _, _, radius, _ in levels[1:]] == [0, 0]
    assert levels[0][0].sum() == 1 and not levels[1][0].any()               # one pixel: level 1 alone
    _, levels = _levels_of('open64')
    assert levels[1][2] in range(427, 434) and annot.level_geometry(levels[1][1]) == (levels[1][2], 64)


def test_probab_equal_to_a_level_stays_out():
    inputs, levels = _levels_of('tie')
    distance = ndimage.distance_transform_edt(inputs['seg'] == 1)
    assert distance.max() == 5 and (distance == 2).sum() == 24
    assert 2. / 5. == 0.4 and levels[1][1] == (distance > 2).sum() == 25   # the 24 pixels at the tie are not counted


def test_the_opening_splits_a_level_mask():
    inputs, levels = _levels_of('split')
    from pyimsegm_amd.ellipse_fitting import ellipse_pixels_host
    _, count, radius, opening = levels[1]
    rows, cols = np.nonzero(inputs['seg'] == 1)
    distance = ndimage.distance_transform_edt(inputs['seg'] == 1)
    before = distance / distance.max() > inputs['levels'][1]
    disc = np.zeros_like(before)
    disc[ellipse_pixels_host(rows.mean(), cols.mean(), radius, radius, 0., before.shape)] = True
    eight = np.ones((3, 3))
    assert ndimage.label(before & disc, eight)[1] == 1 and ndimage.label(levels[1][0], eight)[1] == 2 and opening == 2


@pytest.mark.parametrize('radius', [1, 2])
def test_rules_of_the_correction_cases(golden, radius):
    name = 'correct_r%d' % radius
    inputs = C.correct_case(name)
    opened = annot.opening_host(inputs['img'] > 0, radius)
    assert opened.sum() < (inputs['img'] > 0).sum()                         # the specks went
    parts, _ = ndimage.label(opened)
    sizes = np.bincount(parts.ravel())[1:].tolist()
    assert inputs['min_size'] - 1 in sizes and inputs['min_size'] in sizes
    seg, seg_lb = annot.correct_segm_host(**inputs)
    assert ndimage.label(seg)[1] == len(sizes) - 1 == seg_lb.max() + 1      # one component removed, two joined by a diagonal
    # raster order of the first pixels; the U is one label, the blob inside it another
    firsts = [np.flatnonzero(seg_lb.ravel() == label)[0] for label in range(1, seg_lb.max() + 1)]
    assert firsts == sorted(firsts)
    u_label = seg_lb[30, 44]
    assert u_label == seg_lb[30, 8] == seg_lb[40, 25] and seg_lb[14, 25] not in (0, u_label)
    assert seg_lb[:, 0].max() > 0 and seg_lb[0].max() > 0                   # blobs on the border


def test_public_names_and_switch(monkeypatch):
    assert annot.DISTANCE_LEVELS == [0., 0.4, 0.8]
    for name in ('correct_segm', 'compute_eggs_center', 'segm_center_levels', 'create_annot_centers'):
        assert callable(getattr(annot, name)) and callable(getattr(annot, name + '_host')) and name in annot.__all__
    monkeypatch.setenv('IMSEGM_CENTER_ANNOT_ON', 'host')
    assert annot._place(None) == 'host' and annot._place('host') == 'host'
    monkeypatch.setenv('IMSEGM_CENTER_ANNOT_ON', 'nowhere')
    with pytest.raises(ValueError):
        annot._place(None)


def test_errors_for_bad_input():
    for function in (annot.segm_center_levels, annot.compute_eggs_center):
        with pytest.raises(ValueError, match='2-D integer'):
            function(np.zeros((3, 4, 5), dtype=np.int32), on='host')
        with pytest.raises(ValueError, match='2-D integer'):
            function(np.zeros((3, 4), dtype=np.float64), on='host')
    for function in (annot.correct_segm, annot.create_annot_centers):
        with pytest.raises(ValueError, match='2-D numeric'):
            function(np.zeros((3, 4, 3), dtype=np.uint8), on='host')
    with pytest.raises(ValueError):
        annot.correct_segm(np.zeros((3, 4)), sel_radius=-1, on='host')
    with pytest.raises(ValueError):
        annot.segm_center_levels(np.zeros((3, 4), dtype=int), [0., np.nan], on='host')
    with pytest.raises(ValueError):
        annot.segm_center_levels(np.zeros((3, 4), dtype=int), on='somewhere')
    empty = np.zeros((5, 6), dtype=np.int16)
    assert not annot.segm_center_levels(empty, on='host').any() and annot.compute_eggs_center(empty, on='host').shape == (0, 2)


def test_doctests():
    from doctests.center_annotation import EXAMPLES
    parser, runner = doctest.DocTestParser(), doctest.DocTestRunner(verbose=False)
    for name, text in EXAMPLES.items():
        runner.run(parser.get_doctest(text, dict(annot.__dict__), name, 'tests/doctests/center_annotation.py', 0))
    result = runner.summarize(verbose=False)
    assert result.failed == 0 and result.attempted >= 12
