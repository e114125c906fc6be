"""``imsegm_center_levels`` / ``imsegm_correct_segm`` (csrc/center_annotation.hip) at the wave, workgroup and search-window edges their
golden cases do not reach (the edge tables of tests/center_annotation_cases.py; CPU twins in
tests/test_center_annotation_reference_host.py).  ``imsegm_debug_center_distances`` hands out what ``imsegm_center_levels`` holds in
front of its code pass, computed by the function that entry calls:

* the squared-distance map equals the brute-force integer minimum over all pixels of another value (and scipy's per-label distance
  transform, squared) where the nearest foreign pixel is exactly 255, 256, 257, 511, 512 or 513 columns away, on the left only or
  on the right only, in the same row or some rows off, for pixels of the first, a middle and the last workgroup of a row; where
  some columns hold no foreign pixel; where two labels alternate column by column; on one row, one column and a map of one value;
* max2, pixel count, row sum and column sum per label equal int64 numpy sums there and on every run-rule map (widths 64 .. 513);
* level maps and centres equal the host statement byte for byte on the same maps;
* the correction chain equals the host statement and its restatement from scipy's parts at a width of 320: a blob across columns
  255 / 256, a component of exactly ``min_size`` pixels in two workgroups, two blobs that touch only diagonally across the boundary;
* every call twice in one context with equal bytes (the order of the atomics)."""
import numpy as np
import pytest

import center_annotation_cases as C
import cut_objects_cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def hip():
    from pyimsegm_amd import _hip
    _hip.default_context()
    return _hip


@pytest.fixture(scope='module')
def annot():
    from pyimsegm_amd import center_annotation
    return center_annotation


def _check_front(hip, seg, max_label, what):
    want_d2 = C.expected_d2(seg, max_label)
    want_max2, want_sums = C.expected_words(seg, want_d2, max_label)
    first = hip.center_distances(seg, max_label)
    d2, max2, sums = first
    assert d2.dtype == np.uint32 and d2.shape == seg.shape and max2.dtype == np.uint32 and sums.dtype == np.int64
    wrong = np.argwhere(d2 != want_d2)
    assert len(wrong) == 0, (what, len(wrong), [(int(r), int(c), int(d2[r, c]), int(want_d2[r, c])) for r, c in wrong[:6]])
    assert max2.tolist() == want_max2 and sums.tolist() == want_sums, what
    again = hip.center_distances(seg, max_label)
    assert all(C.same(a, b) for a, b in zip(first, again)), what
    return want_d2


@pytest.mark.parametrize('name', list(C.ROW_CASES))
def test_row_case_distances_and_words(hip, name):
    case = C.row_case(name)
    seg = case['seg']
    want = _check_front(hip, seg, int(seg.max()), name)
    assert np.array_equal(want, np.where(seg > 0, C.edt_d2(seg), 0)) or name == 'no_foreign_3x257'
    for r, c, dc, side, dr in case['probes']:
        assert want[r, c] == dc * dc + dr * dr
    if name not in ('alternate_columns', 'one_column'):
        assert want.max() >= C.WINDOW ** 2                                  # a search of 256 columns or more
    # a larger table than the map needs: slots without a pixel stay 0
    d2, max2, sums = hip.center_distances(seg, 7)
    assert np.array_equal(d2, want) and not max2[int(seg.max()):].any() and not sums[int(seg.max()):].any()


@pytest.mark.parametrize('name', list(C.ROW_CASES))
def test_row_case_levels_and_centres_equal_the_host_statement(hip, annot, name):
    case = C.row_case(name)
    seg = case['seg']
    for _ in range(2):
        assert C.same(annot.segm_center_levels(seg, case['levels'], on='device'), annot.segm_center_levels_host(seg, case['levels'])), name
        assert C.same(annot.compute_eggs_center(seg, on='device'), annot.compute_eggs_center_host(seg)), name
    finer = [0., 0.1, 0.3, 0.33, 0.5, 0.66, 0.9, 0.99]
    assert C.same(annot.segm_center_levels(seg, finer, on='device'), annot.segm_center_levels_host(seg, finer)), name


@pytest.mark.parametrize('width', cut_objects_cases.RUN_WIDTHS)
def test_run_rule_sums_distances_and_levels(hip, annot, width):
    assert (-(-width // cut_objects_cases.CHUNK) > 1) == (width > 256)
    for layout in cut_objects_cases.RUN_LAYOUTS:
        seg = cut_objects_cases.run_map(width, layout)
        reached = cut_objects_cases.run_branches(seg)
        for need, widths in cut_objects_cases.RUN_REACH[layout] + cut_objects_cases.RUN_REACH_ALWAYS:
            if (widths is None or width in widths) and need != 'unlisted between listed':
                assert need in reached, (width, layout, need)
        _check_front(hip, seg, 3, (width, layout))
        _check_front(hip, seg, 2, (width, layout, 'labels above 2 are background'))
        assert C.same(annot.compute_eggs_center(seg, on='device'), annot.compute_eggs_center_host(seg)), (width, layout)
        assert C.same(annot.segm_center_levels(seg, C.LEVELS, on='device'), annot.segm_center_levels_host(seg, C.LEVELS)), (width, layout)


@pytest.mark.parametrize('name', list(C.CORRECT_EDGE_CASES))
def test_correction_chain_at_the_workgroup_boundary(hip, annot, name):
    case = C.correct_edge_case(name)
    host_seg, host_lb = annot.correct_segm_host(**case)
    scipy_seg, scipy_lb = C.scipy_correct(**case)
    assert C.same(host_seg, scipy_seg) and C.same(host_lb, scipy_lb)
    assert (host_seg[:, 255] & host_seg[:, 256]).any() and case['img'].shape[1] == 320
    for _ in range(2):
        seg, seg_lb = annot.correct_segm(case['img'], case['sel_radius'], case['min_size'], on='device')
        assert C.same(seg, host_seg) and C.same(seg_lb, host_lb), name
        level_map, centres = annot.create_annot_centers(case['img'], C.LEVELS, on='device', sel_radius=case['sel_radius'],
                                                        min_size=case['min_size'])
        want_map, want_centres = annot.create_annot_centers_host(case['img'], C.LEVELS, case['sel_radius'], case['min_size'])
        assert C.same(level_map, want_map) and C.same(centres, want_centres), name
    # min_size + 1: the components of exactly min_size pixels go as well
    seg_more, _ = annot.correct_segm(case['img'], case['sel_radius'], case['min_size'] + 1, on='device')
    assert C.same(seg_more, annot.correct_segm_host(case['img'], case['sel_radius'], case['min_size'] + 1)[0])
    assert seg_more.sum() < host_seg.sum()
