"""``imsegm_correct_segm`` / ``imsegm_center_levels`` / ``imsegm_create_annot_centers`` (csrc/center_annotation.hip, the label-aware
disc kernels of csrc/morphology.hip) behind pyimsegm_amd/center_annotation.py:

* every case of tests/center_annotation_cases.py through ``on='device'`` equals the host statement and the arrays the reference
  wrote (tests/golden/center_annotation.npz) byte for byte, centres to the last bit;
* ``create_annot_centers`` equals the three single calls;
* the capped cases take the host path: the entry answers with the caps status (None) or is never called;
* the same bytes on a context whose scratch holds stale data."""
import numpy as np
import pytest

import center_annotation_cases as C

pytestmark = pytest.mark.gpu

WORDS = (0x00000001, 0x7F7F7F7F)


@pytest.fixture(scope='module')
def hip():
    from pyimsegm_amd import _hip
    _hip.default_context()
    return _hip


@pytest.fixture(scope='module')
def annot():
    from pyimsegm_amd import center_annotation
    return center_annotation


@pytest.fixture(scope='module')
def golden():
    return C.load_golden()


def _check_levels(annot, golden, name):
    inputs = C.level_case(name)
    got = annot.segm_center_levels(inputs['seg'], inputs['levels'], on='device')
    assert C.same(got, golden[name + '_levels'].astype(np.int32)), name
    centres = annot.compute_eggs_center(inputs['seg'], on='device')
    assert C.same(centres, golden[name + '_centres']), name
    return inputs, got, centres


@pytest.mark.parametrize('name', list(C.LEVEL_CASES))
def test_levels_and_centres_equal_the_reference_and_the_host_statement(annot, golden, name):
    inputs, got, centres = _check_levels(annot, golden, name)
    assert C.same(got, annot.segm_center_levels_host(inputs['seg'], inputs['levels']))
    assert C.same(centres, annot.compute_eggs_center_host(inputs['seg']))


@pytest.mark.parametrize('dtype', [np.uint8, np.int64, np.uint16])
def test_levels_keep_the_dtype_of_the_map(annot, golden, dtype):
    seg = C.level_case('missing_label')['seg'].astype(dtype)
    got = annot.segm_center_levels(seg, on='device')
    assert C.same(got, golden['missing_label_levels'].astype(dtype))


def _check_correct(annot, golden, name):
    inputs = C.correct_case(name) if name in C.CORRECT_CASES else dict(sel_radius=25, min_size=64)
    img = golden[name + '_img']
    seg, seg_lb = annot.correct_segm(img, inputs['sel_radius'], inputs['min_size'], on='device')
    assert C.same(seg, golden[name + '_seg']) and C.same(seg_lb, golden[name + '_seg_lb']), name
    level_map, centres = annot.create_annot_centers(img, C.LEVELS, on='device', sel_radius=inputs['sel_radius'], min_size=inputs['min_size'])
    assert C.same(level_map, golden[name + '_levels']) and C.same(centres, golden[name + '_centres']), name
    return img, inputs, seg_lb, level_map, centres


@pytest.mark.parametrize('name', list(C.CORRECT_CASES) + ['sample'])
def test_correction_equals_the_reference_and_the_chain_its_parts(annot, golden, name):
    img, inputs, seg_lb, level_map, centres = _check_correct(annot, golden, name)
    if name in C.CORRECT_CASES:
        assert C.same(img, C.correct_case(name)['img'])
    host_seg, host_lb = annot.correct_segm_host(img, inputs['sel_radius'], inputs['min_size'])
    assert C.same(seg_lb, host_lb)
    # the three single calls
    assert C.same(annot.segm_center_levels(seg_lb, C.LEVELS, on='device').astype(np.uint8), level_map)
    assert C.same(annot.compute_eggs_center(seg_lb, on='device'), centres)
    # int32 pixels and pixels the entry does not read itself
    for other in (img.astype(np.int32) - 3 * (img == 0), img.astype(np.float64) / 7, img > 0):
        seg, again = annot.correct_segm(other, inputs['sel_radius'], inputs['min_size'], on='device')
        assert C.same(again, host_lb) and C.same(seg, host_seg)


def test_capped_requests_take_the_host_path(hip, annot, golden, monkeypatch):
    calls = []
    original = hip.center_levels
    monkeypatch.setattr(hip, 'center_levels', lambda *args, **kwargs: calls.append(1) or original(*args, **kwargs))
    # an opening radius of 65: the entry is asked and answers with the caps status, the host statement runs
    inputs = C.level_case('open65')
    assert original(inputs['seg'], int(inputs['seg'].max()), inputs['levels']) is None
    got = annot.segm_center_levels(inputs['seg'], inputs['levels'], on='device')
    assert len(calls) == 1 and C.same(got, golden['open65_levels'].astype(np.int32))
    # levels that descend, nine levels, 1025 labels: the entry is not called at all
    for name in ('descending', 'nine_levels'):
        inputs = C.level_case(name)
        assert C.same(annot.segm_center_levels(inputs['seg'], inputs['levels'], on='device'), golden[name + '_levels'].astype(np.int32))
    seg = np.zeros((8, 2 * (hip.CENTER_ANNOT_MAX_LABELS + 1)), dtype=np.int32)
    seg[2:6, ::2] = np.arange(1, hip.CENTER_ANNOT_MAX_LABELS + 2)
    assert C.same(annot.segm_center_levels(seg, on='device'), annot.segm_center_levels_host(seg))
    assert C.same(annot.compute_eggs_center(seg, on='device'), annot.compute_eggs_center_host(seg))
    assert len(calls) == 1
    seg[seg > hip.CENTER_ANNOT_MAX_LABELS] = 0
    assert C.same(annot.segm_center_levels(seg, on='device'), annot.segm_center_levels_host(seg)) and len(calls) == 2
    # a radius of the first opening above the cap
    calls_correct = []
    monkeypatch.setattr(hip, 'correct_segm', lambda *args, **kwargs: calls_correct.append(1))
    img = np.ones((140, 150), dtype=np.uint8)
    seg, _ = annot.correct_segm(img, hip.MORPH_MAX_RADIUS + 1, on='device')
    assert seg.all() and not calls_correct
    with pytest.raises(hip.HipError, match='descend'):
        original(C.level_case('tie')['seg'], 1, [0.5, 0.1])


@pytest.mark.parametrize('word', WORDS, ids=['%08x' % w for w in WORDS])
def test_same_bytes_on_stale_scratch(hip, annot, golden, monkeypatch, word):
    """tests/test_gpu_stale_scratch.py for these entries: a larger, different call first, every buffer of the context filled with
    the word, then each entry from scratch and once more on what the others left"""
    ctx = hip.Context()
    try:
        monkeypatch.setattr(hip, 'default_context', lambda: ctx)
        rng = np.random.default_rng(31)
        seg1, seg2 = (rng.integers(0, 900, (300, 300)).astype(np.int32) for _ in range(2))
        hip.labels_overlap(seg1, seg2, 900, 900, ctx=ctx)
        annot.segm_center_levels(np.tile(C.level_case('missing_label')['seg'], (3, 3)), on='device')
        assert ctx.poison(word) > 0
        for _ in range(2):
            for name in ('touching', 'small_egg', 'split', 'many_levels'):
                _check_levels(annot, golden, name)
            for name in ('correct_r1', 'correct_r2'):
                _check_correct(annot, golden, name)
    finally:
        ctx.close()
