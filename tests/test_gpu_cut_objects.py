"""``imsegm_cut_objects`` (csrc/cut_objects.hip) behind ``cut_objects`` / ``cut_object`` of pyimsegm_amd/utilities/data_io.py:

* byte for byte, shapes included, the crops the reference's ``cut_object`` returned (tests/golden/cut_objects.npz) on every case of
  tests/cut_objects_cases.py, through ``cut_objects`` (one call per case) and through ``cut_object`` (one call per label);
* byte for byte the host statement on two further seeded cases that are in no golden file;
* the ten words per label equal int64 numpy sums;
* the same bytes on reused scratch that holds stale data; the caps status without a launch; host-only dtypes on the host path."""
import numpy as np
import pytest

import cut_objects_cases as C

pytestmark = pytest.mark.gpu

WORDS = (0x00000001, 0x7F7F7F7F)


@pytest.fixture(scope='module')
def hip():
    from pyimsegm_amd import _hip
    _hip.default_context()
    return _hip


@pytest.fixture(scope='module')
def data_io():
    from pyimsegm_amd.utilities import data_io
    return data_io


@pytest.fixture(scope='module')
def golden():
    return C.load_golden()


def _kwargs(inputs):
    return {key: inputs[key] for key in ('padding', 'use_mask', 'bg_color', 'allow_rotate')}


def _same(got, want):
    return got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()


def _check_case(data_io, golden, name):
    inputs = C.case(name, golden[name + '_seed'])
    crops = data_io.cut_objects(inputs['img'], inputs['segm'], inputs['labels'], on='device', **_kwargs(inputs))
    assert len(crops) == len(inputs['labels'])
    for k, crop in enumerate(crops):
        assert _same(crop, golden['%s_crop%d' % (name, k)]), (name, inputs['labels'][k])
    return inputs, crops


@pytest.mark.parametrize('name', list(C.CASES))
def test_cut_objects_equals_the_reference(data_io, golden, name):
    _check_case(data_io, golden, name)


@pytest.mark.parametrize('name', [n for n in C.CASES if n != 'sparse33'])
def test_cut_object_equals_the_reference(data_io, golden, name):
    inputs = C.case(name, golden[name + '_seed'])
    for k, (label, mask) in enumerate(C.masks_of(name, inputs)):
        assert mask.dtype == np.bool_
        assert _same(data_io.cut_object(inputs['img'], mask, on='device', **_kwargs(inputs)), golden['%s_crop%d' % (name, k)]), (name, label)


@pytest.mark.parametrize('name,seed', [('rgb_p4_mask', 1001), ('border', 1002)])
def test_device_equals_the_host_statement_off_the_golden_cases(data_io, name, seed):
    inputs = C.case(name, seed)
    got = data_io.cut_objects(inputs['img'], inputs['segm'], on='device', **_kwargs(inputs))
    want = data_io.cut_objects(inputs['img'], inputs['segm'], on='host', **_kwargs(inputs))
    assert len(got) == len(want) == 3
    for a, b in zip(got, want):
        assert _same(a, b)
    # any order, a label twice
    again = data_io.cut_objects(inputs['img'], inputs['segm'], [3, 1, 3], on='device', **_kwargs(inputs))
    assert _same(again[0], want[2]) and _same(again[1], want[0]) and _same(again[2], want[2])


def _raw(hip, data_io, inputs, labels=None, ctx=None):
    image = inputs['img'].reshape(inputs['img'].shape[0], inputs['img'].shape[1], -1)
    bg = inputs['bg_color'] if inputs['bg_color'] else data_io.get_image2d_boundary_color(inputs['img'])
    return hip.cut_objects(np.ascontiguousarray(image), inputs['segm'], inputs['labels'] if labels is None else labels, inputs['padding'],
                           inputs['use_mask'], bg, inputs['allow_rotate'], data_io._hook_geometry, ctx=ctx)


@pytest.mark.parametrize('name', ['sparse33', 'two_pieces', 'large', 'one_pixel'])
def test_moments_equal_int64_sums(hip, data_io, golden, name):
    inputs = C.case(name, golden[name + '_seed'])
    _, moments, boxes = _raw(hip, data_io, inputs)
    assert moments.dtype == np.int64 and moments.shape == (len(inputs['labels']), 10)
    rows, cols = np.indices(inputs['segm'].shape).astype(np.int64)
    for k, label in enumerate(inputs['labels']):
        mask = inputs['segm'] == label
        r, c = rows[mask], cols[mask]
        want = [mask.sum(), r.sum(), c.sum(), (r * r).sum(), (c * c).sum(), (r * c).sum(), r.min(), r.max(), c.min(), c.max()]
        assert moments[k].tolist() == [int(v) for v in want], (name, label)
        assert boxes[k, 0] >= 0 and boxes[k, 1] >= 0 and boxes[k, 2] > boxes[k, 0] and boxes[k, 3] > boxes[k, 1]


def test_absent_label_raises_index_error(data_io, golden):
    inputs = C.case('rgb_p0', golden['rgb_p0_seed'])
    with pytest.raises(IndexError):
        data_io.cut_objects(inputs['img'], inputs['segm'], [1, 2, 77], on='device')
    with pytest.raises(IndexError):
        data_io.cut_object(inputs['img'], inputs['segm'] == 77, 0, on='device')
    with pytest.raises(ValueError):
        data_io.cut_object(inputs['img'], np.ones((3, 3), dtype=bool), 0, on='device')
    # the context is as good as before
    assert _same(data_io.cut_objects(inputs['img'], inputs['segm'], [2], on='device')[0], golden['rgb_p0_crop1'])


@pytest.mark.parametrize('word', WORDS, ids=['%08x' % w for w in WORDS])
def test_same_bytes_on_stale_scratch(hip, data_io, golden, monkeypatch, word):
    """tests/test_gpu_stale_scratch.py for this entry: a larger, different call first, every buffer of the context filled with the
    word, then the small cases from scratch and once more on what they left"""
    ctx = hip.Context()
    try:
        monkeypatch.setattr(hip, 'default_context', lambda: ctx)
        rng = np.random.default_rng(24)
        seg1, seg2 = (rng.integers(0, 3200, (300, 300)).astype(np.int32) for _ in range(2))
        hip.labels_overlap(seg1, seg2, 3200, 3200, ctx=ctx)                      # 82 MB of int64 counts in the shared scratch
        big = C.case('sparse33', 7)
        data_io.cut_objects(np.ascontiguousarray(np.tile(big['img'], (2, 2, 1))), np.ascontiguousarray(np.tile(big['segm'], (2, 2))),
                            padding=9, use_mask=True, allow_rotate=False, on='device')
        filled = ctx.poison(word)
        assert filled > 0
        for _ in range(2):
            for name in ('rgb_p4_mask', 'border', 'gray_p0_mask', 'rgb_p60_mask'):
                _check_case(data_io, golden, name)
    finally:
        ctx.close()


def test_caps_status_without_a_launch(hip, data_io, golden):
    inputs = C.case('rgb_p0', golden['rgb_p0_seed'])
    ctx = hip.Context()
    try:
        labels = np.arange(1, hip.CUT_OBJECTS_MAX_LABELS + 2)
        assert _raw(hip, data_io, inputs, labels=labels, ctx=ctx) is None
        five = dict(inputs, img=np.zeros(inputs['segm'].shape + (5, ), dtype=np.uint8), bg_color=(1, 2, 3, 4, 5))
        assert _raw(hip, data_io, five, ctx=ctx) is None
        assert ctx.poison(WORDS[0]) == 0, 'the context has allocated scratch: something was launched'
        with pytest.raises(hip.HipError, match='ascending'):
            _raw(hip, data_io, inputs, labels=[2, 1], ctx=ctx)
    finally:
        ctx.close()
    # the public function cuts more labels than one call takes in several calls
    segm = np.zeros((40, 2 * (hip.CUT_OBJECTS_MAX_LABELS + 3)), dtype=np.int32)
    for label in range(1, hip.CUT_OBJECTS_MAX_LABELS + 4):
        segm[3 + label % 5:9 + label % 7, 2 * label - 2] = label
    img = np.random.RandomState(5).randint(0, 256, segm.shape).astype(np.uint8)
    got = data_io.cut_objects(img, segm, padding=1, allow_rotate=False, on='device')
    assert len(got) == hip.CUT_OBJECTS_MAX_LABELS + 3
    for label in (1, 500, hip.CUT_OBJECTS_MAX_LABELS, hip.CUT_OBJECTS_MAX_LABELS + 3):
        assert _same(got[label - 1], data_io.cut_object_host(img, segm == label, 1, allow_rotate=False))


def test_host_only_inputs_take_the_host_path(hip, data_io, golden, monkeypatch):
    calls = []
    original = hip.cut_objects
    monkeypatch.setattr(hip, 'cut_objects', lambda *args, **kwargs: calls.append(1) or original(*args, **kwargs))
    inputs = C.case('rgb_p4_mask', golden['rgb_p4_mask_seed'])
    kwargs = _kwargs(inputs)
    mask = inputs['segm'] == 2
    want = golden['rgb_p4_mask_crop1']
    assert _same(data_io.cut_object(inputs['img'], mask, **kwargs), want) and len(calls) == 1
    for img in (inputs['img'].astype(np.float64), inputs['img'].astype(np.int64),
                np.concatenate([inputs['img'], inputs['img']], axis=2)):
        got = data_io.cut_object(img, mask, **kwargs)
        assert _same(got, data_io.cut_object_host(img, mask, **kwargs))
        assert len(data_io.cut_objects(img, inputs['segm'], **kwargs)) == 3
    for other in (mask.astype(np.int64), mask.astype(np.uint8)):
        assert _same(data_io.cut_object(inputs['img'], other, **kwargs), data_io.cut_object_host(inputs['img'], other, **kwargs))
    assert len(calls) == 1
    name = 'int_mask_turned'
    inputs = C.case(name, golden[name + '_seed'])
    for k, (label, int_mask) in enumerate(C.masks_of(name, inputs)):
        assert _same(data_io.cut_object(inputs['img'], int_mask, **_kwargs(inputs)), golden['%s_crop%d' % (name, k)])
    assert len(calls) == 1
