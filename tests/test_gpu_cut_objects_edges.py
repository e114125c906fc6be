"""``imsegm_cut_objects`` (csrc/cut_objects.hip) at the wave, workgroup, tile and rounding edges its golden cases stay away from
(the edge tables of tests/cut_objects_cases.py; their CPU twins are in tests/test_cut_objects_reference_host.py):

* the ten words per label equal int64 numpy sums on every run-rule map -- widths of 64 to 513 (one to three workgroups per row, with
  and without invalid lanes), runs that open at lane 63, 64 heads in a wave, runs of 64 that go on in the next wave or workgroup, an
  unlisted value between two listed ones, negative, zero and largest-int32 labels, one pixel in the last corner;
* the same maps through ``cut_objects`` and through ``cut_object`` (boolean masks) equal the host statement byte for byte;
* device == ``cut_object_host`` == the reference's statements with scipy's own ``shift`` and ``rotate`` on every geometry case:
  shifts at k + 0.5, rotation coordinates on the last pixel, turns of exactly 0, +-90 and 180 degrees (the last two through a geometry
  hook that hands ``_cut_geometry`` the orientation), one channel as H x W and H x W x 1, two (``k_cut_write<2>``), three and four
  channels, ``use_mask`` on and off, a background whose bytes all differ, crops of one tile, one more row and column, two tiles and one;
* every call twice in one context with equal bytes (the order of the atomics)."""
import numpy as np
import pytest

import cut_objects_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def hip():
    from pyimsegm_amd import _hip
    _hip.default_context()
    return _hip


@pytest.fixture(scope='module')
def data_io():
    from pyimsegm_amd.utilities import data_io
    return data_io


def _same(got, want):
    return got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()


def _int64_words(segm, label, rows, cols):
    mask = segm == label
    r, c = rows[mask], cols[mask]
    return [int(v) for v in (mask.sum(), r.sum(), c.sum(), (r * r).sum(), (c * c).sum(), (r * c).sum(), r.min(), r.max(), c.min(), c.max())]


@pytest.mark.parametrize('width', C.RUN_WIDTHS)
def test_run_rule_moments_equal_int64_sums(hip, data_io, width):
    assert (-(-width // C.CHUNK) > 1) == (width > 256)
    for layout in C.RUN_LAYOUTS:
        img, segm, labels, listed = C.run_cut_inputs(width, layout)
        reached = C.run_branches(C.run_map(width, layout), listed)
        for need, widths in C.RUN_REACH[layout] + C.RUN_REACH_ALWAYS:
            if widths is None or width in widths:
                assert need in reached, (width, layout, need)
        rows, cols = np.indices(segm.shape).astype(np.int64)
        results = [hip.cut_objects(img[:, :, None].copy(), segm, labels, 1, False, 9, False, data_io._hook_geometry) for _ in range(2)]
        crops, moments, boxes = results[0]
        assert moments.dtype == np.int64 and moments.shape == (len(labels), 10)
        for k, label in enumerate(labels):
            assert moments[k].tolist() == _int64_words(segm, label, rows, cols), (width, layout, label)
        # twice in one context: the same words, boxes and bytes
        assert _same(results[1][1], moments) and _same(results[1][2], boxes)
        assert all(_same(a, b) for a, b in zip(results[1][0], crops))


@pytest.mark.parametrize('width', C.RUN_WIDTHS)
def test_run_rule_maps_through_cut_objects_and_cut_object(data_io, width):
    for layout in C.RUN_LAYOUTS:
        img, segm, labels, _ = C.run_cut_inputs(width, layout)
        for allow_rotate in (False, True):
            kwargs = dict(padding=1, use_mask=True, bg_color=200, allow_rotate=allow_rotate)
            want = {}
            for label in labels:
                try:
                    want[label] = data_io.cut_object_host(img, segm == label, **kwargs)
                except IndexError:                     # the shift or the turn left no pixel of the mask: regionprops(...)[0] of the reference
                    assert allow_rotate
                    for call in (lambda: data_io.cut_objects(img, segm, [label], on='device', **kwargs),
                                 lambda: data_io.cut_object(img, segm == label, on='device', **kwargs)):
                        with pytest.raises(IndexError):
                            call()
            got = data_io.cut_objects(img, segm, list(want), on='device', **kwargs)
            assert len(got) == len(want) >= 1
            for (label, b), a in zip(want.items(), got):
                assert _same(a, b), (width, layout, label, allow_rotate)
                assert _same(data_io.cut_object(img, segm == label, on='device', **kwargs), b), (width, layout, label, allow_rotate)


def _raw(hip, name, inputs, ctx=None):
    image = np.ascontiguousarray(inputs['img'].reshape(inputs['img'].shape[0], inputs['img'].shape[1], -1))
    seen = []

    def hook(moments, shape, allow_rotate):
        geometry = C.edge_geometry(name, moments, shape, allow_rotate)
        seen.append(geometry['angle'])
        return geometry

    crops, _, _ = hip.cut_objects(image, inputs['segm'], inputs['labels'], inputs['padding'], inputs['use_mask'], inputs['bg_color'],
                                  inputs['allow_rotate'], hook, ctx=ctx)
    if inputs['allow_rotate']:
        assert seen and all(angle == inputs['turn'] for angle in seen)          # exactly 0, +-90 or 180 degrees
    return [crop[:, :, 0] if inputs['img'].ndim == 2 else crop for crop in crops]


@pytest.mark.parametrize('name', list(C.EDGE_CASES))
def test_edge_case_equals_the_host_statement_and_scipy(hip, data_io, name):
    base = C.EDGE_CASES[name]
    if base['allow_rotate']:
        ties = np.array([C.edge_ties(name, label) for label in base['labels']])
        assert ties[:, 0].sum() > 0 and ties[:, 2].sum() > 0                    # shifts at k + 0.5, coordinates equal to n - 1
    channels = set()
    for tag, inputs in C.edge_variants(name):
        channels.add(inputs['img'].shape[2] if inputs['img'].ndim == 3 else 0)
        got = _raw(hip, name, inputs)
        again = _raw(hip, name, inputs)
        for k, label in enumerate(inputs['labels']):
            host, scipy_crop = C.edge_host_crop(name, inputs, label), C.edge_scipy_crop(name, inputs, label)
            assert _same(host, scipy_crop), (name, tag, label)
            assert _same(got[k], host), (name, tag, label, got[k].shape, host.shape)
            assert _same(again[k], got[k]), (name, tag, label)
            if 'crop' in base:
                assert got[k].shape[:2] == base['crop']
        if base['turn'] in (0, 90):
            # the object's own orientation gives these turns: the public function, no hook of the test's
            kwargs = {key: inputs[key] for key in ('padding', 'use_mask', 'bg_color', 'allow_rotate')}
            public = data_io.cut_objects(inputs['img'], inputs['segm'], inputs['labels'], on='device', **kwargs)
            assert all(_same(a, b) for a, b in zip(public, got)), (name, tag)
    assert channels == {0, 1, 2, 3, 4}                                          # C == 2 among them
