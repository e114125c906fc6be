"""The volume kernels of csrc/boundary3d.hip and the slice passes of csrc/boundary.hip against the numpy / scipy definitions of
tests/boundary3d_cases.py: thick masks, whole distance maps, boundary points and their distances of every case, bit for bit with
dtype and shape; the session form against the stateless one; the capacity contract; a run on scratch a larger call left dirty."""
import ctypes

import numpy as np
import pytest

import boundary3d_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def hip():
    from pyimsegm_amd import _hip
    _hip.default_context()
    return _hip


@pytest.fixture(scope='module')
def labeling(hip):
    from pyimsegm_amd import labeling
    return labeling


def _i32(seg):
    return np.ascontiguousarray(seg, dtype=np.int32)


def test_thick_masks(hip):
    for name, seg in C.maps().items():
        assert C.same(hip.boundary_mask3d(_i32(seg)), C.thick(seg).astype(np.uint8)), name


def test_distance_maps(hip):
    for name, seg in C.maps().items():
        assert C.same(hip.distance_map3d(_i32(seg)), C.distance_map(name)), name


def test_boundary_distances(hip, labeling):
    empty = 0
    for ref_name, name in C.pair_cases():
        want_points, want_dist = C.boundary_distances(ref_name, name)
        points, dist = hip.boundary_distances3d(_i32(C.maps()[ref_name]), _i32(C.maps()[name]))
        assert C.same(points, want_points.astype(np.int32)) and C.same(dist, want_dist), (ref_name, name)
        for on in (None, 'device'):
            points, dist = labeling.compute_boundary_distances(C.maps()[ref_name], C.maps()[name], on=on)
            assert C.same(points, want_points) and C.same(dist, want_dist), (ref_name, name, on)
        empty += len(points) == 0
    assert empty >= 3                                  # the 0-point results: shapes (0, 3) and (0,)


def test_stateless_call_twice_gives_the_same_bytes(hip):
    seg_ref, seg = _i32(C.maps()['blocks_12x40x48']), _i32(C.maps()['blocks_shifted_12x40x48'])
    first, second = hip.boundary_distances3d(seg_ref, seg), hip.boundary_distances3d(seg_ref, seg)
    assert len(first[0]) > 0 and first[0].tobytes() == second[0].tobytes() and first[1].tobytes() == second[1].tobytes()


def test_session_form_equals_the_stateless_call(hip, labeling):
    shape = (6, 40, 48)
    volume = np.random.default_rng(C.SEED).random(shape).astype(np.float32)
    z, y, x = np.indices(shape)
    annot = ((z // 3) * 4 + (y // 20) * 2 + x // 24).astype(np.int64)          # eight blocks
    sess = hip.Volume3D(*shape).upload(volume)
    try:
        assert sess.slic(30, 0.1) > 1
        labels = sess.get_labels()
        assert labels.shape == shape
        got = sess.boundary_distances(annot)
        through = labeling.compute_boundary_distances(annot, None, _session=sess)
        with pytest.raises(labeling.ImageDimensionError):
            labeling.compute_boundary_distances(annot[:, :, :-1], None, _session=sess)
    finally:
        sess.close()
    want = hip.boundary_distances3d(_i32(annot), _i32(labels))
    assert len(want[0]) > 0 and got[0].dtype == np.int32 and got[0].shape == (len(got[1]), 3)
    assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
    assert C.same(through[0], want[0].astype(np.int64)) and C.same(through[1], want[1])
    # ... and both are the definitions on the downloaded map
    on_ref = C.thick(annot)
    assert C.same(through[0], np.argwhere(on_ref).astype(np.int64)) and C.same(through[1], C.edt(C.thick(labels))[on_ref])


def test_reference_of_the_wrong_shape_raises(labeling):
    seg = C.maps()['rand_5x6x7_L3']
    with pytest.raises(labeling.ImageDimensionError):
        labeling.compute_boundary_distances(seg[:, :, :-1], seg)
    with pytest.raises(labeling.ImageDimensionError):
        labeling.compute_boundary_distances(seg[0], seg)


def test_too_small_a_capacity_reports_the_count(hip):
    seg_ref, seg = _i32(C.maps()['rand_5x6x7_L3']), _i32(C.maps()['rand_5x6x7_L3'])
    want = int(C.thick(seg_ref).sum())
    assert want > 4
    lib, ctx = hip.load_library(), hip.default_context()
    for capacity in (0, 4, want - 1):
        points, dist, count = np.full((max(capacity, 1), 3), -7, dtype=np.int32), np.full(max(capacity, 1), -7.), ctypes.c_int(-1)
        status = lib.imsegm_boundary_distances3d(ctx._h, hip._ptr(seg_ref), hip._ptr(seg), 5, 6, 7, hip._ptr(points), hip._ptr(dist), capacity,
                                                 ctypes.byref(count))
        assert status != 0 and count.value == want, capacity
        assert str(want) in lib.imsegm_last_error().decode() and (points == -7).all() and (dist == -7.).all()
    points, dist, count = np.empty((want, 3), dtype=np.int32), np.empty(want), ctypes.c_int(-1)
    assert lib.imsegm_boundary_distances3d(ctx._h, hip._ptr(seg_ref), hip._ptr(seg), 5, 6, 7, hip._ptr(points), hip._ptr(dist), want,
                                           ctypes.byref(count)) == 0
    assert count.value == want and C.same(points.astype(np.int64), np.argwhere(C.thick(seg_ref)).astype(np.int64))
    # volumes beyond the limits are refused before anything is launched
    with pytest.raises(hip.HipError):
        hip.boundary_mask3d(np.zeros((1, 1, 65536), dtype=np.int32))


def test_on_scratch_a_larger_call_left_dirty(hip):
    """first a 17 x 65 x 257 random pair, then the case whose slices are mostly empty (their g and slice distances are whatever the
    larger call left there), in a context of its own"""
    ctx = hip.Context()
    try:
        big_ref, big = _i32(C.maps()['rand_17x65x257_L5']), _i32(C.maps()['rand_17x65x257_L2'])
        points, dist = hip.boundary_distances3d(big_ref, big, ctx=ctx)
        want_points, want_dist = C.boundary_distances('rand_17x65x257_L5', 'rand_17x65x257_L2')
        assert C.same(points, want_points.astype(np.int32)) and C.same(dist, want_dist)
        hip.distance_map3d(big, ctx=ctx)
        # as the larger call left it, then with every scratch buffer of the context filled with a word (tests/test_gpu_stale_scratch.py)
        for word in (None, 0x00000001, 0x7F7F7F7F):
            assert word is None or ctx.poison(word) >= 17 * 65 * 257 * 4
            for name, ref_name in (('middle_slices_9x12x70', 'first_slices_9x12x70'), ('constant_4x6x70', 'rand_4x6x70_L2')):
                seg = _i32(C.maps()[name])
                assert C.same(hip.boundary_mask3d(seg, ctx=ctx), C.thick(seg).astype(np.uint8)), (name, word)
                assert C.same(hip.distance_map3d(seg, ctx=ctx), C.distance_map(name)), (name, word)
                points, dist = hip.boundary_distances3d(_i32(C.maps()[ref_name]), seg, ctx=ctx)
                want_points, want_dist = C.boundary_distances(ref_name, name)
                assert C.same(points, want_points.astype(np.int32)) and C.same(dist, want_dist), (name, word)
    finally:
        ctx.close()


def test_input_of_the_host_test_goes_through_the_device(hip, labeling, monkeypatch):
    """tests/test_boundary_reference_host.py::test_host_statement_of_the_boundary_distances_in_three_dimensions: its input is an
    integer 3-D pair, with a device it runs the kernels (seen on the call count) and gives the same bytes as the host statement"""
    from scipy import ndimage
    rng = np.random.RandomState(5)
    seg_ref, seg = rng.randint(0, 3, (5, 6, 7)), rng.randint(0, 3, (5, 6, 7))
    calls, plain = [], hip.boundary_distances3d
    monkeypatch.setattr(hip, 'boundary_distances3d', lambda *args, **kwargs: calls.append(1) or plain(*args, **kwargs))
    monkeypatch.delenv('IMSEGM_BOUNDARY3D_ON', raising=False)
    points, dist = labeling.compute_boundary_distances(seg_ref, seg)
    assert calls == [1]
    host_points, host_dist = labeling.compute_boundary_distances(seg_ref, seg, on='host')
    assert calls == [1] and C.same(points, host_points) and C.same(dist, host_dist)
    cross = ndimage.generate_binary_structure(3, 1)
    on_ref, on_seg = [ndimage.grey_dilation(s, footprint=cross) != ndimage.grey_erosion(s, footprint=cross) for s in (seg_ref, seg)]
    assert C.same(points, np.argwhere(on_ref).astype(np.int64)) and C.same(dist, ndimage.distance_transform_edt(~on_seg)[on_ref])
