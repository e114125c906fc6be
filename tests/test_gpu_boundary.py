"""The scoring functions of ``pyimsegm_amd.labeling`` on the device (csrc/boundary.hip, ``k_label_hist``) against the numpy / scipy
restatement of tests/boundary_cases.py and against tests/golden/boundary.npz (the reference itself under scikit-image 0.18.3):
masks, contour points, distance maps, boundary points and distances, overlap matrices and both relabellings, bit for bit with
dtype and shape.  Every input here is a 2-D integer map, so every call runs the kernels (there is no host path for them)."""
import os

import numpy as np
import pytest

import boundary_cases as B

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'boundary.npz')


@pytest.fixture(scope='module')
def hip():
    from pyimsegm_amd import _hip
    _hip.default_context()
    return _hip


@pytest.fixture(scope='module')
def labeling(hip):
    import imsegm.labeling
    return imsegm.labeling


@pytest.fixture(scope='module')
def golden():
    return np.load(GOLDEN)


def test_stand_alone_names_are_this_package(labeling):
    import pyimsegm_amd.labeling
    assert labeling is pyimsegm_amd.labeling
    for name in ('contour_binary_map', 'contour_coords', 'binary_image_from_coords', 'compute_distance_map', 'compute_boundary_distances',
                 'compute_labels_overlap_matrix', 'relabel_max_overlap_unique', 'relabel_max_overlap_merge'):
        assert callable(vars(labeling).get(name)), name        # (defined here: a reference fallback would not be in vars())


def test_thick_masks(hip):
    for name, seg in B.maps().items():
        mask = hip.boundary_mask(np.ascontiguousarray(seg, dtype=np.int32), hip.BOUNDARY_THICK)
        assert B.same(mask, B.thick(seg).astype(np.uint8)), name


def test_contour_maps_and_points(labeling):
    for name, label in B.contour_cases():
        seg = B.maps()[name]
        for include_boundary in (False, True):
            assert B.same(labeling.contour_binary_map(seg, label, include_boundary), B.contour(seg, label, include_boundary)), (name, label)
            assert labeling.contour_coords(seg, label, include_boundary) == B.contour_points(seg, label, include_boundary), (name, label)


def test_distance_maps(labeling):
    for name, label in B.contour_cases():
        seg = B.maps()[name]
        assert B.same(labeling.compute_distance_map(seg, label), B.distance_map(seg, label)), (name, label)


def test_distance_maps_of_thick_masks(hip):
    """the transform under compute_boundary_distances, whole maps (the stateless call returns the points only)"""
    for name, seg in B.maps().items():
        dist = hip.distance_map(np.ascontiguousarray(seg, dtype=np.int32), hip.BOUNDARY_THICK)
        assert B.same(dist, B.edt(B.thick(seg))), name


def test_boundary_distances(labeling):
    empty = 0
    for ref_name, name in B.pair_cases():
        seg_ref, seg = B.maps()[ref_name], B.maps()[name]
        points, dist = labeling.compute_boundary_distances(seg_ref, seg)
        want_points, want_dist = B.boundary_distances(seg_ref, seg)
        assert B.same(points, want_points) and B.same(dist, want_dist), (ref_name, name)
        empty += len(points) == 0
    assert empty >= len(B.SHAPES)                      # the 0-point results: shapes (0, 2) and (0,)


def test_overlap_and_relabelling(labeling):
    pairs = [(B.maps()[a], B.maps()[b], (a, b)) for a, b in B.pair_cases()] + [(s1, s2, key) for key, (s1, s2) in B.negative_pairs().items()]
    for seg1, seg2, key in pairs:
        assert B.same(labeling.compute_labels_overlap_matrix(seg1, seg2), B.overlap_matrix(seg1, seg2)), key
        for keep_bg in (False, True):
            assert B.same_outcome(B.outcome(labeling.relabel_max_overlap_unique, seg1, seg2, keep_bg),
                                  B.outcome(B.relabel_unique, seg1, seg2, keep_bg)), (key, keep_bg)
            assert B.same_outcome(B.outcome(labeling.relabel_max_overlap_merge, seg1, seg2, keep_bg),
                                  B.outcome(B.relabel_merge, seg1, seg2, keep_bg)), (key, keep_bg)


def test_golden(labeling, golden):
    for name in B.GOLDEN_MAPS:
        seg = B.maps()[name]
        for flag in (0, 1):
            assert B.same(labeling.contour_binary_map(seg, 1, bool(flag)), golden['%s_contour%d' % (name, flag)]), name
            coords = np.array(labeling.contour_coords(seg, 1, bool(flag)), dtype=np.int64).reshape(-1, 2)
            assert B.same(coords, golden['%s_coords%d' % (name, flag)]), name
        assert B.same(labeling.compute_distance_map(seg, 1), golden[name + '_distance']), name
    for ref_name, name in B.GOLDEN_PAIRS:
        seg_ref, seg = B.maps()[ref_name], B.maps()[name]
        key = ref_name + '__' + name
        points, dist = labeling.compute_boundary_distances(seg_ref, seg)
        assert B.same(points, golden[key + '_points']) and B.same(dist, golden[key + '_dist']), key
        assert B.same(labeling.compute_labels_overlap_matrix(seg_ref, seg), golden[key + '_overlap']), key
        for keep_bg in (0, 1):
            for kind, call in (('unique', labeling.relabel_max_overlap_unique), ('merge', labeling.relabel_max_overlap_merge)):
                stored = '%s_%s%d' % (key, kind, keep_bg)
                result = B.outcome(call, seg_ref, seg, bool(keep_bg))
                assert (B.same(result[1], golden[stored]) if stored in golden.files else result[0] == 'raises'), stored


def test_session_form_equals_stateless_form(hip, labeling):
    from pyimsegm_amd import superpixels
    from pyimsegm_amd.utilities.synthetic import disc_image
    image = disc_image(192)
    annot = B.block_map((192, 192), (50, 70))
    slic = superpixels.segment_slic_img2d(image, sp_size=18, relative_compact=0.2)
    stateless = labeling.compute_boundary_distances(annot, slic)
    want = B.boundary_distances(annot, slic)
    assert B.same(stateless[0], want[0]) and B.same(stateless[1], want[1])
    sess = hip.Image2D(192, 192).set_labels(slic)
    try:
        with_session = labeling.compute_boundary_distances(annot, None, _session=sess)
        assert B.same(with_session[0], stateless[0]) and B.same(with_session[1], stateless[1])
        with pytest.raises(labeling.ImageDimensionError):
            labeling.compute_boundary_distances(annot[:-1], None, _session=sess)
    finally:
        sess.close()


def test_session_form_on_the_map_slic_left_behind(hip, labeling):
    """the session ran SLIC itself: its resident map, never set from the host, is the one measured"""
    from pyimsegm_amd.utilities.synthetic import disc_image
    annot = B.block_map((192, 192), (50, 70))
    sess = hip.Image2D(192, 192).upload(disc_image(192))
    try:
        assert sess.slic(100, 10.) > 1
        with_session = labeling.compute_boundary_distances(annot, None, _session=sess)
        want = B.boundary_distances(annot, sess.get_labels())
        assert len(want[0]) and B.same(with_session[0], want[0]) and B.same(with_session[1], want[1])
    finally:
        sess.close()


def test_two_calls_give_the_same_bytes(hip, labeling):
    seg_ref, seg = B.maps()['annot_512x700'], B.maps()['slic_like_512x700']
    first, second = labeling.compute_boundary_distances(seg_ref, seg), labeling.compute_boundary_distances(seg_ref, seg)
    assert first[0].tobytes() == second[0].tobytes() and first[1].tobytes() == second[1].tobytes()
    assert labeling.compute_distance_map(seg, 1).tobytes() == labeling.compute_distance_map(seg, 1).tobytes()
    assert labeling.compute_labels_overlap_matrix(seg_ref, seg).tobytes() == labeling.compute_labels_overlap_matrix(seg_ref, seg).tobytes()


def test_errors(hip, labeling):
    small, other = np.zeros((5, 6), dtype=int), np.zeros((6, 5), dtype=int)
    for call in (labeling.compute_boundary_distances, labeling.compute_labels_overlap_matrix, labeling.relabel_max_overlap_unique,
                 labeling.relabel_max_overlap_merge):
        with pytest.raises(labeling.ImageDimensionError):
            call(small, other)
    work = np.zeros((5, 6), dtype=np.int32)
    with pytest.raises(hip.HipError):                   # an unknown mode is an error status, not a guess
        hip.boundary_mask(work, 7)
    with pytest.raises(hip.HipError):
        hip.distance_map(work, -1)
    # squared distances beyond 32 bits are refused before anything is uploaded (1 x 65536: 1 + 2^32)
    wide = np.zeros((1, 65536), dtype=np.int32)
    with pytest.raises(hip.HipError, match='32 bits'):
        hip.distance_map(wide, hip.BOUNDARY_THICK)
    with pytest.raises(hip.HipError, match='32 bits'):
        hip.boundary_distances(wide, wide)
    # the package answers such a map with scipy's statement of the same definition (documented in the docstring)
    assert B.same(labeling.compute_distance_map(wide, 1), B.distance_map(wide, 1))
