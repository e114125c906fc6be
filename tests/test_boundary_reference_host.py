"""CPU checks of the restatement in tests/boundary_cases.py that tests/test_gpu_boundary.py holds the device to: it reproduces
every example of the reference's docstrings (``imsegm/labeling.py:42-57, 90-96, 153-162, 497-512, 537-577, 629-660, 691-703``,
copied here as data), it equals tests/golden/boundary.npz (a run of the reference itself under scikit-image 0.18.3), its thick
mask equals the morphological form scikit-image evaluates, and scipy's transform equals the square root of the brute-force
integer minimum bit for bit.  The host paths of ``pyimsegm_amd.labeling`` (inputs the device does not take) are held to the same
restatement, and the build is checked to pass no fast-math flag to the kernels' one square root."""
import os

import numpy as np
import pytest

import boundary_cases as B

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'boundary.npz')


@pytest.fixture(scope='module')
def golden():
    return np.load(GOLDEN)


def _object_image():
    img = np.zeros((6, 6), dtype=int)
    img[1:5, 2:] = 1
    return img


def _atlases():
    atlas1, atlas2 = np.zeros((7, 15), dtype=int), np.zeros((7, 15), dtype=int)
    atlas1[1:4, 5:10] = 1
    atlas1[5:7, 3:13] = 2
    atlas2[0:3, 7:12] = 1
    atlas2[3:7, 1:7] = 2
    atlas2[4:7, 7:14] = 3
    atlas2[:2, :3] = 5
    return atlas1, atlas2


def _rows(*rows):
    return np.array([[int(c) for c in row.split()] for row in rows], dtype=np.int64)


def test_docstring_examples_of_the_contours():
    img = _object_image()
    plain = _rows('0 0 0 0 0 0', '0 0 1 1 1 0', '0 0 1 0 0 0', '0 0 1 0 0 0', '0 0 1 1 1 0', '0 0 0 0 0 0')
    with_border = _rows('0 0 0 0 0 0', '0 0 1 1 1 1', '0 0 1 0 0 1', '0 0 1 0 0 1', '0 0 1 1 1 1', '0 0 0 0 0 0')
    assert B.same(B.contour(img), plain) and B.same(B.contour(img, include_boundary=True), with_border)
    points = [[1, 2], [1, 3], [1, 4], [2, 2], [3, 2], [4, 2], [4, 3], [4, 4]]
    assert B.contour_points(img) == points
    assert B.contour_points(img, include_boundary=True) == points + [[1, 5], [2, 5], [3, 5], [4, 5]]
    dist = np.array([[2.24, 1.41, 1., 1., 1., 1.41], [2., 1., 0., 0., 0., 1.], [2., 1., 0., 1., 1., 1.41], [2., 1., 0., 1., 1., 1.41],
                     [2., 1., 0., 0., 0., 1.], [2.24, 1.41, 1., 1., 1., 1.41]])
    assert np.array_equal(np.round(B.distance_map(img), 2), dist)


def test_docstring_examples_of_the_overlap_and_the_distances():
    seg1, seg2 = np.zeros((7, 15), dtype=int), np.zeros((7, 15), dtype=int)
    seg1[1:4, 5:10] = 3
    seg1[5:7, 6:13] = 2
    seg2[2:5, 7:12] = 1
    seg2[4:7, 7:14] = 3
    assert B.same(B.overlap_matrix(seg1, seg1), _rows('76 0 0 0', '0 0 0 0', '0 0 14 0', '0 0 0 15'))
    assert B.same(B.overlap_matrix(seg1, seg2), _rows('63 4 0 9', '0 0 0 0', '2 0 0 12', '9 6 0 0'))
    segm_ref, segm = np.zeros((6, 10), dtype=int), np.zeros((6, 10), dtype=int)
    segm_ref[3:4, 4:5] = 1
    segm[:, 2:9] = 1
    points, dist = B.boundary_distances(segm_ref, segm)
    assert B.same(points, _rows('2 4', '3 3', '3 4', '3 5', '4 4')) and dist.tolist() == [2.0, 1.0, 2.0, 3.0, 2.0]


def test_docstring_examples_of_the_relabellings():
    atlas1, atlas2 = _atlases()
    unique12 = _rows('5 5 5 0 0 0 0 1 1 1 1 1 0 0 0', '5 5 5 0 0 0 0 1 1 1 1 1 0 0 0', '0 0 0 0 0 0 0 1 1 1 1 1 0 0 0',
                     '0 3 3 3 3 3 3 0 0 0 0 0 0 0 0', '0 3 3 3 3 3 3 2 2 2 2 2 2 2 0', '0 3 3 3 3 3 3 2 2 2 2 2 2 2 0',
                     '0 3 3 3 3 3 3 2 2 2 2 2 2 2 0')
    unique21 = _rows('0 0 0 0 0 0 0 0 0 0 0 0 0 0 0', '0 0 0 0 0 1 1 1 1 1 0 0 0 0 0', '0 0 0 0 0 1 1 1 1 1 0 0 0 0 0',
                     '0 0 0 0 0 1 1 1 1 1 0 0 0 0 0', '0 0 0 0 0 0 0 0 0 0 0 0 0 0 0', '0 0 0 3 3 3 3 3 3 3 3 3 3 0 0',
                     '0 0 0 3 3 3 3 3 3 3 3 3 3 0 0')
    assert B.same(B.relabel_unique(atlas1, atlas2, keep_bg=True), unique12)
    assert B.same(B.relabel_unique(atlas2, atlas1, keep_bg=True), unique21)
    assert B.same(B.relabel_unique(atlas1, atlas2, keep_bg=False), unique12)
    negative = atlas2.copy()
    negative[0, 0] = -1
    kept = unique12.copy()
    kept[0, 0] = -1
    assert B.same(B.relabel_unique(atlas1, negative, keep_bg=True), kept)
    merge12 = _rows('1 1 1 0 0 0 0 1 1 1 1 1 0 0 0', '1 1 1 0 0 0 0 1 1 1 1 1 0 0 0', '0 0 0 0 0 0 0 1 1 1 1 1 0 0 0',
                    '0 2 2 2 2 2 2 0 0 0 0 0 0 0 0', '0 2 2 2 2 2 2 2 2 2 2 2 2 2 0', '0 2 2 2 2 2 2 2 2 2 2 2 2 2 0',
                    '0 2 2 2 2 2 2 2 2 2 2 2 2 2 0')
    merge21 = np.where(unique21 == 3, 2, unique21)
    merge12_all = np.where(merge12 == 2, 2, 0) * (np.arange(15) >= 7) * (np.arange(7)[:, None] >= 4)
    assert B.same(B.relabel_merge(atlas1, atlas2, keep_bg=True), merge12)
    assert B.same(B.relabel_merge(atlas2, atlas1, keep_bg=True), merge21)
    assert B.same(B.relabel_merge(atlas1, atlas2, keep_bg=False), merge12_all)


def test_thick_mask_is_the_morphological_form_and_scipy_is_the_integer_minimum():
    for name, seg in B.maps().items():
        mask = B.thick(seg)
        assert np.array_equal(mask, B.thick_morphology(seg)), name
        if mask.any() and seg.size <= 65 * 65:
            assert B.same(B.edt(mask), B.edt_brute(mask)), name
    for name in ('far_corner_64x300', 'one_column_33x300', 'one_row_65x63'):
        mask = B.contour(B.maps()[name]).astype(bool)
        assert mask.any() and B.same(B.edt(mask), B.edt_brute(mask)), name
    # no set pixel: scipy answers with the distance to (row -1, column 0); the kernel restates exactly this
    for shape in ((1, 1), (3, 4), (33, 65)):
        rows, cols = np.indices(shape)
        assert B.same(B.edt(np.zeros(shape, dtype=bool)), np.sqrt(((rows + 1)**2 + cols**2).astype(np.float64))), shape


def test_cases_cover_the_edges():
    maps = B.maps()
    assert B.contour(maps['far_corner_64x300']).sum() == 1 and B.thick(maps['corner_64x300']).sum() == 3
    assert set(np.nonzero(B.contour(maps['one_column_33x300']))[1]) == {5} and set(np.nonzero(B.contour(maps['one_row_65x63']))[0]) == {60}
    assert not B.thick(maps['rand_33x65_L1']).any()
    big = B.overlap_matrix(maps['slic_like_512x700'], maps['annot_512x700'])
    assert big.shape[0] > 10 * big.shape[1] and big.sum() == 512 * 700
    raised = [B.outcome(B.relabel_merge, maps[a], maps[b])[0] for a, b in B.pair_cases()]
    assert 'ok' in raised and 'raises' in raised       # both ends of the `max_axis` branch


def test_restatement_equals_the_reference_run(golden):
    import zlib
    for name in B.GOLDEN_MAPS:
        seg = B.maps()[name]
        assert zlib.crc32(np.ascontiguousarray(seg).tobytes()) == int(golden[name + '_crc']), name
        for flag in (0, 1):
            assert B.same(B.contour(seg, 1, bool(flag)), golden['%s_contour%d' % (name, flag)]), name
            points = np.array(B.contour_points(seg, 1, bool(flag)), dtype=np.int64).reshape(-1, 2)
            assert B.same(points, golden['%s_coords%d' % (name, flag)]), name
        assert B.same(B.distance_map(seg, 1), golden[name + '_distance']), name
    for ref_name, name in B.GOLDEN_PAIRS:
        seg_ref, seg = B.maps()[ref_name], B.maps()[name]
        key = ref_name + '__' + name
        points, dist = B.boundary_distances(seg_ref, seg)
        assert B.same(points, golden[key + '_points']) and B.same(dist, golden[key + '_dist']), key
        assert B.same(B.overlap_matrix(seg_ref, seg), golden[key + '_overlap']), key
        for keep_bg in (0, 1):
            for kind, call in (('unique', B.relabel_unique), ('merge', B.relabel_merge)):
                stored = '%s_%s%d' % (key, kind, keep_bg)
                result = B.outcome(call, seg_ref, seg, bool(keep_bg))
                assert (B.same(result[1], golden[stored]) if stored in golden.files else result[0] == 'raises'), stored


def test_host_statements_of_the_package():
    """inputs the device does not take -- float labels -- go through numpy / scipy statements in pyimsegm_amd.labeling: the same
    definitions, no GPU needed; plain-numpy helpers and the error types likewise"""
    from pyimsegm_amd import labeling
    for name in ('rand_33x65_L5', 'ragged_33x65', 'rand_1x7_L2', 'rand_7x1_L2', 'rand_33x65_L1', 'far_corner_64x300'):
        seg = B.maps()[name]
        as_float = seg.astype(np.float64)
        for flag in (False, True):
            assert B.same(labeling.contour_binary_map(as_float, 1, flag), B.contour(seg, 1, flag)), name
            assert labeling.contour_coords(as_float, 1, flag) == B.contour_points(seg, 1, flag), name
        assert B.same(labeling.compute_distance_map(as_float, 1), B.distance_map(seg, 1)), name
        assert B.same(labeling.binary_image_from_coords(B.contour_points(seg, 1), seg.shape), B.contour(seg, 1)), name
        other = B.maps()['rand_%dx%d_L2' % seg.shape] if name.startswith('rand') else seg
        points, dist = labeling.compute_boundary_distances(as_float, other.astype(np.float64))
        want = B.boundary_distances(seg, other)
        assert B.same(points, want[0]) and B.same(dist, want[1]), name
    assert B.same(labeling.binary_image_from_coords([[1, 2], [-1, 0], [0, 9], [5, 1]], (4, 5)), _rows('0 0 0 0 0', '0 0 1 0 0', '0 0 0 0 0', '0 0 0 0 0'))
    assert B.same(labeling.binary_image_from_coords([], (2, 3)), np.zeros((2, 3), dtype=np.int64))
    small, other = np.zeros((5, 6), dtype=int), np.zeros((6, 5), dtype=int)
    for call, text in ((labeling.compute_boundary_distances, 'Ref. segm (5, 6) and segm (6, 5) should match'),
                       (labeling.compute_labels_overlap_matrix, 'segm (5, 6) and segm (6, 5) should match'),
                       (labeling.relabel_max_overlap_unique, 'Reference segm. (5, 6) and input segm. (6, 5) should match'),
                       (labeling.relabel_max_overlap_merge, 'Ref. segm (5, 6) and segm (6, 5) should match')):
        with pytest.raises(labeling.ImageDimensionError) as caught:
            call(small, other)
        assert str(caught.value) == text


def test_no_fast_math_reaches_the_square_root():
    """csrc/boundary.hip relies on hipcc's correctly rounded fp64 sqrt: one list of flags for every file, none of them relaxing it"""
    from pyimsegm_amd import build
    assert 'boundary.hip' in build.SOURCES and 'api_boundary.hip' in build.SOURCES
    assert '-ffp-contract=off' in build.FLAGS
    assert not [flag for flag in build.FLAGS if 'fast' in flag or 'unsafe' in flag or 'approx' in flag or 'finite-math' in flag]


def test_names_next_to_an_installed_reference(tmp_path):
    """with a reference package installed behind the overlay the scoring names are still this package's own functions, all but
    ``compute_boundary_distances`` without a session (imsegm.REFERENCE_KEEPS: the reference's own, until the CPU dry run of
    run_eval_superpixels.py has a stand-in for the device call); with ``_session`` it is this package's (a stand-in tree, one child)"""
    import subprocess
    import sys
    pkg = tmp_path / 'imsegm'
    (pkg / 'utilities').mkdir(parents=True)
    for name, text in (('__init__.py', ''), ('pipelines.py', ''), ('utilities/__init__.py', ''),
                       ('labeling.py', 'def compute_boundary_distances(segm_ref, segm):\n    return "reference"\n')):
        (pkg / name).write_text(text)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ('import sys; sys.path[:0] = [%r, %r]\n'
            'import numpy as np, imsegm, imsegm.labeling as lb, pyimsegm_amd.labeling as own\n'
            'assert imsegm.REFERENCE_PATH and lb is own and imsegm.REFERENCE_KEEPS == {"labeling": ("compute_boundary_distances",)}\n'
            'for name in ("contour_binary_map", "contour_coords", "binary_image_from_coords", "compute_distance_map",\n'
            '             "compute_labels_overlap_matrix", "relabel_max_overlap_unique", "relabel_max_overlap_merge"):\n'
            '    call = getattr(lb, name)\n'
            '    assert call.__module__ == "pyimsegm_amd.labeling" and not hasattr(call, "device"), name\n'
            'assert lb.compute_boundary_distances(None, None) == "reference"\n'
            'assert lb.compute_boundary_distances.device.__module__ == "pyimsegm_amd.labeling"\n'
            'class Session(object):\n'
            '    shape = (2, 3)\n'
            '    def boundary_distances(self, ref):\n'
            '        return np.zeros((0, 2), dtype=np.int32), np.zeros(0)\n'
            'points, dist = lb.compute_boundary_distances(np.zeros((2, 3), dtype=int), None, _session=Session())\n'
            'assert points.shape == (0, 2) and points.dtype == np.int64 and dist.shape == (0,)\n' % (root, str(tmp_path)))
    env = dict(os.environ)
    env.pop('IMSEGM_REFERENCE', None)
    res = subprocess.run([sys.executable, '-c', code], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True,
                         timeout=120)
    assert res.returncode == 0, res.stderr[-2000:]


def test_host_statement_of_the_boundary_distances_in_three_dimensions():
    """maps that are not 2-D take numpy / scipy as in the reference (find_boundaries and the distance transform work in n dimensions)"""
    from scipy import ndimage
    from pyimsegm_amd import labeling
    rng = np.random.RandomState(5)
    seg_ref, seg = rng.randint(0, 3, (5, 6, 7)), rng.randint(0, 3, (5, 6, 7))
    cross = ndimage.generate_binary_structure(3, 1)
    on_ref, on_seg = [ndimage.grey_dilation(s, footprint=cross) != ndimage.grey_erosion(s, footprint=cross) for s in (seg_ref, seg)]
    points, dist = labeling.compute_boundary_distances(seg_ref, seg)
    assert B.same(points, np.argwhere(on_ref).astype(np.int64)) and B.same(dist, ndimage.distance_transform_edt(~on_seg)[on_ref])
