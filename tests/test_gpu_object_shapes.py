"""``imsegm_object_shapes`` (csrc/object_shapes.hip) against the numpy / scipy statement of the same definitions
(pyimsegm_amd/region_growing.py, on='host'): labels, int64 moments, centres and raw float32 rays byte for byte, the finished lists
equal.  Maps are the smallest at which the kernels can go wrong: widths beside and across a wave (64 pixels) and a run segment,
single rows and columns, unions that close late, rounding ties, more angles than lanes."""
import importlib

import numpy as np
import pytest

from tests import object_shapes_cases as C
from tests.test_object_shapes_reference_host import check_doctests

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def rg():
    return importlib.import_module('pyimsegm_amd.region_growing')


@pytest.fixture(scope='module')
def hip():
    from pyimsegm_amd import _hip
    _hip.default_context()
    return _hip


def check(rg, hip, img, ray_step=45, objects=None, interp_order=3):
    """the wrapper itself (no fall-back can hide behind it) against the host statement, then the public function both ways"""
    from pyimsegm_amd.descriptors import _ray_directions
    segm = rg._int32_map(img)
    assert segm is not None
    directions = _ray_directions(float(ray_step))
    count, labels, moments, centres, rays = hip.object_shapes(segm, directions, rg.OBJECT_SHAPES_CAPACITY)
    assert labels is not None, 'the device did not take the map (%d)' % count
    want = rg._object_shape_rays_host(segm, directions)
    assert count == len(want[0]) and (objects is None or count == objects)
    for name, got, ref in zip(('labels', 'moments', 'centres', 'rays'), (labels, moments, centres, rays), want):
        assert got.dtype == ref.dtype and got.shape == ref.shape and got.tobytes() == ref.tobytes(), name
    assert rays.shape == (count, len(directions))
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')                      # (np.polyfit through few known rays)
        assert (rg.compute_object_shapes([img], ray_step, interp_order, on='device')
                == rg.compute_object_shapes([img], ray_step, interp_order, on='host'))
    return labels, moments, centres, rays


def blobs(height, width, seed, values, relabel=False):
    """discs of the given values scattered over the map, some cut by its border"""
    rng = np.random.RandomState(seed)
    img = np.zeros((height, width), dtype=np.int32)
    rows, cols = np.indices(img.shape)
    for value in values:
        cy, cx, ry, rx = rng.randint(0, height), rng.randint(0, width), rng.randint(3, 9), rng.randint(3, 12)
        img[((rows - cy) / float(ry))**2 + ((cols - cx) / float(rx))**2 <= 1.] = value
    return (img != 0).astype(np.int32) if relabel else img


@pytest.mark.parametrize('shape', [(61, 67), (64, 130)])
@pytest.mark.parametrize('relabel', [False, True])
def test_widths_beside_and_across_a_wave(rg, hip, shape, relabel):
    img = blobs(shape[0], shape[1], 3, (1, 2, 3, 5, 8, 9), relabel)
    img[10, :] = 1 if relabel else 4                         # a run across every wave segment of the row
    labels, moments, centres, rays = check(rg, hip, img, 45)
    assert len(labels) >= 2 and (rays == -1).any()


@pytest.mark.parametrize('shape', C.SEAM_SHAPES)
@pytest.mark.parametrize('multi', [False, True])
def test_rows_of_more_than_one_chunk(rg, hip, shape, multi):
    """wider than 256 pixels: a workgroup is one of several chunks of its row, and runs, unions and single pixels sit on the seam"""
    labels, moments, centres, rays = check(rg, hip, C.seam_map(shape, multi), 45, objects=3, interp_order=None)
    assert labels.tolist() == ([2, 3, 5] if multi else [1, 2, 3])
    assert moments[:, 0].tolist() == [min(shape[1], 290) - 240, 11, 1] and centres[2].tolist() == [7, 256]


def test_border_components_are_the_background_of_the_inverted_map(rg, hip):
    """two labellings of one map agree: the components of ``m`` that touch the image border (object shapes, pixels != 0) are the
    background that hole filling leaves of ``1 - m`` (pixels <= 0)"""
    from scipy import ndimage
    m = C.seam_map(C.SEAM_SHAPES[1], False)
    m[3:5, 0:3] = 1                                          # one more component on the border, and the U and the pixel inside
    moments = check(rg, hip, m, 45, objects=4, interp_order=None)[1]
    seg_bg, _ = hip.split_background_foreground((1 - m).astype(np.int32), 0, 0)
    numbered, count = ndimage.label(m)                       # scipy's numbering is the order of the device's objects (check)
    on_border = np.unique(np.concatenate([numbered[0], numbered[-1], numbered[:, 0], numbered[:, -1]]))
    on_border = on_border[on_border > 0]
    assert count == 4 and on_border.tolist() == [1, 3]
    assert np.array_equal(seg_bg != 0, np.isin(numbered, on_border))
    rows, cols = np.nonzero(seg_bg)
    assert moments[on_border - 1].sum(axis=0).tolist() == [len(rows), rows.sum(), cols.sum()]


@pytest.mark.parametrize('shape', [(1, 97), (97, 1)])
def test_single_row_and_column(rg, hip, shape):
    line = np.zeros(97, dtype=np.int32)
    line[3:20], line[40:41], line[70:97] = 1, 1, 1
    # (one ray of eight meets an edge in such a map, and np.polyfit cannot fill the others from it: no interpolation)
    check(rg, hip, line.reshape(shape), 45, objects=3, interp_order=None)
    line[40:41], line[70:97] = 2, 3
    check(rg, hip, line.reshape(shape), 45, objects=3, interp_order=None)


def test_late_union_spiral_diagonal_checkerboard(rg, hip):
    u = np.zeros((40, 90), dtype=np.int32)
    u[2:30, 5:15] = 1
    u[2:30, 70:85] = 1
    u[30:38, 5:8] = 1                                        # the arm: down from the left blob, along the bottom, up into the right
    u[36:38, 5:85] = 1
    u[30:38, 82:85] = 1
    check(rg, hip, u, 45, objects=1)
    spiral = np.zeros((31, 70), dtype=np.int32)
    top, left, bottom, right = 1, 1, 29, 68
    while bottom - top > 3 and right - left > 3:
        spiral[top, left:right + 1] = 1
        spiral[top:bottom + 1, right] = 1
        spiral[bottom, left + 2:right + 1] = 1
        spiral[top + 2:bottom + 1, left + 2] = 1
        spiral[top + 2, left + 2:left + 5] = 1              # joins this turn to the next one
        top, left, bottom, right = top + 2, left + 4, bottom - 2, right - 2
    assert check(rg, hip, spiral, 45)[0].tolist() == [1]
    diagonal = np.zeros((9, 70), dtype=np.int32)
    diagonal[0:4, 60:64] = 1
    diagonal[4:8, 64:68] = 1                                 # touches the first at a corner only
    check(rg, hip, diagonal, 45, objects=2)
    board = (np.indices((8, 8)).sum(axis=0) % 2).astype(np.int32)
    labels, moments, centres, rays = check(rg, hip, board, 45, objects=32)
    assert labels.tolist() == list(range(1, 33)) and (moments[:, 0] == 1).all()


def test_two_valued_and_constant_maps(rg, hip):
    base = blobs(30, 70, 5, (1, 1, 1), relabel=True)
    for fg, bg in ((7, 0), (-1, 0)):
        labels = check(rg, hip, np.where(base != 0, fg, bg).astype(np.int32), 45)[0]
        assert len(labels) >= 1 and labels.tolist() == list(range(1, len(labels) + 1))
    check(rg, hip, np.where(base != 0, 2, 1).astype(np.int32), 45, objects=0)          # {1, 2}: one component, dropped
    check(rg, hip, np.zeros((30, 70), dtype=np.int32), 45, objects=0)
    check(rg, hip, np.full((30, 70), 4, dtype=np.int32), 45, objects=0)


def test_multi_label_maps(rg, hip):
    sparse = np.full((40, 80), -3, dtype=np.int32)
    sparse[5:15, 5:30] = 5
    sparse[20:35, 40:75] = 1000
    assert check(rg, hip, sparse, 45)[0].tolist() == [5, 1000]
    covered = np.full((20, 70), 2, dtype=np.int32)           # no background: the smallest value, 2, is no object
    covered[:, 30:50] = 3
    covered[5:9, 60:66] = 9
    assert check(rg, hip, covered, 45)[0].tolist() == [3, 9]
    pieces = np.zeros((50, 140), dtype=np.int32)
    pieces[5:15, 5:15] = 2
    pieces[35:45, 120:135] = 2                               # the centre of 2 lies between its pieces, outside it
    pieces[20:30, 60:80] = 1
    labels, moments, centres, rays = check(rg, hip, pieces, 7)
    assert labels.tolist() == [1, 2] and pieces[centres[1, 0], centres[1, 1]] != 2
    border = np.zeros((33, 66), dtype=np.int32)
    border[0:5, 10:20], border[28:33, 30:40], border[10:20, 0:4], border[12:22, 62:66] = 1, 2, 3, 4
    assert (check(rg, hip, border, 45, objects=4)[3] == -1).any()
    dots = np.zeros((20, 66), dtype=np.int32)
    dots[0, 0], dots[19, 65], dots[7, 63], dots[7, 64] = 1, 2, 3, 5
    labels, moments, centres, rays = check(rg, hip, dots, 45, objects=4)
    assert centres.tolist() == [[0, 0], [19, 65], [7, 63], [7, 64]]


def test_rounding_ties(rg, hip):
    ties = np.zeros((5, 6), dtype=np.int32)
    ties[0:2, 1] = 1
    ties[1:3, 4] = 2
    ties[4, 0] = 3
    labels, moments, centres, rays = check(rg, hip, ties, 45, objects=3)
    assert centres[:2].tolist() == [[0, 1], [2, 4]]          # 0.5 -> 0 and 1.5 -> 2: half to even


@pytest.mark.parametrize('ray_step', [45, 7, 1])
def test_angles(rg, hip, ray_step):
    img = blobs(61, 67, 11, (1, 2, 3))
    rays = check(rg, hip, img, ray_step)[3]
    assert rays.shape[1] == {45: 8, 7: 52, 1: 360}[ray_step]


def test_capacity_and_span(rg, hip):
    from pyimsegm_amd.descriptors import _ray_directions
    six = np.zeros((20, 70), dtype=np.int32)
    for k in range(6):
        six[5:12, 10 * k + 2:10 * k + 8] = k + 1
    result = hip.object_shapes(six, _ray_directions(45.), 4)
    assert result == (6, None, None, None, None)
    assert hip.object_shapes(six, _ray_directions(45.), 0)[0] == 6
    assert hip.object_shapes((six != 0).astype(np.int32), _ray_directions(45.), 4) == (6, None, None, None, None)
    check(rg, hip, six, 45, objects=6)
    wide = six.copy()
    wide[six == 6] = hip.OBJECT_SHAPES_MAX_SPAN                # max - min = the span itself: one beyond the table
    assert hip.object_shapes(wide, _ray_directions(45.), 16) == (-1, None, None, None, None)
    assert rg.compute_object_shapes([wide], 45, on='device') == rg.compute_object_shapes([wide], 45, on='host')
    wide[six == 6] = hip.OBJECT_SHAPES_MAX_SPAN - 1            # the last entry of the table
    assert check(rg, hip, wide, 45, objects=6)[0][-1] == hip.OBJECT_SHAPES_MAX_SPAN - 1
    with pytest.raises(hip.HipError, match='angles'):
        hip.object_shapes(six, np.zeros((hip.RAY_MAX_ANGLES + 1, 2), dtype=np.float32), 4)
    fractional = six * 0.5
    assert rg.compute_object_shapes([fractional], 45, on='device') == rg.compute_object_shapes([six], 45, on='host')


def test_float_doctest_maps_take_the_device(rg, hip, monkeypatch):
    calls = []
    wrapper = hip.object_shapes
    monkeypatch.setattr(hip, 'object_shapes', lambda *a, **k: calls.append(1) or wrapper(*a, **k))
    check_doctests(rg, 'device')
    assert len(calls) == 3                                     # every one of the three float maps went to the device


def test_fixture_cases_on_the_device(rg, hip):
    for name in sorted(C.CASES):
        img, ray_step = C.case(name, 1)
        check(rg, hip, img, ray_step)


def test_scratch_reuse_across_sizes(rg, hip):
    """two maps of different sizes one after the other on the same context, the larger first and again last"""
    large, small = blobs(64, 130, 21, (1, 2, 3, 4)), blobs(17, 23, 22, (1, 2))
    first = check(rg, hip, large, 45)
    check(rg, hip, small, 45)
    check(rg, hip, (small != 0).astype(np.int32), 45)
    again = check(rg, hip, large, 45)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(first, again))
