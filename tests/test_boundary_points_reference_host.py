"""The host statement of the boundary-point step (pyimsegm_amd/ellipse_fitting.py: ``split_host``, ``ray_walk_host`` and the
``prepare_boundary_points_ray_*`` functions with ``on='host'``) against what is known without a device: the results the reference
records in its docstrings and in tests/golden/ellipse.npz, brute-force erosion and dilation by the disc footprint, and
``scipy.ndimage.binary_fill_holes``.  tests/test_gpu_boundary_points.py then holds the kernels to this statement byte for byte."""
import numpy as np
import pytest
from scipy import ndimage

import boundary_points_cases as C

EDGE = C.edge_cases()


@pytest.fixture(scope='module')
def ell():
    from pyimsegm_amd import build, ellipse_fitting
    build.build(verbose=False)
    return ellipse_fitting


def brute_opening(mask, radius):
    """erosion, then dilation, by explicit loops over the offsets of the disc; pixels outside the image are ignored"""
    mask = np.asarray(mask, dtype=bool)
    height, width = mask.shape
    offsets = [(dy, dx) for dy in range(-radius, radius + 1) for dx in range(-radius, radius + 1) if dy * dy + dx * dx <= radius * radius]

    def shifted(image, dy, dx, fill):
        out = np.full(image.shape, fill, dtype=bool)
        ys, ye, xs, xe = max(0, -dy), min(height, height - dy), max(0, -dx), min(width, width - dx)
        if ys < ye and xs < xe:
            out[ys:ye, xs:xe] = image[ys + dy:ye + dy, xs + dx:xe + dx]
        return out

    eroded = np.ones_like(mask)
    for dy, dx in offsets:
        eroded &= shifted(mask, dy, dx, True)
    opened = np.zeros_like(mask)
    for dy, dx in offsets:
        opened |= shifted(eroded, dy, dx, False)
    return opened


def test_host_statement_reproduces_the_docstrings(ell):
    fixture = C.doctest_fixture()
    for name, example in fixture['examples'].items():
        arguments = {k: v for k, v in example.items() if k not in ('points', 'decimals', 'close_points')}
        points = getattr(ell, name)(fixture['seg'], fixture['centers'], example['close_points'], on='host', **arguments)
        assert np.round(points, example['decimals']).tolist() == example['points'], name


def test_host_statement_reproduces_the_golden_points(ell):
    call = dict(C.ELLIPSE_CALL)
    points = ell.prepare_boundary_points_ray_dist(C.ellipse_map(), call.pop('centers'), call.pop('close_points'), on='host', **call)
    want = C.golden_points()
    assert len(points) == 1 and points[0].shape == want.shape
    measured = float(np.abs(points[0] - want).max())
    print('largest difference to doctest_points: %r (recorded: %r, tolerance %r)' % (measured, C.ELLIPSE_MEASURED_DIFF, C.ELLIPSE_TOLERANCE))
    assert measured <= C.ELLIPSE_TOLERANCE


@pytest.mark.parametrize('name', sorted(EDGE))
def test_opening_equals_brute_force(ell, name):
    case = EDGE[name]
    seg = case['seg']
    background = ~ndimage.binary_fill_holes(seg > 0)
    for mask, radius in ((background, case['sel_bg']), (seg == 1, case['sel_fg'])):
        if radius > 0:
            assert np.array_equal(ell.opening_host(mask, radius), brute_opening(mask, radius)), (name, radius)
    seg_bg, seg_fg = ell.split_host(seg, case['sel_bg'], case['sel_fg'])
    assert np.array_equal(seg_bg, brute_opening(background, case['sel_bg']) if case['sel_bg'] > 0 else background)
    assert np.array_equal(seg_fg, brute_opening(seg == 1, case['sel_fg']) if case['sel_fg'] > 0 else seg == 1)


@pytest.mark.parametrize('name', sorted(EDGE))
def test_fill_holes_equals_scipy(ell, name):
    seg = EDGE[name]['seg']
    for mask in (seg > 0, seg == 1, seg == 0):
        assert np.array_equal(ell.fill_holes_host(mask), ndimage.binary_fill_holes(mask)), name


def test_the_edge_maps_hold_what_they_are_for(ell):
    seg = EDGE['diagonal_hole']['seg']
    assert seg[1, 1] == 0 and ell.fill_holes_host(seg > 0)[1, 1] and not ell.fill_holes_host(seg > 0)[0, 0]
    assert ell.fill_holes_host(seg > 0)[5, 5] and ell.fill_holes_host(seg > 0)[3, 3] == (seg[3, 3] > 0)
    nested = EDGE['nested']['seg']
    filled = ell.fill_holes_host(nested > 0)
    assert nested[42, 40] == 0 and nested[40, 16] == 1 and filled[42, 40] and filled[40, 41 - 25]
    assert set(np.unique(EDGE['labels_above_1_int64']['seg'])) >= {0, 1, 4} and EDGE['labels_above_1_int64']['seg'].dtype == np.int64
    # the reflecting border: the background of `reflect_background` has zeros only within the radius of the border
    case = EDGE['reflect_background']
    rows, cols = np.nonzero(case['seg'] > 0)
    height, width = case['seg'].shape
    assert np.all(np.minimum(np.minimum(rows, height - 1 - rows), np.minimum(cols, width - 1 - cols)) <= case['sel_bg'])
    assert sorted({case['sel_bg'] for case in EDGE.values()} | {case['sel_fg'] for case in EDGE.values()}) == [0, 1, 2, 5, 15, 33, 40]


def test_point_functions_errors_and_types(ell):
    from pyimsegm_amd import descriptors
    with pytest.raises(ValueError):
        descriptors.reduce_close_points(np.zeros((2, 2)), 1)
    with pytest.raises(ValueError):
        ell.reconstruct_ray_features_2d((1, 1), np.array([1., 2.]))
    with pytest.raises(ValueError):
        ell.reconstruct_ray_features_2d((1, 1, 1), np.array([1., 2., 3.]))
    assert (ell.STRUC_ELEM_BG, ell.STRUC_ELEM_FG, ell.MIN_ELLIPSE_DAIM) == (15, 5, 25.)
    seg_bg, seg_fg = ell.split_segm_background_foreground(EDGE['nested']['seg'], 2, 1, on='host')
    assert seg_bg.dtype.kind == 'i' and seg_fg.dtype == bool
    with pytest.raises(ValueError):
        ell.split_segm_background_foreground(EDGE['nested']['seg'], 2, 1, on='somewhere')
    # every ray of a centre off the map is -1, and the reference's ValueError follows from the empty point list
    case = EDGE['nested']
    with pytest.raises(ValueError):
        ell.prepare_boundary_points_ray_edge(case['seg'], [(-3, 5)], on='host')
    # ray_dist: the list ends at the last centre that got a point
    far = ell.prepare_boundary_points_ray_dist(case['seg'], [(40, 41), (40, 41)], 2, 2, 1, on='host')
    assert len(far) == 1
