"""The centre-candidate point descriptors on the device (csrc/points.hip) through the public names of ``pyimsegm_amd.descriptors``:
label rings bit for bit against the numpy statement of tests/points_cases.py, probability rings within the bound of float64
summation against long-double sums, ray features bit for bit against the per-position calls on a host-built mask, the smoothing
within one float32 spacing of ``scipy.ndimage.gaussian_filter1d``."""
import numpy as np
import pytest
from scipy import ndimage

import points_cases as PC

pytestmark = pytest.mark.gpu

LABEL_CASES = PC.label_ring_cases()
LAYER_CASES = PC.layer_ring_cases()
RAY_CASES = [(border, edge) for border in PC.RAY_BORDER_SETS for edge in ('up', 'down')]
SMOOTH_CASES = [(1.0, 45), (3.0, 45), (1.0, 5)]
assert LABEL_CASES and LAYER_CASES and RAY_CASES and SMOOTH_CASES and PC.RAY_POSITIONS


@pytest.fixture(scope='module')
def hip():
    from pyimsegm_amd import _hip
    _hip.default_context()
    return _hip


@pytest.fixture(scope='module')
def descriptors(hip):
    import imsegm.descriptors
    import pyimsegm_amd.descriptors
    assert imsegm.descriptors is pyimsegm_amd.descriptors
    for name in ('compute_label_histograms_positions', 'compute_label_hist_proba', 'compute_ray_features_positions', 'shift_ray_features'):
        assert callable(vars(imsegm.descriptors).get(name)), name
    return imsegm.descriptors


# ---- label rings ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', LABEL_CASES, ids=[c[0] for c in LABEL_CASES])
def test_label_rings_equal_the_statement(descriptors, hip, case):
    _, segm, positions, radii, nb_labels = case
    if 'error' in case[0]:
        with pytest.raises(ValueError) as stated:
            PC.label_ring_table(segm, positions, radii, nb_labels)
        with pytest.raises(ValueError) as raised:
            descriptors.compute_label_histograms_positions(segm, positions, radii, nb_labels)
        assert str(raised.value) == str(stated.value) == 'norm or element should be positive'
        return
    table, names = descriptors.compute_label_histograms_positions(segm, positions, radii, nb_labels)
    expected = PC.label_ring_table(segm, positions, radii, nb_labels)
    assert names == PC.ring_names(radii, nb_labels)
    assert table.dtype == np.float64 and table.shape == expected.shape
    assert np.array_equal(table, expected)
    on_device = len(radii) * (nb_labels + 1) <= hip.RING_MAX_BINS
    assert on_device == ('composed' not in case[0])


def test_label_rings_counts_and_sizes(hip):
    """the integers behind the rings: counts per disc and label, sizes of the clipped discs whatever the label"""
    _, segm, positions, radii, nb_labels = [c for c in LABEL_CASES if c[0] == 'labels -1 and nb_labels'][0]
    assert segm.min() == -1 and segm.max() == nb_labels
    hist, size = hip.ring_hist2d(segm, positions, radii, nb_labels)
    assert hist.dtype == np.uint32 and size.dtype == np.uint32
    for p, pos in enumerate(positions):
        for d, radius in enumerate(radii):
            counts, pixels = PC.label_counts(segm, pos, PC.disc(radius), nb_labels)
            assert hist[p, d].tolist() == counts.tolist() and size[p, d] == pixels, (pos, radius)
    assert np.any(hist.sum(axis=2) < size)                  # some pixel counted for the size and for no label


def test_label_rings_default_nb_labels_and_default_radii(descriptors):
    segm = PC.random_label_map()
    positions = PC.random_positions(segm.shape, 9, seed=4)
    table, names = descriptors.compute_label_histograms_positions(segm, positions)
    assert names == PC.ring_names(PC.DEFAULT_RADII, 3)
    assert np.array_equal(table, PC.label_ring_table(segm, positions, PC.DEFAULT_RADII, 3))


@pytest.mark.parametrize('radii', [[4, 2], [3, 3]])
def test_label_rings_raise_the_reference_errors(descriptors, radii):
    for segm in (PC.doctest_label_map(), PC.doctest_layers()):
        with pytest.raises(ValueError) as raised:
            descriptors.compute_label_histograms_positions(segm, PC.DOCTEST_POINTS, radii)
        assert str(raised.value) == 'norm or element should be positive'


def test_library_refuses_what_the_kernels_do_not_take(hip):
    segm = PC.doctest_label_map()
    for radii, nb_labels, positions in (([4, 2], 3, [[1, 1]]), ([1, 2, 3, 4, 5, 6], 5, [[1, 1]]), ([1, 2], 3, [[10, 0]]),
                                        ([1, 2], 3, [[0, -1]])):
        with pytest.raises(hip.HipError):
            hip.ring_hist2d(segm, positions, radii, nb_labels)
    with pytest.raises(hip.HipError):
        hip.ring_hist_proba2d(PC.doctest_layers(), [[1, 1]], list(range(1, 18)))
    with pytest.raises(hip.HipError):
        hip.ray_features_labels2d(segm, list(range(65)), [[1, 1]], np.ones((8, 2)), 1)


def test_no_position(descriptors):
    nothing = np.zeros((0, 2), dtype=int)
    table, names = descriptors.compute_label_histograms_positions(PC.doctest_label_map(), nothing, [1, 2, 4])
    assert table.shape == (0, 9) and names == PC.DOCTEST_NAMES
    table, names = descriptors.compute_label_histograms_positions(PC.doctest_layers(), nothing, [1, 2, 4])
    assert table.shape == (0, 6)
    rays, shifts, names = descriptors.compute_ray_features_positions(PC.ray_map(), nothing, 45)
    assert rays.shape == (0, 8) and shifts == [] and len(names) == 8


# ---- probability rings ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', LAYER_CASES, ids=[c[0] for c in LAYER_CASES])
def test_layer_sums_within_the_float64_bound_and_repeatable(hip, case):
    _, layers, positions, radii = case
    total, size = hip.ring_hist_proba2d(layers, positions, radii)
    again, size_again = hip.ring_hist_proba2d(layers, positions, radii)
    assert total.dtype == np.float64 and total.tobytes() == again.tobytes() and np.array_equal(size, size_again)
    worst = 0.
    for p, pos in enumerate(positions):
        for d, radius in enumerate(radii):
            exact, magnitude, pixels = PC.layer_sums(layers, pos, PC.disc(radius))
            assert size[p, d] == pixels
            bound = pixels * np.longdouble(2.) ** -53 * magnitude        # float64 summation of n values in any order
            error = np.abs(total[p, d].astype(np.longdouble) - exact)
            worst = max(worst, float(np.max(error / bound)))
            assert np.all(error <= bound), (pos, radius, error, bound)
    print('largest error / bound: %.3g' % worst)


@pytest.mark.parametrize('case', LAYER_CASES[:2], ids=[c[0] for c in LAYER_CASES[:2]])
def test_layer_rings_table(descriptors, case):
    """the ring values: differences of two such sums over an exact integer.  Every sum is within n 2^-53 sum|x| of the exact one
    (the test above, for the device; the same bound holds for the float64 rounding of the long-double sum with n >= 1), so a ring
    value differs by at most (bound_d + bound_{d-1}) / inter_size before the one division, which adds half a spacing"""
    _, layers, positions, radii = case
    table, names = descriptors.compute_label_histograms_positions(layers, positions, radii)
    channels = layers.shape[2]
    assert names == PC.ring_names(radii, channels) and table.shape == (len(positions), len(radii) * channels)
    expected = PC.layer_ring_table(layers, positions, radii)
    eps = 2. ** -53
    for p, pos in enumerate(positions):
        bound_last, size_last = np.zeros(channels), 0
        for d, radius in enumerate(radii):
            _, magnitude, pixels = PC.layer_sums(layers, pos, PC.disc(radius))
            bound = 2 * pixels * eps * magnitude.astype(float)                       # both sides carry the bound
            cells = slice(d * channels, (d + 1) * channels)
            allowed = (bound + bound_last) / (pixels - size_last) * (1 + 4 * eps) + 4 * eps * np.abs(expected[p, cells])
            assert np.all(np.abs(table[p, cells] - expected[p, cells]) <= allowed), (pos, radius)
            bound_last, size_last = bound, pixels


def test_layer_rings_doctest(descriptors):
    table, _ = descriptors.compute_label_histograms_positions(PC.doctest_layers(), PC.DOCTEST_POINTS, PC.DOCTEST_RADII)
    assert np.array_equal(table, PC.layer_ring_table(PC.doctest_layers(), PC.DOCTEST_POINTS, PC.DOCTEST_RADII))   # integers: exact
    assert np.array_equal(np.round(table, 2), PC.DOCTEST_LAYER_TABLE)


# ---- rays --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def plain_rays(descriptors):
    """per border set, edge and angle step: the rows of the existing per-position call on the host-built mask (computed once)"""
    segm, rows = PC.ray_map(), {}
    for border, edge in RAY_CASES:
        mask = np.isin(segm, border)
        for step in (45, 5):
            rows[tuple(border), edge, step] = np.array([descriptors.compute_ray_features_segm_2d(mask, pos, step, 0, edge)
                                                        for pos in PC.RAY_POSITIONS])
    return rows


@pytest.mark.parametrize('border,edge', RAY_CASES, ids=['%s-%s' % (''.join(map(str, b)), e) for b, e in RAY_CASES])
def test_rays_equal_the_per_position_calls(descriptors, plain_rays, border, edge):
    for step in (45, 5):
        rays, shifts, names = descriptors.compute_ray_features_positions(PC.ray_map(), PC.RAY_POSITIONS, step, border_labels=border,
                                                                         shifting=False, edge=edge)
        expected = plain_rays[tuple(border), edge, step]
        assert rays.dtype == np.float32 and rays.shape == expected.shape == (len(PC.RAY_POSITIONS), 360 // step)
        assert rays.tobytes() == expected.tobytes()
        assert shifts == [0.] * len(PC.RAY_POSITIONS) and all(isinstance(s, float) for s in shifts)
        assert names == PC.ray_names(border, step, 360 // step)
    if border == [7]:
        assert np.all(expected == -1)                       # nothing to meet
    else:
        assert np.any(expected > 0) and (edge == 'down' or np.any(expected == 0))


def test_rays_of_layers_go_through_argmax(descriptors, plain_rays):
    segm = PC.ray_map()
    layers = (segm[:, :, None] == np.arange(4)).astype(float)
    rays, _, _ = descriptors.compute_ray_features_positions(layers, PC.RAY_POSITIONS, 45, border_labels=[1, 2], shifting=False)
    assert rays.tobytes() == plain_rays[(1, 2), 'up', 45].tobytes()


@pytest.mark.parametrize('sigma,step', SMOOTH_CASES)
def test_smoothed_rays_within_one_spacing_of_scipy(descriptors, plain_rays, sigma, step):
    """float64 accumulation in scipy's order: only a float32 rounding at a tie can move"""
    for border, edge in RAY_CASES:
        rays, _, _ = descriptors.compute_ray_features_positions(PC.ray_map(), PC.RAY_POSITIONS, step, border_labels=border,
                                                                smooth_ray=sigma, shifting=False, edge=edge)
        expected = np.array([ndimage.gaussian_filter1d(row, sigma) for row in plain_rays[tuple(border), edge, step]])
        assert rays.dtype == expected.dtype == np.float32
        spacing = np.spacing(np.abs(expected))
        print('%s %s sigma %g step %d: %d of %d values differ' % (border, edge, sigma, step, np.count_nonzero(rays != expected), rays.size))
        assert np.all(np.abs(rays.astype(np.float64) - expected) <= spacing), (border, edge)


def test_shifted_rays_equal_the_row_by_row_shift(descriptors, plain_rays):
    for border, edge in RAY_CASES:
        rays, shifts, names = descriptors.compute_ray_features_positions(PC.ray_map(), PC.RAY_POSITIONS, 5, border_labels=border, edge=edge)
        rows = [descriptors.shift_ray_features(row) for row in plain_rays[tuple(border), edge, 5]]
        expected = np.array([row for row, _ in rows])
        assert rays.dtype == expected.dtype and rays.tobytes() == expected.tobytes()
        assert shifts == [float(shift) for _, shift in rows]
        assert names == PC.ray_names(border, 5, 72)


def test_rays_opened_mask_and_default_border(descriptors, monkeypatch):
    """``segm_open`` opens the host-built mask with ``skimage.morphology`` (imported only in that branch; a stand-in with the same
    two functions here) before the upload; border_labels defaults to [0]"""
    import sys
    import types
    morphology = types.ModuleType('skimage.morphology')
    morphology.disk = PC.disc
    morphology.opening = lambda image, footprint: ndimage.binary_opening(image, structure=footprint)
    package = types.ModuleType('skimage')
    package.morphology = morphology
    monkeypatch.setitem(sys.modules, 'skimage', package)
    monkeypatch.setitem(sys.modules, 'skimage.morphology', morphology)
    segm = PC.ray_map()
    opened = morphology.opening(segm == 0, PC.disc(3))
    assert np.any(opened != (segm == 0))
    rays, _, names = descriptors.compute_ray_features_positions(segm, PC.RAY_POSITIONS, 45, segm_open=3, shifting=False)
    expected = np.array([descriptors.compute_ray_features_segm_2d(opened, pos, 45, 0, 'up') for pos in PC.RAY_POSITIONS])
    assert rays.tobytes() == expected.tobytes() and names == PC.ray_names([0], 45, 8)
