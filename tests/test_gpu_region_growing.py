"""The region-growing kernels (csrc/region_growing.hip) against the numpy statement of the same definitions
(pyimsegm_amd/region_growing.py, on='host') on the same inputs, and against the reference: the shape prior and six whole growths of
tests/golden/region_growing.npz, and the vectors the reference's docstrings print (imsegm/region_growing.py:1227-1291, :1552-1617)."""
import importlib

import numpy as np
import pytest

from tests import region_growing_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def rg():
    return importlib.import_module('pyimsegm_amd.region_growing')


def _states(rg, slic, nb_objects):
    host, dev = rg._HostState(slic, nb_objects), rg._DeviceState(slic, nb_objects)
    neighbours = C.neighbour_lists(host.edges, host.n_labels)
    host.attach(*rg._csr_neighbours(neighbours, host.n_labels))
    assert np.array_equal(host.edges, dev.edges) and np.array_equal(host.sums(), dev.sums())
    assert np.array_equal(host.points(), dev.points())
    return host, dev, neighbours


def _squares_map(nb_labels):
    """nb_labels superpixels in a row of width-3 strips whose rounded centres step by 3 columns"""
    return np.repeat(np.arange(nb_labels), 3)[None, :].repeat(2, axis=0)


@pytest.mark.parametrize('nb_labels', [1, 63, 64, 65, 257, 2049])
def test_shape_cost_sizes(rg, nb_labels):
    """every block boundary of k_rg_shape_cost; 1, 2 and 9 objects, two of them with tables of other sizes in one call"""
    height, width = (3, 5) if nb_labels == 1 else (64, 96) if nb_labels < 300 else (120, 160)
    slic = C.random_map(nb_labels, height, width, nb_labels)
    for nb_objects in (1, 2, 9):
        host, dev, _ = _states(rg, slic, nb_objects)
        try:
            rng = np.random.RandomState(nb_labels + nb_objects)
            dims = [(4, 2), (8, 9), (36, 50)]
            tables = [C.smooth_cdf(*dims[(i + nb_labels) % 3], seed=i) for i in range(nb_objects)]
            centres = np.round(rng.rand(nb_objects, 2) * [height, width], 3) + 0.137       # not integers: the centre_init clamp
            shifts = np.round(rng.rand(nb_objects) * 360, 2) + 0.003
            for table, centre, shift in zip(tables, centres, shifts):
                margins = C.shape_margins(host.points(), centre, shift, *table.shape)
                assert margins[0] > 1e-6 and margins[1] > 1e-9 and margins[2] > 1e-9, 'choose another seed: %r' % (margins, )
            start = np.zeros((nb_labels, nb_objects + 1))
            host.set_costs(start, start)
            dev.set_costs(start, start)
            objects = np.arange(nb_objects)[::-1]
            want = host.update_shape_costs(objects, centres, shifts, tables, with_proba=True)
            got = dev.update_shape_costs(objects, centres, shifts, tables, with_proba=True)
            print('shape prior, K %d objects %d: max |device - host| %.3g' % (nb_labels, nb_objects, np.max(np.abs(got - want))))
            assert float(np.max(np.abs(got - want))) <= 1e-12
            cost_h, cost_d = host.shape_costs(), dev.shape_costs()
            assert np.array_equal(cost_d[:, 0], start[:, 0])
            # -log(p + 0.01) moves by at most 1e-12 / 0.01 (plus the last bits of log)
            assert float(np.max(np.abs(cost_d - cost_h))) <= 1e-10 + 1e-14
        finally:
            dev.close()


def test_shape_cost_edge_cases(rg):
    """a point on the centre, points at exactly D - 1 and D - 2, the wrap row, a table holding 0 and a value that gives inf;
    integer geometry, so both sides take the same branch and the interpolation weights are exact"""
    slic = _squares_map(12)                                   # rounded centres (0 or 1, 1 + 3 k)
    host, dev, _ = _states(rg, slic, 2)
    try:
        points = host.points()
        row = int(points[0, 0])
        assert np.array_equal(points[:, 1], 1 + 3 * np.arange(12)) and (points[:, 0] == row).all()
        table = np.arange(4 * 7, dtype=float).reshape(4, 7) / 40.
        table[0, 3], table[0, 6] = 0., -rg.MIN_SHAPE_PROB      # -log(0.01) at distance 3, inf at distance >= 6 (both on row 0)
        centre = (float(row), 1.)                             # the first point; distances 0, 3, 6 (= D - 1), ...: row 0 of the table
        zeros = np.zeros((12, 3))
        host.set_costs(zeros, zeros)
        dev.set_costs(zeros, zeros)
        objects, centres, shifts = [0, 1], [centre, (row + 4., 4.)], [0., 300.]
        want = host.update_shape_costs(objects, centres, shifts, [table, table], with_proba=True)
        got = dev.update_shape_costs(objects, centres, shifts, [table, table], with_proba=True)
        assert want[0, 0] == table[1, 0]                      # atan2(0, 0) = 0: 90 degrees, row 1
        assert want[0, 1] == 0. and want[0, 2] == -rg.MIN_SHAPE_PROB and want[0, 3] == -rg.MIN_SHAPE_PROB
        assert float(np.max(np.abs(got - want))) <= 1e-12
        assert np.array_equal(got[0], want[0])                # exact geometry on object 0: the same table entries
        cost = dev.shape_costs()
        assert abs(cost[1, 1] + np.log(0.01)) <= 4e-15 and cost[2, 1] == rg.GC_REPLACE_INF
        # object 1: 3-4-5 triangles give dist = 5 = D - 2 exactly at the point (row, 1) and the wrap row for angles past 270 degrees
        assert np.allclose(cost[:, 2], host.shape_costs()[:, 2], rtol=0, atol=1e-10)
    finally:
        dev.close()


@pytest.mark.parametrize('nb_labels', [2, 64, 65, 300])
def test_candidates_and_scores(rg, nb_labels):
    slic = C.random_map(nb_labels, 40, 56, nb_labels)
    nb_objects = min(3, nb_labels)
    host, dev, neighbours = _states(rg, slic, nb_objects)
    try:
        lut_data, lut_shape = C.random_costs(nb_labels, nb_labels, nb_objects)
        host.set_costs(lut_data, lut_shape)
        dev.set_costs(lut_data, lut_shape)
        labels = C.grown_labels(nb_labels + 1, host.edges, nb_labels, nb_objects)
        trans = (0.1, 0.03)
        twice = 0
        for allow_obj_swap in (True, False):
            for coef_pairwise in (0., 1.5):
                coefs = (1., 2., coef_pairwise)
                want = host.greedy_step(labels, allow_obj_swap, *coefs, *rg._penalties(trans))
                got = dev.greedy_step(labels, allow_obj_swap, *coefs, *rg._penalties(trans))
                assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
                brute = C.brute_candidates(rg, labels, neighbours, nb_objects, allow_obj_swap)
                assert np.array_equal(got[0], brute[0]) and np.array_equal(got[1], brute[1])
                twice += len(got[1]) - len(set(got[1].tolist()))
                crit, full = C.brute_changes(rg, got[0], got[1], labels, lut_data, lut_shape, host.sums()[:, 0], host.edges, coefs, trans)
                bound = (nb_labels + len(host.edges)) * 2.**-53 * crit
                if len(full):
                    print('K %d swap %d pairwise %g: max |device - full sums| %.3g, bound %.3g' %
                          (nb_labels, allow_obj_swap, coef_pairwise, np.max(np.abs(got[2] - full)), bound))
                    assert float(np.max(np.abs(got[2] - full))) <= bound
                    assert np.array_equal(got[2], want[2])                       # the same operations in the same order
                only = dev.greedy_step(None, allow_obj_swap, *coefs, *rg._penalties(trans), with_scores=False)
                assert np.array_equal(only[0], got[0]) and np.array_equal(only[1], got[1]) and only[2] is None
        if nb_labels in (64, 65):
            assert twice > 0, 'the case needs a superpixel that is a candidate of two objects'
        if nb_labels >= 64:
            assert (labels == nb_objects).sum() == 1, 'the case needs an object of one superpixel'
    finally:
        dev.close()


def test_object_without_free_neighbour(rg):
    slic = _squares_map(5)
    host, dev, _ = _states(rg, slic, 2)
    try:
        zeros = np.zeros((5, 3))
        dev.set_costs(zeros, zeros)
        objects, superpixels, _ = dev.greedy_step([2, 1, 2, 2, 2], False, 1., 1., 1., 2., 3.)       # object 1 walled in, no background
        assert len(objects) == 0 and len(superpixels) == 0
        objects, superpixels, _ = dev.greedy_step(None, True, 1., 1., 1., 2., 3.)
        assert objects.tolist() == [1, 1, 2] and superpixels.tolist() == [0, 2, 1]
    finally:
        dev.close()


@pytest.mark.parametrize('nb_labels', [1, 255, 256, 257, 1025])
def test_criterion(rg, nb_labels):
    height, width = (3, 5) if nb_labels == 1 else (64, 96)
    slic = C.random_map(nb_labels, height, width, nb_labels)
    nb_objects = 2
    host, dev, _ = _states(rg, slic, nb_objects)
    try:
        lut_data, lut_shape = C.random_costs(nb_labels, nb_labels, nb_objects)
        host.set_costs(lut_data, lut_shape)
        dev.set_costs(lut_data, lut_shape)
        labels = np.random.RandomState(nb_labels).randint(0, nb_objects + 1, nb_labels)
        for coef_pairwise in (0., 2.):
            terms = (1., 3., coef_pairwise) + rg._penalties((0.1, 0.03))
            first, second = dev.criterion(labels, *terms), dev.criterion(labels, *terms)
            assert np.float64(first).tobytes() == np.float64(second).tobytes()
            assert first == host.criterion(labels, *terms)                       # the same tree
            want = rg.compute_rg_crit(labels, lut_data, lut_shape, host.sums()[:, 0], host.edges.reshape(-1, 2), 1., 3., coef_pairwise,
                                      (0.1, 0.03))
            assert abs(first - want) <= (nb_labels + len(host.edges)) * 2.**-53 * want
    finally:
        dev.close()


@pytest.mark.parametrize('shape, nb_labels', [((7, 9), 12), ((96, 128), 200)])
@pytest.mark.parametrize('nb_angles', [4, 36, 72])
def test_object_rays(rg, shape, nb_labels, nb_angles):
    from scipy import ndimage
    from pyimsegm_amd.descriptors import _ray_directions, hip_ray_features_positions
    slic = C.random_map(nb_labels + 1, shape[0], shape[1], nb_labels)
    slic[shape[0] // 2 + 1, shape[1] // 2 + 2] = nb_labels                  # a superpixel of one pixel
    nb_labels, nb_objects = nb_labels + 1, 4
    host, dev, _ = _states(rg, slic, nb_objects)
    try:
        labels = np.zeros(nb_labels, dtype=int)
        labels[slic[0, 0]] = 1                                              # touches the border: rays that leave the image
        for s in C.neighbour_lists(host.edges, nb_labels)[slic[0, 0]]:
            labels[s] = 1
        inner = slic[shape[0] // 2, shape[1] // 2]
        if labels[inner] == 0:
            labels[inner] = 2
        labels[nb_labels - 1] = 3                                           # object 3: one pixel; object 4: absent
        assert host.sums()[nb_labels - 1, 0] == 1
        segm = labels[slic]
        positions = rg._mass_centres(host.sums(), labels, nb_objects)
        for i in range(nb_objects):
            if (segm == i + 1).any():
                assert positions[i].tolist() == [int(round(c)) for c in ndimage.center_of_mass(segm == i + 1)]
            else:
                assert positions[i].tolist() == [-1, -1]
        directions = _ray_directions(360. / nb_angles)
        got = dev.object_rays(labels, positions, directions)
        assert got.dtype == np.float32 and got.shape == (nb_objects, nb_angles)
        for i in range(nb_objects):
            want = hip_ray_features_positions(segm == i + 1, [positions[i]], 360. / nb_angles, 'down')[0]
            assert np.array_equal(got[i].view(np.uint32), want.view(np.uint32)), i
            assert np.array_equal(got[i], rg.ray_distances_down(segm == i + 1, positions[i], directions))
        assert (got[0] == -1).any() and (got[3] == -1).all()
    finally:
        dev.close()


def _doctest_inputs(disc):
    slic = C.grid_slic()
    if disc:
        return slic, C.prob_fg(slic, np.ones((15, 20), dtype=int), [0.1, 0.9]), [(6.5, 9)], (None, C.disc_chist())
    return slic, C.prob_fg(slic, C.doctest_block(), [0.1, 0.9]), [(7.5, 10)], (None, C.DOCTEST_CHIST)


def test_segm_prob_fg(rg):
    slic = np.array([[0, 0, 0, 0, 1, 1, 1, 1], [2, 2, 2, 2, 3, 3, 3, 3]])
    segm = np.array([0, 1, 1, 0])[slic]
    assert rg.compute_segm_prob_fg(slic, segm, [0.3, 0.8]).tolist() == [0.3, 0.8, 0.8, 0.3]


def test_reference_greedy_examples_on_the_device(rg):
    slic, prob, centres, model = _doctest_inputs(False)
    for coef_pairwise, head, tail in C.DOCTEST_GREEDY:
        history = {}
        labels = rg.region_growing_shape_slic_greedy(slic, prob, centres, model, coef_pairwise=coef_pairwise, debug_history=history,
                                                     on='device')
        criteria = np.round(history['criteria']).astype(int).tolist()
        assert criteria[:len(head)] == head and criteria[-2:] == tail
        assert np.array_equal(labels[slic], C.doctest_expected_block())
    slic, prob, centres, model = _doctest_inputs(True)
    history = {}
    labels = rg.region_growing_shape_slic_greedy(slic, prob, centres, model, coef_shape=10, coef_pairwise=1, debug_history=history,
                                                 on='device')
    assert np.round(history['criteria']).astype(int).tolist() == C.DOCTEST_GREEDY_DISC
    assert np.array_equal(labels[slic], C.doctest_expected_disc())


def test_reference_graphcut_examples(rg):
    slic, prob, centres, model = _doctest_inputs(False)
    for coef_pairwise, want in C.DOCTEST_GRAPHCUT:
        for on in ('device', 'host'):
            history = {}
            labels = rg.region_growing_shape_slic_graphcut(slic, prob, centres, model, coef_pairwise=coef_pairwise, debug_history=history,
                                                           on=on)
            assert np.round(history['criteria']).astype(int).tolist() == want
            assert np.array_equal(labels[slic], C.doctest_expected_block())
    slic, prob, centres, model = _doctest_inputs(True)
    history = {}
    labels = rg.region_growing_shape_slic_graphcut(slic, prob, centres, model, coef_shape=10., coef_pairwise=1, debug_history=history,
                                                   on='device')
    assert np.round(history['criteria']).astype(int).tolist() == C.DOCTEST_GRAPHCUT_DISC
    assert np.array_equal(labels[slic], C.doctest_expected_disc())


@pytest.fixture(scope='module')
def fixture():
    return C.load_fixture()


@pytest.mark.parametrize('name', C.GROWTH_CASES)
@pytest.mark.parametrize('method', ['greedy', 'graphcut'])
def test_whole_growth_against_the_reference(rg, fixture, method, name):
    """the six growths of tests/golden/region_growing.npz on the device: labels of every iteration, returned labels, centres and
    shifts equal to the reference's, criteria within the re-ordering bound, the shape prior of the first and last table within
    ``shape_prior_tol``, the rays of k_rg_object_rays bit for bit"""
    C.check_growth_against_fixture(rg, fixture, method, name, 'device')


def test_shape_cost_against_the_reference(rg, fixture):
    """k_rg_shape_cost against the reference's ``interp2d`` values: the grid points are the single-pixel superpixels 1 .. 60"""
    at = 0
    for points, centre, shift, table in C.shape_prior_grid():
        dev = rg._DeviceState(C.pixel_map(points), 1)
        try:
            assert np.array_equal(dev.points()[1:], points)
            zeros = np.zeros((len(points) + 1, 2))
            dev.set_costs(zeros, zeros)
            got = dev.update_shape_costs([0], [centre], [shift], [table], with_proba=True)[0, 1:]
        finally:
            dev.close()
        want = fixture['shape_prior'][at:at + len(points)]
        at += len(points)
        gap = float(np.max(np.abs(got - want)))
        print('A %d D %d: max |device - reference| %.3g, tol %.3g' % (table.shape + (gap, float(fixture['shape_prior_tol']))))
        assert gap <= float(fixture['shape_prior_tol'])


def test_graphcut_per_object(rg):
    slic, prob, centres, model, shape_type = C.growth_case('three_cdf')
    got = rg.region_growing_shape_slic_graphcut(slic, prob, centres, model, shape_type, optim_global=False, nb_iter=10, on='device')
    want = rg.region_growing_shape_slic_graphcut(slic, prob, centres, model, shape_type, optim_global=False, nb_iter=10, on='host')
    assert np.array_equal(got, want) and set(np.unique(got)) == {0, 1, 2, 3}


def test_rejected_arguments(rg):
    from pyimsegm_amd import _hip
    slic, prob, centres, model = _doctest_inputs(False)
    with pytest.raises(ValueError, match='dims of probs'):
        rg.region_growing_shape_slic_greedy(slic, prob[:10], centres, model, on='device')
    with pytest.raises(NameError, match='Not supported type of shape model'):
        rg.region_growing_shape_slic_graphcut(slic, prob, centres, model, shape_type='nope', on='device')
    with pytest.raises(ValueError, match='outside the map'):
        rg.region_growing_shape_slic_greedy(slic, prob, [(15, 3)], model, on='device')
    with pytest.raises(ValueError, match="on is 'host' or 'device'"):
        rg.region_growing_shape_slic_graphcut(slic, prob, centres, model, on='nonsense')
    dev = rg._DeviceState(slic, 1)
    try:
        with pytest.raises(_hip.HipError, match='outside'):
            dev.criterion(np.full(dev.n_labels, 2), 1., 1., 1., 1., 1.)              # a label without a column
        with pytest.raises(_hip.HipError, match='finite'):
            dev.update_shape_costs([0], [(np.inf, 0.)], [0.], [np.ones((4, 4))])
        with pytest.raises(_hip.HipError, match='object'):
            dev.update_shape_costs([1], [(1., 0.)], [0.], [np.ones((4, 4))])
        with pytest.raises(_hip.HipError, match='edges'):
            _hip.RegionGrowing(dev.sess, dev.edges[:-1], 1)
    finally:
        dev.close()


def test_state_outlives_its_session_safely(rg):
    """a session closed first: the state refuses every call (it would read the freed session) and still frees its own buffers"""
    from pyimsegm_amd import _hip
    dev = rg._DeviceState(C.grid_slic(), 1)
    dev.sess.close()
    with pytest.raises(_hip.HipError, match='closed'):
        dev.rg.sums()
    with pytest.raises(_hip.HipError, match='closed'):
        dev.rg.criterion(None, 1., 1., 1., 1., 1.)
    dev.close()
    assert dev.rg._h is None
