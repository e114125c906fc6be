"""The numpy statement of the region growing (pyimsegm_amd/region_growing.py, on='host') against the reference's doctest vectors,
against long double, and against the plain forms the kernels shorten (two full sums per candidate, the vertex-by-vertex graph
assembly).  No GPU."""
import doctest
import importlib

import numpy as np
import pytest

from tests import region_growing_cases as C


@pytest.fixture(scope='module')
def rg():
    return importlib.import_module('pyimsegm_amd.region_growing')


def test_doctest_vectors(rg):
    examples = importlib.import_module('tests.doctests.region_growing').EXAMPLES
    parser, runner = doctest.DocTestParser(), doctest.DocTestRunner(verbose=False)
    for name, text in examples.items():
        runner.run(parser.get_doctest(text, dict(rg.__dict__, cases=C, np=np), 'region_growing.' + name, rg.__name__, 0))
    result = runner.summarize(verbose=False)
    assert result.failed == 0 and result.attempted >= 40


def test_interpolate_ray_dist():
    from pyimsegm_amd.descriptors import interpolate_ray_dist
    assert interpolate_ray_dist([-1] * 5).tolist() == [-1] * 5
    vals = np.sin(np.linspace(0, 2 * np.pi, 20)) * 10
    vals[3:7] = -1
    vals[16:] = -1
    assert np.round(interpolate_ray_dist(vals, order='spline')).astype(int).tolist() == \
        [0, 3, 6, 8, 9, 10, 9, 7, 5, 2, -2, -5, -7, -9, -10, -10, -9, -7, -5, -3]
    cubic = interpolate_ray_dist(vals, order=3)
    assert (cubic != -1).all() and np.array_equal(cubic[~np.isin(np.arange(20), [3, 4, 5, 6, 16, 17, 18, 19])],
                                                  vals[~np.isin(np.arange(20), [3, 4, 5, 6, 16, 17, 18, 19])])
    with pytest.raises(NotImplementedError):
        interpolate_ray_dist(vals, order='cos')


@pytest.mark.parametrize('nb_angles, nb_dists', [(4, 2), (8, 9), (36, 50), (72, 30)])
def test_shape_prior_is_bilinear_to_long_double(rg, nb_angles, nb_dists):
    """float64 bilinear against long double on the same cell: a few roundings of values <= 1, bound 1e-12 (the floor of the
    tolerance the fixtures of the reference are held to)"""
    rng = np.random.RandomState(nb_angles * 100 + nb_dists)
    table = C.smooth_cdf(nb_angles, nb_dists, 1)
    points = rng.randint(-5, 70, (500, 2))
    centre, shift = (31.25, 28.5), 37.3
    got = rg.shape_prior_points(points, table, centre, shift)
    want = C.shape_prior_longdouble(points, table, centre, shift)
    assert float(np.max(np.abs(got - want))) < 1e-12
    assert got.min() >= 0 and got.max() <= 1


def test_shape_prior_edge_cases(rg):
    table = np.arange(4 * 6, dtype=float).reshape(4, 6) / 24.
    centre = (10, 10)
    # on the centre: distance 0, atan2(0, 0) = 0 -> angle 810 % 360 = 90 -> row 1, column 0
    assert rg.compute_shape_prior_table_cdf([10, 10], table, centre) == table[1, 0]
    # exactly D - 1 = 5 (3-4-5): the far branch, last column; exactly D - 2 = 4: the near branch on a grid line
    far = rg.compute_shape_prior_table_cdf([13, 14], table, centre)
    angle_norm = ((810 - np.rad2deg(np.arctan2(4, 3))) % 360) / 90.
    assert far == table[int(round(angle_norm)) % 4, 5]
    near = rg.compute_shape_prior_table_cdf([10, 14], table, centre)            # dy = 4, dx = 0: angle 90 -> 0 deg -> row 0
    assert near == table[0, 4]
    # the last cell wraps to row 0
    wrap = rg.compute_shape_prior_table_cdf([9, 12], table, centre)             # between 270 and 360 deg
    angle_norm = ((810 - np.rad2deg(np.arctan2(2, -1))) % 360) / 90.
    assert 3 < angle_norm < 4
    dist = np.sqrt(5.)
    low = table[3, 2] + (table[3, 3] - table[3, 2]) * (dist - 2)
    high = table[0, 2] + (table[0, 3] - table[0, 2]) * (dist - 2)
    assert abs(wrap - (low + (high - low) * (angle_norm - 3))) < 1e-15
    # a table holding 0 gives -log(0.01); a prior of -0.01 an infinite cost, replaced
    costs = rg._shape_cost(np.array([0., -rg.MIN_SHAPE_PROB]))
    assert costs[0] == -np.log(0.01) and costs[1] == rg.GC_REPLACE_INF


@pytest.mark.parametrize('nb_labels', [2, 64, 65, 300])
@pytest.mark.parametrize('allow_obj_swap', [True, False])
@pytest.mark.parametrize('coef_pairwise', [0., 1.5])
def test_delta_scores_against_two_full_sums(rg, nb_labels, allow_obj_swap, coef_pairwise):
    slic = C.random_map(nb_labels, 40, 56, nb_labels)
    nb_objects = min(3, nb_labels)
    state = rg._HostState(slic, nb_objects)
    neighbours = C.neighbour_lists(state.edges, nb_labels)
    state.attach(*rg._csr_neighbours(neighbours, nb_labels))
    lut_data, lut_shape = C.random_costs(nb_labels, nb_labels, nb_objects)
    state.set_costs(lut_data, lut_shape)
    labels = C.grown_labels(nb_labels + 1, state.edges, nb_labels, nb_objects)
    trans = (0.1, 0.03)
    coefs = (1., 2., coef_pairwise)
    objects, superpixels, changes = state.greedy_step(labels, allow_obj_swap, *coefs, *rg._penalties(trans))
    want_obj, want_sp = C.brute_candidates(rg, labels, neighbours, nb_objects, allow_obj_swap)
    assert np.array_equal(objects, want_obj) and np.array_equal(superpixels, want_sp)
    weights = state.sums()[:, 0]
    crit, want = C.brute_changes(rg, objects, superpixels, labels, lut_data, lut_shape, weights, state.edges, coefs, trans)
    bound = (nb_labels + len(state.edges)) * 2.**-53 * crit
    assert len(changes) == 0 or float(np.max(np.abs(changes - want))) <= bound
    got = state.criterion(labels, *coefs, *rg._penalties(trans))
    assert abs(got - crit) <= bound
    assert state.criterion(labels, *coefs, *rg._penalties(trans)) == got


def _graphcut_variables_by_vertex(rg, candidates, neighbours, weights, labels, nb_objects, lut_data, lut_shape, coefs):
    """unary rows, vertexes and edges vertex by vertex, with list.index for the first position of a neighbour"""
    vertexes, edges, unary = list(candidates), [], []
    for idx in candidates:
        row = weights[idx] * (coefs[0] * lut_data[idx] + coefs[1] * lut_shape[idx])
        unary.append([row[lb] if lb in labels[neighbours[idx]] else rg.GC_REPLACE_INF for lb in range(nb_objects + 1)])
    for i, idx in enumerate(candidates):
        for near in neighbours[idx]:
            if near not in vertexes:
                vertexes.append(near)
                unary.append([0 if lb == labels[near] else rg.GC_REPLACE_INF for lb in range(nb_objects + 1)])
            edges.append((i, vertexes.index(near)))
    return vertexes, np.array(edges), np.maximum(np.array(unary, dtype=float), -np.log(rg.MAX_UNARY_PROB))


def test_prepare_graphcut_variables_keeps_the_vertex_order(rg):
    nb_labels, nb_objects = 120, 3
    slic = C.random_map(5, 48, 64, nb_labels)
    state = rg._HostState(slic, nb_objects)
    neighbours = C.neighbour_lists(state.edges, nb_labels)
    labels = C.grown_labels(9, state.edges, nb_labels, nb_objects)
    lut_data, lut_shape = C.random_costs(3, nb_labels, nb_objects)
    objects, candidates = C.brute_candidates(rg, labels, neighbours, nb_objects, True)
    assert len(set(candidates.tolist())) < len(candidates), 'the case needs a superpixel that is a candidate twice'
    weights = state.sums()[:, 0]
    got = rg.prepare_graphcut_variables(candidates.tolist(), state.points(), neighbours, weights, labels, nb_objects, lut_data,
                                        lut_shape, 1., 2., 1.5, (0.1, 0.03))
    vertexes, edges, unary = _graphcut_variables_by_vertex(rg, candidates.tolist(), neighbours, weights, labels, nb_objects, lut_data,
                                                          lut_shape, (1., 2.))
    assert got[0] == vertexes and np.array_equal(got[1], edges) and np.array_equal(got[3], unary)
    assert got[2].shape == (len(edges), ) and np.isclose(np.mean(1. / got[2]), 1.)
    pairwise = got[4]
    assert pairwise[0, 0] == 0 and pairwise[0, 1] == -np.log(0.1) * 1.5 and pairwise[1, 2] == -np.log(0.03) * 1.5


def test_ray_walk_of_a_square(rg):
    from pyimsegm_amd.descriptors import _ray_directions
    img = np.zeros((100, 100), dtype=bool)
    img[20:70, 30:80] = True
    rays = rg.ray_distances_down(img, (45, 55), _ray_directions(45.))
    # imsegm/region_growing.py:272-276 prints these after the phase shift (a rotation of the vector)
    tenths = [int(r * 10) for r in rays]
    assert any(np.roll(tenths, k).tolist() == [367, 260, 353, 250, 353, 250, 353, 260] for k in range(8))
    assert (rg.ray_distances_down(img, (-1, 5), _ray_directions(45.)) == -1).all()


@pytest.fixture(scope='module')
def fixture():
    return C.load_fixture()


def test_shape_prior_against_the_reference(rg, fixture):
    """the bilinear statement against the reference's ``interp2d`` values (tests/golden/region_growing.npz), within the
    tolerance the generator derived from long double"""
    got = np.concatenate([rg.shape_prior_points(points, table, centre, shift) for points, centre, shift, table in C.shape_prior_grid()])
    far = np.concatenate([np.hypot(*(points - np.array(centre)).T) >= table.shape[1] - 1
                          for points, centre, shift, table in C.shape_prior_grid()])
    assert far.sum() >= 60 and (~far).sum() >= 60, 'the grid needs both branches'
    gap = float(np.max(np.abs(got - fixture['shape_prior'])))
    print('shape prior: max |host - reference| %.3g, tol %.3g' % (gap, float(fixture['shape_prior_tol'])))
    assert gap <= float(fixture['shape_prior_tol']) < 1e-9
    assert np.array_equal(got[far], fixture['shape_prior'][far])                # a table entry, no arithmetic


@pytest.mark.parametrize('name', C.GROWTH_CASES)
@pytest.mark.parametrize('method', ['greedy', 'graphcut'])
def test_host_growth_against_the_reference(rg, fixture, monkeypatch, method, name):
    """the host statement against the whole ``debug_history`` of the reference's growth; the cut of the graph-cut cases by the CPU
    oracle here as in the fixture's generator"""
    from oracle import oracle as orc
    monkeypatch.setattr(rg, 'cut_general_graph', orc.cut_general_graph)
    C.check_growth_against_fixture(rg, fixture, method, name, 'host')


def test_longer_probability_vector_is_accepted(rg):
    """the reference reads ``slic_prob_fg`` only up to the last label (imsegm/region_growing.py:1294 rejects too short a vector)"""
    slic, prob, centres, model, shape_type = C.growth_case('one_cdf')
    want = rg.region_growing_shape_slic_greedy(slic, prob, centres, model, shape_type, nb_iter=4, on='host')
    got = rg.region_growing_shape_slic_greedy(slic, np.concatenate([prob, [0.5, 0.5]]), centres, model, shape_type, nb_iter=4, on='host')
    assert np.array_equal(got, want)


def test_host_state_without_labels(rg):
    state = rg._HostState(C.grid_slic(), 1)
    state.attach(*rg._csr_neighbours(C.neighbour_lists(state.edges, state.n_labels), state.n_labels))
    zeros = np.zeros((state.n_labels, 2))
    state.set_costs(zeros, zeros)
    assert state.criterion(None, 1., 1., 0., 1., 1.) == 0.
    assert len(state.greedy_step(None, True, 1., 1., 1., 1., 1.)[0]) == 0


def test_rejected_arguments(rg):
    slic, segm = C.grid_slic(), C.doctest_block()
    prob = C.prob_fg(slic, segm, [0.1, 0.9])
    model = (None, C.DOCTEST_CHIST)
    with pytest.raises(ValueError, match='dims of probs'):
        rg.region_growing_shape_slic_greedy(slic, prob[:10], [(7, 10)], model, on='host')
    with pytest.raises(ValueError, match='dims of probs'):
        rg.region_growing_shape_slic_graphcut(slic, prob[:10], [(7, 10)], model, on='host')
    with pytest.raises(NameError, match='Not supported type of shape model "nope"'):
        rg.region_growing_shape_slic_greedy(slic, prob, [(7, 10)], model, shape_type='nope', on='host')
    with pytest.raises(ValueError, match='outside the map'):
        rg.region_growing_shape_slic_greedy(slic, prob, [(7, 40)], model, on='host')
    with pytest.raises(ValueError, match="on is 'host' or 'device'"):
        rg.region_growing_shape_slic_greedy(slic, prob, [(7, 10)], model, on='nonsense')
    with pytest.raises(ValueError, match=r'number of points \(5\) and labels \(4\) should match'):
        rg.update_shape_costs_points(np.zeros((5, 2)), None, np.zeros((5, 2), dtype=int), np.ones(4), [(0, 0)], [(np.inf, np.inf)],
                                     [0], [0], model, 'cdf')
    with pytest.raises(NameError):
        rg.update_shape_costs_points(np.zeros((5, 2)), None, np.zeros((5, 2), dtype=int), np.ones(5), [(0, 0)], [(np.inf, np.inf)],
                                     [0], [0], model, 'other')
    with pytest.raises(ValueError, match='max candidate idx: 9 for 4 centres'):
        rg.prepare_graphcut_variables([9], np.zeros((4, 2)), [[1], [0]], np.ones(4), np.zeros(4, dtype=int), 1, None, None, 1, 1, 1,
                                      (.1, .1))


def test_environment_switch(rg, monkeypatch):
    monkeypatch.setenv('IMSEGM_RG_ON', 'host')
    assert rg._place(None) == 'host'
    assert rg._place('device') == 'device'
    monkeypatch.setenv('IMSEGM_RG_ON', 'elsewhere')
    with pytest.raises(ValueError):
        rg._place(None)
