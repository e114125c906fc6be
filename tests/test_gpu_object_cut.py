"""The object cuts on the device: ``imsegm_object_cut_pixels`` against the host statement and the CPU oracle, ``cut_grid_graph``
through ``imsegm_cut_grid_graph`` against the route it replaces (edges in numpy, then ``cut_general_graph``), and the superpixel
variant with its dropped self-edges."""
import numpy as np
import pytest

from tests import object_cut_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def rg():
    from pyimsegm_amd import region_growing
    return region_growing


@pytest.fixture(scope='module')
def hip():
    from pyimsegm_amd import _hip
    assert callable(_hip.object_cut_pixels) and callable(_hip.cut_general_graph_scaled)
    return _hip


@pytest.fixture(scope='module')
def fixture():
    return C.load_fixture()


def _device_against_host(rg, hip, oracle, segm, centres, labels_fg_prob=(0.1, 0.9), gc_regul=1, seed_size=0, coef_shape=0.,
                         shape_mean_std=(50., 10.)):
    centres = [np.round(c).astype(int) for c in centres]
    tables = rg._object_tables(labels_fg_prob, coef_shape, shape_mean_std, rg._max_centre_distance(segm.shape, centres))
    seeds = rg._object_pixels_refusals(segm, centres, tables, coef_shape, seed_size)
    unary = rg._object_pixels_unary(segm, centres, tables, coef_shape, seed_size)
    flat = unary.reshape(-1, unary.shape[-1])
    edges = C.grid_edges(*segm.shape)
    pairwise = (1 - np.eye(len(centres) + 1)) * gc_regul
    ui, wi, si, dwf = rg.pygco_integers(flat, np.ones(len(edges)), pairwise)
    rows = np.array([[c[0], c[1], s[0], s[1]] for c, s in zip(centres, seeds)], dtype=np.int32)
    labels, energy, unary_int, factor = hip.object_cut_pixels(segm, rows, *tables, coef_shape=coef_shape, gc_regul=gc_regul,
                                                              seed_size=seed_size, debug=True)
    assert factor == dwf and np.array_equal(unary_int.reshape(flat.shape), ui)
    host_labels, host_energy = hip.cut_general_graph(edges, np.ones(len(edges)), flat, pairwise, n_iter=999, return_energy=True)
    assert energy == host_energy and np.array_equal(labels.ravel(), host_labels)
    want, want_energy = oracle.cut_general_graph(edges, np.ones(len(edges)), flat, pairwise, n_iter=999, return_energy=True)
    assert energy == want_energy and np.array_equal(labels.ravel(), want)
    public = rg.object_segmentation_graphcut_pixels(segm, centres, labels_fg_prob, gc_regul, seed_size, coef_shape, shape_mean_std)
    assert public.dtype == np.int32 and np.array_equal(public, labels)
    return labels


def test_doctest_image(rg, hip, oracle):
    for kwargs, answer in C.DOCTEST_PIXELS:
        labels = _device_against_host(rg, hip, oracle, C.DOCTEST_SEGM, C.DOCTEST_CENTRES, **kwargs)
        assert labels.tolist() == answer
        debug = {}
        assert rg.object_segmentation_graphcut_pixels(C.DOCTEST_SEGM, C.DOCTEST_CENTRES, debug_visual=debug, **kwargs).tolist() == answer
        assert len(debug['unary_imgs']) == 3
        assert rg.object_segmentation_graphcut_pixels(C.DOCTEST_SEGM, C.DOCTEST_CENTRES, on='host', **kwargs).tolist() == answer


@pytest.mark.parametrize('name', list(C.PIXEL_CASES))
def test_device_against_host_statement(rg, hip, oracle, fixture, name):
    key = 'pixels_%s_' % name
    segm, centres, kwargs = C.pixel_case(name, int(fixture[key + 'seed']))
    labels = _device_against_host(rg, hip, oracle, segm, centres, **kwargs)
    assert np.array_equal(labels, fixture[key + 'labels'])


def test_more_than_63_centres(rg, hip):
    segm, centres, kwargs = C.pixel_case('many', 1)
    with pytest.raises(hip.HipError, match='more than 64 labels'):
        rg.object_segmentation_graphcut_pixels(segm, centres + [(10, 10)], **kwargs)


@pytest.mark.parametrize('height, width', [(7, 9), (1, 17), (17, 1), (90, 93)])
def test_grid_entry_against_the_general_route(hip, height, width):
    rng = np.random.RandomState(height * 100 + width)
    n_labels = 4
    unary = rng.rand(height, width, n_labels) * 3
    cost_v, cost_h = rng.rand(height - 1, width) * 2 + 0.1, rng.rand(height, width - 1) * 2 + 0.1
    pairwise = (1 - np.eye(n_labels)) * 0.7
    edges = C.grid_edges(height, width)
    weights = np.concatenate([cost_v.ravel(), cost_h.ravel()])
    want, want_energy = hip.cut_general_graph(edges, weights, unary.reshape(-1, n_labels), pairwise, n_iter=999, return_energy=True)
    got, energy = hip.cut_grid_graph(unary, pairwise, cost_v, cost_h, n_iter=999, return_energy=True)
    assert got.dtype == np.int32 and energy == want_energy and np.array_equal(got, want)
    assert len(np.unique(got)) > 1


@pytest.mark.parametrize('height, width', [(1, 1), (1, 6), (5, 1), (2, 2), (4, 7), (33, 47)])
def test_grid_arcs_against_the_host_loop(hip, height, width):
    """what ``k_grid_arcs`` writes against the loop of ``imsegm_cut_general_graph`` on pyGCO's edge list"""
    edges, arc_start, arc_to, arc_rev, edge_arc = hip.grid_arcs(height, width)
    assert np.array_equal(edges, C.grid_edges(height, width))
    for got, want in zip((arc_start, arc_to, arc_rev, edge_arc), C.arcs_by_loop(edges, height * width)):
        assert np.array_equal(got, want)


def test_grid_entry_refuses_large_smoothness(hip):
    """|int weight| * max |int pairwise| above GCO_MAX_ENERGYTERM (a negative pairwise cost does not enter pyGCO's scaling)"""
    unary = np.zeros((3, 3, 2))
    unary[0, 0, 0] = 1.
    pairwise = (np.eye(2) - 1) * 1000.
    with pytest.raises(hip.HipError, match='GCO_MAX_ENERGYTERM'):
        hip.cut_general_graph(C.grid_edges(3, 3), np.ones(12), unary.reshape(9, 2), pairwise)
    with pytest.raises(hip.HipError, match='GCO_MAX_ENERGYTERM'):
        hip.cut_grid_graph(unary, pairwise, np.ones((2, 3)), np.ones((3, 2)))


def test_superpixel_doctests(rg):
    for kwargs, answer in C.DOCTEST_SLIC_RUNS:
        debug = {}
        labels = rg.object_segmentation_graphcut_slic(C.DOCTEST_SLIC, C.DOCTEST_SLIC_SEGM, C.DOCTEST_SLIC_CENTRES, debug_visual=debug, **kwargs)
        assert labels.dtype == np.int32 and labels.tolist() == answer and len(debug['unary_imgs']) == 2


@pytest.mark.parametrize('name', list(C.SLIC_CASES))
def test_superpixel_case_against_the_reference(rg, fixture, name):
    key = 'slic_%s_' % name
    slic, segm, centres = C.slic_case(int(fixture[key + 'seed']))
    labels = rg.object_segmentation_graphcut_slic(slic, segm, centres, labels_fg_prob=C.LABELS_FG_PROB, **C.SLIC_CASES[name])
    assert labels.dtype == np.int32 and np.array_equal(labels, fixture[key + 'labels'])


def test_scaled_cut_is_the_general_cut_without_a_maximum(hip, fixture):
    key = 'slic_const_'
    args = fixture[key + 'edges'], fixture[key + 'weights'], fixture[key + 'unary'], fixture[key + 'pairwise']
    want = hip.cut_general_graph(*args, n_iter=999, return_energy=True)
    for weight_max in (-1., 0.5):
        got = hip.cut_general_graph_scaled(*args, weight_max, n_iter=999, return_energy=True)
        assert got[1] == want[1] and np.array_equal(got[0], want[0])


def test_scaled_cut_without_any_edge_left(hip, oracle):
    """every edge dropped: the weight maximum still scales the unary integers, and the labels are their argmin"""
    rng = np.random.RandomState(3)
    unary, pairwise = rng.rand(50, 3), (1 - np.eye(3)) * 2.
    none = np.zeros((0, 2), dtype=np.int32)
    labels, energy = hip.cut_general_graph_scaled(none, np.zeros(0), unary, pairwise, 4., n_iter=999, return_energy=True)
    want = ((unary / (8. + 1e-10)) * 100000).astype(np.int32)
    assert np.array_equal(labels, np.argmin(want, axis=1)) and energy == int(want.min(axis=1).sum())
