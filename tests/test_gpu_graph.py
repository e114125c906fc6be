"""The region adjacency graph and the superpixel centres on the device (csrc/graph.hip ``k_adjacency_centres``, ``k_edge_*``,
``k_table_*``, ``k_gather_*``; csrc/volume_graph.hip ``k_vol_adjacency_runs<0|1>``; csrc/terms.hip ``k_adj_*`` / ``k_tab_*``)
against the numpy reference of tests/graph_cases.py on label maps that SLIC never produces: salt, runs of one and of exactly 64
pixels, borders on the wave, row-block and slice-group seams, label counts around a bitmap word, hubs of the neighbour table.
Edges with order and dtype, centres over all rows and the present flags: bit for bit, no tolerance (both sides divide the same
exact integer sums).  tests/test_graph_reference_host.py shows the reference equal to the C oracle on the same cases."""
import functools

import numpy as np
import pytest

import graph_cases as G

pytestmark = pytest.mark.gpu

MAKERS = dict(G.CASES_2D + G.CASES_3D)
_GRAPH_KEYS = ('edges', 'centres', 'edge_weights', 'edge_weights_int', 'unary_int', 'graph_labels', 'segm', 'energy')


@pytest.fixture(scope='module')
def hip():
    from pyimsegm_amd import _hip
    _hip.default_context()
    return _hip


@functools.lru_cache(maxsize=None)
def case(name):
    """(map, n_labels as installed or None, n_labels, (edges, centres, present)); computed once, read-only"""
    labels = MAKERS[name]()
    given = G.N_LABELS.get(name)
    n_labels = given if given is not None else int(labels.max()) + 1
    reference = G.graph_reference(labels, n_labels)
    for array in (labels, ) + reference:
        array.setflags(write=False)
    return labels, given, n_labels, reference


def open_session(hip, name):
    labels, given, n_labels, _ = case(name)
    kind = hip.Image2D if labels.ndim == 2 else hip.Volume3D
    sess = kind(*labels.shape)
    try:
        sess.set_labels(labels) if given is None else sess.set_labels(labels, given)
    except Exception:
        sess.close()
        raise
    assert sess.n_labels == n_labels
    return sess


def assert_graph(result, reference, what=''):
    edges, centres, present = result
    want_edges, want_centres, want_present = reference
    assert edges.dtype == np.int32 and edges.shape == want_edges.shape, (what, edges.shape, want_edges.shape)
    assert np.array_equal(edges, want_edges), what
    assert centres.dtype == np.float64 and centres.shape == want_centres.shape, what
    assert np.array_equal(centres, want_centres), what                        # every row, the -1 rows of absent labels included
    if present is not None:
        assert present.dtype == np.bool_ and np.array_equal(present, want_present), what


# ---- staged graph call ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', G.IDS_2D)
def test_image_graph(hip, name):
    sess = open_session(hip, name)
    try:
        assert_graph(sess.graph(), case(name)[3])
    finally:
        sess.close()


@pytest.mark.parametrize('store', ['bitmap', 'table'])
@pytest.mark.parametrize('name', G.IDS_3D)
def test_volume_graph(hip, monkeypatch, name, store):
    if store == 'table':
        monkeypatch.setenv('IMSEGM_ADJACENCY_TABLE', '1')
    sess = open_session(hip, name)
    try:
        assert_graph(sess.graph(), case(name)[3])
    finally:
        sess.close()


# ---- fused call, graph only -----------------------------------------------------------------------------------------------------
def _fused_graph(hip, name, fits=True):
    """the fused call alone and after graph_prepare(): 'edges' and 'centres' of both equal the reference, and each other in every
    other key; ``fits`` False: HipFusedPathError from both (a label with more neighbours than a row of the table)"""
    from pyimsegm_amd.graph_cuts import compute_pairwise_cost
    labels, _, n_labels, reference = case(name)
    proba = np.random.default_rng([G.SEED, n_labels]).dirichlet(np.ones(2), size=n_labels)
    pairwise = compute_pairwise_cost(1., proba.shape)
    sess = open_session(hip, name)
    try:
        if not fits:
            with pytest.raises(hip.HipFusedPathError, match='64 neighbours'):
                sess.segment(pairwise, 'model', proba=proba, debug=True, pinned=False)
            sess.graph_prepare()                               # (enqueues only: the call that reads the graph's head reports it)
            with pytest.raises(hip.HipFusedPathError, match='64 neighbours'):
                sess.segment(pairwise, 'model', proba=proba, debug=True, pinned=False)
            return
        alone = sess.segment(pairwise, 'model', proba=proba, debug=True, pinned=False)
        assert_graph((alone['edges'], alone['centres'], None), reference, 'alone')
        assert len(alone['edge_weights']) == len(alone['edges']) == len(alone['edge_weights_int'])
        sess.graph_prepare()
        ahead = sess.segment(pairwise, 'model', proba=proba, debug=True, pinned=False)
        assert_graph((ahead['edges'], ahead['centres'], None), reference, 'prepared')
        for key in _GRAPH_KEYS:                                # (bytes: a map whose neighbours share one centre has NaN weights)
            assert np.asarray(alone[key]).tobytes() == np.asarray(ahead[key]).tobytes(), key
        assert alone['segm'].shape == labels.shape and np.array_equal(alone['segm'], alone['graph_labels'][labels])
    finally:
        sess.close()


@pytest.mark.parametrize('name', G.IDS_2D)
def test_fused_image_graph(hip, name):
    _fused_graph(hip, name)


@pytest.mark.parametrize('name', G.IDS_3D)
def test_fused_volume_graph_from_the_bitmap(hip, name):
    _fused_graph(hip, name)


@pytest.mark.parametrize('name', G.IDS_3D)
def test_fused_volume_graph_from_the_table(hip, monkeypatch, name):
    """64 slots per label: the reference's own degrees say which cases fit (tests/test_gpu_fused.py
    test_fused_volume_call_when_a_label_has_more_neighbours_than_a_table_row fixes the error for the others)"""
    monkeypatch.setenv('IMSEGM_ADJACENCY_TABLE', '1')
    _, _, n_labels, reference = case(name)
    _fused_graph(hip, name, fits=G.max_degree(reference[0], n_labels) <= 64)


# ---- reuse of a session ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('store', ['image', 'bitmap', 'table'])
def test_stores_are_cleared_between_calls(hip, monkeypatch, store):
    """salt, then a single label, then salt of fewer labels on ONE session: each graph is its own map's (bitmap, table and sums
    start from nothing every time), staged and fused"""
    from pyimsegm_amd.graph_cuts import compute_pairwise_cost
    if store == 'table':
        monkeypatch.setenv('IMSEGM_ADJACENCY_TABLE', '1')
    shape = (33, 130) if store == 'image' else (9, 20, 70)
    sess = (hip.Image2D if store == 'image' else hip.Volume3D)(*shape)
    try:
        for labels in (G.salt(shape, 200), np.zeros(shape, dtype=np.int32), G.salt(shape, 40, seed=1), G.salt(shape, 40, seed=2) * 3):
            reference = G.graph_reference(labels)
            sess.set_labels(labels)
            assert_graph(sess.graph(), reference, 'staged')
            if store == 'table' and G.max_degree(reference[0], len(reference[1])) > 64:
                continue
            proba = np.random.default_rng(7).dirichlet(np.ones(2), size=sess.n_labels)
            fused = sess.segment(compute_pairwise_cost(1., proba.shape), 'model', proba=proba, debug=True, pinned=False)
            assert_graph((fused['edges'], fused['centres'], None), reference, 'fused')
            assert_graph(sess.graph(), reference, 'staged again')
    finally:
        sess.close()


# ---- gathers --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n_pixels', [1, 2, 3, 4, 5, 7, 8, 4099])
def test_gathers(hip, n_pixels):
    """``lut[labels]`` and ``proba[labels]``: the four-per-lane body and the tail of k_gather_i32, C = 1, 2, 3, 7, LUTs longer
    than the label count, the caller's own output array"""
    rng = np.random.default_rng([G.SEED, n_pixels])
    n_labels = min(n_pixels, 11)
    for shape in ((1, n_pixels), (n_pixels, 1)):
        labels = rng.integers(0, n_labels, shape).astype(np.int32)
        labels.flat[-1] = n_labels - 1
        sess = hip.Image2D(*shape).set_labels(labels)
        try:
            for extra in (0, 5):
                lut = rng.integers(-2**31, 2**31, n_labels + extra).astype(np.int32)
                segm, soft = sess.gather(graph_labels=lut)
                assert soft is None and segm.dtype == np.int32 and np.array_equal(segm, lut[labels])
                own = np.full(shape, -7, dtype=np.int32)
                segm, _ = sess.gather(graph_labels=lut, segm_out=own)
                assert segm is own and np.array_equal(own, lut[labels])
                for n_classes in (1, 2, 3, 7):
                    proba = rng.random((n_labels + extra, n_classes))
                    segm, soft = sess.gather(graph_labels=lut, proba=proba)
                    assert np.array_equal(segm, lut[labels])
                    assert soft.dtype == np.float64 and soft.shape == shape + (n_classes, ) and np.array_equal(soft, proba[labels])
                    segm, soft = sess.gather(proba=proba)
                    assert segm is None and np.array_equal(soft, proba[labels])
        finally:
            sess.close()
