"""CPU checks of tests/graph_cases.py, which tests/test_gpu_graph.py holds the adjacency kernels to: on every case its numpy
reference equals the C oracle (``oracle.adjacency`` / ``oracle.centers``: vertices, edges in order, centres bit for bit), and the
cases have the properties they were built for -- more than 64 labels in a tile, more edges than the first capacity of ``graph()``,
hubs with exactly N neighbours, label changes on the named seams.  A case that drifts fails here, not silently on the device."""
import numpy as np
import pytest

import graph_cases as G

ALL_CASES = G.CASES_2D + G.CASES_3D
ALL_IDS = G.IDS_2D + G.IDS_3D


@pytest.fixture(scope='module')
def built():
    """id -> (map, n_labels, reference)"""
    out = {}
    for name, make in ALL_CASES:
        labels = make()
        n_labels = G.N_LABELS.get(name, int(labels.max()) + 1)
        out[name] = (labels, n_labels, G.graph_reference(labels, n_labels))
    return out


def test_ids_are_unique_and_maps_are_small_int32():
    assert len(set(ALL_IDS)) == len(ALL_IDS)
    for (name, make), ndim in [(case, 2) for case in G.CASES_2D] + [(case, 3) for case in G.CASES_3D]:
        labels = make()
        assert labels.dtype == np.int32 and labels.ndim == ndim and labels.flags.c_contiguous, name
        assert 0 < labels.size <= 2**17 and labels.min() >= 0, name
        assert np.array_equal(labels, make()), name                          # seeded: the same map every time


@pytest.mark.parametrize('name', ALL_IDS)
def test_reference_equals_the_oracle(oracle, built, name):
    labels, n_labels, (edges, centres, present) = built[name]
    top = int(labels.max()) + 1
    ref_vertices, ref_edges = oracle.adjacency(labels)
    assert np.array_equal(np.flatnonzero(present), ref_vertices)
    assert edges.dtype == np.int64 and np.array_equal(edges, np.array(ref_edges, dtype=np.int64).reshape(-1, 2))
    assert centres.dtype == np.float64 and centres.shape == (n_labels, labels.ndim)
    assert np.array_equal(centres[:top], oracle.centers(labels))
    assert np.all(centres[top:] == -1) and not present[top:].any()
    assert np.array_equal(np.all(centres == -1, axis=1), ~present)


def test_salt_cases_fill_the_hash_table_or_not(built):
    assert sorted(G.SALT_TILES.values()).count('within') == 3
    for name, kind in G.SALT_TILES.items():
        labels = built[name][0]
        distinct = G.distinct_per_tile(labels, G.TILE_2D if labels.ndim == 2 else G.TILE_3D)
        if kind == 'over':
            assert max(distinct) > 64, name                  # the sums of some labels go to the global atomics
        else:
            assert max(distinct) <= 64 and int(labels.max()) + 1 == 64, name


def test_retry_cases_exceed_the_first_capacity(built):
    assert len(G.RETRY) == 2 and {built[name][0].ndim for name in G.RETRY} == {2, 3}
    for name in G.RETRY:
        labels, n_labels, (edges, _, _) = built[name]
        assert len(edges) > G.first_capacity(n_labels, labels.ndim), name


def test_hubs_have_exactly_their_neighbours(built):
    assert sorted(count for _, count in G.HUBS.values()) == [31, 32, 33, 64, 65, 150, 300]
    for name, (label, count) in G.HUBS.items():
        edges = built[name][2][0]
        smaller, larger = int(np.sum(edges[:, 1] == label)), int(np.sum(edges[:, 0] == label))
        assert smaller + larger == count and smaller > 0 and larger > 0, name


def test_seam_cases_have_a_border_on_the_seam(built):
    for name, seams in G.SEAMS.items():
        labels = built[name][0]
        for axis, coordinate in seams:
            assert G.has_border(labels, axis, coordinate), (name, axis, coordinate)
    for axis, coordinate in ((1, 63), (1, 64), (1, 65)):                                  # every wave seam, 2-D and 3-D
        assert any((axis, coordinate) in G.SEAMS[name] for name in G.IDS_2D if name in G.SEAMS)
        assert any((axis + 1, coordinate) in G.SEAMS[name] for name in G.IDS_3D if name in G.SEAMS)
    for coordinate in (3, 4, 5, 15, 16, 17):
        assert (0, coordinate) in G.SEAMS['hband_y%d' % coordinate]
    for coordinate in (7, 8, 15, 16):
        assert (0, coordinate) in G.SEAMS['slabs_K2_D17']


def test_row_cases_hold_the_run_lengths(built):
    """one label per row: a run of exactly 64, runs cut at the wave's edge, rows of fewer than 64 active lanes"""
    for width in (1, 63, 64, 65, 127, 128, 129):
        labels = built['rows_W%d' % width][0]
        assert labels.shape == (5, width) and np.all(labels == np.arange(5)[:, np.newaxis])
    for name in ('vstripes_K2', 'vstripes_K65', 'checker_1'):
        labels = built[name][0]
        assert np.all(labels[:, 1:] != labels[:, :-1]), name                               # runs of one pixel


def test_word_cases_join_the_last_label_with_the_first(built):
    for prefix in ('words', 'words3'):
        for count in G.WORD_COUNTS:
            labels, n_labels, (edges, _, present) = built['%s_K%d' % (prefix, count)]
            assert n_labels == count and present.all()
            if count > 1:
                assert [0, count - 1] in edges.tolist()
            holes = built['%s_K%d_holes' % (prefix, count)]
            assert holes[1] == 3 * (count - 1) + 1 and int(holes[2][2].sum()) == count
            assert np.array_equal(holes[2][0], 3 * edges)
            trailing = built['%s_K%d_trailing' % (prefix, count)]
            assert trailing[1] == count + 40 and int(trailing[2][2].sum()) == count and np.array_equal(trailing[2][0], edges)


def test_table_rows_of_the_fused_call_fit_some_cases_and_not_others(built):
    """the fused call keeps 64 neighbour slots per label on the table path: both outcomes occur among the 3-D cases"""
    degrees = {name: G.max_degree(built[name][2][0], built[name][1]) for name in G.IDS_3D}
    assert degrees['hub_N64'] == 64 and degrees['hub_N65'] == 65
