"""The device path of the ellipse placement (csrc/ellipse_place.hip behind ``imsegm_ellipse_place`` and ``imsegm_ellipse_overlaps``)
against the host statement of pyimsegm_amd/ellipse_fitting.py, which tests/test_ellipse_place_reference_host.py ties to the
reference's recorded results.  Integer counting, one fp64 expression per pixel evaluated operation by operation and one IEEE
division per label: maps, flags and tables are compared byte for byte, and every call runs twice."""
import numpy as np
import pytest

import ellipse_place_cases as C

pytestmark = pytest.mark.gpu
CASES = C.cases()
BEYOND = C.beyond_cases()


@pytest.fixture(scope='module')
def hip():
    from pyimsegm_amd import _hip
    _hip.default_context()
    return _hip


@pytest.fixture(scope='module')
def ell(hip):
    from pyimsegm_amd import ellipse_fitting
    return ellipse_fitting


@pytest.fixture(scope='module')
def host_results(ell):
    """map and flags of the host fold, and the overlap tables, for every case, computed once"""
    results = {}
    for name, case in list(CASES.items()) + list(BEYOND.items()):
        segm = case['segm'].copy()
        placed = ell.place_host(segm, case['params'], case['labels'], case['thr'])
        results[name] = segm, placed, ell.overlaps_host(case['segm'], case['params'], int(case['segm'].max()) + 1)
    return results


def same_bytes(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def geometry(ell, case):
    return ell.ellipse_geometry([ell._int_params(p) for p in case['params']], case['segm'].shape)


@pytest.mark.parametrize('name', sorted(CASES))
def test_place_entry_point_equals_the_host_statement(hip, ell, host_results, name):
    case = CASES[name]
    want_segm, want_placed, _ = host_results[name]
    geom, sincos = geometry(ell, case)
    runs = []
    for _ in range(2):
        segm = case['segm'].astype(np.int32)
        placed = hip.ellipse_place(segm, geom, sincos, case['labels'], case['thr'])
        runs.append((segm, placed))
    assert same_bytes(runs[0][0], want_segm.astype(np.int32)), name
    assert same_bytes(runs[0][1], want_placed.astype(np.uint8)), name
    assert same_bytes(runs[0][0], runs[1][0]) and same_bytes(runs[0][1], runs[1][1])


@pytest.mark.parametrize('name', sorted(CASES))
def test_overlaps_entry_point_equals_the_host_statement(hip, ell, host_results, name):
    case = CASES[name]
    _, _, (want_counts, want_areas) = host_results[name]
    geom, sincos = geometry(ell, case)
    segm = case['segm'].astype(np.int32)
    counts, areas = hip.ellipse_overlaps(segm, geom, sincos, want_counts.shape[1])
    assert same_bytes(counts, want_counts) and same_bytes(areas, want_areas), name
    again = hip.ellipse_overlaps(segm, geom, sincos, want_counts.shape[1])
    assert same_bytes(again[0], counts) and same_bytes(again[1], areas)
    one, _ = hip.ellipse_overlaps(segm, geom, sincos, 1)
    assert same_bytes(one, np.ascontiguousarray(want_counts[:, :1]))


@pytest.mark.parametrize('name', sorted(CASES))
def test_public_functions_equal_the_host_statement(ell, host_results, name):
    case = CASES[name]
    want_segm, want_placed, (want_counts, want_areas) = host_results[name]
    for dtype in (np.int64, np.int32, np.float64):
        for _ in range(2):
            segm = case['segm'].astype(dtype)
            out, placed = ell.add_overlap_ellipses(segm, case['params'], case['labels'], case['thr'], on='device')
            assert out is segm and out.dtype == dtype and same_bytes(out, want_segm.astype(dtype)), (name, dtype)
            assert same_bytes(placed, want_placed)
    single = case['segm'].copy()
    for params, label in zip(case['params'], case['labels']):
        assert ell.add_overlap_ellipse(single, params, label, case['thr'], on='device') is single
    assert same_bytes(single, want_segm), name
    default = case['segm'].copy()
    for params, label in zip(case['params'], case['labels']):
        ell.add_overlap_ellipse(default, params, label, case['thr'])
    assert same_bytes(default, want_segm), name
    counts, areas = ell.ellipse_label_overlaps(case['segm'], case['params'], on='device')
    assert same_bytes(counts, want_counts) and same_bytes(areas, want_areas), name


def test_dependent_fold_over_the_map_another_fold_left(hip, ell):
    """the fold with rejections over a map from which labels have vanished"""
    case = CASES['chain_dependent']
    start = C.stacked(ell, CASES['chain_vanishing'], case)
    want = start.copy()
    want_placed = ell.place_host(want, case['params'], case['labels'], case['thr'])
    assert 0 < want_placed.sum() < len(want_placed)
    segm = start.copy()
    _, placed = ell.add_overlap_ellipses(segm, case['params'], case['labels'], case['thr'], on='device')
    assert same_bytes(segm, want) and same_bytes(placed, want_placed)


def test_no_ellipse_and_skipped_ellipses(hip, ell):
    segm = C._blocks(30, 40, 4).astype(np.int32)
    before = segm.copy()
    placed = hip.ellipse_place(segm, np.zeros((0, 8), dtype=np.int32), np.zeros((0, 2)), [], 1.)
    assert placed.shape == (0, ) and same_bytes(segm, before)
    counts, areas = hip.ellipse_overlaps(segm, np.zeros((0, 8), dtype=np.int32), np.zeros((0, 2)), 10)
    assert counts.shape == (0, 10) and areas.shape == (0, )
    out, placed = ell.add_overlap_ellipses(segm, [], on='device')
    assert out is segm and placed.shape == (0, ) and same_bytes(segm, before)
    out, placed = ell.add_overlap_ellipses(segm, [None, (15, 20, 4, 6, 0.3), ()], [7, 8, 9], 1., on='device')
    want = before.copy()
    assert placed.tolist() == ell.place_host(want, [None, (15, 20, 4, 6, 0.3), ()], [7, 8, 9], 1.).tolist() == [False, True, False]
    assert same_bytes(segm, want)


@pytest.mark.parametrize('name', sorted(BEYOND))
def test_one_past_the_label_table_goes_to_the_host(hip, ell, host_results, name):
    case = BEYOND[name]
    want_segm, want_placed, _ = host_results[name]
    segm = case['segm'].copy()
    _, placed = ell.add_overlap_ellipses(segm, case['params'], case['labels'], case['thr'])
    assert same_bytes(segm, want_segm) and same_bytes(placed, want_placed)
    # the entry point refuses and leaves the map as it came
    geom, sincos = geometry(ell, case)
    segm = case['segm'].astype(np.int32)
    with pytest.raises(hip.HipError):
        hip.ellipse_place(segm, geom, sincos, case['labels'], case['thr'])
    assert same_bytes(segm, case['segm'].astype(np.int32))


def test_calls_the_device_does_not_take_agree_with_the_host(ell):
    case = CASES['odd_labels']
    for change in ({'thr': -0.5}, {'params': [(40, 50, 0, 6, 0.1)] + case['params'][:3]}, {'segm': case['segm'] + 0.5},
                   {'labels': [1.5] + case['labels'][1:]}, {'segm': case['segm'] > 0, 'labels': [5] + [1] * 12}):
        changed = dict(case, **change)
        changed['labels'] = changed['labels'][:len(changed['params'])]
        want = changed['segm'].copy()
        with np.errstate(all='ignore'):
            want_placed = ell.place_host(want, changed['params'], changed['labels'], changed['thr'])
            segm = changed['segm'].copy()
            _, placed = ell.add_overlap_ellipses(segm, changed['params'], changed['labels'], changed['thr'])
        assert same_bytes(segm, want) and same_bytes(placed, want_placed), sorted(change)


def test_boundary_points_close_reproduces_the_docstring(ell):
    fixture = C.doctest_fixture()['prepare_boundary_points_close']
    seg = ell.add_overlap_ellipse(np.zeros(fixture['shape'], dtype=int), C.deg(fixture['params_deg']), 1)
    points = ell.prepare_boundary_points_close(seg, [tuple(c) for c in fixture['centers']])
    assert len(points) == 1 and points[0].ndim == 2 and points[0].shape[1] == 2
    assert [points[0][0].tolist(), points[0][1].tolist(), points[0][-1].tolist()] == [fixture['first'], fixture['second'], fixture['last']]
    slic = ell.get_slic_points_labels(seg, slic_size=25, slic_regul=0.3)[0]
    assert same_bytes(ell.filter_boundary_points(seg, slic), points[0])
