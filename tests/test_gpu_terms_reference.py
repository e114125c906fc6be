"""terms.hip -- k_gmm_proba (all four instantiations), k_gc_terms and the whole-device k_terms_* -- against the 80-bit reference of
tests/terms_cases.py at F = 3 .. 256 features, C = 1 .. 16 classes, on feature tables the test chooses (Image2D.put_features) and
on graphs it knows (label k is a 2 x 2 block of pixels: a 4-connected grid).  tests/test_terms_reference_host.py shows on the CPU
that these cases see a dropped feature or class; the tolerances are 16 x scikit-learn's / the host mirror's own fp64 deviation
from the reference (terms_cases.PROBA_DEVIATION / TERMS_DEVIATION), floors 1e-12 / 1e-13.  The device's own figures are printed
(pytest -s) and tabulated in DESIGN.md section 5.

Not compared: the six scalars of the terms (mean length, mean distance, deviation, maxima, down-weight factor) -- the debug
block of imsegm_image2d_segment does not carry them; the weights are a function of the first three, the integers of the others."""
import numpy as np
import pytest

import terms_cases as T

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not T.LONGDOUBLE_OK, reason=T.LONGDOUBLE_REASON)]

#: what the device writes for the integer of a NaN edge weight (every distance of the graph equal to zero: std = 0, 0 / 0): the
#: float-to-int conversion of gfx950 returns 0 for NaN where numpy's astype gives INT_MIN
NAN_WEIGHT_INT = 0


def pygco_integers(unary, weights, pairwise):
    """float -> int conversion of gco-wrapper's pygco.cut_general_graph in fp64 numpy"""
    with np.errstate(all='ignore'):
        mu, mw, mp = np.abs(unary).max(), np.abs(weights).max() if len(weights) else 0., pairwise.max()
        dwf = (mw * mp if (len(weights) and mw * mp > mu) else mu) + 1e-10
        return ((unary / dwf) * 100000).astype(np.int32), ((weights / dwf) * 1000).astype(np.int32)


def open_session(h, w, table=None, block=2):
    from pyimsegm_amd import _hip
    labels = T.block_labels(h, w, block)
    image = np.random.RandomState(h * 1000 + w).randint(0, 256, labels.shape + (3, )).astype(np.uint8)
    sess = _hip.Image2D(*labels.shape).upload(image).set_labels(labels, h * w)
    if table is not None:
        sess.put_features(np.ascontiguousarray(table, dtype=np.float64))
    return sess


def check_graph(out, h, w, block=2):
    edges, centres = T.grid_graph(h, w, block)
    assert np.array_equal(out['edges'], edges) and np.array_equal(out['centres'], centres)
    return edges, centres


def check_terms(out, table, edge_type, cost, pairwise, tol):
    """unary cost, edge weights and both integer forms of one fused call against reference_terms ON THE DEVICE'S OWN
    probabilities (the error of that step is not counted twice); returns the worst relative deviation"""
    proba, edges, centres = out['proba'], out['edges'], out['centres']
    want = T.reference_terms(proba, edges, centres, table, edge_type, cost, pairwise)
    worst = float(np.max(np.abs(out['unary'] - want['unary']) / np.abs(want['unary'])))
    nan = np.isnan(want['weights'])
    assert np.array_equal(np.isnan(out['edge_weights']), nan), edge_type
    if len(edges) and not nan.any():
        worst = max(worst, float(np.max(np.abs(out['edge_weights'] - want['weights']) / np.abs(want['weights']))))
    assert worst <= tol, (edge_type, cost, worst)
    # the longdouble integers, but for the elements the tolerance leaves open (decided by the reference alone; at most 1 %)
    for got, key in ((out['unary_int'], 'unary_scaled'), (out['edge_weights_int'], 'weights_scaled')):
        if got.size == 0:
            continue
        skip = T.ambiguous(want[key], tol)
        assert skip.mean() <= 0.01, (edge_type, key)
        skip |= np.isnan(want[key])
        assert np.array_equal(got[~skip], T.truncated(want[key])[~skip]), (edge_type, cost, key)
    # the integers pygco forms from the device's floats: everywhere (a NaN weight: the conversion of the hardware)
    ui, wi = pygco_integers(out['unary'], out['edge_weights'], pairwise)
    assert np.array_equal(out['unary_int'], ui), (edge_type, cost)
    assert np.array_equal(out['edge_weights_int'][~nan], wi[~nan]), (edge_type, cost)
    assert np.all(out['edge_weights_int'][nan] == NAN_WEIGHT_INT), out['edge_weights_int'][nan][:4]
    return worst


@pytest.mark.parametrize('case', T.CASES, ids=T.case_id)
def test_probabilities_against_the_80_bit_reference(case):
    from pyimsegm_amd import _hip
    F, C, K, _ = case
    model, table, ref = T.case_data(case)
    h, w = T.grid_shape(K)
    sess = open_session(h, w, table)
    try:
        assert np.array_equal(sess.get_features(F), table)
        out = sess.segment(T.pairwise_cost(C), 'model', gmm=_hip.DeviceGmm(model), debug=True, want_proba=True, want_graph_labels=True)
    finally:
        sess.close()
    check_graph(out, h, w)
    worst = float(np.abs(out['proba'] - ref).max())
    print('%s: device against longdouble %.3e (tolerance %.3e, scikit-learn %.3e)'
          % (T.case_id(case), worst, T.proba_tolerance(case), T.PROBA_DEVIATION[T.case_id(case)]))
    assert worst <= T.proba_tolerance(case)


@pytest.mark.parametrize('case,feature', [(T.CASES[10], 192), (T.CASES[5], 64)], ids=['F256-f192', 'F65-f64'])
def test_one_knocked_out_feature_is_far_beyond_the_tolerance(case, feature):
    """the proof that the comparison above would fail on a kernel that loses the first feature of its last 64-feature block: the
    device, given the table with that feature at the scaler's mean, is as far from the full table's reference as the reference says
    (a correct computation on another input)"""
    from pyimsegm_amd import _hip
    F, C, K, _ = case
    model, table, ref = T.case_data(case)
    without = T.knocked_out(model, table, feature)
    h, w = T.grid_shape(K)
    sess = open_session(h, w, without)
    try:
        out = sess.segment(T.pairwise_cost(C), 'model', gmm=_hip.DeviceGmm(model), want_proba=True, want_segm=False)
    finally:
        sess.close()
    moved = float(np.abs(out['proba'] - ref)[2:].max())
    print('%s without feature %d: %.3g from the full table\'s reference' % (T.case_id(case), feature, moved))
    assert moved >= 1e-3 and moved > 1e6 * T.proba_tolerance(case)
    assert np.abs(out['proba'] - T.reference_proba(model, without)).max() <= T.proba_tolerance(case)


@pytest.mark.parametrize('variant', [dict(scaler=False), dict(with_std=False), dict(with_mean=False)], ids=['bare', 'mean-only', 'scale-only'])
@pytest.mark.parametrize('case', [T.CASES[2], T.CASES[7]], ids=T.case_id)
def test_model_without_scaler_mean_or_scale(case, variant):
    """the two null-pointer branches of k_gmm_proba (no scaler_mean, no scaler_scale)"""
    from pyimsegm_amd import _hip
    F, C, K, _ = case
    model, table = T.build_case(case, **variant)
    gmm = _hip.DeviceGmm(model)
    assert (gmm.scaler_mean is None) == (not variant.get('with_mean', True) or not variant.get('scaler', True))
    assert (gmm.scaler_scale is None) == (not variant.get('with_std', True) or not variant.get('scaler', True))
    ref = T.reference_proba(model, table)
    h, w = T.grid_shape(K)
    sess = open_session(h, w, table)
    try:
        out = sess.segment(T.pairwise_cost(C), 'model', gmm=gmm, want_proba=True, want_segm=False)
    finally:
        sess.close()
    worst = float(np.abs(out['proba'] - ref).max())
    # (another model than the case's: its tolerance by the same rule from scikit-learn's own deviation on THIS model)
    tol = max(16 * float(np.abs(model.predict_proba(table) - ref).max()), 1e-12)
    print('%s %r: %.3e (tolerance %.3e)' % (T.case_id(case), variant, worst, tol))
    assert worst <= tol
    top = ref.max(axis=1)
    assert np.sum((top > 0.01) & (top < 0.99)) >= 0.75 * K


@pytest.mark.parametrize('rows', [1, 2, 3, 4, 5])
def test_last_wave_of_four_rows_per_wave(rows):
    """F = 129 (k_gmm_proba<3, 4>) on 1 .. 5 rows: the last wave repeats the last row and writes only below K"""
    from pyimsegm_amd import _hip
    case = T.CASES[7]
    model, table, ref = T.case_data(case)
    sess = open_session(1, rows, table[:rows])
    try:
        out = sess.segment(T.pairwise_cost(case[1]), 'model_l2', gmm=_hip.DeviceGmm(model), want_proba=True, want_segm=False)
    finally:
        sess.close()
    assert out['proba'].shape == (rows, case[1])
    assert np.abs(out['proba'] - ref[:rows]).max() <= T.proba_tolerance(case)


@pytest.mark.parametrize('case', T.CASES, ids=T.case_id)
def test_terms_against_the_80_bit_reference(case):
    """every edge type of the fused call ('features' up to 64 columns: its loop runs in one workgroup) at two edge costs"""
    from pyimsegm_amd import _hip
    F, C, K, _ = case
    model, table, _ = T.case_data(case)
    h, w = T.grid_shape(K)
    pairwise, gmm, tol = T.pairwise_cost(C), _hip.DeviceGmm(model), T.terms_tolerance(case)
    sess = open_session(h, w, table)
    worst = 0.
    try:
        for edge_type in T.EDGE_TYPES:
            if edge_type == 'features' and F > 64:
                continue
            for cost in T.EDGE_COSTS:
                out = sess.segment(pairwise, edge_type, edge_cost=cost, gmm=gmm, debug=True)
                check_graph(out, h, w)
                worst = max(worst, check_terms(out, table, edge_type, cost, pairwise, tol))
    finally:
        sess.close()
    print('%s: terms against longdouble %.3e relative (tolerance %.3e)' % (T.case_id(case), worst, tol))


def test_clip_edges_of_the_unary_cost():
    """probabilities on both sides of the 0.01 / 0.99 clip, 0, 1, a row of zeros, a row of 1 / C, handed in from the host.

    Asserted: (a) the clipped entries are the SAME bits as log(0.01) / log(0.99) of the unclipped constants -- clipping is exact;
    (b) every unary cost is within one ulp of the correctly rounded longdouble value -- not bit equality: the device's log is the
    1-ulp log of the ROCm device library, not a correctly rounded one; (c) the integers equal the reference's everywhere -- the
    reference shows first that no scaled cost lies within two ulp of an integer, so one ulp cannot move a truncation."""
    lo, hi = 0.01, 1 - 0.01
    proba = np.array([[0., lo, hi], [np.nextafter(lo, 0), np.nextafter(lo, 1), 1.], [np.nextafter(hi, 0), np.nextafter(hi, 1), 0.5],
                      [1. / 3, 1. / 3, 1. / 3], [0., 0., 0.]])
    pairwise = T.pairwise_cost(3)
    sess = open_session(1, 5)
    try:
        for edge_type in ('model', 'const'):
            out = sess.segment(pairwise, edge_type, proba=proba, debug=True)
            assert np.array_equal(out['proba'], proba)
            want = T.reference_terms(proba, out['edges'], out['centres'], None, edge_type, 1., pairwise)
            unary = out['unary']
            assert unary[0, 0] == unary[0, 1] == unary[1, 0] and np.all(unary[4] == unary[0, 1])              # (a) below 0.01
            assert unary[0, 2] == unary[1, 2] == unary[2, 1]                # (a) above 0.99
            rounded = want['unary'].astype(np.float64)
            assert np.all(np.abs(unary - rounded) <= np.spacing(rounded))                                       # (b)
            for got, key in ((out['unary_int'], 'unary_scaled'), (out['edge_weights_int'], 'weights_scaled')):
                assert not T.ambiguous(want[key], 2 * np.finfo(np.float64).eps).any()
                assert np.array_equal(got, T.truncated(want[key])), (edge_type, key)                            # (c)
    finally:
        sess.close()


def brute_force_minimum(unary_int, edges, weights_int, pairwise):
    smooth = (pairwise * 100).astype(np.int64)
    K, C = unary_int.shape
    best = None
    for code in range(C**K):
        lab = [(code // C**k) % C for k in range(K)]
        e = sum(int(unary_int[k, lab[k]]) for k in range(K)) + sum(int(wt) * int(smooth[lab[a], lab[b]]) for (a, b), wt in zip(edges, weights_int))
        best = e if best is None else min(best, e)
    return best, smooth


SMALL = {1: [[0.3, 0.7]], 2: [[0.62, 0.38], [0.45, 0.55]], 3: [[0.6, 0.4], [0.45, 0.55], [0.7, 0.3]]}


@pytest.mark.parametrize('edge_type', ['model', 'const', 'spatial'])
@pytest.mark.parametrize('K', [1, 2, 3])
def test_graphs_of_one_two_and_three_nodes(K, edge_type):
    """K = 1 (no edge at all: E = 0 inside the fused call), one edge, a chain of two: the terms equal the reference, the call
    returns normally (a status word that is not clear raises), and the labels reach the minimum of the integer energy over all
    C^K labellings (two classes: one expansion move is an exact minimum cut).  K = 2 with 'model': ONE distance, its deviation is
    0, d / 0 = inf, exp(-inf) = 0 -> the weight is the lower clip 1e-3 in numpy and on the device."""
    proba = np.array(SMALL[K])
    pairwise = T.pairwise_cost(2, 3.0)
    sess = open_session(1, K, block=4 if K == 1 else 2)
    try:
        out = sess.segment(pairwise, edge_type, proba=proba, debug=True)
    finally:
        sess.close()
    check_graph(out, 1, K, 4 if K == 1 else 2)
    assert len(out['edges']) == K - 1
    check_terms(out, None, edge_type, 1., pairwise, 1e-13)
    best, smooth = brute_force_minimum(out['unary_int'], out['edges'], out['edge_weights_int'], pairwise)
    lab = out['graph_labels']
    energy = int(out['unary_int'][np.arange(K), lab].sum()) + sum(int(wt) * int(smooth[lab[a], lab[b]]) for (a, b), wt in zip(out['edges'], out['edge_weights_int']))
    assert energy == best and out['energy'] == best
    assert np.array_equal(out['segm'], lab[T.block_labels(1, K, 4 if K == 1 else 2)])
    if K == 1:
        assert np.all(out['segm'] == 1)
    if K == 2 and edge_type == 'model':
        assert out['edge_weights'][0] == 1e-3


def test_equal_probabilities_at_both_ends_of_every_edge():
    """every distance 0: std = 0, 0 / 0 = NaN.  NaN compares false in both clips, so the float weight is NaN on the device exactly
    where the host mirror (numpy) has NaN; the call returns normally; the integer of a NaN weight is 0 (numpy: INT_MIN) -- no
    smoothness term, the labels are the cheapest class of each node"""
    from pyimsegm_amd import graph_cuts as G
    proba = np.array([[0.6, 0.4], [0.6, 0.4]])
    pairwise = T.pairwise_cost(2, 3.0)
    sess = open_session(1, 2)
    try:
        for edge_type in ('model', 'model_l1', 'model_l2'):
            out = sess.segment(pairwise, edge_type, proba=proba, debug=True)
            with np.errstate(all='ignore'):
                mirror = G.edge_weights_from_graph(out['edges'], out['centres'], None, proba, edge_type)
            assert np.isnan(mirror).all() and np.array_equal(np.isnan(out['edge_weights']), np.isnan(mirror))
            print('integer of a NaN weight:', out['edge_weights_int'])
            check_terms(out, None, edge_type, 1., pairwise, 1e-13)
            assert np.array_equal(out['graph_labels'], [0, 0])
    finally:
        sess.close()


@pytest.mark.parametrize('edge_type', ['model_l2', 'spatial'])
def test_terms_by_the_whole_device_against_the_80_bit_reference(monkeypatch, edge_type):
    """K = 16 384 = TERMS_WIDE_FROM single-block labels on 128 x 128, 32 512 edges (edge capacity 3 K + 64 >= 2 048): launch_gc_terms
    hands the terms to k_terms_elem / _partial / _reduce / _weights / _integers.  Both forms -- that one and the one workgroup behind
    IMSEGM_TERMS_ONE_WORKGROUP -- are held against the reference, and against each other bit for bit.  (The library counts no
    launches: that the first call took the wide form follows from the conditions asserted here, which are launch_gc_terms' own.)"""
    from pyimsegm_amd import _hip
    case = T.WIDE_CASE
    F, C, K, _ = case
    model, table, ref = T.case_data(case)
    h, w = 128, 128
    assert h * w == K >= 16384 and 3 * K + 64 >= 2048 and edge_type != 'features'
    pairwise, gmm, tol = T.pairwise_cost(C), _hip.DeviceGmm(model), T.terms_tolerance(case)
    fallbacks = _hip.gc_grid_fallbacks()
    outs = []
    for one in (False, True):
        if one:
            monkeypatch.setenv('IMSEGM_TERMS_ONE_WORKGROUP', '1')
        sess = open_session(h, w, table)
        try:
            outs.append(sess.segment(pairwise, edge_type, gmm=gmm, debug=True))
        finally:
            sess.close()
    wide, narrow = outs
    assert len(wide['edges']) == 2 * 128 * 127
    check_graph(wide, h, w)
    assert np.abs(wide['proba'] - ref).max() <= T.proba_tolerance(case)
    worst = check_terms(wide, table, edge_type, 1., pairwise, tol)
    check_terms(narrow, table, edge_type, 1., pairwise, tol)
    print('whole device, %s: %.3e relative (tolerance %.3e)' % (edge_type, worst, tol))
    for key in ('proba', 'unary', 'unary_int', 'edge_weights', 'edge_weights_int', 'graph_labels'):
        assert np.array_equal(wide[key], narrow[key]), key
    assert _hip.gc_grid_fallbacks() == fallbacks


def test_put_features_and_the_table_pointer_refuse_what_they_cannot_do():
    import ctypes as C
    from pyimsegm_amd import _hip
    sess = open_session(1, 5)
    try:
        ptr = C.c_void_p()
        assert _hip.load_library().imsegm_image2d_device_ptr(sess._h, 3, C.byref(ptr)) != 0        # no table yet
        for bad in (np.zeros((5, 2)), np.zeros((5, 257)), np.zeros((4, 9)), np.zeros((5, 9), np.float32), np.zeros((9, 5)).T):
            with pytest.raises(ValueError):
                sess.put_features(bad)
        table = np.arange(45, dtype=np.float64).reshape(5, 9)
        sess.put_features(table)
        assert _hip.load_library().imsegm_image2d_device_ptr(sess._h, 3, C.byref(ptr)) == 0 and ptr.value
        assert np.array_equal(sess.get_features(9), table)
    finally:
        sess.close()
