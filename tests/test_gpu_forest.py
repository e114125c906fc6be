"""Tree-ensemble class models on the device (csrc/forest.hip, api_forest.hip): every comparison is ``array_equal`` on the float64
probabilities of the host statement ``classification.forest_proba_host``, which tests/test_forest_reference_host.py holds to
scikit-learn's bytes."""
import logging

import numpy as np
import pytest

import forest_cases as FC
from test_forest_reference_host import load_golden

pytestmark = pytest.mark.gpu

_REF = {}


@pytest.fixture(scope='module')
def hip():
    from pyimsegm_amd import _hip
    _hip.default_context()
    return _hip


def host(forest, table):
    from pyimsegm_amd.classification import forest_proba_host
    return forest_proba_host(forest, table)


def forest_20(hip):
    """20 random trees of 40 leaves, 9 features, 3 classes, a scaler: shared by the row-count cases"""
    if 'forest_20' not in _REF:
        _REF['forest_20'] = FC.random_forest(20, 40, 9, 3, seed=11)
    return _REF['forest_20']


# one row, a wave less / exactly / more than one, and one row on either side of a workgroup's block of rows and of two blocks
@pytest.mark.parametrize('rows', (1, 63, 64, 65, 255, 256, 257, 511, 513))
def test_rows(hip, rows):
    assert hip.FOREST_ROWS == 256
    forest, table = forest_20(hip), FC.hand_table(rows, 9, seed=rows)
    assert np.array_equal(hip.forest_proba(forest, table), host(forest, table))


@pytest.mark.parametrize('trees', (1, 2, 20, 80))
def test_trees(hip, trees):
    forest, table = FC.random_forest(trees, 24, 5, 4, seed=trees, scaler=trees != 2), FC.hand_table(300, 5, seed=3)
    assert np.array_equal(hip.forest_proba(forest, table), host(forest, table))


@pytest.mark.parametrize('name', FC.GOLDEN)
def test_golden_forests(hip, name):
    forest, table, expected = load_golden(name)
    got = hip.forest_proba(forest, table)
    assert np.array_equal(got, expected)                       # scikit-learn's recorded bytes
    assert np.array_equal(got, host(forest, table))


def test_single_leaf(hip):
    forest, table = FC.single_leaf_forest(3, 4), FC.hand_table(70, 3, seed=1)
    got = hip.forest_proba(forest, table)
    assert np.array_equal(got, host(forest, table)) and np.array_equal(got, np.full((70, 4), 0.25))


@pytest.mark.parametrize('side', ('left', 'right'))
def test_chain_of_depth_200(hip, side):
    forest, table = FC.chain_forest(200, 7, 3, seed=5, side=side), FC.hand_table(400, 7, seed=6)
    expected = host(forest, table)
    assert len(np.unique(expected, axis=0)) > 20               # rows stop at many depths, and some walk to the end
    assert np.array_equal(hip.forest_proba(forest, table), expected)


# a tree one node below and one above what a workgroup stages in LDS (a full binary tree has an odd number of nodes): the walk
# in LDS and the same walk in global memory
@pytest.mark.parametrize('nodes', (4095, 4097))
def test_tree_around_the_lds_share(hip, nodes):
    assert hip.FOREST_LDS_NODES == 4096
    forest = FC.chain_forest((nodes - 1) // 2, 6, 3, seed=nodes, side='right', threshold=-3.)
    assert len(forest.nodes) == nodes
    table = FC.hand_table(300, 6, seed=8)
    expected = host(forest, table)
    assert len(np.unique(expected, axis=0)) > 20
    assert np.array_equal(hip.forest_proba(forest, table), expected)


def test_mixed_forest_both_paths(hip):
    """trees in LDS and trees in global memory in ONE forest: the order of the sum does not depend on where a tree is walked"""
    rng = np.random.RandomState(4)
    big = FC.chain_forest(2100, 6, 3, seed=1, side='right', threshold=-3.)
    small = FC.random_forest(3, 30, 6, 3, seed=2, scaler=False)
    words = [small.nodes, big.nodes.copy(), small.nodes.copy()]
    words[1]['word'][words[1]['word'] < 0] -= len(small.leaf_values)               # (leaf rows behind the first small forest's)
    words[2]['word'][words[2]['word'] < 0] -= len(small.leaf_values) + len(big.leaf_values)
    starts = np.concatenate([small.tree_start, small.tree_start[-1] + big.tree_start[1:],
                             small.tree_start[-1] + big.tree_start[-1] + small.tree_start[1:]])
    values = np.concatenate([small.leaf_values, big.leaf_values, rng.rand(*small.leaf_values.shape)])
    forest = hip.DeviceForest.from_arrays(np.concatenate(words), starts, values, 6)
    table = FC.hand_table(300, 6, seed=9)
    assert np.array_equal(hip.forest_proba(forest, table), host(forest, table))


def test_column_and_class_limits(hip):
    forest, table = FC.random_forest(3, 20, 256, 16, seed=21), FC.hand_table(130, 256, seed=22)
    assert np.array_equal(hip.forest_proba(forest, table), host(forest, table))
    out = np.full((130, 17), -7.)
    for refused, columns in ((FC.random_forest(2, 8, 257, 3, seed=23), 257), (FC.random_forest(2, 8, 5, 17, seed=24), 5)):
        with pytest.raises(hip.HipForestInputError):
            hip.forest_proba(refused, FC.hand_table(130, columns, seed=25), out=out[:, :refused.n_classes].copy())
    too_many = FC.random_forest(1025, 2, 3, 2, seed=26, scaler=False)
    with pytest.raises(hip.HipForestInputError):
        hip.forest_proba(too_many, FC.hand_table(10, 3, seed=27))


def test_refusals_leave_the_output_untouched(hip):
    forest = forest_20(hip)
    table = FC.hand_table(200, 9, seed=30)
    for value in (np.nan, np.inf, -np.inf, 1e300):                  # (1e300: finite as a double, not as the float32 the trees see)
        bad = table.copy()
        bad[137, 4] = value
        out = np.full((200, 3), -7.)
        with pytest.raises(hip.HipForestInputError):
            hip.forest_proba(forest, bad, out=out)
        assert (out == -7.).all()
    inner = np.flatnonzero(forest.nodes['word'] >= 0)

    def broken(change):
        import copy
        other = copy.copy(forest)
        other.nodes = forest.nodes.copy()
        change(other.nodes['word'])
        return other

    def child_out_of_range(word):
        word[inner[3]] = (word[inner[3]] & 0xff) | (100000 << 8)

    def cycle(word):
        word[inner[5]] = (word[inner[5]] & 0xff) | (0 << 8)         # back to the root

    def leaf_row_out_of_range(word):
        word[np.flatnonzero(word < 0)[2]] = ~len(forest.leaf_values)

    def feature_out_of_range(word):
        word[inner[1]] = (word[inner[1]] & ~0xff) | 200

    for change in (child_out_of_range, cycle, leaf_row_out_of_range, feature_out_of_range):
        out = np.full((200, 3), -7.)
        with pytest.raises(hip.HipForestInputError):
            hip.forest_proba(broken(change), table, out=out)
        assert (out == -7.).all()
    assert np.array_equal(hip.forest_proba(forest, table), host(forest, table))       # the context is as good as before


@pytest.mark.parametrize('word', (0x00000001, 0x7F7F7F7F))
def test_stale_scratch(hip, word):
    """a large call, then a small one on the same context; then the small one on scratch filled with a word, and once more"""
    ctx = hip.Context()
    try:
        large, large_table = FC.random_forest(80, 40, 60, 8, seed=40), FC.hand_table(5000, 60, seed=41)
        small, small_table = FC.random_forest(2, 5, 3, 2, seed=42), FC.hand_table(5, 3, seed=43)
        assert np.array_equal(hip.forest_proba(large, large_table, ctx=ctx), host(large, large_table))
        expected = host(small, small_table)
        assert np.array_equal(hip.forest_proba(small, small_table, ctx=ctx), expected)
        assert ctx.poison(word) > 0
        assert np.array_equal(hip.forest_proba(small, small_table, ctx=ctx), expected)
        assert np.array_equal(hip.forest_proba(small, small_table, ctx=ctx), expected)
    finally:
        ctx.close()


def table_forest(table, n_classes, seed):
    """random trees whose thresholds are values of the table's own columns, so that its rows spread over the leaves"""
    forest = FC.random_forest(12, 16, table.shape[1], n_classes, seed=seed, scaler=False)
    rng = np.random.RandomState(seed)
    inner = np.flatnonzero(forest.nodes['word'] >= 0)
    columns = forest.nodes['word'][inner] & 0xff
    forest.nodes['threshold'][inner] = table[rng.randint(len(table), size=len(inner)), columns].astype(np.float32)
    return forest


def check_session(hip, sess, table):
    """forest_proba + segment(gmm=None, proba=None) against segment(proba=host probabilities), then the drop after set_labels"""
    from pyimsegm_amd.graph_cuts import compute_pairwise_cost
    forest = table_forest(table, 3, seed=50)
    expected = host(forest, table)
    assert len(np.unique(expected.argmax(axis=1))) > 1
    pairwise = compute_pairwise_cost(1., (len(table), 3))
    wanted = dict(want_soft=True, want_graph_labels=True, want_proba=True)
    ref = sess.segment(pairwise, 'model', proba=expected, **wanted)
    assert np.array_equal(sess.forest_proba(forest, to_host=True), expected)
    assert sess.forest_proba(forest) is None                   # (no wait: the probabilities stay on the device)
    got = sess.segment(pairwise, 'model', **wanted)
    for name in ('segm', 'soft', 'graph_labels', 'proba'):
        assert np.array_equal(got[name], ref[name]), name
    assert len(np.unique(got['segm'])) > 1
    again = sess.segment(pairwise, 'model', **wanted)          # they stay until the labels or the table change
    assert np.array_equal(again['segm'], ref['segm'])
    sess.set_labels(sess.get_labels_int32(), sess.n_labels)
    with pytest.raises(hip.HipError, match='either a class model or probabilities are required'):
        sess.segment(pairwise, 'model', **wanted)


def test_session_image(hip):
    from pyimsegm_amd.pipelines import _ResidentImage
    from pyimsegm_amd.utilities.synthetic import voronoi_image
    res = _ResidentImage(voronoi_image(96, 128, nb_seeds=6), {'color': ['mean', 'std', 'energy']}, 10, 0.2)
    try:
        check_session(hip, res.sess, res.features)
    finally:
        res.close()


def test_session_volume(hip):
    from pyimsegm_amd.superpixels import _open_volume, _run_slic3d
    from pyimsegm_amd.utilities.synthetic import ellipsoid_volume
    sess = _open_volume(ellipsoid_volume((8, 32, 32)))
    try:
        _run_slic3d(sess, 6, 0.2, (1, 1, 1))
        check_session(hip, sess, sess.features_color(to_host=True))
    finally:
        sess.close()


@pytest.fixture(scope='module')
def trained():
    """(image, fitted scaler + random forest of the supervised pipeline with ``n_jobs=1``, features) on a synthetic image"""
    from pyimsegm_amd import pipelines as pipe
    from pyimsegm_amd.utilities.synthetic import voronoi_image
    image, annot = voronoi_image(96, 128, nb_seeds=6, return_classes=True)
    features = {'color': ['mean', 'std', 'energy']}
    np.random.seed(0)
    model, _, tables, _ = pipe.train_classif_color2d_slic_features([image], [annot], features, sp_size=10, sp_regul=0.2, pca_coef=None,
                                                                   feature_balance=None)
    model.set_params(classif__n_jobs=1)
    return image, model, features, tables[0]


def test_pipeline(hip, trained, monkeypatch):
    from pyimsegm_amd import pipelines as pipe
    image, model, features, _ = trained
    monkeypatch.delenv('IMSEGM_CLASSIF_ON', raising=False)
    results = {}
    for place in ('host', 'device', None):
        results[place] = pipe.segment_color2d_slic_features_model_graphcut(image, model, features, sp_size=10, sp_regul=0.2,
                                                                           classif_on=place)
    monkeypatch.setenv('IMSEGM_CLASSIF_ON', 'device')
    results['env'] = pipe.segment_color2d_slic_features_model_graphcut(image, model, features, sp_size=10, sp_regul=0.2)
    results['batch'] = (pipe.segment_batch_color2d_slic_features_model_graphcut([image], model, features, sp_size=10, sp_regul=0.2,
                                                                                nb_workers=1)[0], None)
    assert len(np.unique(results['host'][0])) >= 2
    for place in ('device', None, 'env'):
        assert np.array_equal(results[place][0], results['host'][0]) and np.array_equal(results[place][1], results['host'][1]), place
    assert np.array_equal(results['batch'][0], results['host'][0])
    monkeypatch.setenv('IMSEGM_CLASSIF_ON', 'gpu')
    with pytest.raises(ValueError):
        pipe.segment_color2d_slic_features_model_graphcut(image, model, features, sp_size=10, sp_regul=0.2)


def test_pipeline_runs_the_device(hip, trained, monkeypatch):
    """``classif_on='device'`` does go through the session's forest call (and 'host' does not)"""
    from pyimsegm_amd import pipelines as pipe
    image, model, features, _ = trained
    calls = []
    entry = hip.Image2D.forest_proba
    monkeypatch.setattr(hip.Image2D, 'forest_proba', lambda self, *a, **k: calls.append(1) or entry(self, *a, **k))
    pipe.segment_color2d_slic_features_model_graphcut(image, model, features, sp_size=10, sp_regul=0.2, classif_on='host')
    assert not calls
    pipe.segment_color2d_slic_features_model_graphcut(image, model, features, sp_size=10, sp_regul=0.2, classif_on='device')
    assert calls == [1]


def test_predict_proba_switch(hip, trained, monkeypatch, caplog):
    from sklearn.ensemble import GradientBoostingClassifier

    from pyimsegm_amd.classification import predict_proba
    _, model, _, table = trained
    expected = model.predict_proba(table)
    monkeypatch.delenv('IMSEGM_CLASSIF_ON', raising=False)
    assert np.array_equal(predict_proba(model, table, on='device'), expected)
    assert np.array_equal(predict_proba(model, table), expected)
    monkeypatch.setenv('IMSEGM_CLASSIF_ON', 'device')
    assert np.array_equal(predict_proba(model, table), expected)
    monkeypatch.setenv('IMSEGM_CLASSIF_ON', 'gpu')
    with pytest.raises(ValueError):
        predict_proba(model, table)
    assert np.array_equal(predict_proba(model, table, on='host'), expected)
    # a model the device does not take: the host's result, and the reason at INFO
    labels = model.predict(table)
    boosted = GradientBoostingClassifier(n_estimators=3, random_state=0).fit(table, labels)
    with caplog.at_level(logging.INFO):
        got = predict_proba(boosted, table, on='device')
    assert np.array_equal(got, boosted.predict_proba(table))
    assert any('evaluated on the host' in record.getMessage() and 'GradientBoostingClassifier' in record.getMessage()
               for record in caplog.records)
    # a table the device does not take
    with caplog.at_level(logging.INFO):
        bad = table.copy()
        bad[0, 0] = 1e300
        with pytest.raises(ValueError):                         # (scikit-learn's own refusal, from the host)
            predict_proba(model, bad, on='device')
    assert any('not finite' in record.getMessage() for record in caplog.records)
