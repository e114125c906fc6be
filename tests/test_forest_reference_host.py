"""The packer of tree ensembles (``_hip.DeviceForest``) and the host statement of their evaluation
(``classification.forest_proba_host``) against scikit-learn: byte for byte with ``n_jobs=1``.  No device is needed."""
import os

import numpy as np
import pytest

import forest_cases as FC

HERE = os.path.dirname(os.path.abspath(__file__))
_FITTED = {}


def fitted(name):
    """(model, packed forest, table) of a case, fitted once for the whole file"""
    if name not in _FITTED:
        from pyimsegm_amd import _hip
        case = FC.fit_by_name(name)
        model = FC.fit_model(case)
        _FITTED[name] = (model, _hip.DeviceForest(model), FC.fit_table(case))
    return _FITTED[name]


def load_golden(name):
    """``_hip.DeviceForest``, table and scikit-learn's probabilities of a golden case"""
    from pyimsegm_amd import _hip
    with np.load(os.path.join(HERE, 'golden', 'forest_proba.npz')) as data:
        part = {key.split('/')[1]: data[key] for key in data.files if key.startswith(name + '/')}
    nodes = np.zeros(len(part['word']), dtype=_hip.FOREST_NODE)
    nodes['threshold'], nodes['word'] = part['threshold'], part['word']
    forest = _hip.DeviceForest.from_arrays(nodes, part['tree_start'], part['leaf_values'], part['table'].shape[1],
                                           part['scaler_mean'] if len(part['scaler_mean']) else None,
                                           part['scaler_scale'] if len(part['scaler_scale']) else None, part['classes'])
    return forest, part['table'], part['expected']


@pytest.mark.parametrize('dtype', (np.float64, np.float32), ids=('f64', 'f32'))
@pytest.mark.parametrize('name', [case.name for case in FC.FITS])
def test_host_statement_equals_sklearn(name, dtype):
    from pyimsegm_amd.classification import forest_proba_host
    model, packed, table = fitted(name)
    table = table.astype(dtype)
    expected = model.predict_proba(table)
    got = forest_proba_host(packed, table)
    assert got.dtype == np.float64 and got.shape == expected.shape
    assert np.array_equal(got, expected)
    assert len(np.unique(expected.argmax(axis=1))) > 1               # (the forest separates the rows: not one leaf for all)


def test_packed_layout():
    from pyimsegm_amd import _hip
    model, packed, _ = fitted('rf_scaled_F9_C3')
    forest = model.steps[-1][1]
    assert packed.nodes.dtype == _hip.FOREST_NODE and packed.nodes.dtype.itemsize == 8
    assert packed.n_trees == 20 and packed.n_features == 9 and packed.n_classes == 3
    assert packed.tree_start[0] == 0 and packed.tree_start[-1] == len(packed.nodes)
    assert list(np.diff(packed.tree_start)) == [tree.tree_.node_count for tree in forest.estimators_]
    assert len(packed.leaf_values) == int((packed.nodes['word'] < 0).sum())
    inner = packed.nodes['word'] >= 0
    # the float32 threshold is the largest one that is not above scikit-learn's
    assert (packed.nodes['threshold'][inner].astype(np.float64) <= packed.threshold64[inner]).all()
    assert (np.nextafter(packed.nodes['threshold'][inner], np.float32(np.inf)).astype(np.float64) > packed.threshold64[inner]).all()
    assert np.array_equal(packed.scaler_mean, model.steps[0][1].mean_) and np.array_equal(packed.scaler_scale, model.steps[0][1].scale_)


def test_ties_occur():
    """the quantised column meets packed thresholds exactly, and only ``<=`` on the rounded-down threshold takes them the way
    scikit-learn does"""
    for name in ('rf_ties', 'et_ties'):
        _, packed, table = fitted(name)
        on_column = (packed.nodes['word'] >= 0) & ((packed.nodes['word'] & 0xff) == 0)
        assert np.isin(table[:, 0].astype(np.float32), packed.nodes['threshold'][on_column]).any()
    from pyimsegm_amd.classification import forest_proba_host
    model, packed, table = fitted('rf_ties')
    # `<` and `<=` differ only where a row visits a node with x == threshold: the defect changing the result is such a visit
    assert not np.array_equal(forest_proba_host(packed, table, _defect='lt'), model.predict_proba(table))


def test_best_first_tree_is_relaid():
    model, packed, table = fitted('bestfirst')
    tree = model.steps[-1][1].tree_
    inner = tree.children_left >= 0
    assert (tree.children_left[inner] != np.flatnonzero(inner) + 1).any()       # scikit-learn's layout is not preorder here
    assert tree.n_leaves == 16 and len(packed.leaf_values) == 16


def test_non_contiguous_classes():
    model, packed, table = fitted('rf_labels_2_5_9')
    assert list(packed.classes) == [2, 5, 9] and list(model.classes_) == [2, 5, 9]


def test_seeded_defects():
    """each wrong statement is caught by a case: ``<`` and the threshold rounded to nearest by 'rf_ties'; the trees added last to
    first and the division per tree by 'rf_scaled_F9_C3' (data seed 20261020, estimator seed 7: both change bits there)"""
    import copy

    from pyimsegm_amd.classification import forest_proba_host
    model, packed, table = fitted('rf_ties')
    expected = model.predict_proba(table)
    assert not np.array_equal(forest_proba_host(packed, table, _defect='lt'), expected)
    nearest = copy.copy(packed)
    nearest.nodes = packed.nodes.copy()
    nearest.nodes['threshold'] = packed.threshold64.astype(np.float32)
    assert (nearest.nodes['threshold'] != packed.nodes['threshold']).any()
    assert not np.array_equal(forest_proba_host(nearest, table), expected)
    model, packed, table = fitted('rf_scaled_F9_C3')
    expected = model.predict_proba(table)
    for defect in ('reverse', 'divide_per_tree'):
        assert not np.array_equal(forest_proba_host(packed, table, _defect=defect), expected), defect


def test_models_the_packer_refuses():
    from sklearn.decomposition import PCA
    from sklearn.ensemble import GradientBoostingClassifier, RandomForestClassifier
    from sklearn.pipeline import Pipeline
    from sklearn.preprocessing import StandardScaler

    from pyimsegm_amd import _hip
    table, labels = FC.fit_data(FC.fit_by_name('rf_scaled_F9_C3'), 80, 3)
    boosted = GradientBoostingClassifier(n_estimators=3).fit(table, labels)
    reduced = Pipeline([('scaler', StandardScaler()), ('pca', PCA(3)), ('classif', RandomForestClassifier(3))]).fit(table, labels)
    two_outputs = RandomForestClassifier(3).fit(table, np.stack([labels, labels], axis=1))
    for model in (boosted, reduced, two_outputs, RandomForestClassifier(3)):
        assert _hip.DeviceForest(model) is None and isinstance(_hip.forest_refusal(model), str)


@pytest.mark.parametrize('name', FC.GOLDEN)
def test_golden_file(name):
    """the committed forests give scikit-learn's recorded probabilities, and -- with the scikit-learn the file was written by -- are
    what the packer makes of a new fit"""
    import sklearn

    from pyimsegm_amd.classification import forest_proba_host
    forest, table, expected = load_golden(name)
    assert np.array_equal(forest_proba_host(forest, table), expected)
    with np.load(os.path.join(HERE, 'golden', 'forest_proba.npz')) as data:
        written_by = str(data['sklearn_version'])
    if written_by == sklearn.__version__:
        _, packed, _ = fitted(name)
        assert np.array_equal(packed.nodes, forest.nodes) and np.array_equal(packed.leaf_values, forest.leaf_values)


def test_place_switch(monkeypatch):
    from pyimsegm_amd import _hip
    from pyimsegm_amd.classification import classif_place, predict_proba
    model, _, table = fitted('rf_scaled_F9_C3')
    monkeypatch.delenv('IMSEGM_CLASSIF_ON', raising=False)
    assert classif_place(None) == 'host' and classif_place('host') == 'host'
    assert np.array_equal(predict_proba(model, table), model.predict_proba(table))
    monkeypatch.setenv('IMSEGM_CLASSIF_ON', 'gpu')
    with pytest.raises(ValueError):
        predict_proba(model, table)
    with pytest.raises(ValueError):
        classif_place('somewhere')
    if _hip.device_count() == 0:
        with pytest.raises(_hip.HipUnavailableError):
            predict_proba(model, table, on='device')
