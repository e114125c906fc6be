"""k_pca_project in front of k_gmm_proba, and the Bayesian mixture's constants, on the device against the 80-bit reference of
tests/reduced_model_cases.py (tests/test_reduced_model_reference_host.py shows on the CPU what these cases see; the tolerance is
16 x scikit-learn's own fp64 deviation from the reference, floor 1e-12), on tables the test chooses (Image2D.put_features; label k
is a 2 x 2 block of pixels).  Then the routing: a model fitted by ``estim_class_model`` with ``pca_coef`` or ``'BGM'`` keeps the
one-call and the batch path, and their class maps are those of the staged path with scikit-learn's ``predict_proba``.  The device's
own figures are printed (pytest -s) and tabulated in DESIGN.md section 5."""
import numpy as np
import pytest

import reduced_model_cases as R
import terms_cases as T

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not R.LONGDOUBLE_OK, reason=R.LONGDOUBLE_REASON)]


def device_proba(model, table, K, edge_type='model'):
    from pyimsegm_amd import _hip
    h, w = T.grid_shape(K)
    labels = T.block_labels(h, w)
    image = np.random.RandomState(h * 1000 + w).randint(0, 256, labels.shape + (3, )).astype(np.uint8)
    sess = _hip.Image2D(*labels.shape).upload(image).set_labels(labels, h * w)
    try:
        sess.put_features(np.ascontiguousarray(table, dtype=np.float64))
        gmm = _hip.DeviceGmm(model)
        out = sess.segment(T.pairwise_cost(gmm.n_classes), edge_type, gmm=gmm, want_proba=True, want_graph_labels=True)
    finally:
        sess.close()
    assert out['proba'].shape == (K, gmm.n_classes)
    return out


@pytest.mark.parametrize('case', R.CASES + R.BAYES_CASES, ids=R.case_id)
def test_probabilities_against_the_80_bit_reference(case):
    model, table, ref = R.case_data(case)
    out = device_proba(model, table, case[3])
    worst = float(np.abs(out['proba'] - ref).max())
    print('%s: device against longdouble %.3e (tolerance %.3e, scikit-learn %.3e)'
          % (R.case_id(case), worst, R.proba_tolerance(case), R.PROBA_DEVIATION[R.case_id(case)]))
    assert worst <= R.proba_tolerance(case)


@pytest.mark.parametrize('edge_type', ['model', 'features'])
def test_reduced_model_in_front_of_the_whole_device_terms(edge_type):
    """K = 16 384 rows (terms.hip TERMS_WIDE_FROM): the projection and the mixture run over 16 384 waves, the terms behind them on
    the whole device ('model') or, for the 'features' edges -- which read the RAW nine-column table, not the projected one --, in
    the one workgroup"""
    case = R.WIDE_CASE
    model, table, ref = R.case_data(case)
    out = device_proba(model, table, case[3], edge_type)
    worst = float(np.abs(out['proba'] - ref).max())
    print('%s, %s edges: device against longdouble %.3e (tolerance %.3e)' % (R.case_id(case), edge_type, worst, R.proba_tolerance(case)))
    assert worst <= R.proba_tolerance(case)
    assert out['graph_labels'].min() >= 0 and out['graph_labels'].max() < case[2]


@pytest.mark.parametrize('case', [R.CASES[8], R.CASES[5]], ids=R.case_id)
def test_a_zeroed_row_of_the_components_is_far_beyond_the_tolerance(case):
    """the comparison above would fail on a kernel that loses the first input column of its last 64-column block: the device, given
    the model without that row of ``components_.T``, is as far from the full model's reference as the reference says, and agrees
    with the reference of the model it was given"""
    model, table, ref = R.case_data(case)
    row = 64 * ((case[0] - 1) // 64)
    other = R.with_zeroed_component_row(model, row)
    out = device_proba(other, table, case[3])
    moved = float(np.abs(out['proba'] - ref).max())
    print('%s without row %d: %.3g from the full model\'s reference' % (R.case_id(case), row, moved))
    assert moved >= 1e-3 and moved > 1e6 * R.proba_tolerance(case)
    assert np.abs(out['proba'] - R.reference_proba(other, table)).max() <= R.proba_tolerance(case)


@pytest.mark.parametrize('rows', [1, 2, 3, 5])
def test_last_wave_of_four_rows_per_wave(rows):
    """129 -> 65 (k_pca_project<3, 4>, k_gmm_proba<2, 4>) on 1 .. 5 rows: the last wave repeats the last row, writes below K only"""
    case = R.CASES[6]
    model, table, ref = R.case_data(case)
    out = device_proba(model, table[:rows], rows, 'model_l2')
    assert np.abs(out['proba'] - ref[:rows]).max() <= R.proba_tolerance(case)


def test_library_refuses_a_model_that_does_not_fit_the_table():
    from pyimsegm_amd import _hip
    model, table, _ = R.case_data(R.CASES[1])
    with pytest.raises(_hip.HipError):
        device_proba(model, table[:, :6], R.CASES[1][3])             # six resident columns, the model reads nine
    assert _hip.load_library().imsegm_version() >= 101


# ---- routing: the pipelines keep the fused paths for the models estim_class_model builds
FEATURES = {'color': ['mean', 'std', 'energy']}
SP_SIZE, SP_REGUL, GC_REGUL = 8, 0.2, 1.5
#: seed of the two synthetic images
IMAGE_SEED = 7


def synthetic_images():
    rng = np.random.RandomState(IMAGE_SEED)
    out = []
    for shift in (0, 25):
        yy, xx = np.mgrid[0:80, 0:90]
        kind = (xx > 30 + shift).astype(int) + ((yy > 45) & (xx > 55)).astype(int)
        base = np.array([[60, 90, 40], [150, 120, 160], [210, 200, 90]])[kind]
        noise = rng.standard_normal((80, 90, 3)) * np.array([12., 25., 40.])[kind][:, :, None]
        out.append(np.clip(base + noise, 0, 255).astype(np.uint8))
    return out


def fitted_model(images, **kwargs):
    from pyimsegm_amd import pipelines as P
    from pyimsegm_amd.graph_cuts import estim_class_model
    tables = []
    for image in images:
        res = P._ResidentImage(image, FEATURES, SP_SIZE, SP_REGUL)
        try:
            tables.append(np.array(res.features))
        finally:
            res.close()
    np.random.seed(0)
    return estim_class_model(np.concatenate(tables), 3, max_iter=25, **kwargs)


def staged(image, model):
    """the staged path with scikit-learn's predict_proba on the host: (class map, label map, excluded superpixels).  Excluded
    -- by the longdouble reference alone -- is a superpixel whose two cheapest integer unary costs differ by at most one unit"""
    from pyimsegm_amd import pipelines as P
    res = P._ResidentImage(image, FEATURES, SP_SIZE, SP_REGUL)
    try:
        table = np.array(res.features)
        proba = model.predict_proba(table)
        pairwise = T.pairwise_cost(proba.shape[1], GC_REGUL)
        out = res.sess.segment(pairwise, 'model', proba=proba, debug=True)
        slic = np.array(res.slic)
    finally:
        res.close()
    want = T.reference_terms(R.reference_proba(model, table), out['edges'], out['centres'], None, 'model', 1., pairwise)
    ints = np.sort(T.truncated(want['unary_scaled']), axis=1)
    excluded = (ints[:, 1] - ints[:, 0]) <= 1
    return out['segm'], slic, excluded


@pytest.mark.parametrize('kind', ['pca', 'bayes', 'pca+bayes'])
def test_one_call_and_batch_paths_take_the_model(kind):
    from pyimsegm_amd import pipelines as P
    images = synthetic_images()
    kwargs = {'pca': dict(estim_model='GMM', pca_coef=0.95), 'bayes': dict(estim_model='BGM'),
              'pca+bayes': dict(estim_model='BGM', pca_coef=0.95)}[kind]
    model = fitted_model(images, **kwargs)
    gmm = P._device_gmm(model)
    assert gmm is not None and gmm.n_inputs == 9
    assert (gmm.n_features < 9) == ('pca' in kind)
    batch = P._segment_color2d_batch_call(images, model, FEATURES, SP_SIZE, SP_REGUL, GC_REGUL, 'model')
    assert batch is not None and len(batch) == 2
    for image, from_batch in zip(images, batch):
        one = P._segment_color2d_one_call(image, model, FEATURES, SP_SIZE, SP_REGUL, GC_REGUL, 'model')
        assert one is not None
        want, slic, excluded = staged(image, model)
        print('%s: %d superpixels, %d excluded, classes %r' % (kind, len(excluded), int(excluded.sum()), np.unique(want).tolist()))
        assert excluded.mean() <= 0.01
        assert len(np.unique(want)) >= 2
        keep = ~excluded[slic]
        assert np.array_equal(np.asarray(one[0])[keep], want[keep])
        assert np.array_equal(np.asarray(from_batch)[keep], want[keep])
        # the resident session takes the model too: the same class map without a host predict_proba
        res = P._ResidentImage(image, FEATURES, SP_SIZE, SP_REGUL, features_to_host=False)
        try:
            segm, _ = res.segment(None, GC_REGUL, 'model', model=model)
            assert res._features is None                              # (nobody downloaded the table)
        finally:
            res.close()
        assert np.array_equal(np.asarray(segm)[keep], want[keep])


# ---- the gray 3-D pipeline: a volume session (three centre coordinates, the prepared graph) in front of the same kernels
VOLUME_SEED = 11


def synthetic_volume():
    rng = np.random.RandomState(VOLUME_SEED)
    zz, yy, xx = np.mgrid[0:12, 0:40, 0:40]
    kind = (xx > 13).astype(int) + ((xx > 26) | ((yy > 28) & (xx > 13))).astype(int)
    base = np.array([50., 120., 200.])[kind]
    noise = rng.standard_normal(kind.shape) * np.array([6., 20., 40.])[kind]
    return np.clip(base + noise, 0, 255).astype(np.uint8)


@pytest.mark.parametrize('kind', ['pca', 'bayes'])
def test_gray3d_pipeline_takes_the_model(monkeypatch, kind):
    """``pipe_gray3d_slic_features_model_graphcut`` on a 12 x 40 x 40 volume with three gray columns (mean, std, energy): with
    ``pca_coef=0.95`` / ``'BGM'`` the fused call on the volume session gets the device model and the normalised table instead of
    host probabilities; its probabilities agree with the 80-bit reference, and the class volume equals, voxel for voxel, that of
    the same pipeline with the model held on the host (same seed, hence the same fit)"""
    from pyimsegm_amd import _hip
    from pyimsegm_amd import pipelines as P
    volume = synthetic_volume()
    features = {'color': ['mean', 'std', 'energy']}
    kwargs = {'pca': dict(pca_coef=0.95), 'bayes': dict(estim_model='BGM')}[kind]
    calls, fits = [], []
    real_segment, real_fit = _hip.Volume3D.segment, P.estim_class_model

    def spy_segment(self, *args, **kw):
        out = real_segment(self, *args, **dict(kw, debug=True, want_proba=True))
        calls.append((kw, out, self.get_labels()))
        return out

    def spy_fit(table, *args, **kw):
        model = real_fit(table, *args, **kw)
        fits.append((np.array(table), model))
        return model

    monkeypatch.setattr(_hip.Volume3D, 'segment', spy_segment)
    monkeypatch.setattr(P, 'estim_class_model', spy_fit)

    def run():
        np.random.seed(0)
        return P.pipe_gray3d_slic_features_model_graphcut(volume, 3, features, spacing=(1, 1, 1), sp_size=5, sp_regul=0.2,
                                                          gc_regul=1., **kwargs)

    on_device = np.array(run())
    monkeypatch.setattr(P, '_reduced_or_bayesian', lambda gmm: False)
    on_host = np.array(run())
    assert len(calls) == 2 and len(fits) == 2
    (kw_dev, out_dev, slic), (kw_host, out_host, slic_host) = calls
    assert kw_dev.get('gmm') is not None and kw_dev.get('proba') is None            # the device model went into the fused call
    assert kw_host.get('gmm') is None and kw_host.get('proba') is not None
    gmm = kw_dev['gmm']
    table, model = fits[0]
    assert table.shape[1] == 3 and gmm.n_inputs == 3 and (gmm.n_features < 3) == (kind == 'pca')
    assert np.array_equal(fits[1][0], table) and np.array_equal(slic, slic_host)
    for a, b in zip(R.model_steps(model), R.model_steps(fits[1][1])):
        assert type(a) is type(b)
    assert np.array_equal(model.predict_proba(table), kw_host['proba'])           # the same fit both times
    # probabilities of the volume session against the reference, by the rule of the cases above on THIS model
    ref = R.reference_proba(model, table)
    tol = max(16 * float(np.abs(model.predict_proba(table) - ref).max()), 1e-12)
    worst = float(np.abs(out_dev['proba'] - ref).max())
    print('gray 3-D, %s: %d supervoxels, device against longdouble %.3e (tolerance %.3e)' % (kind, len(ref), worst, tol))
    assert worst <= tol
    assert out_dev['centres'].shape[1] == 3 and np.array_equal(out_dev['edges'], out_host['edges'])
    # class volumes: equal but for the supervoxels the reference calls a tie of the two cheapest integer costs (at most 1 %)
    pairwise = T.pairwise_cost(3, 1.)                     # (compute_pairwise_cost of the scalar gc_regul = 1)
    want = T.reference_terms(ref, out_host['edges'], out_host['centres'], None, 'model', 1., pairwise)
    ints = np.sort(T.truncated(want['unary_scaled']), axis=1)
    excluded = (ints[:, 1] - ints[:, 0]) <= 1
    print('gray 3-D, %s: %d excluded, classes %r' % (kind, int(excluded.sum()), np.unique(on_host).tolist()))
    assert excluded.mean() <= 0.01 and len(np.unique(on_host)) >= 2
    keep = ~excluded[slic]
    assert on_device.shape == volume.shape and np.array_equal(on_device[keep], on_host[keep])
