"""What of the wide device fit (``fit_on='device_wide'``, 17 to 256 features) can be checked without a GPU: the cases of
tests/mixture_fit_wide_cases.py qualify (scikit-learn alone keeps every cluster, raises nothing and converges on them), the
comparison of the GPU tests sees a planted defect, and the keyword is accepted and never falls back to the CPU."""
import numpy as np
import pytest

import mixture_fit_wide_cases as WC


@pytest.mark.parametrize('name', sorted(WC.CASES))
def test_scikit_learn_alone_meets_the_conditions_of_the_case(name):
    table = WC.load_table(name)
    n_components, n_restarts = WC.CASES[name]
    assert 17 <= table.shape[1] <= 256 and table.shape[0] % 256
    labels, _, _, _ = WC.host_lloyd(name)
    assert labels.shape == (n_restarts, len(table))
    for lab in labels:
        assert np.bincount(lab, minlength=n_components).min() > 0
        run = WC.reference_em(table, lab, 1e-3, 99)
        assert run['failed'] == 0 and run['converged'], (name, run['n_iter'])
    assert WC.EM_TOLERANCE[name] >= 1e-12


def planted(monkeypatch, defect):
    """scikit-learn's mixture with a defect in the place the device code could have one"""
    import sklearn.mixture
    from sklearn.mixture._gaussian_mixture import _compute_precision_cholesky

    class Defective(sklearn.mixture.GaussianMixture):
        def _m_step(self, X, log_resp):
            super()._m_step(X, log_resp)
            if defect == 'column':               # the last feature column left out of the centred products
                cov = self.covariances_.copy()
                cov[:, -1, :] = 0.
                cov[:, :, -1] = 0.
                cov[:, -1, -1] = self.reg_covar
                self.covariances_ = cov
                self.precisions_cholesky_ = _compute_precision_cholesky(cov, 'full')

        def _estimate_log_weights(self):
            log_weights = np.log(self.weights_)
            if defect == 'weight':               # the last component's weight left out of the log density
                log_weights[-1] = 0.
            return log_weights

    monkeypatch.setattr(sklearn.mixture, 'GaussianMixture', Defective)


@pytest.mark.parametrize('defect', ('column', 'weight'))
@pytest.mark.parametrize('name', sorted(WC.CASES))
def test_the_comparison_sees_a_planted_defect(name, defect, monkeypatch):
    table = WC.load_table(name)
    lab = WC.host_lloyd(name)[0][0]
    plain = WC.reference_em(table, lab, 0., 2)
    planted(monkeypatch, defect)
    broken = WC.reference_em(table, lab, 0., 2)
    assert plain['n_iter'] == 2 and not plain['failed']
    seen = WC.deviation(broken, plain)
    print('%s, %s: deviation %.3g (tolerance %.3g)' % (name, defect, seen, WC.EM_TOLERANCE[name]))
    assert seen > WC.EM_TOLERANCE[name]


def test_fit_place_takes_the_new_value(monkeypatch):
    from pyimsegm_amd import graph_cuts
    monkeypatch.delenv('IMSEGM_FIT_ON', raising=False)
    assert graph_cuts._fit_place('device_wide') == 'device_wide'
    assert graph_cuts._fit_place('device') == 'device' and graph_cuts._fit_place(None) == 'host'
    monkeypatch.setenv('IMSEGM_FIT_ON', 'device_wide')
    assert graph_cuts._fit_place(None) == 'device_wide'
    with pytest.raises(ValueError):
        graph_cuts._fit_place('gpu')
    calls = []
    monkeypatch.setattr(graph_cuts, 'fit_mixture_device_wide', lambda mixture, table, ctx=None: calls.append(table.shape) or mixture)
    graph_cuts.estim_class_model(WC.raw_table('c3_17'), 3)
    assert calls == [(1954, 17)]
    with pytest.raises(ValueError):
        graph_cuts.estim_class_model(WC.raw_table('c3_17'), 3, fit_on='gpu')


def test_no_library_is_an_error_not_a_host_fit(monkeypatch):
    from pyimsegm_amd import _hip, graph_cuts
    monkeypatch.setattr(_hip, '_lib', None)
    monkeypatch.setattr(_hip, 'LIB_PATH', '/nonexistent/libimsegm_hip.so')
    monkeypatch.setattr(_hip, '_default_ctx', {})
    with pytest.raises(_hip.HipUnavailableError):
        graph_cuts.estim_class_model(WC.raw_table('c3_17'), 3, fit_on='device_wide')
