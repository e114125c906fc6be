"""Leung-Malik texture descriptors with the 'median' and 'meanGrad' statistics on the device (descriptors.py:1041-1106 of the
reference): against the reference's own outputs (tests/golden/texture_flags.npz, see tests/golden/make_golden_texture_flags.py),
without any host filtering, against numpy on the device's own response, and with the prepared state surviving the calls."""
import importlib.util
import itertools
import os
import zlib

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
_spec = importlib.util.spec_from_file_location('make_golden_texture_flags', os.path.join(GOLDEN, 'make_golden_texture_flags.py'))
GEN = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(GEN)
VEC = np.load(os.path.join(GOLDEN, 'texture_flags.npz'), allow_pickle=False)
FIVE = ('mean', 'std', 'energy', 'median', 'meanGrad')


def fixture_input(name):
    data = GEN.make_input(name)
    assert zlib.crc32(np.ascontiguousarray(data).tobytes()) == int(VEC[name + '_crc']), 'input generator drifted'
    return data, VEC[name + '_seg']


def test_fixture_inputs_cover_empty_odd_and_even_labels():
    for name in ('color', 'gray2d', 'gray3d'):
        data, seg = fixture_input(name)
        assert seg.dtype == np.int32 and seg.shape == data.shape[:seg.ndim]
        sizes = np.bincount(seg.ravel())
        assert sizes[GEN.EMPTY_LABEL] == 0 and np.any(sizes[sizes > 0] % 2 == 0) and np.any(sizes % 2 == 1)


@pytest.fixture
def no_host_filtering(monkeypatch):
    """the banks built first (their construction calls ndimage.gaussian_filter legitimately), then every host filtering entry
    point of the texture path raises"""
    from scipy import ndimage

    from pyimsegm_amd import descriptors as D
    for bank in ('normal', 'short'):
        D._select_bank(bank)

    def refuse(*args, **kwargs):
        raise AssertionError('host filtering on the texture path')

    monkeypatch.setattr(ndimage, 'convolve', refuse)
    monkeypatch.setattr(ndimage, 'gaussian_filter', refuse)
    monkeypatch.setattr(D, 'compute_img_filter_response3d', refuse)
    monkeypatch.setattr(D, 'image_subtract_gauss_smooth', refuse)
    return D


def _close_to(fts, names, tag):
    ref = VEC[tag + '_features']
    assert list(names) == VEC[tag + '_names'].tolist() and fts.shape == ref.shape
    np.testing.assert_allclose(fts, ref, rtol=1e-5, atol=1e-5 * np.abs(ref).max())


@pytest.mark.gpu
@pytest.mark.parametrize('tag,key', [('color_tlm', 'tLM'), ('color_short', 'tLM_short')])
def test_colour_texture_five_flags_follow_the_reference(tag, key, no_host_filtering):
    image, seg = fixture_input('color')
    fts, names = no_host_filtering.compute_selected_features_img2d(image, seg, {key: FIVE})
    _close_to(fts, names, tag)


@pytest.mark.gpu
def test_gray_texture_five_flags_follow_the_reference(no_host_filtering):
    D = no_host_filtering
    gray, seg = fixture_input('gray2d')
    _close_to(*D.compute_selected_features_gray2d(gray, seg, {'tLM_short': FIVE}), 'gray2d')
    vol, seg = fixture_input('gray3d')
    _close_to(*D.compute_selected_features_gray3d(vol, seg, {'tLM_short': FIVE}), 'gray3d')


@pytest.mark.gpu
def test_features_set_all_texture_runs_without_host_filtering(no_host_filtering):
    """FEATURES_SET_ALL's tLM (the default of compute_selected_features_color2d / _gray2d) in 2-D and 3-D"""
    D = no_host_filtering
    flags = D.FEATURES_SET_ALL['tLM']
    image, seg = fixture_input('color')
    fts, names = D.compute_selected_features_img2d(image, seg, {'tLM': flags})
    _close_to(fts, names, 'color_tlm')
    vol, seg = fixture_input('gray3d')
    fts, names = D.compute_selected_features_gray3d(vol, seg, {'tLM': flags})
    assert fts.shape == (seg.max() + 1, 20 * 5) and len(names) == fts.shape[1] and np.all(np.isfinite(fts))
    assert names[3] == 'tLM_sigma1.4-edge_median' and names[4] == 'tLM_sigma1.4-edge_meanGrad'


def _labels(shape, seed):
    """blocks of 9 x 13 pixels (2 slices in z), one pixel in ten moved to a random label, label 2 empty: odd and even counts"""
    rng = np.random.default_rng(seed)
    steps = (2, 9, 13)[-len(shape):]
    grid = tuple(-(-n // s) for n, s in zip(shape, steps))
    seg = np.ravel_multi_index(tuple(g // s for g, s in zip(np.indices(shape), steps)), grid)
    moved = rng.random(shape) < 0.1
    seg[moved] = rng.integers(0, seg.max() + 1, int(moved.sum()))
    seg[seg >= 2] += 1
    return seg.astype(np.int32)


def _host_median(values, seg, nb):
    out = np.full(nb, np.nan)
    for k in range(nb):
        sel = values[seg == k]
        if sel.size:
            out[k] = np.median(sel)
    return out


def _case(kind, rng):
    """(a factory of empty device sessions, image / volume, label map)"""
    from pyimsegm_amd import _hip
    if kind == '2d':
        shape = (57, 70)
        return (lambda: _hip.Image2D(*shape)), rng.random(shape + (3, )), _labels(shape, 1)
    shape = (3, 38, 45)
    return (lambda: _hip.Volume3D(*shape)), rng.random(shape), _labels(shape, 2)


@pytest.mark.gpu
@pytest.mark.parametrize('kind', ['2d', '3d'])
def test_response_median_and_gradient_equal_numpy_on_the_device_response(kind):
    from pyimsegm_amd import _hip, descriptors as D
    rng = np.random.default_rng(4)
    new_session, data, seg = _case(kind, rng)
    nb = int(seg.max()) + 1
    sizes = np.bincount(seg.ravel(), minlength=nb)
    assert sizes[2] == 0 and np.any(sizes % 2 == 1) and np.any(sizes[sizes > 0] % 2 == 0)
    filters, _ = D._select_bank('short')
    sess = new_session().upload(data).set_labels(seg).lm_prepare(150.)
    try:
        for battery in (filters[0], filters[2], filters[4]):
            norm = sess.lm_battery(battery, D.MAX_SIGNAL_RESPONSE)
            assert 0 < norm < np.inf
            mul = np.log(1 + norm) / 0.03
            resp = sess.get_response()
            v = (resp * mul) / norm                        # descriptors.py:1094
            median = sess.response_median(mul, norm)
            grad = sess.response_mean_gradient(mul, norm)
            if kind == '2d':
                ref_median = np.stack([_host_median(v[c], seg, nb) for c in range(3)], axis=1)
                slopes = np.stack([np.sum(np.gradient(v[c]), axis=0) for c in range(3)], axis=-1)
                ref_grad = D.hip_img2d_color_mean(np.ascontiguousarray(slopes), seg)
            else:
                ref_median = _host_median(v, seg, nb)
                slopes = np.array([np.sum(np.gradient(plane), axis=0) for plane in v])
                ref_grad = D.cython_img3d_gray_mean(slopes, seg)
            assert median.shape == ref_median.shape and np.all(np.isnan(median[2])) and np.all(np.isnan(ref_median[2]))
            present = ~np.isnan(ref_median)                # bit for bit: the same NaNs, the same int64 views everywhere else
            assert np.array_equal(np.isnan(median), ~present)
            assert np.array_equal(median[present].view(np.int64), ref_median[present].view(np.int64))
            np.testing.assert_allclose(grad, ref_grad, rtol=1e-6, atol=1e-6 * np.nanmax(np.abs(ref_grad)))
            with pytest.raises(_hip.HipError):
                sess.response_median(mul, 0.)
    finally:
        sess.close()


@pytest.mark.gpu
@pytest.mark.parametrize('kind', ['2d', '3d'])
def test_constant_image_gives_zeros(kind):
    from pyimsegm_amd import descriptors as D
    rng = np.random.default_rng(5)
    _, data, seg = _case(kind, rng)
    data = np.zeros_like(data)
    if kind == '2d':
        fts, names = D.compute_texture_desc_lm_img2d_clr(data, seg, FIVE, bank_type='short')
        assert fts.shape == (seg.max() + 1, 15 * 15)
    else:
        fts, names = D.compute_texture_desc_lm_img3d_val(data, seg, FIVE, bank_type='short')
        assert fts.shape == (seg.max() + 1, 15 * 5)
    assert len(names) == fts.shape[1] and not np.any(fts)


def _battery_outputs(sess, mul, div, order):
    out = {}
    for what in order:
        if what == 'stats':
            out[what] = np.concatenate([np.ravel(a) for a in sess.response_stats(mul, div)])
        elif what == 'median':
            out[what] = sess.response_median(mul, div)
        else:
            out[what] = sess.response_mean_gradient(mul, div)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize('kind', ['2d', '3d'])
def test_prepared_state_survives_median_and_gradient(kind):
    """response_median / response_mean_gradient / response_stats in every order leave the planes and the response: the next
    battery, without another lm_prepare, gives what a fresh session gives"""
    from pyimsegm_amd import descriptors as D
    filters, _ = D._select_bank('short')
    first, second = filters[1], filters[3]
    rng = np.random.default_rng(6)
    new_session, data, seg = _case(kind, rng)
    fresh = new_session().upload(data).set_labels(seg).lm_prepare(150.)
    norm = fresh.lm_battery(second, D.MAX_SIGNAL_RESPONSE)
    mul = np.log(1 + norm) / 0.03
    want = _battery_outputs(fresh, mul, norm, ('stats', 'median', 'grad'))
    want_resp = fresh.get_response()
    fresh.close()
    for order in itertools.permutations(('stats', 'median', 'grad')):
        sess = new_session().upload(data).set_labels(seg).lm_prepare(150.)
        try:
            n1 = sess.lm_battery(first, D.MAX_SIGNAL_RESPONSE)
            resp1 = sess.get_response()
            _battery_outputs(sess, np.log(1 + n1) / 0.03, n1, order)
            assert np.array_equal(sess.get_response(), resp1)
            assert np.isclose(sess.lm_battery(second, D.MAX_SIGNAL_RESPONSE), norm, rtol=1e-12, atol=0)
            assert np.array_equal(sess.get_response(), want_resp)
            got = _battery_outputs(sess, mul, norm, order)
        finally:
            sess.close()
        for what in want:
            np.testing.assert_array_equal(got[what], want[what], err_msg='%s after %r' % (what, order))


@pytest.mark.gpu
def test_sums_next_to_median_match_the_fused_call():
    """mean / std / energy columns of the battery-by-battery path (asked together with median) against the fused lm_features
    call (mean / std / energy only): mul and the fixed-point scale are derived differently, one float32 ulp inside std at most"""
    from pyimsegm_amd import descriptors as D
    image, seg = fixture_input('color')
    sums, sums_names = D.compute_texture_desc_lm_img2d_clr(image, seg, ('mean', 'std', 'energy'), bank_type='normal')
    full, full_names = D.compute_texture_desc_lm_img2d_clr(image, seg, ('mean', 'std', 'energy', 'median'), bank_type='normal')
    pick = [full_names.index(name) for name in sums_names]
    assert len(full_names) == len(sums_names) * 4 // 3
    np.testing.assert_allclose(full[:, pick], sums, rtol=1e-6, atol=1e-6 * np.abs(sums).max())
