"""csrc/volume.hip voxel by voxel against the 80-bit reference of tests/volpre_cases.py: the pre-processed plane of
``imsegm_volume_slic`` (``Volume3D.get_pre_scalar()``) and the centroid table its one update leaves (``Volume3D.get_centroids()``).

Every case goes through ``Volume3D(D, H, W).upload(vol).slic(K <= 4, compactness, sigma, spacing, max_iter=1,
enforce_connectivity=False)``, one session per case and path.  float64 planes (uint8, float64, uint16, int16 volumes): within
16 x scipy's own deviation from the reference, floor 1e-14, relative to S = max |reference|; ``premax`` bit for bit.  float32
planes: bit for bit outside the voxels the builder marked from the reference alone (an exact sum next to a float32 rounding
midpoint), two float32 spacings at S inside; and ``array_equal`` to scipy's float32 result.  ``pytest -s`` prints the figures of
DESIGN.md section 5; tests/test_volpre_reference_host.py shows on the CPU that these cases see a subtly wrong kernel.

Which kernel writes the plane of a case (launch_vol_preprocess / launch_vol_preprocess_f32; RZ, RY, RX = radii along z, y, x):

| cases                                   | kernels                                                                                  |
|-----------------------------------------|------------------------------------------------------------------------------------------|
| ``yxAB-3x33x65`` (A, B = 0 .. 4)        | k_vol_blur_z32<(5 A + B) % 5, 1>, k_vol_blur_yx32<A, B>: all 25 pairs, 2 x 2 tiles         |
| ``zR-3x33x64`` (R = 0 .. 4)             | k_vol_blur_z32<R, 4>, k_vol_blur_yx32<(R + 2) % 5, (R + 3) % 5>                            |
| ``small-*``, ``slice-*``, ``tile-*``, ``ragged-*``, ``short-*`` | k_vol_blur_z32<4, 1 or 4>, k_vol_blur_yx32<4, 4>: axes shorter than the radius, one tile, three tile columns |
| ``chunk-DxHxW-rR`` (R = 4, 1)           | k_vol_blur_z32<R, 4> over 2, 2, 3 and 1 z chunks (17 + 16, 18 + 17, 3 x 16, 31), k_vol_blur_yx32<4, 4> |
| ``r8-*``, ``r16-*``                     | k_vol_blur_r32<0>, <1>, <2>: interior shortcut on x (5x9x40), z (40x5x9), y (5x40x9), reflected branch on the others |
| ``*-3pass`` (IMSEGM_PRE_3PASS)          | k_vol_blur_r32<0 / 1 / 2> at radii 0 .. 4, both branches on every axis of 3x33x65          |
| ``u8-*``                                | k_vol_to_f64<uint8_t>, k_vol_blur<0 / 1 / 2> (radius -1 .. 16), launch_absmax_f64        |
| ``f64-*``, ``u16-*``, ``i16-*``         | k_vol_to_f64<double> (offset, scale of img_as_float), k_vol_blur<0 / 1 / 2>, launch_absmax_f64 |
| ``upd-f32-*``                           | k_vol_assign_f32<true> (boxes), k_vol_update_f32_lane                                    |
| ``upd-f64-*``                           | k_vol_assign<true> (fixed-point sums), k_vol_centroid_finalize                           |
"""
import numpy as np
import pytest

import volpre_cases as V

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not V.LONGDOUBLE_OK, reason='numpy.longdouble is not an 80-bit type here')]

CASES = V.cases() if V.LONGDOUBLE_OK else ()
IDS = [c['id'] for c in CASES]
UPDATES = V.update_cases() if V.LONGDOUBLE_OK else ()
THREE_PASS = 'IMSEGM_PRE_3PASS'

_RUNS = {}


def slic(sess, c, max_iter=1, spacing=None):
    return sess.slic(c['n_segments'], c['compactness'], sigma=c['sigma'], spacing=spacing or c['spacing'], max_iter=max_iter,
                     enforce_connectivity=False)


def run(hip, c, monkeypatch=None):
    """(plane, premax) of a case on the device, once per process (a ``-3pass`` case: under IMSEGM_PRE_3PASS), read-only"""
    if c['id'] not in _RUNS:
        if c['three_pass']:
            monkeypatch.setenv(THREE_PASS, '1')
        sess = hip.Volume3D(*c['shape'])
        try:
            sess.upload(c['volume'])
            slic(sess, c)
            plane, premax = sess.get_pre_scalar()
        finally:
            sess.close()
            if c['three_pass']:
                monkeypatch.delenv(THREE_PASS)
        plane.setflags(write=False)
        _RUNS[c['id']] = plane, premax
    return _RUNS[c['id']]


@pytest.fixture(scope='module')
def hip():
    from pyimsegm_amd import _hip
    _hip.default_context()
    return _hip


def check_plane(c, plane, premax):
    ref = V.reference(c['id'])
    if V.is_f32(c):
        assert plane.dtype == np.float32 and premax is None
        differ, worst = V.check32(plane, ref)
        return 'marked %d of %d  scipy differs on %d  device differs on %d (%.2g spacings at S)' % (
            ref['n_marked'], plane.size, ref['yardstick'], differ, worst)
    assert plane.dtype == np.float64 and plane.shape == ref['ref'].shape
    dev = V.rel_dev(plane, ref['ref'])
    assert dev <= ref['tol'], (c['id'], dev, ref['tol'])
    assert premax == float(np.abs(plane).max()), (c['id'], premax, float(np.abs(plane).max()))
    return 'yardstick %.2e  tolerance %.2e  device %.2e' % (ref['yardstick'], ref['tol'], dev)


@pytest.mark.parametrize('c', CASES, ids=IDS)
def test_plane_against_the_80_bit_reference(hip, monkeypatch, c):
    plane, premax = run(hip, c, monkeypatch)
    print('%-26s %s' % (c['id'], check_plane(c, plane, premax)))


@pytest.mark.parametrize('c', [c for c in CASES if V.is_f32(c)], ids=[c['id'] for c in CASES if V.is_f32(c)])
def test_float32_plane_equals_scipy(hip, monkeypatch, c):
    """the kernels state scipy's order: centre tap first, then the pairs from the farthest in"""
    assert np.array_equal(run(hip, c, monkeypatch)[0], V.reference(c['id'])['scipy']), c['id']


@pytest.mark.parametrize('c', [c for c in CASES if not V.is_f32(c)], ids=[c['id'] for c in CASES if not V.is_f32(c)])
def test_premax(hip, c):
    plane, premax = run(hip, c)
    assert premax == float(np.abs(plane).max()) and premax > 0


@pytest.mark.parametrize('c', [c for c in CASES if c['three_pass']], ids=[c['id'] for c in CASES if c['three_pass']])
def test_fast_path_equals_three_passes(hip, monkeypatch, c):
    assert V.fast_path(c)
    fast = run(hip, V.case(c['id'][:-len('-3pass')]))[0]
    assert np.array_equal(run(hip, c, monkeypatch)[0], fast), c['id']


def test_radius_17_is_refused_and_the_session_goes_on(hip):
    c = V.case('yx24-3x33x65')
    assert int(4 * V.sigma_over_spacing(np.float32, 1., (V.REFUSED_SPACING, ) * 3)[0] + 0.5) == 17
    image = hip.Image2D(8, 8)
    try:
        with pytest.raises(hip.HipError, match='volume session'):
            hip.Volume3D.get_pre_scalar(image)
        with pytest.raises(hip.HipError, match='volume session'):
            hip.Volume3D.get_centroids(image)
    finally:
        image.close()
    sess = hip.Volume3D(*c['shape'])
    try:
        sess.upload(c['volume'])
        with pytest.raises(hip.HipError, match='slic has not been run'):
            sess.get_pre_scalar()                             # nothing to report before the first slic
        with pytest.raises(hip.HipError, match='slic has not been run'):
            sess.get_centroids()
        with pytest.raises(hip.HipError, match='radius > 16'):
            slic(sess, c, spacing=(1., V.REFUSED_SPACING, 1.))
        slic(sess, c)
        plane, premax = sess.get_pre_scalar()
    finally:
        sess.close()
    assert premax is None and np.array_equal(plane, run(hip, c)[0])


def test_two_volumes_through_one_session(hip):
    """a float32 volume, then a float64 one of the same shape (the plane buffer changes its type), then the first again"""
    first, second = V.case('reuse-f32'), V.case('reuse-f64')
    sess = hip.Volume3D(*first['shape'])
    try:
        got = []
        for c in (first, second, first):
            sess.upload(c['volume'])
            slic(sess, c)
            got.append((c, ) + sess.get_pre_scalar())
    finally:
        sess.close()
    for c, plane, premax in got:
        check_plane(c, plane, premax)
        fresh = run(hip, c)
        assert plane.dtype == fresh[0].dtype and np.array_equal(plane, fresh[0]) and premax == fresh[1], c['id']


# ---- the centroid update, on the device's own plane and assignment -----------------------------------------------------------
def run_update(hip, c):
    """(plane, premax, labels of the first sweep, centroids after the one update).  ``max_iter=2`` is sweep, update, sweep: no
    update follows the last sweep, so the table read back is what the update formed from the FIRST sweep's assignment -- which is
    the label map of a ``max_iter=1`` run of the same upload"""
    key = ('update', c['id'])
    if key not in _RUNS:
        sess = hip.Volume3D(*c['shape'])
        try:
            sess.upload(c['volume'])
            slic(sess, c, max_iter=1)
            plane, premax = sess.get_pre_scalar()
            labels = sess.get_labels().reshape(c['shape'])
            initial = sess.get_centroids()
            slic(sess, c, max_iter=2)
            centroids = sess.get_centroids()
            assert np.array_equal(sess.get_pre(), plane)
        finally:
            sess.close()
        _RUNS[key] = plane, premax, labels, initial, centroids
    return _RUNS[key]


@pytest.mark.parametrize('c', UPDATES, ids=[c['id'] for c in UPDATES])
def test_centroid_update(hip, c):
    plane, premax, labels, initial, cen = run_update(hip, c)
    count = cen.shape[0]
    assert labels.min() >= 0 and labels.max() < count and initial.shape == cen.shape
    assert np.all(initial[:, 3] == 0)                          # after max_iter=1: the grid, no update
    empty = sorted(set(range(count)) - set(np.unique(labels).tolist()))
    for k in empty:                                           # a centroid without members keeps its previous position
        assert np.array_equal(cen[k, :3], initial[k, :3]), (c['id'], k)
    if V.is_f32(c):
        assert cen.dtype == np.float32 and premax is None
        ref = V.update_reference32(plane, labels, count)
        bad = [k for k in ref if not np.array_equal(ref[k], cen[k])]
        print('%-24s K %d (%d without members): %d centroids with other bits' % (c['id'], count, len(empty), len(bad)))
        assert not bad, (c['id'], bad[:5], [(ref[k], cen[k]) for k in bad[:2]])
    else:
        assert cen.dtype == np.float64
        worst = 0.
        for k, (mean, bound) in V.update_bound64(plane, labels, count, premax).items():
            assert all(cen[k, j] == float(mean[j]) for j in range(3)), (c['id'], k, cen[k], mean)
            err = float(abs(V.LD(cen[k, 3]) - mean[3]))
            assert err <= bound, (c['id'], k, err, bound)
            worst = max(worst, err / bound)
        print('%-24s K %d (%d without members): f = %d, worst value error / bound %.3f' % (c['id'], count, len(empty), V.fix_bits_of(premax), worst))
