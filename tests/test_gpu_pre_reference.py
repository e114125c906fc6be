"""csrc/slic_pre.hip pixel by pixel against the 80-bit reference of tests/pre_cases.py: k_minmax<float / double>, k_minmax_u8,
k_pre_fused<uint8_t / float / double> at radius -1, 4, 5 and 8, and the three-pass path (k_pre_lab_u8, k_pre_lab_f<float / double>,
k_blur_axis<0 / 1>, k_absmax_f64) at radius 9 and 16 and, through IMSEGM_PRE_3PASS, at the fused radii -- on images from 1 x 1 to
47 x 129, smaller than the radius, exactly one tile, one row and column into the next tiles.

Every case goes through ``Image2D(H, W).upload(img).slic(K <= 4, compactness, sigma, normalize, max_iter=1,
enforce_connectivity=False)``; ``get_lab()`` returns the planes and ``get_pre_scalars()`` the device's min, max and premax.
Tolerance per case (pre_cases.reference): 16 x what numpy's and scipy's float64 functions deviate from the reference on the same
image, floor 1e-14, relative to S = max |reference|.  The figures are printed (pytest -s) and tabulated in DESIGN.md section 5;
tests/test_pre_reference_host.py shows on the CPU that these cases see a subtly wrong kernel."""
import numpy as np
import pytest

import pre_cases as P

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not P.LONGDOUBLE_OK, reason=P.LONGDOUBLE_REASON)]

CASES = P.cases() if P.LONGDOUBLE_OK else ()
IDS = [c['id'] for c in CASES]
THREE_PASS = 'IMSEGM_PRE_3PASS'
#: fused against three-pass: sigma 0, 1.0, 1.2, 2.0 at 3 x 5, 17 x 65, 33 x 130 for the three dtypes (the grid), and the corner case
BOTH_PATHS = [c for c in CASES if (c['id'].startswith('grid-') and c['sigma'] in P.FUSED_SIGMAS) or c.get('corner')]

_RUNS = {}


def run(hip, c, path='default'):
    """(planes, (min, max, premax)) of a case on the device, once per process and path, read-only"""
    key = (c['id'], path)
    if key not in _RUNS:
        sess = hip.Image2D(*c['shape'])
        try:
            sess.upload(c['image'])
            sess.slic(P.n_segments_of(c), c['compactness'], sigma=c['sigma'], normalize=c['normalize'], max_iter=1,
                      enforce_connectivity=False)
            lab, scalars = sess.get_lab(), sess.get_pre_scalars()
        finally:
            sess.close()
        lab.setflags(write=False)
        _RUNS[key] = lab, scalars
    return _RUNS[key]


@pytest.fixture(scope='module')
def hip():
    from pyimsegm_amd import _hip
    _hip.default_context()
    return _hip


def check_scalars(c, lab, scalars):
    """min and max as numpy finds them; premax the largest |value| of the planes fetched, bit for bit"""
    vmin, vmax, premax = scalars
    assert vmin == float(c['image'].min()) and vmax == float(c['image'].max()), (c['id'], vmin, vmax)
    assert premax == float(np.abs(lab).max()), (c['id'], premax, float(np.abs(lab).max()))


@pytest.mark.parametrize('c', CASES, ids=IDS)
def test_planes_against_the_80_bit_reference(hip, c):
    ref = P.reference(c['id'])
    lab, scalars = run(hip, c)
    assert lab.shape == ref['ref'].shape
    dev = P.rel_dev(lab, ref['ref'])
    print('%-42s yardstick %.2e  tolerance %.2e  device %.2e' % (c['id'], ref['yardstick'], ref['tol'], dev))
    assert dev <= ref['tol'], (c['id'], dev, ref['tol'])
    if c.get('gray'):
        from test_pre_reference_host import check_gray
        check_gray(lab, ref)


@pytest.mark.parametrize('c', [c for c in CASES if c['dtype'] != 'f32'], ids=[c['id'] for c in CASES if c['dtype'] != 'f32'])
def test_planes_equal_the_oracle(hip, oracle, c):
    """the existing contract, at radius -1, 5, 8, 9 and 16 and on the tiny shapes"""
    from test_pre_reference_host import oracle_pre
    lab, _ = run(hip, c)
    assert np.array_equal(lab, oracle_pre(oracle, c)), 'pre-processed planes of %s differ from the oracle' % c['id']


@pytest.mark.parametrize('c', CASES, ids=IDS)
def test_min_max_and_premax(hip, c):
    lab, scalars = run(hip, c)
    check_scalars(c, lab, scalars)
    if c.get('corner'):              # the largest |value| is a negative b value in the one pixel of the last ragged tile
        h, w = c['shape']
        assert lab[2, h - 1, w - 1] < 0 and scalars[2] == -lab[2, h - 1, w - 1]


@pytest.mark.parametrize('c', BOTH_PATHS, ids=[c['id'] for c in BOTH_PATHS])
def test_fused_equals_three_pass(hip, monkeypatch, c):
    assert P.radius_of(c['sigma']) <= P.PF_MAXR
    fused, _ = run(hip, c)
    monkeypatch.setenv(THREE_PASS, '1')
    try:
        lab, scalars = run(hip, c, 'three-pass')
    finally:
        monkeypatch.delenv(THREE_PASS)
    assert np.array_equal(lab, fused), c['id']
    check_scalars(c, lab, scalars)
    ref = P.reference(c['id'])
    assert P.rel_dev(lab, ref['ref']) <= ref['tol']


def test_radius_17_is_refused_and_the_session_goes_on(hip):
    c = P.case('grid-17x65-s1-u8')
    assert P.radius_of(4.2) == 17
    sess = hip.Image2D(*c['shape'])
    try:
        sess.upload(c['image'])
        with pytest.raises(hip.HipError):
            sess.get_pre_scalars()                       # nothing to report before the first slic
        with pytest.raises(hip.HipError, match='radius'):
            sess.slic(4, c['compactness'], sigma=4.2, normalize=c['normalize'], max_iter=1, enforce_connectivity=False)
        sess.slic(4, c['compactness'], sigma=1.0, normalize=c['normalize'], max_iter=1, enforce_connectivity=False)
        lab, scalars = sess.get_lab(), sess.get_pre_scalars()
    finally:
        sess.close()
    assert np.array_equal(lab, run(hip, c)[0])
    check_scalars(c, lab, scalars)


def test_second_image_of_a_session(hip):
    """the extremes of the second image lie inside those of the first: right only if the reduction words came back to zero"""
    first, second = P.case('reuse-first'), P.case('reuse-second')
    sess = hip.Image2D(*first['shape'])
    try:
        got = []
        for c in (first, second, first):
            sess.upload(c['image'])
            sess.slic(4, c['compactness'], sigma=c['sigma'], normalize=c['normalize'], max_iter=1, enforce_connectivity=False)
            got.append((c, sess.get_lab(), sess.get_pre_scalars()))
    finally:
        sess.close()
    for c, lab, scalars in got:
        ref = P.reference(c['id'])
        assert P.rel_dev(lab, ref['ref']) <= ref['tol'], c['id']
        assert np.array_equal(lab, run(hip, c)[0]), c['id']
        check_scalars(c, lab, scalars)
