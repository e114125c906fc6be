"""The cases of tests/pre_cases.py can catch a subtly wrong pre-processing kernel, shown on the CPU before any GPU sees them: the
oracle's own pre-processing (until now pinned to scikit-image through label maps only) lies inside the tolerance of the 80-bit
reference on every uint8 / float64 case; the float64 model of the device equals the oracle bit for bit there (and stands in for it
on the float32 cases); the model with ONE defect leaves the tolerance on every case the defect applies to; two restatements that
must not change a bit do not, and a permitted reordering stays inside; the two hand-written functions keep the ulp figures DESIGN.md
section 5 quotes.  ``pytest -s`` prints the per-case table and the defect summary of DESIGN.md."""
import numpy as np
import pytest

import pre_cases as P

pytestmark = pytest.mark.skipif(not P.LONGDOUBLE_OK, reason=P.LONGDOUBLE_REASON)

CASES = P.cases() if P.LONGDOUBLE_OK else ()
IDS = [c['id'] for c in CASES]
REAL_DEFECTS = [d for d in P.DEFECTS if d not in P.HARMLESS_EQUAL + P.HARMLESS_INSIDE]


def oracle_pre(oracle, c):
    """the oracle's planes [3, H, W]; the min-max scaling decided as superpixels.py:53-54 decides it"""
    x = P.widen(c['image'])
    vmin, vmax = float(x.min()), float(x.max())
    norm = (vmin, vmax) if P.scaled(c['normalize'], vmin, vmax) else None
    _, info = oracle.slic(np.array(c['image']), P.n_segments_of(c), c['compactness'], sigma=c['sigma'], normalize=norm, max_iter=1,
                          enforce_connectivity=False, return_internals=True)
    return info['pre'].reshape((3, ) + c['shape'])


def model(c, defect=None):
    return P.model64(c['image'], c['sigma'], c['normalize'], c['compactness'], defect)


@pytest.mark.parametrize('c', CASES, ids=IDS)
def test_oracle_and_model_against_the_reference(oracle, c):
    ref = P.reference(c['id'])
    mod = model(c)
    dev_model = P.rel_dev(mod, ref['ref'])
    print('%-42s S %.4g  yardstick %.2e  tolerance %.2e  model %.2e' % (c['id'], ref['scale'], ref['yardstick'], ref['tol'], dev_model))
    assert dev_model <= ref['tol'], (c['id'], dev_model, ref['tol'])
    assert float(np.abs(mod).max()) > 0
    if c['dtype'] != 'f32':
        pre = oracle_pre(oracle, c)
        dev = P.rel_dev(pre, ref['ref'])
        assert dev <= ref['tol'], (c['id'], dev, ref['tol'])
        assert np.array_equal(pre, mod), 'the model of the device is not the oracle on %s' % c['id']
    if c.get('gray'):
        check_gray(mod, ref)


def check_gray(planes, ref):
    """R = G = B.  The a and b planes are NOT zero under the definition: the rows of colorconv.py's matrix sum to 0.950456 and
    1.088754, not to the white point 0.95047 and 1.08883, so X / Xn = 0.9999853 Y and Z / Zn = 0.9999302 Y, and a = 500 (fx - fy),
    b = 200 (fy - fz) come out near -2.5e-3 fy and +4.7e-3 fy (times the blur and 1 / compactness): about 5e-5 S.  What holds is that
    they carry their sign everywhere, stay below 1e-4 S, and agree with the reference to the tolerance relative to S"""
    exact = ref['ref']
    assert np.all(exact[1] < 0) and np.all(exact[2] > 0) and float(np.abs(exact[1:]).max()) < 1e-4 * ref['scale']
    assert P.rel_dev(planes[1:], exact[1:]) * float(np.abs(exact[1:]).max()) / ref['scale'] <= ref['tol']


@pytest.mark.parametrize('defect', REAL_DEFECTS)
def test_one_defect_leaves_the_tolerance(defect):
    seen = []
    for c in CASES:
        if not P.applies(c, defect):
            continue
        ref = P.reference(c['id'])
        dev = P.rel_dev(model(c, defect), ref['ref'])
        assert dev > ref['tol'], 'case %s does not see the defect %r: %.3e within %.3e' % (c['id'], defect, dev, ref['tol'])
        seen.append(dev / ref['tol'])
    assert seen, 'no case is meant for the defect %r' % defect
    print('%-20s seen on %3d cases, deviation / tolerance %.0e .. %.0e' % (defect, len(seen), min(seen), max(seen)))


@pytest.mark.parametrize('defect', P.HARMLESS_EQUAL)
def test_restatements_that_change_no_bit(defect):
    """reflect_idx without its n == 1 return; the table index clamped instead of wrapped: the same planes on every case"""
    for c in CASES:
        assert np.array_equal(model(c, defect), model(c)), (c['id'], defect)


def test_a_permitted_reordering_stays_inside():
    """1 / compactness applied before the x pass rounds differently: other bits, inside the tolerance -- the comparison with the
    reference does not demand the oracle's bits"""
    differs = 0
    for c in CASES:
        ref = P.reference(c['id'])
        out = model(c, 'ratio-early')
        differs += not np.array_equal(out, model(c))
        assert P.rel_dev(out, ref['ref']) <= ref['tol'], c['id']
    assert differs, 'the reordering changed no bit anywhere: it shows nothing'
    print('ratio-early: other bits on %d of %d cases, inside the tolerance on all' % (differs, len(CASES)))


def test_hand_written_functions_keep_their_ulp_figures(oracle):
    """det_cbrt <= 1 ulp, det_pow24 <= 7 ulp of the true value on the domains the pre-processing uses (libm: 0.55 / 2.3), and the
    numpy transcriptions are the oracle's functions bit for bit"""
    ulps = P.function_ulps()
    print('ulp against 80 bit: det_cbrt %.2f (np.cbrt %.2f), det_pow24 %.2f (np.power %.2f)'
          % (ulps['det_cbrt'], ulps['np.cbrt'], ulps['det_pow24'], ulps['np.power']))
    assert ulps['det_cbrt'] <= P.ULP_BOUND['det_cbrt'] and ulps['det_pow24'] <= P.ULP_BOUND['det_pow24'], ulps
    lib = oracle.lib()
    points = np.random.RandomState(P.SEED).uniform(0.009, 1.3, 2000)
    assert all(lib.orc_det_cbrt(float(t)) == c for t, c in zip(points, P.det_cbrt(points)))
    points = points[points > 0.09]
    assert all(lib.orc_det_pow24(float(t)) == p for t, p in zip(points, P.det_pow24(points)))


def test_the_cases_cover_what_they_claim():
    by = {}
    for c in CASES:
        by.setdefault((c['shape'], c['sigma']), set()).add(c['dtype'])
    for shape in P.GRID_SHAPES:
        for sigma in P.SIGMAS:
            assert by[(shape, sigma)] >= {'u8', 'f32', 'f64'}
    assert {c['shape'] for c in CASES} >= set(P.GRID_SHAPES + P.OTHER_SHAPES)
    assert [P.radius_of(s) for s in P.SIGMAS] == [-1, 4, 5, 8, 9, 16] and P.radius_of(4.2) == 17
    assert all(len(np.unique(P.block_image()[..., ch])) == 256 for ch in range(3))
    routes = {(c['dtype'], r) for c in CASES if c['extremes'] for r in c['extremes']['routes']}
    assert routes == {('u8', 'vector'), ('u8', 'last-vector'), ('u8', 'tail'), ('f32', 'unrolled'), ('f32', 'remainder')}
    assert {c['image'].size % 16 for c in CASES if c['extremes'] and c['dtype'] == 'u8'} >= {1, 15}
    first, second = P.case('reuse-first')['image'], P.case('reuse-second')['image']
    assert first.min() < second.min() and second.max() < first.max() and first.shape == second.shape
    # both arms of both thresholds occur among the threshold pixels, and the value 0.04045 itself
    t, v = P.xyz_over_white80(P.case('threshold-f64')['image'], 0)
    assert np.any(v == P.LD(P.SRGB_T)) and np.any(v > P.LD(P.SRGB_T)) and np.any(v < P.LD(P.SRGB_T))
    near = (t > 0.0088) & (t < 0.0089)
    assert np.any(near & (t > P.LD(P.LAB_T))) and np.any(near & (t < P.LD(P.LAB_T)))
    z = P.xyz_over_white80(P.case('threshold-u8')['image'], 0)[0][2] * P.LD(1.08883)
    assert 5.8e-6 < float(z[z > 0].min()) < 5.9e-6
