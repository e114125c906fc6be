"""The cases of tests/volpre_cases.py can catch a subtly wrong volume pre-processing or centroid update, shown on the CPU before any
GPU sees them.  The numpy model of the device (volpre_cases.model32 / model64: fp64 accumulation in the kernels' order, float32
stores per pass, the z chunks, the ``ahead`` plane, the 64 x 32 tiles with their ``extra`` columns and the interior shortcut as index
maps) passes every case and, on the float32 cases, equals scipy bit for bit; with ONE defect it leaves the tolerance (float64
plane) or the bit comparison (float32 plane) on every case the defect applies to.  The builder's own conditions run here too: at
most 0.5 % of a float32 case's voxels are marked, and scipy differs from the 80-bit reference inside the marked set only.

The oracle: ``oracle.slic(..., multichannel=False, return_internals=True)`` exposes the float64 plane, which is held to the
reference below.  ``oracle.slic_gray3d_float32`` computes its float32 plane but does not return it, so the float32 oracle is left
out here (the model stands in for it, and is pinned to scipy).

``pytest -s`` prints the per-case table and the defect summary of DESIGN.md section 5."""
import numpy as np
import pytest

import volpre_cases as V

pytestmark = pytest.mark.skipif(not V.LONGDOUBLE_OK, reason='numpy.longdouble is not an 80-bit type here')

CASES = V.cases() if V.LONGDOUBLE_OK else ()
IDS = [c['id'] for c in CASES]
UPDATES = V.update_cases() if V.LONGDOUBLE_OK else ()


def model(c, defect=None):
    if V.is_f32(c):
        return V.model32(c, 'three-pass' if c['three_pass'] else 'default', defect)
    return V.model64(c, defect)


def outside(c, got, ref):
    """(does ``got`` fail the case's check, a figure for the table)"""
    if V.is_f32(c):
        try:
            V.check32(got, ref)
        except AssertionError:
            return True, float(np.sum(got != ref['ref'])) / got.size
        return False, 0.
    dev = V.rel_dev(got, ref['ref'])
    return dev > ref['tol'], dev / ref['tol']


@pytest.mark.parametrize('c', CASES, ids=IDS)
def test_model_against_the_reference_and_scipy(c):
    ref = V.reference(c['id'])                  # (asserts the cap on marked voxels and the yardstick inside the marked set)
    got = model(c)
    assert float(np.abs(got).max()) > 0
    if V.is_f32(c):
        differ, worst = V.check32(got, ref)
        print('%-26s radii %-12s S %.4g  marked %d of %d  scipy differs on %d  model differs on %d (%.2g spacings)'
              % (c['id'], V.radii_of(c), ref['scale'], ref['n_marked'], got.size, ref['yardstick'], differ, worst))
        assert np.array_equal(got, ref['scipy']), 'the model of the device is not scipy on %s' % c['id']
    else:
        dev = V.rel_dev(got, ref['ref'])
        print('%-26s radii %-12s S %.4g  yardstick %.2e  tolerance %.2e  model %.2e' % (c['id'], V.radii_of(c), ref['scale'], ref['yardstick'], ref['tol'], dev))
        assert dev <= ref['tol'], (c['id'], dev, ref['tol'])


@pytest.mark.parametrize('c', [c for c in CASES if not V.is_f32(c)], ids=[c['id'] for c in CASES if not V.is_f32(c)])
def test_oracle_plane_against_the_reference(oracle, c):
    ref = V.reference(c['id'])
    _, info = oracle.slic(np.array(c['volume']), c['n_segments'], c['compactness'], sigma=c['sigma'], spacing=c['spacing'], multichannel=False,
                          max_iter=1, enforce_connectivity=False, return_internals=True)
    pre = info['pre'].reshape(c['shape'])
    dev = V.rel_dev(pre, ref['ref'])
    assert dev <= ref['tol'], (c['id'], dev, ref['tol'])
    assert np.array_equal(pre, model(c)), 'the model of the device is not the oracle on %s' % c['id']


@pytest.mark.parametrize('c', [c for c in CASES if c['three_pass']], ids=[c['id'] for c in CASES if c['three_pass']])
def test_model_fast_path_equals_three_passes(c):
    assert V.fast_path(c)
    assert np.array_equal(V.model32(c, 'default'), V.model32(c, 'three-pass'))


@pytest.mark.parametrize('defect', V.DEFECTS)
def test_one_defect_is_seen(defect):
    seen = []
    for c in CASES:
        if not V.applies(c, defect):
            continue
        bad, figure = outside(c, model(c, defect), V.reference(c['id']))
        assert bad, 'case %s does not see the defect %r' % (c['id'], defect)
        seen.append((V.is_f32(c), figure))
    assert seen, 'no case is meant for the defect %r' % defect
    f32 = [f for is32, f in seen if is32]
    f64 = [f for is32, f in seen if not is32]
    print('%-16s seen on %3d cases' % (defect, len(seen)) +
          ('; float32: %d, share of voxels with other bits %.1e .. %.1e' % (len(f32), min(f32), max(f32)) if f32 else '') +
          ('; float64: %d, deviation / tolerance %.0e .. %.0e' % (len(f64), min(f64), max(f64)) if f64 else ''))


def test_the_cases_reach_what_they_claim():
    f32 = [c for c in CASES if V.is_f32(c) and not c['three_pass']]
    fast = [c for c in f32 if V.fast_path(c)]
    assert {V.radii_of(c)[1:] for c in fast} >= {(ry, rx) for ry in range(5) for rx in range(5)}
    assert {(V.radii_of(c)[0], V.z_chunks(c['shape'])[0]) for c in fast} >= {(r, vec) for r in range(5) for vec in (1, 4)}
    chunks = {c['id']: [z1 - z0 for z0, z1 in V.z_chunks(c['shape'])[1]] for c in fast}
    assert chunks['chunk-33x5x8-r4'] == [17, 16] and chunks['chunk-35x6x12-r1'] == [18, 17]
    assert chunks['chunk-48x4x4-r4'] == [16, 16, 16] and chunks['chunk-31x5x8-r4'] == [31]
    slow = [c for c in f32 if not V.fast_path(c)]
    assert {V.radii_of(c) for c in slow} == {(8, 8, 8), (16, 16, 16)}
    for axis in range(3):                                       # k_vol_blur_r32<AXIS>: positions inside and at the border
        lens = [(c['shape'][axis], V.radii_of(c)[axis]) for c in slow + [c for c in CASES if c['three_pass']]]
        assert any(n > 2 * r for n, r in lens) and any(r >= 1 for n, r in lens)
    other = [c for c in CASES if not V.is_f32(c)]
    assert {c['dtype'] for c in other} >= {'u8', 'f64', 'u16', 'i16'}
    assert {r for c in other for r in V.radii_of(c)} >= {-1, 0, 1, 3, 4, 8, 16}
    assert any(c['volume'].min() < 0 and c['volume'].max() > 1 for c in other if c['dtype'] == 'f64')
    assert any(c['volume'].min() < 0 for c in f32)
    assert any(c['volume'].size % 256 for c in other)
    assert V.sigma_over_spacing(np.float32, 1., (V.REFUSED_SPACING, ) * 3)[0] * 4 + 0.5 >= 17
    assert max(c['volume'].size for c in CASES + UPDATES) <= 150000


# ---- centroid update ---------------------------------------------------------------------------------------------------------
def _update_input(c):
    plane = model(c)
    labels, count = V.grid_assignment(plane.astype(np.float64), c['n_segments'], c['spacing'])
    return plane, labels, count


@pytest.mark.parametrize('c', [c for c in UPDATES if V.is_f32(c)], ids=[c['id'] for c in UPDATES if V.is_f32(c)])
def test_update_model_float32_and_its_defects(c):
    """the lane's walk (bounding box, rounds of four quads, +0.0f for every voxel that is not a member) gives the bits of the plain
    sequential loop; without a row's last partial quad, or summed by pairs, it does not"""
    plane, labels, count = _update_input(c)
    ref = V.update_reference32(plane, labels, count)
    got = V.update_model32(plane, labels, count)
    assert ref.keys() == got.keys() and len(ref) >= 2
    assert all(np.array_equal(ref[k], got[k]) for k in ref)
    for defect in V.UPDATE_DEFECTS:
        bad = V.update_model32(plane, labels, count, defect)
        differ = sum(not np.array_equal(ref[k], bad[k], equal_nan=True) for k in ref)
        print('%-24s %-13s other bits on %d of %d centroids' % (c['id'], defect, differ, len(ref)))
        assert differ, (c['id'], defect)


@pytest.mark.parametrize('c', [c for c in UPDATES if not V.is_f32(c)], ids=[c['id'] for c in UPDATES if not V.is_f32(c)])
def test_update_model_float64_inside_its_bound(c):
    plane, labels, count = _update_input(c)
    premax = float(np.abs(plane).max())
    got = V.update_model64(plane, labels, count, premax)
    worst = 0.
    for k, (mean, bound) in V.update_bound64(plane, labels, count, premax).items():
        assert all(got[k][j] == float(mean[j]) for j in range(3)), (c['id'], k)           # exact sums, one rounding
        err = float(abs(V.LD(got[k][3]) - mean[3]))
        assert err <= bound, (c['id'], k, err, bound)
        worst = max(worst, err / bound)
        # a member truncated one bit coarser (f - 1) may leave the bound; a member dropped does
        zz, yy, xx = np.nonzero(labels == k)
        if len(zz) > 1:
            dropped = float(plane[zz[:-1], yy[:-1], xx[:-1]].astype(V.LD).sum() / V.LD(len(zz)))
            assert abs(V.LD(dropped) - mean[3]) > bound or plane[zz[-1], yy[-1], xx[-1]] == 0
    print('%-24s f = %d, worst error / bound %.3f' % (c['id'], V.fix_bits_of(premax), worst))
