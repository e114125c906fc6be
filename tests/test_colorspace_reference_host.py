"""The cases of tests/colorspace_cases.py on the CPU: the float64 transcription of csrc/colorspace.hip (``model64``) against the
80-bit reference within the tolerance the GPU test uses, its hsv bit for bit numpy's, and every ``defect=`` of the transcription
seen by at least one case -- so the cases would see a kernel that is subtly wrong in that way.  Also: the two white-point
literals of the kernel are what the Python expression of ``data_io.rgb2luv`` evaluates to."""
import os
import re

import numpy as np
import pytest

import colorspace_cases as CC

pytestmark = pytest.mark.skipif(not CC.LONGDOUBLE_OK, reason=CC.LONGDOUBLE_REASON)

CASES = CC.cases() if CC.LONGDOUBLE_OK else ()
IDS = [c['id'] for c in CASES]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def passes(c, space, defect=None):
    """what the GPU test asserts of the device's image, asked of the transcription"""
    ref = CC.reference(c['id'], space)
    got = CC.model64(c['image'], space, defect=defect)
    if not CC.rel_dev(got, ref['ref']) <= ref['tol']:
        return False
    if space == 'hsv':
        return np.array_equal(got, CC.yardstick64(c['image'], 'hsv'))
    if space != 'hed':
        return np.array_equal(got, CC.model64(c['image'], space))
    return True


@pytest.mark.parametrize('c', CASES, ids=IDS)
def test_no_value_sits_on_a_threshold(c):
    CC.check_conditions(c)


@pytest.mark.parametrize('space', CC.SPACES)
@pytest.mark.parametrize('c', CASES, ids=IDS)
def test_model_against_the_80_bit_reference(c, space):
    ref = CC.reference(c['id'], space)
    got = CC.model64(c['image'], space)
    dev = CC.rel_dev(got, ref['ref'])
    print('%-20s %-3s yardstick %.2e  tolerance %.2e  model %.2e' % (c['id'], space, ref['yardstick'], ref['tol'], dev))
    assert got.shape == c['shape'] + (3, ) and got.dtype == np.float64
    assert dev <= ref['tol'], (c['id'], space, dev, ref['tol'])


@pytest.mark.parametrize('c', CASES, ids=IDS)
def test_model_hsv_is_numpys_bit_for_bit(c):
    from pyimsegm_amd.utilities.data_io import rgb2hsv
    with np.errstate(all='ignore'):
        expected = np.nan_to_num(rgb2hsv(c['image']))
    assert np.array_equal(CC.model64(c['image'], 'hsv'), expected)


def test_hue_wraps_as_numpys_floored_modulo():
    """the two pixels of the special case whose hue / 6 is a tiny negative number (-> 1.0) and -0 (-> +0)"""
    c = CC.case('special-f64')
    hue = CC.model64(c['image'], 'hsv')[0, :, 0]
    tiny = int(np.flatnonzero((c['image'][0] == (1., 0., 1e-300)).all(-1))[0])
    signed = int(np.flatnonzero((c['image'][0, :, 0] == .5) & np.signbit(c['image'][0, :, 1]))[0])
    assert hue[tiny] == 1.0
    assert hue[signed] == 0.0 and not np.signbit(hue[signed])


@pytest.mark.parametrize('defect', CC.DEFECTS)
def test_every_defect_is_seen(defect):
    failing = [(c['id'], space) for c in CASES for space in CC.SPACES if not passes(c, space, defect)]
    print(defect, failing[:6], len(failing))
    assert failing, defect


@pytest.mark.parametrize('defect', CC.HARMLESS_EQUAL)
def test_harmless_restatements_change_no_bit(defect):
    for c in CASES:
        assert np.array_equal(CC.model64(c['image'], 'hsv', defect=defect), CC.model64(c['image'], 'hsv')), (defect, c['id'])


def test_the_sound_model_passes_everything():
    assert all(passes(c, space) for c in CASES for space in CC.SPACES)


def test_white_point_literals_of_the_kernel():
    """LUV_U0 / LUV_V0 of csrc/colorspace.hip are the values numpy gives the expression of data_io.rgb2luv"""
    source = open(os.path.join(ROOT, 'pyimsegm_amd', 'csrc', 'colorspace.hip')).read()
    k = CC.constants()
    for name, key in (('LUV_U0', 'u0'), ('LUV_V0', 'v0')):
        literal = re.search(r'constexpr double %s = ([0-9.eE+-]+);' % name, source).group(1)
        assert float(literal) == k[key], (name, literal, k[key])
