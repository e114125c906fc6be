"""The cases of tests/texture_cases.py can catch a subtly wrong texture kernel, shown on the CPU from the 80-bit reference alone --
before any GPU sees them: scipy agrees with the reference to the deviation the tolerances are 16 x of; the split of every case is
the one its kernels need; and a float64 numpy restatement of the device's evaluation (dense sums, mirror pairs, separable passes,
merge, clip, sum of squares) with ONE defect leaves the tolerance by a factor of 100 at least on every case the defect applies to,
while the same restatement without a defect stays inside."""
import numpy as np
import pytest

import texture_cases as X

pytestmark = pytest.mark.skipif(not X.LONGDOUBLE_OK, reason=X.LONGDOUBLE_REASON)

MARGIN = 100
PADS = {'nearest': 'edge', 'mirror': 'reflect'}          # numpy.pad's names: 'edge' repeats the border, 'reflect' is whole-sample


def model64(planes, c, clip=1e6, defect=None):
    """the response of a case in float64 numpy, evaluated the way the device does (the host's own split): dense kernels as shifted
    sums (the second kernel of a mirror pair as m x the mirrored first one), separable kernels as an x pass and a y pass per
    component, the two merged by a maximum, the clip on the upper side -- with one ``defect`` or none"""
    from pyimsegm_amd._hip import Image2D
    if defect == 'seam':             # input column 64 read as column 63 for the outputs right of the seam
        out = model64(planes, c, clip)
        moved = np.array(planes)
        moved[..., 64] = moved[..., 63]
        out[..., 64:] = model64(moved, c, clip)[..., 64:]
        return out
    bat = X.battery(c['battery'])
    if defect == 'correlation':      # (the host flips: a battery flipped beforehand comes out unflipped)
        bat = bat[:, ::-1, ::-1]
    separable = c['route'] == 'features' and c['separable']
    weights, n_dense, taps, groups, rank, _, parity = Image2D._split_battery(bat, separable, separable, False)
    pad = PADS.get(defect, 'symmetric')
    dense = [weights[:, :, j].T for j in range(n_dense)]
    parts = []
    pairs = Image2D._mirror_pairs(dense) if (separable and c['mirror'] and parity and bat.shape[1] == 33 and n_dense % 2 == 0) else None
    if pairs is not None:
        for i, (a, _, m) in enumerate(pairs):
            if defect == 'mirror-sign' and i == 0:
                m = -m
            parts += [X.shifted_sum(planes, dense[a], pad, np.float64), X.shifted_sum(planes, m * dense[a][:, ::-1], pad, np.float64)]
    else:
        assert defect != 'mirror-sign'
        parts = [X.shifted_sum(planes, k, pad, np.float64) for k in dense]
    seps = []
    for g in range(groups):
        comps = range(1 if defect == 'rank1' else rank)
        seps.append(sum(X.shifted_sum(X.shifted_sum(planes, taps[g, i, 0][None, :], pad, np.float64), taps[g, i, 1][:, None], pad,
                                      np.float64) for i in comps))
    if defect == 'overwrite':
        assert seps and parts
        parts = []
    resp = np.max(parts + seps, axis=0)
    if defect == 'clip-abs':
        return np.where(np.abs(resp) > clip, clip, resp)
    return X.clip_upper(resp, clip)


def applies(c, defect):
    """the cases a defect can show on (decided by the split and the battery alone)"""
    bat = X.battery(c['battery'])
    exp = c['expect'] if c['route'] == 'features' else (c['expect'], 0, 0, 0)
    if defect == 'correlation':          # an odd battery: the flipped kernel is the negated one
        return all(np.abs(k[::-1, ::-1] + k).max() <= 1e-12 * np.abs(k).max() for k in bat)
    if defect == 'mirror-sign':
        return abs(exp[1]) == 2
    if defect == 'rank1':
        return exp[3] == 2
    if defect == 'overwrite':
        return exp[0] > 0 and exp[2] > 0
    return True                          # the border modes, the seam (W = 83 > 64)


@pytest.fixture(scope='module')
def planes():
    out = X.host_planes(X.SHAPE)
    out.setflags(write=False)
    return out


def test_the_split_of_every_case_is_the_listed_one():
    from pyimsegm_amd._hip import Image2D
    reached = set()
    for c in X.CASES:
        assert X.split_of(c) == c['expect'], (c['id'], X.split_of(c))
        assert X.sep_truncation(X.battery(c['battery'])) <= 1e-14, c['id']          # (measured 3e-17 .. 9e-16)
        reached |= set(c['kernels'])
    want = {'k_conv_battery<%d>' % n for n in (1, 2, 4, 6, 8)} | {'k_conv_battery_sym<%d>' % n for n in (1, 2, 4, 6, 8)}
    want |= {'k_conv_battery_quad<%d,16>' % n for n in (1, 2, 3, 4)} | {'k_sep_battery_tall', 'k_sep_battery<33>', 'k_sep_battery<0>'}
    assert reached == want
    # both signs of the symmetric and of the quad form
    signs = {(abs(c['expect'][1]), np.sign(c['expect'][1])) for c in X.CASES if c['route'] == 'features' and c['expect'][1]}
    assert signs == {(1, -1), (1, 1), (2, -1), (2, 1)}
    # no rank <= 2 kernel among the non-axis orientations; no quad form at another side
    for name in ('sym1-edge', 'sym4-bar', 'sym8-edge', 'sym8-bar', 'quad4-edge', 'quad4-bar'):
        assert X.CASE[name]['expect'][2] == 0
    packed = Image2D._pack_bank(list(X.banks()['side17']), True, True)
    assert packed['radius'] == 8 and sorted(packed['parity'].tolist()) == [-1, 0, 0, 0, 1]
    # the five batteries of one sigma: five jobs of the separable launch
    assert Image2D._pack_bank([X.battery(n) for n in X.ONE_SIGMA], True, True)['groups'].tolist() == [2, 2, 1, 1, 1]
    assert set(X.BORDER_CASES + X.CLIP_CASES) <= set(X.CASE)


@pytest.mark.parametrize('name', [c['id'] for c in X.CASES])
def test_reference_scipy_and_the_restatement_agree(name, planes):
    """scipy.ndimage.convolve (mode 'reflect') and the defect-free restatement lie within the case's tolerance of the reference"""
    from pyimsegm_amd import descriptors as D
    c = X.CASE[name]
    ref = X.reference(c['battery'], planes)
    tol = X.tolerance(c, ref)
    scipy_dev = X.rel_dev(D.compute_img_filter_response3d(planes, X.battery(c['battery'])), ref['raw'], ref['scale'])
    model_dev = X.rel_dev(model64(planes, c), ref['raw'], ref['scale'])
    print('%s: scipy %.3e restatement %.3e tolerance %.3e' % (name, scipy_dev, model_dev, tol))
    assert scipy_dev <= ref['scipy'] <= X.FLOOR / X.FACTOR and tol <= 2 * X.FLOOR          # the floor governs; scipy is far inside
    assert model_dev <= tol


@pytest.mark.parametrize('defect', ['nearest', 'mirror', 'correlation', 'mirror-sign', 'rank1', 'overwrite', 'seam'])
def test_one_defect_leaves_the_tolerance(defect, planes):
    cases = [c for c in X.CASES if applies(c, defect)]
    assert len(cases) >= 3, defect
    if defect == 'correlation':
        assert any(abs(c['expect'][1]) == 2 for c in cases if c['route'] == 'features')
    for c in cases:
        ref = X.reference(c['battery'], planes)
        tol = X.tolerance(c, ref)
        dev = X.rel_dev(model64(planes, c, defect=defect), ref['raw'], ref['scale'])
        print('%s on %s: %.3e = %.1e x tolerance' % (defect, c['id'], dev, dev / tol))
        assert dev >= MARGIN * tol, (defect, c['id'], dev, tol)


@pytest.mark.parametrize('shape', X.BORDER_SHAPES, ids=lambda s: '%dx%d' % s)
def test_border_defects_show_at_the_border_shapes(shape):
    """'nearest' and 'mirror' (the off-by-one of the reflection) at the shapes whose border is crossed more than once; the seam where
    there is one"""
    small = X.host_planes(shape)
    for name in X.BORDER_CASES:
        c = X.CASE[name]
        ref = X.reference(c['battery'], small)
        tol = X.tolerance(c, ref)
        assert X.rel_dev(model64(small, c), ref['raw'], ref['scale']) <= tol, name
        for defect in ['nearest', 'mirror'] + (['seam'] if shape[1] > 64 else []):
            dev = X.rel_dev(model64(small, c, defect=defect), ref['raw'], ref['scale'])
            print('%s on %s at %r: %.3e = %.1e x tolerance' % (defect, name, shape, dev, dev / tol))
            assert dev >= MARGIN * tol, (defect, name, shape)


@pytest.mark.parametrize('name', X.CLIP_CASES)
def test_the_clip_on_the_absolute_value_shows(name, planes):
    c = X.CASE[name]
    ref = X.reference(c['battery'], planes)
    tol = X.tolerance(c, ref)
    raw = ref['raw']
    clip = float(np.median(raw[raw > 0]))
    want = X.clip_upper(raw, clip)
    margin = tol * ref['scale']
    assert (raw > clip + margin).mean() > 0.1 and (raw < -clip - margin).sum() >= 10    # the clip is alive; negatives beyond it exist
    assert X.rel_dev(model64(planes, c, clip), want, ref['scale']) <= tol
    dev = X.rel_dev(model64(planes, c, clip, defect='clip-abs'), want, ref['scale'])
    print('clip on |r| on %s: %.3e = %.1e x tolerance' % (name, dev, dev / tol))
    assert dev >= MARGIN * tol


def test_a_lost_ragged_tile_row_shows_in_the_sum_of_squares(planes):
    """the rows of the last, ragged tile row (16-row tiles of the dense kernels, 96-row tiles of k_sep_battery_tall) left out of the
    sum of squares, against the tolerance of the norm: 16 x numpy's fp64 deviation from the 80-bit sum, floor 1e-13"""
    shapes = [X.SHAPE] + [s for s in X.BORDER_SHAPES if s[0] % 16]
    assert len(shapes) == 4
    for shape in shapes:
        src = planes if shape == X.SHAPE else X.host_planes(shape)
        for name in ('quad1-edge', 'tall-lap'):
            resp = X.reference(X.CASE[name]['battery'], src)['raw'].astype(np.float64)
            ssq = X.sumsq80(resp)
            numpy_dev = abs(float((X.LD(np.sum(resp**2)) - ssq) / ssq))
            tol = X.rule(numpy_dev)
            for tile in (16, 96):
                kept = (shape[0] // tile) * tile if shape[0] % tile else shape[0] - 1          # (no ragged row: the last row itself)
                dev = abs(float((X.sumsq80(resp[:, :kept]) - ssq) / ssq))
                print('%s at %r, %d-row tiles: numpy %.3e, without the last tile row %.3e' % (name, shape, tile, numpy_dev, dev))
                assert numpy_dev <= X.FLOOR / X.FACTOR and dev >= MARGIN * tol


@pytest.mark.parametrize('shape,dtype', X.HIGHPASS_IMAGES, ids=lambda v: 'x'.join(map(str, v)) if isinstance(v, tuple) else v)
def test_highpass_reference_agrees_with_scipy_and_sees_a_missing_channel_pass(shape, dtype):
    from scipy import ndimage
    image = X.noise(tuple(shape) + (3, ), dtype)
    ref = X.highpass80(image)
    scale = float(np.abs(image).max())
    scipy_dev = X.rel_dev(X.highpass_scipy(image), ref, scale)
    tol = X.rule(scipy_dev)
    lost = np.rollaxis(image - ndimage.gaussian_filter(image.astype(float), (150, 150, 0)), -1, 0)
    dev = X.rel_dev(lost, ref, scale)
    print('high-pass %r %s: scipy %.3e tolerance %.3e; without the channel pass %.3e' % (shape, dtype, scipy_dev, tol, dev))
    assert scipy_dev <= X.FLOOR / X.FACTOR and dev >= MARGIN * tol
    # the border modes of the long blur
    for mode in ('nearest', 'mirror'):
        other = np.rollaxis(image - ndimage.gaussian_filter(image.astype(float), 150, mode=mode), -1, 0)
        dev = X.rel_dev(other, ref, scale)
        print('  border %s: %.3e' % (mode, dev))
        assert dev >= MARGIN * tol


@pytest.mark.parametrize('shape,dtype', X.HIGHPASS_VOLUMES, ids=lambda v: 'x'.join(map(str, v)) if isinstance(v, tuple) else v)
def test_highpass_reference_of_a_volume(shape, dtype):
    """slice by slice; a blur that also ran along the slices (the colour path's third pass) would show"""
    from scipy import ndimage
    volume = X.noise(shape, dtype)
    ref = X.highpass80_volume(volume)
    scale = float(np.abs(volume).max())
    scipy_dev = X.rel_dev(X.highpass_scipy_volume(volume), ref, scale)
    tol = X.rule(scipy_dev)
    print('high-pass volume %r %s: scipy %.3e tolerance %.3e' % (shape, dtype, scipy_dev, tol))
    assert scipy_dev <= X.FLOOR / X.FACTOR
    if shape[0] > 1:
        dev = X.rel_dev(volume - ndimage.gaussian_filter(volume.astype(float), 150), ref, scale)
        assert dev >= MARGIN * tol
