"""csrc/texture.hip pixel by pixel against the 80-bit reference of tests/texture_cases.py: the sigma = 150 high-pass (k_corr1d_col, the
transposes, the channel mix) on whole images, borders included, and every instantiation of the battery kernels the Python layer can
reach -- k_conv_battery<1, 2, 4, 6, 8>, k_conv_battery_sym<1, 2, 4, 6, 8>, k_conv_battery_quad<1 .. 4, 16>, k_sep_battery_tall,
k_sep_battery<33> and k_sep_battery<0> -- with the clip dead and alive, the norms (k_sumsq_partial / k_sumsq_final, the per-workgroup
sums of k_sep_battery_tall and k_sumsq_jobs), several batteries in one launch, and the volume path.

How a response is read back (no entry point of its own):
  1. ``lm_battery`` with the side-33 kernel that is 1 at the centre copies the high-pass planes into the response buffer bit for bit
     (every other product is 0 x); the battery tests convolve THESE planes, so a battery kernel is not charged with the high-pass;
  2. ``lm_features([battery])`` with ONE battery leaves that battery's response at the start of the response buffer, where
     ``get_response()`` finds it; the split of the battery (asserted per case) decides which kernels wrote it.

Tolerances (texture_cases.tolerance, relative to max|plane|): 16 x scipy's own fp64 deviation from the reference on the same planes,
floor 1e-13 (the worst case of a 1089-term fp64 sum with unit-L1 weights, whatever its order), plus -- for kernels run as separable
passes -- the L1 norm of what the host's SVD split leaves out.  The figures are printed (pytest -s) and tabulated in DESIGN.md
section 5; tests/test_texture_reference_host.py shows on the CPU that these cases see a subtly wrong kernel."""
import numpy as np
import pytest

import texture_cases as X

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not X.LONGDOUBLE_OK, reason=X.LONGDOUBLE_REASON)]

DEAD_CLIP = 1e6               # descriptors.MAX_SIGNAL_RESPONSE: never reached by 0 .. 255 images and L1-normalised kernels
WIDE = 'IMSEGM_SEP_WIDE_TILE'


def open_image(shape, dtype='u8', labels=None):
    """session of the seeded noise image of ``shape`` with its high-pass prepared and a label map (all zero: one label)"""
    from pyimsegm_amd import _hip
    image = X.noise(tuple(shape) + (3, ), dtype)
    labels = np.zeros(shape, dtype=np.int32) if labels is None else labels
    sess = _hip.Image2D(*shape).upload(image).set_labels(labels)
    sess.lm_prepare(150.)
    return sess, image


def device_planes(sess):
    """the prepared high-pass planes, through the centre kernel"""
    sess.lm_battery(X.battery('centre'), DEAD_CLIP)
    return sess.get_response()


def run_case(sess, c, clip, monkeypatch):
    """(response planes, norm of lm_battery or None, 1 x 6 table [mean | energy] of lm_features or None)"""
    assert X.split_of(c) == c['expect'], (c['id'], X.split_of(c))
    bat = X.battery(c['battery'])
    if c['route'] == 'battery':
        norm = sess.lm_battery(bat, clip)
        return sess.get_response(), norm, None
    if c['wide']:
        monkeypatch.setenv(WIDE, '1')
    try:
        table = sess.lm_features([bat], clip, mean=True, std=False, energy=True, separable=c['separable'], mirror=c['mirror'])
        resp = sess.get_response()
    finally:
        if c['wide']:
            monkeypatch.delenv(WIDE)
    return resp, None, table


def check_norm(what, resp, norm, table):
    """``lm_battery``: the returned norm squared against the 80-bit sum of squares OF THE DEVICE'S RESPONSE (16 x numpy's own fp64
    deviation, floor 1e-13, relative).  ``lm_features``: the norm stays on the device; the table of ONE label (mean, energy) against
    the same statistics formed in 80 bits from the fetched response and its 80-bit norm, within the bound of tests/test_gpu_stats.py:
    1e-12 |ref| + B, B from the pixel count and M = mul (|value| <= mul = log(1 + norm) / 0.03)"""
    from test_gpu_stats import RTOL, fixed_point_bound
    ssq = X.sumsq80(resp)
    if norm is not None:
        numpy_dev = abs(float((X.LD(np.sum(resp**2)) - ssq) / ssq))
        tol = X.rule(numpy_dev)
        dev = abs(float((X.LD(norm) * X.LD(norm) - ssq) / ssq))
        print('%s: sum of squares: numpy %.3e tolerance %.3e device %.3e' % (what, numpy_dev, tol, dev))
        assert dev <= tol, (what, dev, tol)
    if table is not None:
        mean, energy, mul = X.stats80(resp, np.sqrt(ssq))
        b_mean, b_sq = fixed_point_bound(resp[0].size, mul)
        assert table.shape == (1, 6)
        for got, ref, bound, name in ((table[0, :3], mean, b_mean, 'mean'), (table[0, 3:], energy, b_sq, 'energy')):
            err = np.abs(got.astype(X.LD) - ref)
            lim = RTOL * np.abs(ref) + bound
            print('%s: %s of the normalised response: worst error / bound %.3e' % (what, name, float(np.max(err / lim))))
            assert np.all(err <= lim), (what, name, got, ref.astype(np.float64), lim.astype(np.float64))


def check_response(c, sess, planes, monkeypatch, clip=DEAD_CLIP, what=None):
    """one case per pixel and its norm; returns (response, tolerance, scale)"""
    what = what or c['id']
    ref = X.reference(c['battery'], planes)
    tol = X.tolerance(c, ref)
    resp, norm, table = run_case(sess, c, clip, monkeypatch)
    want = X.clip_upper(ref['raw'], clip)
    dev = X.rel_dev(resp, want, ref['scale'])
    print('%s %s: scipy %.3e tolerance %.3e device %.3e (%s)' % (what, planes.shape, ref['scipy'], tol, dev, ', '.join(c['kernels'])))
    assert dev <= tol, (what, dev, tol)
    check_norm(what, resp, norm, table)
    return resp, tol, ref


# ---- the high-pass ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape,dtype', X.HIGHPASS_IMAGES, ids=lambda v: 'x'.join(map(str, v)) if isinstance(v, tuple) else v)
def test_highpass_of_an_image_per_pixel(shape, dtype):
    """image - gaussian_filter(image, 150) over H, W and the channel axis, whole image: (70, 131) three 64-column groups and a
    ragged row block; (5, 203) and (1, 40) reflected dozens of times; (131, 67) two 64-column groups and three 32-wide transpose
    tiles on each axis after the transpose; (33, 1300) wider than 2 x 600 + 64: the x pass takes its branch with all sixteen
    source rows inside the plane as well as the reflected one"""
    sess, image = open_image(shape, dtype)
    try:
        got = device_planes(sess)
    finally:
        sess.close()
    ref = X.highpass80(image)
    scale = float(np.abs(image).max())
    scipy_dev = X.rel_dev(X.highpass_scipy(image), ref, scale)
    tol = X.rule(scipy_dev)
    dev = X.rel_dev(got, ref, scale)
    print('high-pass %s %s: scipy %.3e tolerance %.3e device %.3e' % (shape, dtype, scipy_dev, tol, dev))
    assert got.shape == ref.shape and dev <= tol, (dev, tol)


@pytest.mark.parametrize('shape,dtype', X.HIGHPASS_VOLUMES, ids=lambda v: 'x'.join(map(str, v)) if isinstance(v, tuple) else v)
def test_highpass_of_a_volume_per_voxel(shape, dtype):
    """slices independent, no channel pass; 6068 voxels (the response buffer is sized in thirds: not divisible by three), D = 1, 2"""
    from pyimsegm_amd import _hip
    volume = X.noise(shape, dtype)
    sess = _hip.Volume3D(*shape).upload(volume)
    try:
        sess.lm_prepare(150.)
        got = device_planes(sess)
    finally:
        sess.close()
    ref = X.highpass80_volume(volume)
    scale = float(np.abs(volume).max())
    scipy_dev = X.rel_dev(X.highpass_scipy_volume(volume), ref, scale)
    tol = X.rule(scipy_dev)
    dev = X.rel_dev(got, ref, scale)
    print('high-pass volume %s %s: scipy %.3e tolerance %.3e device %.3e' % (shape, dtype, scipy_dev, tol, dev))
    assert got.shape == ref.shape and dev <= tol, (dev, tol)


# ---- every instantiation at (113, 83) -------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def at_shape():
    """one session of the (113, 83) noise image for the module, and its planes as the device prepared them"""
    sess, _ = open_image(X.SHAPE)
    planes = device_planes(sess)
    planes.setflags(write=False)
    yield sess, planes
    sess.close()


def test_the_centre_kernel_returns_the_planes(at_shape):
    """fact 1, as far as it can be seen from outside: what the centre kernel returns is the high-pass (within its tolerance) and
    comes back bit for bit when asked again"""
    sess, planes = at_shape
    image = X.noise(X.SHAPE + (3, ), 'u8')
    ref = X.highpass80(image)
    assert X.rel_dev(planes, ref, 255.) <= X.rule(X.rel_dev(X.highpass_scipy(image), ref, 255.))
    assert np.array_equal(device_planes(sess), planes)


@pytest.mark.parametrize('name', [c['id'] for c in X.CASES])
def test_every_instantiation_per_pixel(name, at_shape, monkeypatch):
    sess, planes = at_shape
    check_response(X.CASE[name], sess, planes, monkeypatch)


@pytest.mark.parametrize('tall,wide', X.TALL_WIDE)
def test_tall_and_wide_tiles_agree(tall, wide, at_shape, monkeypatch):
    """k_sep_battery_tall and k_sep_battery<33> on the same battery: within the same tolerance of each other"""
    sess, planes = at_shape
    ref = X.reference(X.CASE[tall]['battery'], planes)
    tol = X.tolerance(X.CASE[tall], ref)
    a = run_case(sess, X.CASE[tall], DEAD_CLIP, monkeypatch)[0]
    b = run_case(sess, X.CASE[wide], DEAD_CLIP, monkeypatch)[0]
    dev = float(np.max(np.abs(a - b))) / ref['scale']
    print('%s / %s: tolerance %.3e apart %.3e' % (tall, wide, tol, dev))
    assert dev <= tol


def test_no_battery_of_another_side_takes_the_quad_form():
    from pyimsegm_amd._hip import Image2D
    packed = Image2D._pack_bank(list(X.banks()['side17']), True, True)
    assert packed['radius'] == 8 and sorted(packed['parity'].tolist()) == [-1, 0, 0, 0, 1]


# ---- borders ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', X.BORDER_SHAPES, ids=lambda s: '%dx%d' % s)
def test_border_shapes_per_pixel(shape, monkeypatch):
    sess, _ = open_image(shape)
    try:
        planes = device_planes(sess)
        for name in X.BORDER_CASES:
            check_response(X.CASE[name], sess, planes, monkeypatch, what='%s at %dx%d' % ((name, ) + tuple(shape)))
    finally:
        sess.close()


# ---- the clip ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', X.CLIP_CASES)
def test_clip_active(name, at_shape, monkeypatch):
    """clip = the median of the positive reference responses: exactly ``clip`` where the reference exceeds it by more than the
    tolerance, the tolerance elsewhere, negative responses untouched"""
    sess, planes = at_shape
    c = X.CASE[name]
    ref = X.reference(c['battery'], planes)
    raw = ref['raw']
    clip = float(np.median(raw[raw > 0]))
    resp, tol, _ = check_response(c, sess, planes, monkeypatch, clip=clip, what=name + ' clipped')
    margin = tol * ref['scale']
    above, negative = raw > clip + margin, raw < -margin
    assert above.mean() > 0.1 and (raw < -clip - margin).sum() >= 10, (above.mean(), negative.mean())
    assert np.all(resp[above] == clip) and resp.max() == clip
    assert np.all(resp[negative] < 0) and np.max(np.abs(resp[negative] - raw[negative])) <= margin


# ---- several batteries in one launch ------------------------------------------------------------------------------------------
def test_five_batteries_in_one_launch(at_shape, monkeypatch):
    """the five batteries of one sigma in one call: k_sep_battery_tall with SEP_MAX_JOBS jobs.  In every rotation of the list the
    first battery's response is held to the reference per pixel, and every column block of the table equals the table of that
    battery's own call bit for bit (same kernels, same grids, the per-workgroup sums of squares added in the same order)"""
    _, planes = at_shape
    h, w = X.SHAPE
    labels = ((np.arange(h)[:, None] // 20) * 4 + np.arange(w)[None, :] // 25).astype(np.int32)
    sess, _ = open_image(X.SHAPE, labels=labels)
    try:
        assert np.array_equal(device_planes(sess), planes)
        bats = [X.battery(n) for n in X.ONE_SIGMA]
        singles = [sess.lm_features([b], DEAD_CLIP) for b in bats]
        assert all(s.shape == (labels.max() + 1, 9) for s in singles)
        for turn in range(5):
            order = [(turn + j) % 5 for j in range(5)]
            table = sess.lm_features([bats[k] for k in order], DEAD_CLIP)
            resp = sess.get_response()
            first = X.ONE_SIGMA[order[0]]
            ref = X.reference(first, planes)
            tol = X.rule(ref['scipy']) + X.sep_truncation(bats[order[0]])
            dev = X.rel_dev(resp, ref['raw'], ref['scale'])
            print('five batteries, %s first: tolerance %.3e device %.3e' % (first, tol, dev))
            assert dev <= tol, (first, dev, tol)
            for j, k in enumerate(order):
                assert np.array_equal(table[:, 9 * j:9 * j + 9], singles[k]), (turn, j, k)
    finally:
        sess.close()


# ---- volumes ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape,dtype', [((4, 41, 37), 'u8'), ((1, 20, 90), 'f64')], ids=['4x41x37', '1x20x90'])
def test_volume_responses_per_voxel(shape, dtype):
    """Volume3D: P = D planes, the response buffer sized by (n + 2) / 3; an 8-kernel and a 1-kernel battery, every plane, the norm"""
    from pyimsegm_amd import _hip
    volume = X.noise(shape, dtype)
    sess = _hip.Volume3D(*shape).upload(volume)
    try:
        sess.lm_prepare(150.)
        planes = device_planes(sess)
        assert planes.shape == shape
        for name in ('normal:0', 'normal:3'):
            ref = X.reference(name, planes)
            tol = X.rule(ref['scipy'])
            norm = sess.lm_battery(X.battery(name), DEAD_CLIP)
            resp = sess.get_response()
            dev = X.rel_dev(resp, ref['raw'], ref['scale'])
            print('volume %s %s: scipy %.3e tolerance %.3e device %.3e' % (shape, name, ref['scipy'], tol, dev))
            assert resp.shape == shape and dev <= tol, (name, dev, tol)
            check_norm('volume %s %s' % (shape, name), resp, norm, None)
    finally:
        sess.close()
