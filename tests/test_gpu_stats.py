"""Per-superpixel statistics (csrc/stats.hip, k_color_stats: mean, energy and variance of every label) against the fp64 oracle
at the magnitudes, label layouts and shapes where a fixed-point segmented reduction goes wrong.

Every comparison is per label: |got - ref| <= 1e-12 |ref| + B, where B is the absolute bound stated in the header of stats.hip,
computed here from the pixel count and the largest magnitude of the input (not read back from the library).  Labels without
pixels must be exactly 0."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KS = (-30, -20, -12, -4, 0, 4, 12, 20, 40, 60)
SIZES = (1, 2, 15, 16, 17, 31, 33, 63, 64, 65, 129)
RTOL = 1e-12


@pytest.fixture(scope='module')
def hip():
    from pyimsegm_amd import _hip
    _hip.default_context()
    return _hip


def fixed_point_bound(n_pixels, maxabs):
    """(B of the mean, B of energy and variance): stats.hip's 2^-(sh + 32) with sh = min(62 - e_n - e_m, 44 - e_m), where
    n_pixels < 2^e_n and M < 2^e_m for M = maxabs (value sums) and 4 maxabs^2 (squared and deviation sums)"""
    def grid(m):
        e_n = np.frexp(float(n_pixels))[1]
        e_m = np.frexp(float(m) if m > 0 else 1.0)[1]
        return 2.0 ** -(min(62 - e_n - e_m, 44 - e_m) + 32)
    maxabs = float(maxabs)
    return grid(maxabs), grid(4.0 * maxabs * maxabs)


def scaled_image(rng, shape, signed, k, dtype):
    """values in [0.5, 1) or signed with 2^-20 <= |u| < 1, times 2^k: every square and deviation square stays a normal float32"""
    if signed:
        u = rng.uniform(2.0 ** -20, 1.0, shape) * rng.choice([-1.0, 1.0], shape)
    else:
        u = rng.uniform(0.5, 1.0, shape)
    return (u * 2.0 ** k).astype(dtype)


def mixed_range_image(rng, shape, dtype):
    """regions at 1, 2^-16 and 2^-40 and a near-constant region whose deviations are a few float32 ulp"""
    img = rng.uniform(0.5, 1.0, shape)
    h = shape[0] // 4
    img[h:2 * h] *= 2.0 ** -16
    img[2 * h:3 * h] *= 2.0 ** -40
    img[3 * h:] = 0.75 + rng.integers(-3, 4, img[3 * h:].shape) * 2.0 ** -24
    return img.astype(dtype)


def block_labels(rng, shape, block, n):
    grid = rng.integers(0, n, tuple(s // block + 1 for s in shape))
    for ax in range(len(shape)):
        grid = grid.repeat(block, ax)
    return np.ascontiguousarray(grid[tuple(slice(0, s) for s in shape)], dtype=np.int32)


def assert_per_label(got, ref, bound, counts, what):
    """|got - ref| <= 1e-12 |ref| + B per label and channel; labels without pixels exactly 0"""
    got = np.asarray(got, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    if got.shape[0] > ref.shape[0]:                   # n_labels above max + 1: the oracle stops at the largest label
        ref = np.concatenate([ref, np.zeros((got.shape[0] - ref.shape[0], ) + ref.shape[1:])])
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = np.abs(got - ref)
    tol = RTOL * np.abs(ref) + bound
    bad = np.argwhere(err > tol)
    assert bad.size == 0, '%s: %d entries off, first %r: got %r, ref %r, bound %r' % (
        what, len(bad), tuple(bad[0]), got[tuple(bad[0])], ref[tuple(bad[0])], tol[tuple(bad[0])])
    empty = np.zeros(got.shape[0], dtype=bool)
    empty[:len(counts)] = counts == 0
    empty[len(counts):] = True
    assert np.all(got[empty] == 0), '%s: a label without pixels is not 0' % what


def image_stats(hip, img, seg, n_labels=None):
    sess = hip.Image2D(*seg.shape).upload(img).set_labels(seg, n_labels)
    try:
        return sess.color_stats()
    finally:
        sess.close()


def volume_stats(hip, vol, seg, n_labels=None):
    sess = hip.Volume3D(*seg.shape).upload(vol).set_labels(seg, n_labels)
    try:
        return sess.gray_stats()
    finally:
        sess.close()


def check_image(hip, oracle, img, seg, n_labels=None, what=''):
    """colour image through Image2D.color_stats against oracle.color2d_* on the float32-staged input"""
    mean, energy, var = image_stats(hip, img, seg, n_labels)
    img32 = np.asarray(img, dtype=np.float32)
    mean_ref = oracle.color2d_mean(img32, seg)
    energy_ref = oracle.color2d_energy(img32, seg)
    var_ref = oracle.color2d_variance(img32, seg, mean_ref.astype(np.float32))
    b_mean, b_sq = fixed_point_bound(seg.size, np.abs(img).max())
    counts = np.bincount(seg.ravel())
    assert_per_label(mean, mean_ref, b_mean, counts, what + ' mean')
    assert_per_label(energy, energy_ref, b_sq, counts, what + ' energy')
    assert_per_label(var, var_ref, b_sq, counts, what + ' variance')
    return mean, energy, var


def check_volume(hip, oracle, vol, seg, n_labels=None, what=''):
    """gray volume through Volume3D.gray_stats (the one-channel kernel) against oracle.gray3d_stat"""
    mean, energy, var = volume_stats(hip, vol, seg, n_labels)
    v32 = np.asarray(vol, dtype=np.float32)
    mean_ref = oracle.gray3d_stat(v32, seg, 'mean')
    energy_ref = oracle.gray3d_stat(v32, seg, 'energy')
    var_ref = oracle.gray3d_stat(v32, seg, 'var', mean_ref.astype(np.float32))
    b_mean, b_sq = fixed_point_bound(seg.size, np.abs(vol).max())
    counts = np.bincount(seg.ravel())
    assert_per_label(mean, mean_ref, b_mean, counts, what + ' mean')
    assert_per_label(energy, energy_ref, b_sq, counts, what + ' energy')
    assert_per_label(var, var_ref, b_sq, counts, what + ' variance')
    return mean, energy, var


# ---- magnitudes -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('k', KS)
@pytest.mark.parametrize('signed', [False, True], ids=['pos', 'signed'])
@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=['f32', 'f64'])
def test_magnitude_sweep_image(hip, oracle, dtype, signed, k):
    rng = np.random.default_rng(100 + k)
    shape = (97, 130)
    img = scaled_image(rng, shape + (3, ), signed, k, dtype)
    seg = block_labels(rng, shape, 12, 80)
    check_image(hip, oracle, img, seg, what='k=%d' % k)


@pytest.mark.parametrize('k', KS)
@pytest.mark.parametrize('signed', [False, True], ids=['pos', 'signed'])
@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=['f32', 'f64'])
def test_magnitude_sweep_volume(hip, oracle, dtype, signed, k):
    rng = np.random.default_rng(200 + k)
    shape = (5, 23, 70)
    vol = scaled_image(rng, shape, signed, k, dtype)
    seg = block_labels(rng, shape, 6, 60)
    check_volume(hip, oracle, vol, seg, what='k=%d' % k)


@pytest.mark.parametrize('volume', [False, True], ids=['image', 'volume'])
@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=['f32', 'f64'])
def test_power_of_two_equivariance(hip, dtype, volume):
    """stats(img * 2^k) == stats(img) * 2^k (mean) and * 2^2k (energy, variance), bit for bit -- as the oracle and the
    reference's running fp64 sums: the fixed-point grid has to follow the magnitude of the data"""
    rng = np.random.default_rng(7)
    shape = (5, 23, 70) if volume else (97, 130)
    base = scaled_image(rng, shape if volume else shape + (3, ), True, 0, dtype)
    seg = block_labels(rng, shape, 6 if volume else 12, 60)
    run = volume_stats if volume else image_stats
    m0, e0, v0 = run(hip, base, seg)
    assert np.any(m0 != 0) and np.all(np.isfinite(e0))
    for k in KS:
        m, e, v = run(hip, base * dtype(2.0 ** k), seg)
        assert np.array_equal(m, m0 * 2.0 ** k), 'mean, k=%d' % k
        assert np.array_equal(e, e0 * 2.0 ** (2 * k)), 'energy, k=%d' % k
        assert np.array_equal(v, v0 * 2.0 ** (2 * k)), 'variance, k=%d' % k


def test_uint8_equals_float32(hip, oracle):
    """the integer block sums of uint8 images (u8_int) and the general path give identical results on the same values"""
    rng = np.random.default_rng(9)
    for shape, block, n in [((97, 130), 12, 80), ((65, 33), 1, 2000), ((129, 64), 16, 7)]:
        img = rng.integers(0, 256, shape + (3, )).astype(np.uint8)
        seg = block_labels(rng, shape, block, n)
        got8 = check_image(hip, oracle, img, seg, what='u8')
        got32 = image_stats(hip, img.astype(np.float32), seg)
        for a, b in zip(got8, got32):
            assert np.array_equal(a, b)
        img32 = img.astype(np.float32)
        assert np.array_equal(got8[0], oracle.color2d_mean(img32, seg))       # integer terms: exact sums
        assert np.array_equal(got8[1], oracle.color2d_energy(img32, seg))


@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=['f32', 'f64'])
def test_mixed_range_in_one_image(hip, oracle, dtype):
    """regions at 1, 2^-16, 2^-40 and near-constant ones: the bound B (set by the bright region) holds everywhere; the 2^-40
    region documents it -- it is not expected to reach 1e-12 relative"""
    rng = np.random.default_rng(11)
    shape = (128, 150)
    img = mixed_range_image(rng, shape + (3, ), dtype)
    seg = block_labels(rng, shape, 8, 300)
    check_image(hip, oracle, img, seg, what='mixed')
    vol = mixed_range_image(rng, (8, 40, 60), dtype)
    check_volume(hip, oracle, vol, block_labels(rng, (8, 40, 60), 5, 200), what='mixed volume')


# ---- label layouts --------------------------------------------------------------------------------------------------------

def _layouts(rng, shape):
    """(name, labels, n_labels) that stress the LDS hash table of a 64-column workgroup tile"""
    h, w = shape
    yy, xx = np.mgrid[0:h, 0:w]
    flat = (yy * w + xx)
    return [
        ('random_K100', rng.integers(0, 100, shape), None),
        ('random_K4096', rng.integers(0, 4096, shape), None),
        ('random_K2^20_sparse', rng.integers(0, 1 << 20, shape), None),       # most labels empty, every tile overflows
        ('mod64_chain', 5 + 64 * rng.integers(0, 150, shape), None),          # one home slot: probe chains wrap
        ('tile_64', flat % 64, None),                                         # w = 128: exactly 64 labels per tile
        ('tile_65', flat % 65, None),                                         # one label more than the table holds
        ('stripes', np.broadcast_to(xx, shape), None),                        # 16 labels per 16-lane row
        ('single_label', np.full(shape, 3), 11),                              # n_labels above max + 1
    ]


@pytest.mark.parametrize('dtype', [np.uint8, np.float32, np.float64], ids=['u8', 'f32', 'f64'])
def test_label_layouts_image(hip, oracle, dtype):
    rng = np.random.default_rng(13)
    shape = (70, 128)
    if dtype == np.uint8:
        img = rng.integers(0, 256, shape + (3, )).astype(np.uint8)
    else:
        img = scaled_image(rng, shape + (3, ), True, -3, dtype)
    for name, seg, n_labels in _layouts(rng, shape):
        check_image(hip, oracle, img, np.ascontiguousarray(seg, dtype=np.int32), n_labels, what=name)


def test_label_layouts_volume(hip, oracle):
    rng = np.random.default_rng(14)
    shape = (70, 128)                       # a 2 x 35 x 128 volume: the kernel sees it as a 70 x 128 image
    vol = scaled_image(rng, (2, 35, 128), True, -3, np.float32)
    for name, seg, n_labels in _layouts(rng, shape):
        check_volume(hip, oracle, vol, np.ascontiguousarray(seg, dtype=np.int32).reshape(2, 35, 128), n_labels, what=name)


# ---- shapes ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('dtype', [np.uint8, np.float32, np.float64], ids=['u8', 'f32', 'f64'])
def test_ragged_shapes_image(hip, oracle, dtype):
    """1 x 1, 1 x W, H x 1 and partial tiles in both directions; the uint8 path's 4-byte load guards its last pixel"""
    rng = np.random.default_rng(15)
    for h in SIZES:
        for w in SIZES:
            if dtype == np.uint8:
                img = rng.integers(0, 256, (h, w, 3)).astype(np.uint8)
            else:
                img = scaled_image(rng, (h, w, 3), True, 2, dtype)
            seg = block_labels(rng, (h, w), 3, max(1, h * w // 20))
            check_image(hip, oracle, img, seg, what='%d x %d' % (h, w))


def test_ragged_shapes_volume(hip, oracle):
    """D * H not a multiple of the tile height, single voxels and single rows"""
    rng = np.random.default_rng(16)
    for shape in [(1, 1, 1), (1, 1, 65), (3, 11, 17), (5, 13, 65), (2, 33, 1), (7, 5, 129), (3, 31, 64)]:
        vol = scaled_image(rng, shape, True, 1, np.float32)
        seg = block_labels(rng, shape, 2, max(1, int(np.prod(shape)) // 10))
        check_volume(hip, oracle, vol, seg, what='%r' % (shape, ))


# ---- Volume3D.features_color, set_labels ----------------------------------------------------------------------------------

@pytest.mark.parametrize('dtype', [np.uint8, np.float32, np.float64], ids=['u8', 'f32', 'f64'])
def test_volume_features_color_replicates_the_gray_statistics(hip, dtype):
    """the gray plane's statistics in every channel: [m m m | s s s | e e e], s = sqrt(variance) of gray_stats"""
    rng = np.random.default_rng(17)
    shape = (4, 30, 50)
    vol = rng.integers(0, 256, shape).astype(dtype) if dtype == np.uint8 else scaled_image(rng, shape, True, 3, dtype)
    seg = block_labels(rng, shape, 5, 40)
    sess = hip.Volume3D(*shape).upload(vol).set_labels(seg)
    try:
        m, e, v = sess.gray_stats()
        table = sess.features_color()
    finally:
        sess.close()
    want = np.repeat(np.stack([m, np.sqrt(v), e], axis=1), 3, axis=1)
    assert table.shape == want.shape
    assert np.array_equal(table, want)


@pytest.mark.parametrize('volume', [False, True], ids=['image', 'volume'])
def test_set_labels_refuses_labels_beyond_n_labels(hip, volume):
    """a label >= n_labels would index past the per-label tables: refused on the host, before anything reaches the device
    (nothing is launched on the session afterwards)"""
    rng = np.random.default_rng(18)
    if volume:
        sess = hip.Volume3D(3, 20, 30)
        seg = rng.integers(0, 50, (3, 20, 30)).astype(np.int32)
    else:
        sess = hip.Image2D(20, 30)
        seg = rng.integers(0, 50, (20, 30)).astype(np.int32)
    try:
        with pytest.raises(ValueError):
            sess.set_labels(seg, int(seg.max()))
    finally:
        sess.close()
