"""Every device entry on reused scratch that holds stale data.

A context and a session carve their working memory out of buffers that grow and never shrink, so in production a kernel sees
whatever a larger, different call left behind -- while nearly every other test of the suite hands it a new object, whose memory is
very often zero.  Here each entry of one table runs on ONE object in this order:

1. the dirtier call: a larger, structurally different case of another entry that shares the scratch;
2. ``poison``: every device buffer of the object is filled with a word over its whole capacity and the host-side bookkeeping is
   put back to that of a new object (``imsegm_debug_poison_context`` / ``imsegm_debug_image2d_poison``).  The bytes filled are > 0
   and no fewer than what the small case alone allocates on a new object, so the step cannot pass vacuously;
3. the small case from scratch (upload, labels, ...), held to the reference of the entry's own test file: the oracle, the package's
   host statement, numpy / scipy or golden results, with that file's exactness or tolerance -- no number is invented here;
4. the small case once more without poisoning: stale data of the same entry at the same size.

Words: 0x00000001 (in bounds as an index, off by one as a counter, 2^32 + 1 as an int64 sum) and 0x7F7F7F7F (3.4e38 as a float,
1.4e306 as a double, non-zero in every flag byte).  Zero is what a fresh allocation usually holds, so it is not tested.  All
first-word cases of the file run before any second-word case, and the second-word case of an entry is skipped when its first-word
case failed: the second word would be a wild index if some kernel took stale scratch for an address.

Session entries poison the session AND its context (a session call borrows the context's scratch).  The stateless entries run
through the public functions of the package with the thread's default context replaced by the test's own, as production calls
them."""
import collections
import importlib.util
import os

import numpy as np
import pytest

import boundary_cases as B
import natives_cases as NC
import points_cases as PC

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
WORDS = (0x00000001, 0x7F7F7F7F)

_spec = importlib.util.spec_from_file_location('make_golden_connectivity', os.path.join(HERE, 'golden', 'make_golden_connectivity.py'))
GEN = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(GEN)


@pytest.fixture(scope='module')
def hip():
    from pyimsegm_amd import _hip
    _hip.default_context()
    return _hip


Env = collections.namedtuple('Env', 'hip oracle ctx sess monkeypatch')
#: shape: None for an entry of the context, (H, W) for one of an image session, (D, H, W) for one of a volume session
Entry = collections.namedtuple('Entry', 'name shape dirty small')

_REF = {}          # references are computed once and shared by both words and both runs


def cached(key, make):
    if key not in _REF:
        _REF[key] = make()
    return _REF[key]


# ---- the dirtier calls -------------------------------------------------------------------------------------------------------

def dirty_ctx_distance_map(env):
    """boundary family, 300 x 300: masks, the distance transform's scratch, compaction counts"""
    seg = np.ascontiguousarray(B.block_map((300, 300), (13, 17), seed=3, jitter=0.2), dtype=np.int32)
    env.hip.distance_map(seg, env.hip.BOUNDARY_THICK, ctx=env.ctx)
    env.hip.boundary_distances(seg, np.ascontiguousarray(seg.T), ctx=env.ctx)
    env.hip.labels_overlap(seg, np.ascontiguousarray(seg.T), int(seg.max()) + 1, int(seg.max()) + 1, ctx=env.ctx)


def dirty_ctx_overlap_wide(env):
    """the overlap matrix of two 300 x 300 maps of 3 200 labels each: 82 MB of int64 counts, more than the colour table of
    annot_color_hist takes whatever the image"""
    rng = np.random.default_rng(24)
    seg1, seg2 = (rng.integers(0, 3200, (300, 300)).astype(np.int32) for _ in range(2))
    env.hip.labels_overlap(seg1, seg2, 3200, 3200, ctx=env.ctx)
    dirty_ctx_distance_map(env)


def dirty_ctx_label_hist(env):
    """window histograms of a 300 x 300 int16 map: 400 windows x 9 labels of uint32 counts behind the map"""
    rng = np.random.default_rng(21)
    seg = rng.integers(0, 9, (300, 300)).astype(np.int16)
    windows = np.zeros((400, 6), dtype=np.int32)       # (row, column, height, width of the window, row, column in the element)
    windows[:, 0] = rng.integers(0, 285, 400)
    windows[:, 1] = rng.integers(0, 285, 400)
    windows[:, 2:4] = 15
    env.hip.label_hist2d(seg, windows, np.ones((15, 15), dtype=np.int16), 9, ctx=env.ctx)


def dirty_ctx_grid_cut(env):
    """alpha-expansion on a 120 x 150 grid of 5 labels: arcs, flows, heights, queues"""
    rng = np.random.default_rng(22)
    unary = rng.random((120, 150, 5))
    env.hip.cut_grid_graph(unary, (1 - np.eye(5)) * 0.3, rng.random((119, 150)) + 0.1, rng.random((120, 149)) + 0.1, ctx=env.ctx)


def dirty_ctx_annotation(env):
    """the colour hash table and the nearest-valid transform of a 300 x 300 annotation"""
    rng = np.random.default_rng(23)
    image = rng.integers(0, 256, (300, 300, 3)).astype(np.uint8)
    env.hip.annot_color_hist(image, ctx=env.ctx)
    labels = rng.integers(-1, 4, (300, 300)).astype(np.int32)
    env.hip.annot_nearest_valid(labels, ctx=env.ctx)


def _random_image(shape, dtype, seed):
    rng = np.random.default_rng(seed)
    if dtype == np.uint8:
        return rng.integers(0, 256, tuple(shape) + (3, )).astype(np.uint8)
    return rng.random(tuple(shape) + (3, )).astype(dtype)


def dirty_image_slic(env):
    """SLIC with superpixels of edge 4 (thousands of labels) and everything that follows it on the label map"""
    sess = env.sess
    sess.upload(_random_image(sess.shape, np.float64, 31))
    n = sess.shape[0] * sess.shape[1]
    sess.slic(max(2, n // 16), 10.)
    sess.color_stats()
    sess.median()
    sess.mean_gradient()
    sess.features_color()
    sess.graph()
    dirty_ctx_grid_cut(env)


def dirty_image_labels(env):
    """a label per pixel (K = H W), its statistics and medians, and the general connectivity path on noise"""
    sess = env.sess
    h, w = sess.shape
    sess.upload(_random_image(sess.shape, np.uint8, 32))
    sess.set_labels(np.arange(h * w, dtype=np.int32).reshape(h, w))
    sess.color_stats()
    sess.median()
    sess.features_color()
    noise = np.random.default_rng(33).integers(0, 6, (h, w)).astype(np.int32)
    sess.enforce_connectivity(noise, 3, 50)
    dirty_ctx_distance_map(env)


def dirty_volume_labels(env):
    """a label per voxel with its statistics, then components of a three-valued noise volume"""
    sess = env.sess
    n = int(np.prod(sess.shape))
    sess.upload(np.random.default_rng(34).random(sess.shape))
    sess.set_labels(np.arange(n, dtype=np.int32).reshape(sess.shape))
    sess.gray_stats()
    sess.median()
    sess.set_labels(np.random.default_rng(35).integers(0, 3, sess.shape))
    sess.label_cc()
    dirty_ctx_distance_map(env)


def dirty_volume_slic(env):
    """supervoxels of edge 3 on a float32 volume and their components"""
    sess = env.sess
    sess.upload(np.random.default_rng(36).random(sess.shape).astype(np.float32))
    sess.slic(max(2, int(np.prod(sess.shape)) // 27), 5., sigma=1.)
    sess.label_cc()
    sess.gray_stats()
    dirty_ctx_grid_cut(env)


# ---- entries of an image session ---------------------------------------------------------------------------------------------

def small_connectivity(name):
    """test_gpu_connectivity.py: bit for bit against the oracle and scikit-image 0.18.3's own result, on the path the case is for"""
    import test_gpu_connectivity as TC
    _, min_size, max_size = GEN.CASES[name]

    def run(env):
        lab = GEN.make(name)
        want = cached(('conn', name), lambda: env.oracle.enforce_connectivity(lab, min_size, max_size, 0))
        general_runs = env.hip.load_library().imsegm_debug_conn_general_runs
        before = general_runs()
        got = env.sess.enforce_connectivity(lab, min_size, max_size, 0)
        assert got.shape == lab.shape and np.array_equal(got, want), '%d pixels differ' % int((got != want).sum())
        assert np.array_equal(got, TC.GOLDEN['%s_start0' % name])
        assert general_runs() - before == (1 if TC.PATH[name] == 'general' else 0)
    return run


SLIC_IMAGE_SHAPE = (192, 192)


def small_slic(slico):
    """test_gpu_parity.py / smoke: the label map of the oracle, bit for bit"""
    def run(env):
        from pyimsegm_amd import superpixels as S
        from pyimsegm_amd.utilities.synthetic import disc_image
        image = disc_image(SLIC_IMAGE_SHAPE[0])
        want = cached(('slic', slico), lambda: env.oracle.segment_slic_img2d(image, 18, 0.2, slico=slico))
        sess = env.sess
        sess.upload(S._as_rgb(image))
        S._run_slic(sess, 2, 18, 0.2, slico=slico)
        assert np.array_equal(sess.get_labels(), want)
    return run


STATS_SHAPE = (97, 130)


def small_color_stats(dtype):
    """test_gpu_stats.py: per label within 1e-12 |ref| + B of the fp64 oracle, B the fixed-point bound of stats.hip"""
    def run(env):
        import test_gpu_stats as TS
        rng = np.random.default_rng(100)
        if dtype == np.uint8:
            img = rng.integers(0, 256, STATS_SHAPE + (3, )).astype(np.uint8)
        else:
            img = TS.scaled_image(rng, STATS_SHAPE + (3, ), True, 4, dtype)
        seg = TS.block_labels(rng, STATS_SHAPE, 12, 80)
        mean, energy, var = env.sess.upload(img).set_labels(seg).color_stats()
        img32 = np.asarray(img, dtype=np.float32)
        mean_ref, energy_ref, var_ref = cached(('stats', np.dtype(dtype).name), lambda: (
            env.oracle.color2d_mean(img32, seg), env.oracle.color2d_energy(img32, seg),
            env.oracle.color2d_variance(img32, seg, env.oracle.color2d_mean(img32, seg).astype(np.float32))))
        b_mean, b_sq = TS.fixed_point_bound(seg.size, np.abs(img).max())
        counts = np.bincount(seg.ravel())
        TS.assert_per_label(mean, mean_ref, b_mean, counts, 'mean')
        TS.assert_per_label(energy, energy_ref, b_sq, counts, 'energy')
        TS.assert_per_label(var, var_ref, b_sq, counts, 'variance')
        # the resident feature table: test_gpu_fused.py test_feature_table_equals_the_separate_statistics, exactly
        assert np.array_equal(env.sess.features_color(), np.hstack([mean, np.sqrt(var), energy]))
        assert np.array_equal(env.sess.features_color(True, False, True), np.hstack([mean, energy]))
        # features_place: two groups put side by side into one resident table (test_gpu_resident_table.py test_placement_is_checked)
        env.sess.features_place(9, 0).features_color(True, True, False, to_host=False)
        env.sess.features_place(9, 6).features_color(False, False, True, to_host=False)
        assert np.array_equal(env.sess.get_features(9), np.hstack([mean, np.sqrt(var), energy]))
    return run


MEDIAN_SHAPE = (67, 93)


def small_median_and_gradient(dtype):
    """test_gpu_natives.py test_device_median_and_mean_gradient_2d: np.median per label and channel, exactly; the gradient means
    against the mean of the numpy gradient image on a new session of a new context (the existing test's reference: it runs
    the device's mean kernel, so a stale-scratch fault of that kernel shows in the color_stats entries, which the oracle holds)"""
    def run(env):
        rng = np.random.default_rng(3)
        img = rng.random(MEDIAN_SHAPE + (3, )) * 255
        img = img.astype(dtype) if dtype == np.uint8 else (img / 255.).astype(dtype)
        seg = (np.arange(67)[:, None] // 9) * 11 + (np.arange(93)[None, :] // 9)
        seg[seg == 5] = 4                                        # label 5 has no pixel
        seg[10:14, 20:23] = 80                                   # an even and an odd sized island
        sess = env.sess.upload(img).set_labels(seg)
        med, grad = sess.median(), sess.mean_gradient()
        ref = np.full((seg.max() + 1, 3), np.nan)
        for k in np.unique(seg):
            ref[k] = [np.median(img[:, :, c][seg == k]) for c in range(3)]
        assert np.array_equal(np.isnan(med), np.isnan(ref)) and np.array_equal(np.nan_to_num(med), np.nan_to_num(ref))
        gimg = np.zeros_like(img)
        for c in range(3):
            gimg[:, :, c] = np.sum(np.gradient(img[:, :, c]), axis=0)
        ref_g = cached(('grad', np.dtype(dtype).name), lambda: _mean_on_a_new_session(env, gimg, seg))
        assert np.array_equal(grad, ref_g)
    return run


def _mean_on_a_new_session(env, image, seg):
    """descriptors.hip_img2d_color_mean as test_gpu_natives.py uses it: the mean statistic on a new session of a new context"""
    ctx = env.hip.Context()
    try:
        sess = env.hip.Image2D(seg.shape[0], seg.shape[1], ctx).upload(image).set_labels(seg)
        try:
            return sess.color_stats(energy=False, var=False)[0]
        finally:
            sess.close()
    finally:
        ctx.close()


# ---- entries of a volume session ---------------------------------------------------------------------------------------------

VOLUME_SHAPE = (24, 40, 48)


def small_volume_slic(dtype):
    """test_gpu_volume.py test_volume_slic_bit_exact ('iso_f64' / 'iso_f32'): SLIC + connectivity, then the components of the map
    the connectivity pass left (label_cc by first voxels), bit for bit against the oracle"""
    def run(env):
        import test_gpu_volume as TV
        from pyimsegm_amd.superpixels import _slic3d_params
        vol = TV._noisy_ellipsoid(VOLUME_SHAPE, dtype=dtype)
        n_seg, compact = _slic3d_params(VOLUME_SHAPE, 7, 0.2, (1, 1, 1))
        ref_raw, ref = cached(('volslic', np.dtype(dtype).name), lambda: _volume_reference(env, TV, vol, n_seg, compact))
        sess = env.sess.upload(vol)
        sess.slic(n_seg, compact, sigma=1., spacing=(1, 1, 1))
        raw = sess.get_labels()
        assert np.array_equal(raw, ref_raw), 'SLIC + connectivity differ in %d voxels' % np.count_nonzero(raw != ref_raw)
        k = sess.label_cc()
        assert np.array_equal(sess.get_labels(), ref) and k == ref.max() + 1
    return run


def _volume_reference(env, TV, vol, n_seg, compact):
    raw = TV._oracle_raw(env.oracle, vol, n_seg, compact, (1, 1, 1))
    return raw, env.oracle.label_cc(raw)


CC_SHAPE = (9, 17, 70)


def small_label_cc_rows(env):
    """test_gpu_volume.py test_label_cc_background_and_diagonals: components of a caller's map (by rows), against the oracle"""
    lab = np.random.default_rng(2).integers(0, 3, CC_SHAPE)
    ref = cached('cc_rows', lambda: env.oracle.label_cc(lab))
    sess = env.sess.set_labels(lab)
    k = sess.label_cc()
    assert np.array_equal(sess.get_labels(), ref) and k == ref.max() + 1
    assert np.all((ref == 0) == (lab == 0))


GRAY_SHAPE = (5, 23, 70)


def small_gray_stats(env):
    """test_gpu_stats.py check_volume: the one-channel kernel against oracle.gray3d_stat within the fixed-point bound"""
    import test_gpu_stats as TS
    rng = np.random.default_rng(200)
    vol = TS.scaled_image(rng, GRAY_SHAPE, True, 4, np.float32)
    seg = TS.block_labels(rng, GRAY_SHAPE, 6, 60)
    mean, energy, var = env.sess.upload(vol).set_labels(seg).gray_stats()
    v32 = np.asarray(vol, dtype=np.float32)

    def reference():
        m = env.oracle.gray3d_stat(v32, seg, 'mean')
        return m, env.oracle.gray3d_stat(v32, seg, 'energy'), env.oracle.gray3d_stat(v32, seg, 'var', m.astype(np.float32))
    mean_ref, energy_ref, var_ref = cached('gray', reference)
    b_mean, b_sq = TS.fixed_point_bound(seg.size, np.abs(vol).max())
    counts = np.bincount(seg.ravel())
    TS.assert_per_label(mean, mean_ref, b_mean, counts, 'mean')
    TS.assert_per_label(energy, energy_ref, b_sq, counts, 'energy')
    TS.assert_per_label(var, var_ref, b_sq, counts, 'variance')


GRAPH_VOLUME_SHAPE = (14, 45, 52)


def small_volume_graph(env):
    """test_gpu_volume.py test_volume_graph_vs_oracle: edges, presence and centres equal the oracle's, exactly"""
    import test_gpu_volume as TV

    def reference():
        seg = env.oracle.segment_slic_img3d_gray(TV._noisy_ellipsoid(GRAPH_VOLUME_SHAPE, seed=5), 8, 0.2, (3, 1, 1))
        return seg, env.oracle.adjacency(seg), env.oracle.centers(seg)
    seg, (ref_v, ref_e), ref_c = cached('volgraph', reference)
    edges, centres, present = env.sess.set_labels(seg).graph()
    assert np.flatnonzero(present).tolist() == ref_v.tolist()
    assert edges.tolist() == ref_e
    assert np.array_equal(centres[present], ref_c[present])
    assert np.all(centres[~present] == -1)


# ---- entries of the context --------------------------------------------------------------------------------------------------

def small_label_hist2d(env):
    """test_gpu_natives.py test_label_hist_doctests_and_random_windows: counts of the cropped window by numpy, exactly"""
    from pyimsegm_amd import descriptors as D
    rng = np.random.default_rng(5)
    big = rng.integers(-1, 7, (90, 130)).astype(np.int16)
    rr, cc = np.mgrid[-6:7, -6:7]
    selem = ((rr**2 + cc**2) <= 36).astype(np.int16)
    positions = np.stack([rng.integers(0, 90, 40), rng.integers(0, 130, 40)], axis=1)
    hists, sizes = D.compute_label_hist_positions(big, positions, selem, 7)
    for pos, hist, size in zip(positions, hists, sizes):
        b0, e0, s0, s1 = D.adjust_bounding_box_crop(big.shape, selem.shape, pos)
        sel, se = big[b0[0]:e0[0], b0[1]:e0[1]], selem[s0[0]:s1[0], s0[1]:s1[1]]
        ref = [np.sum(np.logical_and(sel == lb, se == 1)) for lb in range(7)]
        assert hist.tolist() == ref and size == se.sum()


def small_ring_hist2d(env):
    """test_gpu_points.py test_label_rings_counts_and_sizes: counts per disc and label, sizes of the clipped discs, exactly"""
    _, segm, positions, radii, nb_labels = [c for c in PC.label_ring_cases() if c[0] == 'labels -1 and nb_labels'][0]
    hist, size = env.hip.ring_hist2d(segm, positions, radii, nb_labels, ctx=env.ctx)
    assert hist.dtype == np.uint32 and size.dtype == np.uint32
    for p, pos in enumerate(positions):
        for d, radius in enumerate(radii):
            counts, pixels = PC.label_counts(segm, pos, PC.disc(radius), nb_labels)
            assert hist[p, d].tolist() == counts.tolist() and size[p, d] == pixels, (pos, radius)


def small_ring_hist_proba2d(env):
    """test_gpu_points.py test_layer_sums_within_the_float64_bound_and_repeatable: n 2^-53 sum|x| against long-double sums"""
    _, layers, positions, radii = PC.layer_ring_cases()[0]
    total, size = env.hip.ring_hist_proba2d(layers, positions, radii, ctx=env.ctx)
    assert total.dtype == np.float64
    for p, pos in enumerate(positions):
        for d, radius in enumerate(radii):
            exact, magnitude, pixels = cached(('layer', p, d), lambda: PC.layer_sums(layers, pos, PC.disc(radius)))
            assert size[p, d] == pixels
            bound = pixels * np.longdouble(2.) ** -53 * magnitude
            error = np.abs(total[p, d].astype(np.longdouble) - exact)
            assert np.all(error <= bound), (pos, radius, error, bound)


def small_rays(env):
    """test_gpu_natives.py (the reference's doctest vectors of the binary rays) and test_gpu_points.py
    test_rays_equal_the_per_position_calls: the batched rays of a label map equal the per-position rays of the host-built mask"""
    from pyimsegm_amd import descriptors as D
    seg = NC.disc_segmentation()
    for position, step, expect in NC.RAY_DOCTESTS:
        assert D.cython_ray_features_seg2d(seg, position, step).astype(int).tolist() == expect
    segm = PC.ray_map()
    for border, edge in ((PC.RAY_BORDER_SETS[0], 'up'), (PC.RAY_BORDER_SETS[1], 'down')):
        mask = np.isin(segm, border)
        rays, shifts, _ = D.compute_ray_features_positions(segm, PC.RAY_POSITIONS, 45, border_labels=border, shifting=False, edge=edge)
        expected = np.array([D.compute_ray_features_segm_2d(mask, pos, 45, 0, edge) for pos in PC.RAY_POSITIONS])
        assert rays.dtype == np.float32 and rays.tobytes() == expected.tobytes()


def small_cut_grid_graph(env):
    """test_gpu_natives.py test_cut_grid_graph_known_answers_and_oracle: the reference's doctest answers and the oracle's labelling"""
    from pyimsegm_amd import graph_cuts as G
    for (gc_regul, seed, coef), expect in (((0., 0, 0.5), NC.GRID_EXPECT_SHAPE), ((.5, 1, 0.), NC.GRID_EXPECT_SEED)):
        unary, pairwise, cost_v, cost_h = NC.grid_problem(gc_regul, seed, coef)
        labels = env.hip.cut_grid_graph(unary, pairwise, cost_v, cost_h, n_iter=999, ctx=env.ctx)
        assert np.array_equal(np.asarray(labels).reshape(NC.GRID_SEGM.shape), expect)
    rng = np.random.default_rng(4)
    unary = rng.random((23, 31, 4))
    pairwise = (1 - np.eye(4)) * 0.4
    cost_v, cost_h = rng.random((22, 31)) + 0.2, rng.random((23, 30)) + 0.2
    want = cached('gridcut', lambda: env.oracle.cut_grid_graph(unary, pairwise, cost_v, cost_h))
    assert np.array_equal(G.cut_grid_graph(unary, pairwise, cost_v, cost_h), want)


def small_cut_general_graph(one_workgroup):
    """test_gpu_parity.py: labelling and energy of the oracle; by the whole device (10 000 sites, no fall-back counted) or by the
    one workgroup (IMSEGM_GC_ONE_WORKGROUP, as that file forces it)"""
    def run(env):
        import test_gpu_parity as TP
        pairs, weights, unary = TP._large_graph(71, 100, 3)
        pairwise = 1.2 * (1 - np.eye(3))
        ref, e_ref = cached('gencut', lambda: env.oracle.cut_general_graph(pairs, weights, unary, pairwise, return_energy=True))
        if one_workgroup:
            env.monkeypatch.setenv('IMSEGM_GC_ONE_WORKGROUP', '1')
        before = env.hip.gc_grid_fallbacks()
        out, e = env.hip.cut_general_graph(pairs, weights, unary, pairwise, return_energy=True, ctx=env.ctx)
        if one_workgroup:
            env.monkeypatch.delenv('IMSEGM_GC_ONE_WORKGROUP')
        assert env.hip.gc_grid_fallbacks() == before and e == e_ref and np.array_equal(out, ref)
    return run


BOUNDARY_PAIRS = (('blocks_64x257', 'ragged_64x257'), ('far_corner_64x300', 'corner_64x300'), ('rand_33x65_L40', 'rand_33x65_L5'))


def small_boundary(env):
    """test_gpu_boundary.py: distance maps of thick masks, boundary points with distances and overlap matrices equal the numpy /
    scipy statement of boundary_cases.py with dtype and shape"""
    from pyimsegm_amd import labeling
    for ref_name, name in BOUNDARY_PAIRS:
        seg_ref, seg = B.maps()[ref_name], B.maps()[name]
        dist = env.hip.distance_map(np.ascontiguousarray(seg, dtype=np.int32), env.hip.BOUNDARY_THICK, ctx=env.ctx)
        assert B.same(dist, B.edt(B.thick(seg))), name
        assert B.same(labeling.compute_distance_map(seg, 1), B.distance_map(seg, 1)), name
        points, dists = labeling.compute_boundary_distances(seg_ref, seg)
        want_points, want_dists = B.boundary_distances(seg_ref, seg)
        assert B.same(points, want_points) and B.same(dists, want_dists), (ref_name, name)
        assert B.same(labeling.compute_labels_overlap_matrix(seg_ref, seg), B.overlap_matrix(seg_ref, seg)), (ref_name, name)


def small_assume_bg(env):
    """test_gpu_output.py: the reference's numpy statements of assume_bg_on_boundary, exactly"""
    import test_gpu_output as TO
    from pyimsegm_amd.labeling import assume_bg_on_boundary
    rng = np.random.default_rng(5)
    for shape, nb, size, bg in (((64, 48), 4, 40, 0), ((90, 70), 6, 70, 1), ((33, 129), 9000, 3, 0)):
        segm = rng.integers(0, nb, shape).astype(np.int32)
        segm[:, : shape[1] // 3] = nb - 1
        got = assume_bg_on_boundary(segm.copy(), bg_label=bg, boundary_size=size)
        assert got.dtype == np.int64 and np.array_equal(got, TO._reference_assume_bg(segm.astype(np.int64), bg, size)), (shape, nb, size)


def small_annotation(env):
    """test_gpu_annotation.py: the five annot_* calls against the host statements of pyimsegm_amd/annotation.py, byte for byte"""
    import test_gpu_annotation as TA
    from pyimsegm_amd import annotation as ann
    hip, ctx = env.hip, env.ctx
    rng = np.random.RandomState(257 * 7 + 256)
    colors = TA.random_table(rng, 256)
    table = np.array(colors, dtype=np.uint8)
    picks = rng.randint(0, len(colors), 257)
    noisy = table[picks].reshape(1, 257, 3).copy()
    noisy[0, ::3] = rng.randint(0, 256, (len(range(0, 257, 3)), 3))
    labels = rng.permutation(1000)[:len(colors)].astype(np.int32)
    found, missed = hip.annot_match(noisy, table, labels, ctx=ctx)
    expected, converted = ann.colors_to_labels_host(noisy, colors, labels)
    unmatched = ~(noisy[:, :, None, :] == table[None, None]).all(axis=3).any(axis=2)
    assert missed == int(unmatched.sum()) == 257 - converted
    assert found.dtype == np.int32 and np.array_equal(found[~unmatched], expected[~unmatched]) and (found[unmatched] == -1).all()
    index = hip.annot_match(noisy, table, mode=hip.ANNOT_MATCH_NEAREST, ctx=ctx)
    assert np.array_equal(index.ravel(), ann.nearest_color_index_host(noisy, colors))
    segm = (picks - 7).astype(np.int32).reshape(1, 257)
    painted = hip.annot_paint(segm, -7, table, ctx=ctx)
    assert painted.dtype == np.uint8 and np.array_equal(painted, ann.labels_to_colors_host(segm, -7, table))
    # histogram: runs that cross lanes and waves, a pixel count that is no multiple of 4 and of 64
    rng = np.random.RandomState(64 * 100 + 65)
    n = 64 * 65
    run_picks = np.repeat(rng.randint(0, 5, n), rng.randint(1, 40, n))[:n]
    few = np.array([(0, 0, 0), (255, 255, 255), (1, 0, 0), (0, 0, 1), (0, 1, 0)], dtype=np.uint8)
    image = few[run_picks].reshape(64, 65, 3)
    keys, counts = hip.annot_color_hist(image, ctx=ctx)
    ref_keys, ref_counts = ann.color_counts_host(image)
    assert np.array_equal(keys, ref_keys) and np.array_equal(counts, ref_counts)
    # nearest valid pixel and the quantisation built on it
    holes = np.ascontiguousarray(np.where(rng.rand(33, 70) < 0.7, -1, rng.randint(0, 5, (33, 70))), dtype=np.int32)
    holes[0, 0] = 2
    nearest = hip.annot_nearest_valid(holes, ctx=ctx)
    assert nearest.dtype == np.int32 and np.array_equal(nearest, ann.nearest_valid_host(holes, holes != -1, rows_per_chunk=16))
    speckled = few[rng.randint(0, 5, (33, 70))].copy()
    speckled[rng.rand(33, 70) < 0.3] = (9, 9, 9)
    colors = [tuple(c) for c in few.tolist()]
    exact = ann.exact_color_index_host(speckled, colors)
    composed = np.asarray(colors)[ann.nearest_valid_host(exact, ~np.isnan(exact)).astype(int)]
    assert TA.same(ann.quantize_image_nearest_pixel(speckled, colors, on='device'), composed)
    raw = hip.annot_quantize_nearest_pixel(speckled, few, ctx=ctx)
    assert raw.dtype == np.uint8 and np.array_equal(raw, composed)


def small_exclusive_scan(env):
    """test_gpu_scan.py: the exclusive prefix sum and the total against numpy.cumsum, exactly (more than one block of the scan).
    imsegm_debug_exclusive_scan allocates and frees its own device memory, so no poison of the context reaches it: this entry
    cannot fail because of stale scratch.  It is here because the issue lists it, and it shows only that the scan still runs beside
    a poisoned context; it is no evidence for the rule."""
    import test_gpu_scan as TSC
    TSC.check(env.hip, np.random.default_rng(4097).integers(0, 1000, size=4097))
    TSC.check(env.hip, np.full(65, 1))


def small_mixture_fit(env):
    """test_gpu_mixture_fit.py: Lloyd from scikit-learn's seeds gives its labels and iteration counts, centres and inertia within
    EM_TOLERANCE; twenty EM iterations from those labels within EM_TOLERANCE of the reference statement"""
    import mixture_fit_cases as MC
    name = 'plan_features'
    table = MC.load_table(name)
    seeds = MC.seeds_of(table)
    tol = 1e-4 * np.mean(np.var(table, axis=0))
    labels, centres, inertia, n_iter = cached('lloyd', lambda: MC.reference_lloyd(table, seeds))
    got = env.hip.kmeans_lloyd(table, seeds, 300, tol, ctx=env.ctx)
    assert not got['empty'].any()
    assert (got['labels'] != labels).sum(axis=1).tolist() == [0] * MC.N_RESTARTS
    assert got['n_iter'].tolist() == n_iter.tolist()
    tolerance = MC.EM_TOLERANCE[name]
    assert np.max(np.abs(got['centres'] - centres) / (1 + np.abs(centres))) <= tolerance
    assert np.max(np.abs(got['inertia'] - inertia) / (1 + np.abs(inertia))) <= tolerance
    refs = cached('em', lambda: [MC.reference_em(table, lab, 0., 20) for lab in labels])
    fit = env.hip.mixture_em(len(labels), MC.N_CLASSES, table.shape[1], labels=np.atleast_2d(labels), tol=0., max_iter=20, ctx=env.ctx)
    for r, ref in enumerate(refs):
        if ref['failed']:
            assert fit['not_pd'][r] and fit['n_iter'][r] == ref['n_iter'], (r, ref['failed'])
        else:
            assert fit['n_iter'][r] == 20 and not fit['converged'][r] and not fit['not_pd'][r]
        dev = MC.deviation({key: fit[key][r] for key in fit}, ref)
        assert dev <= tolerance, (r, dev)


# ---- further entries of an image session -------------------------------------------------------------------------------------

LM_SHAPE = (57, 70)


def small_lm_features(env):
    """test_gpu_texture_flags.py test_response_median_and_gradient_equal_numpy_on_the_device_response and
    test_prepared_state_survives_median_and_gradient: per battery the median of the normalised response bit for bit against
    np.median, the gradient means within 1e-6 of the numpy gradient; the response and the norm of a battery, and the fused
    lm_features table, equal those of a new session of a new context, exactly"""
    import test_gpu_texture_flags as TF
    from pyimsegm_amd import descriptors as D
    data = np.random.default_rng(4).random(LM_SHAPE + (3, ))
    seg = TF._labels(LM_SHAPE, 1)
    nb = int(seg.max()) + 1
    filters, _ = D._select_bank('short')

    def on_a_new_session():
        ctx = env.hip.Context()
        try:
            new = env.hip.Image2D(LM_SHAPE[0], LM_SHAPE[1], ctx).upload(data).set_labels(seg).lm_prepare(150.)
            try:
                table = new.lm_features(filters, D.MAX_SIGNAL_RESPONSE)
                new.lm_prepare(150.)
                return table, [(new.lm_battery(b, D.MAX_SIGNAL_RESPONSE), new.get_response()) for b in (filters[0], filters[2])]
            finally:
                new.close()
        finally:
            ctx.close()
    want_table, want_batteries = cached('lm', on_a_new_session)
    sess = env.sess.upload(data).set_labels(seg).lm_prepare(150.)
    assert np.array_equal(sess.lm_features(filters, D.MAX_SIGNAL_RESPONSE), want_table)
    sess.lm_prepare(150.)
    for battery, (want_norm, want_resp) in zip((filters[0], filters[2]), want_batteries):
        norm = sess.lm_battery(battery, D.MAX_SIGNAL_RESPONSE)
        assert 0 < norm < np.inf and np.isclose(norm, want_norm, rtol=1e-12, atol=0)
        mul = np.log(1 + norm) / 0.03
        resp = sess.get_response()
        assert np.array_equal(resp, want_resp)
        v = (resp * mul) / norm
        median = sess.response_median(mul, norm)
        grad = sess.response_mean_gradient(mul, norm)
        ref_median = np.stack([TF._host_median(v[c], seg, nb) for c in range(3)], axis=1)
        slopes = np.stack([np.sum(np.gradient(v[c]), axis=0) for c in range(3)], axis=-1)
        ref_grad = D.hip_img2d_color_mean(np.ascontiguousarray(slopes), seg)
        present = ~np.isnan(ref_median)
        assert np.array_equal(np.isnan(median), ~present)
        assert np.array_equal(median[present].view(np.int64), ref_median[present].view(np.int64))
        np.testing.assert_allclose(grad, ref_grad, rtol=1e-6, atol=1e-6 * np.nanmax(np.abs(ref_grad)))


CONVERT_SHAPE = (37, 53)


def small_convert_color(env):
    """test_gpu_colorspace.py: the Lab image equals the fp64 model of the kernel (colorspace_cases.model64) exactly, and every
    statistic on it equals the same statistic of a new session that was handed the converted image (the same bytes through the
    same kernels); convert_color(0) returns to the statistics of the upload"""
    import colorspace_cases as CC
    rng = np.random.RandomState(CC.SEED)
    image = rng.randint(0, 256, CONVERT_SHAPE + (3, )).astype(np.uint8)
    segm = (np.indices(CONVERT_SHAPE)[0] // 8) * 7 + np.indices(CONVERT_SHAPE)[1] // 8

    def everything(s):
        return list(s.color_stats()) + [s.median(), s.mean_gradient(), s.features_color()]
    lab_model = cached('lab', lambda: CC.model64(image, 'lab'))

    def on_a_new_session():
        ctx = env.hip.Context()
        try:
            other = env.hip.Image2D(CONVERT_SHAPE[0], CONVERT_SHAPE[1], ctx)
            try:
                return everything(other.upload(lab_model).set_labels(segm)), everything(other.upload(image).set_labels(segm))
            finally:
                other.close()
        finally:
            ctx.close()
    want_lab, want_rgb = cached('labstats', on_a_new_session)
    sess = env.sess.upload(image).set_labels(segm)
    assert np.array_equal(sess.convert_color('lab').converted(), lab_model)
    for a, b in zip(everything(sess), want_lab):
        assert np.array_equal(a, b, equal_nan=True)
    sess.convert_color(0)
    for a, b in zip(everything(sess), want_rgb):
        assert np.array_equal(a, b, equal_nan=True)


def _terms_case():
    import terms_cases as T
    return T.CASES[2]                       # 9 features, 3 classes, 37 superpixels of 2 x 2 pixels


def _terms_shape():
    import terms_cases as T
    return T.block_labels(*T.grid_shape(_terms_case()[2])).shape


def small_segment_gmm(env):
    """test_gpu_terms_reference.py: graph_prepare + segment with a device GMM on a table the test puts there -- the graph of the
    block map exactly, the probabilities within proba_tolerance of the 80-bit reference, unary costs, edge weights and their
    integers by check_terms within terms_tolerance; test_gpu_fused.py: the prepared graph gives what the call alone gives"""
    import terms_cases as T
    import test_gpu_terms_reference as TT
    case = _terms_case()
    F, C, K, _ = case
    model, table, ref = T.case_data(case)
    h, w = T.grid_shape(K)
    labels = T.block_labels(h, w)
    image = np.random.RandomState(h * 1000 + w).randint(0, 256, labels.shape + (3, )).astype(np.uint8)
    pairwise, gmm = T.pairwise_cost(C), env.hip.DeviceGmm(model)
    sess = env.sess.upload(image).set_labels(labels, h * w)
    sess.put_features(np.ascontiguousarray(table, dtype=np.float64))
    assert np.array_equal(sess.get_features(F), table)
    sess.graph_prepare()
    ahead = sess.segment(pairwise, 'model', gmm=gmm, debug=True, want_proba=True, want_graph_labels=True)
    alone = sess.segment(pairwise, 'model', gmm=gmm, debug=True, want_proba=True, want_graph_labels=True)
    for out in (ahead, alone):
        TT.check_graph(out, h, w)
        assert float(np.abs(out['proba'] - ref).max()) <= T.proba_tolerance(case)
        TT.check_terms(out, table, 'model', 1., pairwise, T.terms_tolerance(case))
    for key in ('edges', 'centres', 'edge_weights', 'edge_weights_int', 'unary_int', 'graph_labels', 'segm', 'energy'):
        assert np.array_equal(alone[key], ahead[key]), key


# ---- further entries of the context --------------------------------------------------------------------------------------------

def small_object_cut_pixels(env):
    """test_gpu_object_cut.py: the reference's doctest answers; integers, labelling and energy of the host statement and the oracle"""
    import importlib
    import test_gpu_object_cut as TOC
    rg = importlib.import_module('pyimsegm_amd.region_growing')
    for kwargs, answer in TOC.C.DOCTEST_PIXELS:
        labels = TOC._device_against_host(rg, env.hip, env.oracle, TOC.C.DOCTEST_SEGM, TOC.C.DOCTEST_CENTRES, **kwargs)
        assert labels.tolist() == answer
    fixture = cached('objcut', TOC.C.load_fixture)
    name = list(TOC.C.PIXEL_CASES)[0]
    segm, centres, kwargs = TOC.C.pixel_case(name, int(fixture['pixels_%s_seed' % name]))
    assert np.array_equal(TOC._device_against_host(rg, env.hip, env.oracle, segm, centres, **kwargs), fixture['pixels_%s_labels' % name])


def small_boundary_points(env):
    """test_gpu_boundary_points.py: masks of split_background_foreground and both ray tables of boundary_rays equal the host
    statement of pyimsegm_amd/ellipse_fitting.py byte for byte"""
    import test_gpu_boundary_points as TBP
    from pyimsegm_amd import descriptors, ellipse_fitting as ell
    directions = descriptors._ray_directions(5.)
    for name in sorted(TBP.EDGE)[:3]:
        case = TBP.EDGE[name]
        (want_bg, want_fg), (rays_want_bg, rays_want_fg) = cached(('bpoints', name), lambda: (
            ell.split_host(case['seg'], case['sel_bg'], case['sel_fg']),
            ell.boundary_rays_host(case['seg'], case['sel_bg'], case['sel_fg'], case['centers'], directions)))
        seg = case['seg'].astype(np.int32)
        seg_bg, seg_fg = env.hip.split_background_foreground(seg, case['sel_bg'], case['sel_fg'], ctx=env.ctx)
        assert TBP.same_bytes(seg_bg, want_bg.astype(np.uint8)) and TBP.same_bytes(seg_fg, want_fg.astype(np.uint8)), name
        rays_bg, rays_fg = env.hip.boundary_rays(seg, case['sel_bg'], case['sel_fg'], case['centers'], directions, ctx=env.ctx)
        assert TBP.same_bytes(rays_bg, rays_want_bg) and TBP.same_bytes(rays_fg, rays_want_fg), name


def small_ellipse_ransac(env):
    """test_gpu_ellipse.py compare: three ragged eggs against score_trials_host -- criteria within CRITERION_RTOL, distances within
    1e-9, best / kept / mask equal"""
    import test_gpu_ellipse as TE
    from pyimsegm_amd import ellipse_fitting as ell
    TE.compare(env.hip, ell, TE.C.device_job(500, [65, 7, 250], [5, 65, 64], 257), 'three eggs')


def small_ellipse_place(env):
    """test_gpu_ellipse_place.py: map and flags of ellipse_place, counts and areas of ellipse_overlaps equal the host fold byte for
    byte"""
    import test_gpu_ellipse_place as TEP
    from pyimsegm_amd import ellipse_fitting as ell
    for name in sorted(TEP.CASES)[:3]:
        case = TEP.CASES[name]

        def host():
            segm = case['segm'].copy()
            placed = ell.place_host(segm, case['params'], case['labels'], case['thr'])
            return segm, placed, ell.overlaps_host(case['segm'], case['params'], int(case['segm'].max()) + 1)
        want_segm, want_placed, (want_counts, want_areas) = cached(('place', name), host)
        geom, sincos = TEP.geometry(ell, case)
        segm = case['segm'].astype(np.int32)
        placed = env.hip.ellipse_place(segm, geom, sincos, case['labels'], case['thr'], ctx=env.ctx)
        assert TEP.same_bytes(segm, want_segm.astype(np.int32)) and TEP.same_bytes(placed, want_placed.astype(np.uint8)), name
        counts, areas = env.hip.ellipse_overlaps(case['segm'].astype(np.int32), geom, sincos, want_counts.shape[1], ctx=env.ctx)
        assert TEP.same_bytes(counts, want_counts) and TEP.same_bytes(areas, want_areas), name


def small_object_shapes(env):
    """test_gpu_object_shapes.py check: labels, moments, centres and rays of the host statement byte for byte, the public function
    both ways; a width across a wave and a run across every wave segment of a row"""
    import importlib
    import test_gpu_object_shapes as TOS
    rg = importlib.import_module('pyimsegm_amd.region_growing')
    img = TOS.blobs(64, 130, 3, (1, 2, 3, 5, 8, 9))
    img[10, :] = 4
    labels, _, _, rays = TOS.check(rg, env.hip, img, 45)
    assert len(labels) >= 2 and (rays == -1).any()


def small_mixture_fit_wide(env):
    """test_gpu_mixture_fit_wide.py ('c3_17': 17 features): scikit-learn's labels and iteration counts, centres and inertia within
    LLOYD_TOLERANCE; twenty EM iterations within the case's EM_TOLERANCE"""
    import mixture_fit_wide_cases as WC
    name = 'c3_17'
    table = WC.load_table(name)
    labels, centres, inertia, n_iter = WC.host_lloyd(name)
    got = env.hip.kmeans_lloyd_wide(table, WC.case_seeds(name), 300, WC.lloyd_tol(table), ctx=env.ctx)
    assert not got['empty'].any()
    assert (got['labels'] != labels).sum(axis=1).tolist() == [0] * WC.CASES[name][1]
    assert got['n_iter'].tolist() == n_iter.tolist()
    assert np.max(np.abs(got['centres'] - centres) / (1 + np.abs(centres))) <= WC.LLOYD_TOLERANCE
    assert np.max(np.abs(got['inertia'] - inertia) / (1 + np.abs(inertia))) <= WC.LLOYD_TOLERANCE
    refs = cached('emwide', lambda: [WC.reference_em(table, lab, 0., 20) for lab in labels])
    fit = env.hip.mixture_em_wide(len(labels), WC.CASES[name][0], table.shape[1], labels=np.atleast_2d(labels), tol=0., max_iter=20,
                                  ctx=env.ctx)
    for r, ref in enumerate(refs):
        assert not ref['failed']
        assert fit['n_iter'][r] == 20 and not fit['converged'][r] and not fit['not_pd'][r]
        assert WC.deviation({key: fit[key][r] for key in fit}, ref) <= WC.EM_TOLERANCE[name], r


def small_reduced_and_bayesian(env):
    """test_gpu_reduced_model.py: probabilities of a PCA-reduced and of a Bayesian mixture within proba_tolerance of the 80-bit
    reference (a session of its own per model, on the poisoned context)"""
    import reduced_model_cases as R
    import test_gpu_reduced_model as TR
    for case in (R.CASES[0], R.BAYES_CASES[0]):
        TR.test_probabilities_against_the_80_bit_reference(case)


def small_region_growing(env):
    """test_gpu_region_growing.py at 65 superpixels: greedy_step against the host statement and the brute-force candidates, the
    criterion against the host tree and compute_rg_crit, update_shape_costs within 1e-12 of the host statement"""
    import importlib
    import test_gpu_region_growing as TRG
    rg = importlib.import_module('pyimsegm_amd.region_growing')
    TRG.test_candidates_and_scores(rg, 65)
    TRG.test_criterion(rg, 257)
    TRG.test_shape_cost_sizes(rg, 65)


def small_batch_run_color(env):
    """test_gpu_batch.py test_batch_equals_one_image_at_a_time (five 97 x 130 images): class maps equal the single-image calls,
    label maps equal the oracle's"""
    import test_gpu_batch as TB
    TB.test_batch_equals_one_image_at_a_time(env.hip, env.oracle, (97, 130), 12, 5)


ENTRIES = [
    # image sessions
    Entry('connectivity-general-noise', (150, 170), dirty_image_slic, small_connectivity('noise')),
    Entry('connectivity-general-oversize', (128, 128), dirty_image_slic, small_connectivity('oversize')),
    Entry('connectivity-tile', (203, 317), dirty_image_slic, small_connectivity('blocks_ragged')),
    Entry('slic', SLIC_IMAGE_SHAPE, dirty_image_labels, small_slic(False)),
    Entry('slico', SLIC_IMAGE_SHAPE, dirty_image_labels, small_slic(True)),
    Entry('lm_features+response-median+gradient', LM_SHAPE, dirty_image_slic, small_lm_features),
    Entry('convert_color+statistics', CONVERT_SHAPE, dirty_image_slic, small_convert_color),
    Entry('graph_prepare+segment-gmm', _terms_shape(), dirty_image_labels, small_segment_gmm),
    Entry('color_stats-u8+features_color+features_place', STATS_SHAPE, dirty_image_slic, small_color_stats(np.uint8)),
    Entry('color_stats-f32+features_color+features_place', STATS_SHAPE, dirty_image_slic, small_color_stats(np.float32)),
    Entry('color_stats-f64+features_color+features_place', STATS_SHAPE, dirty_image_slic, small_color_stats(np.float64)),
    Entry('median+mean_gradient-u8', MEDIAN_SHAPE, dirty_image_slic, small_median_and_gradient(np.uint8)),
    Entry('median+mean_gradient-f64', MEDIAN_SHAPE, dirty_image_slic, small_median_and_gradient(np.float64)),
    # volume sessions
    Entry('volume-slic+label_cc-first-voxels-f32', VOLUME_SHAPE, dirty_volume_labels, small_volume_slic(np.float32)),
    Entry('volume-slic+label_cc-first-voxels-f64', VOLUME_SHAPE, dirty_volume_labels, small_volume_slic(np.float64)),
    Entry('volume-label_cc-rows', CC_SHAPE, dirty_volume_slic, small_label_cc_rows),
    Entry('volume-gray_stats', GRAY_SHAPE, dirty_volume_slic, small_gray_stats),
    Entry('volume-graph', GRAPH_VOLUME_SHAPE, dirty_volume_slic, small_volume_graph),
    # the context
    Entry('label_hist2d', None, dirty_ctx_distance_map, small_label_hist2d),
    Entry('ring_hist2d', None, dirty_ctx_grid_cut, small_ring_hist2d),
    Entry('ring_hist_proba2d', None, dirty_ctx_distance_map, small_ring_hist_proba2d),
    Entry('ray_features_binary2d+labels2d', None, dirty_ctx_annotation, small_rays),
    Entry('cut_grid_graph', None, dirty_ctx_distance_map, small_cut_grid_graph),
    Entry('cut_general_graph-whole-device', None, dirty_ctx_annotation, small_cut_general_graph(False)),
    Entry('cut_general_graph-one-workgroup', None, dirty_ctx_distance_map, small_cut_general_graph(True)),
    Entry('boundary-distances+maps+overlap', None, dirty_ctx_grid_cut, small_boundary),
    Entry('assume_bg_on_boundary', None, dirty_ctx_grid_cut, small_assume_bg),
    Entry('annot-five', None, dirty_ctx_overlap_wide, small_annotation),
    Entry('exclusive_scan', None, dirty_ctx_label_hist, small_exclusive_scan),
    Entry('kmeans_lloyd+mixture_em', None, dirty_ctx_grid_cut, small_mixture_fit),
    Entry('kmeans_lloyd_wide+mixture_em_wide', None, dirty_ctx_grid_cut, small_mixture_fit_wide),
    Entry('object_cut_pixels', None, dirty_ctx_distance_map, small_object_cut_pixels),
    Entry('split_background_foreground+boundary_rays', None, dirty_ctx_grid_cut, small_boundary_points),
    Entry('ellipse_ransac', None, dirty_ctx_distance_map, small_ellipse_ransac),
    Entry('ellipse_place+ellipse_overlaps', None, dirty_ctx_grid_cut, small_ellipse_place),
    Entry('object_shapes', None, dirty_ctx_grid_cut, small_object_shapes),
    Entry('reduced+bayesian-model', None, dirty_ctx_distance_map, small_reduced_and_bayesian),
    Entry('rg-greedy_step+criterion+update_shape_costs', None, dirty_ctx_distance_map, small_region_growing),
    Entry('batch2d-run_color', None, dirty_ctx_overlap_wide, small_batch_run_color),
]

#: all first-word cases of the file, then all second-word cases
PARAMS = [pytest.param(entry, word, id='%s-%08x' % (entry.name, word)) for word in WORDS for entry in ENTRIES]
_FAILED_FIRST = set()
_BASELINE = {}


def _open(hip, entry, ctx):
    if entry.shape is None:
        return None
    return (hip.Image2D if len(entry.shape) == 2 else hip.Volume3D)(*entry.shape, ctx=ctx)


def _poison(ctx, sess, word):
    """the context, the entry's session and the sessions the context keeps for reuse (a batch owns its arena: not poisoned)"""
    from pyimsegm_amd import _hip
    idle = [s for s in ctx.idle_sessions.values() if isinstance(s, _hip.Image2D)]
    return ctx.poison(word) + sum(s.poison(word) for s in idle + ([sess] if sess is not None else []))


def _baseline_bytes(hip, oracle, monkeypatch, entry):
    """capacity the small case alone leaves on a new object"""
    if entry.name not in _BASELINE:
        ctx = hip.Context()
        sess = _open(hip, entry, ctx)
        try:
            monkeypatch.setattr(hip, 'default_context', lambda: ctx)
            entry.small(Env(hip, oracle, ctx, sess, monkeypatch))
            _BASELINE[entry.name] = _poison(ctx, sess, 0)
        finally:
            if sess is not None:
                sess.close()
            ctx.close()
    return _BASELINE[entry.name]


@pytest.mark.parametrize('entry,word', PARAMS)
def test_entry_on_poisoned_scratch(hip, oracle, monkeypatch, entry, word):
    if word != WORDS[0] and entry.name in _FAILED_FIRST:
        pytest.skip('%s failed with the word 0x%08x, which is in bounds as an index: 0x%08x is not tried' % (entry.name, WORDS[0], word))
    try:
        baseline = _baseline_bytes(hip, oracle, monkeypatch, entry)
        ctx = hip.Context()
        sess = _open(hip, entry, ctx)
        try:
            monkeypatch.setattr(hip, 'default_context', lambda: ctx)
            env = Env(hip, oracle, ctx, sess, monkeypatch)
            entry.dirty(env)
            filled = _poison(ctx, sess, word)
            print('%s: %d bytes poisoned with 0x%08x (the small case alone: %d)' % (entry.name, filled, word, baseline))
            assert filled > 0 and filled >= baseline
            entry.small(env)               # from scratch on the poisoned object
            entry.small(env)               # and on what the same entry left behind
        finally:
            if sess is not None:
                sess.close()
            ctx.close()
    except BaseException:
        if word == WORDS[0]:
            _FAILED_FIRST.add(entry.name)
        raise


def test_mixture_em_refuses_a_poisoned_table(hip):
    """poisoned between kmeans_lloyd and mixture_em: the documented error for a missing table, not a fit on garbage"""
    import mixture_fit_cases as MC
    table = MC.load_table('plan_features')
    seeds = MC.seeds_of(table)
    ctx = hip.Context()
    try:
        got = hip.kmeans_lloyd(table, seeds, 300, 0., ctx=ctx)
        for word in WORDS:
            assert ctx.poison(word) > 0
            with pytest.raises(hip.HipError, match='no resident table'):
                hip.mixture_em(MC.N_RESTARTS, MC.N_CLASSES, table.shape[1], labels=got['labels'], ctx=ctx)
            with pytest.raises(hip.HipError, match='no resident table'):
                hip.mixture_em(MC.N_RESTARTS, MC.N_CLASSES, table.shape[1], ctx=ctx)
    finally:
        ctx.close()


@pytest.mark.parametrize('word', WORDS, ids=['%08x' % w for w in WORDS])
def test_getters_of_the_slic_state_refuse_a_poisoned_session(hip, word):
    """get_lab / get_nearest / get_pre_scalars go by a host flag, not by the capacity of their buffers: after a poison they say
    'slic has not been run' and do not hand out the word; after the next slic they report again"""
    from pyimsegm_amd.utilities.synthetic import disc_image
    ctx = hip.Context()
    sess = hip.Image2D(64, 64, ctx)
    try:
        sess.upload(disc_image(64)).slic(16, 10.)
        lab, nearest, scalars = sess.get_lab(), sess.get_nearest(), sess.get_pre_scalars()
        assert sess.poison(word) > 0
        for getter in (sess.get_lab, sess.get_nearest, sess.get_pre_scalars):
            with pytest.raises(hip.HipError, match='slic has not been run'):
                getter()
        sess.upload(disc_image(64)).slic(16, 10.)
        assert np.array_equal(sess.get_lab(), lab) and np.array_equal(sess.get_nearest(), nearest)
        assert np.array_equal(sess.get_pre_scalars(), scalars)
    finally:
        sess.close()
        ctx.close()
