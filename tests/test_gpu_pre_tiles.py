"""The radius-4 k_pre_fused of csrc/slic_pre.hip (64 x 32 tiles, the y blur out of register windows of 8 rows, written back in
place) bit for bit against the oracle's planes, at the sizes where that layout can go wrong: 3 x 5 (both extents below the halo:
reflection folds twice), exactly one tile, one tile plus one row and one column, two tiles minus one in each direction, and
2 T_y + 7 rows by 130 columns -- for uint8, float32 and float64 images, with the min / max normalisation on (uint8 0 .. 255,
float32 in [-1, 2]) and off (a float64 image already in 0 .. 1), and for a batch of two images of different content through
Batch2D.  ``premax`` is compared with the largest |value| of the oracle's planes.

Planes are fetched as tests/test_gpu_pre_reference.py fetches them (``Image2D.slic(max_iter=1)`` then ``get_lab()`` and
``get_pre_scalars()``).  A float32 image reaches the oracle widened to float64 (exact), which is what the kernel does with it."""
import numpy as np
import pytest

import pre_cases as P

pytestmark = pytest.mark.gpu

T_X, T_Y = 64, 32                  # the tile of the radius-4 kernel (P4_TY, PF_TX)
SHAPES = [(3, 5), (T_Y, T_X), (T_Y + 1, T_X + 1), (2 * T_Y - 1, 2 * T_X - 1), (2 * T_Y + 7, 130)]
KINDS = ['u8-full', 'f32-wide', 'f64-unit']      # normalisation on, on, off
SIGMA = 1.0                        # radius 4


def _cases():
    out = []
    for shape in SHAPES:
        for kind in KINDS:
            out.append(P._case('tiles-%dx%d-%s' % (shape + (kind, )), P.make_image(kind, shape, 5), SIGMA, P.NORMALIZE_OF[kind]))
    return out


CASES = _cases()
_ORACLE = {}


@pytest.fixture(scope='module')
def hip():
    from pyimsegm_amd import _hip
    _hip.default_context()
    return _hip


def oracle_planes(oracle, image, n_segments, compactness, normalize):
    """the oracle's [3, H, W] planes and whether it scaled the image, decided as superpixels.py:53-54 decides it"""
    x = P.widen(image)
    vmin, vmax = float(x.min()), float(x.max())
    on = P.scaled(normalize, vmin, vmax)
    _, info = oracle.slic(np.array(image if image.dtype != np.float32 else x), n_segments, compactness, sigma=SIGMA,
                          normalize=(vmin, vmax) if on else None, max_iter=1, enforce_connectivity=False, return_internals=True)
    return info['pre'].reshape((3, ) + image.shape[:2]), on


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a, np.float64).view(np.uint64),
                                                 np.ascontiguousarray(b, np.float64).view(np.uint64))


def test_the_cases_take_the_radius_4_kernel_with_both_normalisation_arms(oracle):
    assert P.radius_of(SIGMA) == 4
    arms = set()
    for c in CASES:
        if c['id'] not in _ORACLE:
            _ORACLE[c['id']] = oracle_planes(oracle, c['image'], P.n_segments_of(c), c['compactness'], c['normalize'])
        arms.add((c['dtype'], _ORACLE[c['id']][1]))
    assert arms == {('u8', True), ('f32', True), ('f64', False)}


@pytest.mark.parametrize('c', CASES, ids=[c['id'] for c in CASES])
def test_planes_and_premax_equal_the_oracle(hip, oracle, c):
    if c['id'] not in _ORACLE:
        _ORACLE[c['id']] = oracle_planes(oracle, c['image'], P.n_segments_of(c), c['compactness'], c['normalize'])
    want, _ = _ORACLE[c['id']]
    sess = hip.Image2D(*c['shape'])
    try:
        sess.upload(c['image'])
        sess.slic(P.n_segments_of(c), c['compactness'], sigma=c['sigma'], normalize=c['normalize'], max_iter=1,
                  enforce_connectivity=False)
        lab, (vmin, vmax, premax) = sess.get_lab(), sess.get_pre_scalars()
    finally:
        sess.close()
    differ = int(np.sum(lab.view(np.uint64) != want.view(np.uint64))) if lab.shape == want.shape else -1
    print('%-28s elements that differ %d  premax %.17g  oracle %.17g' % (c['id'], differ, premax, float(np.abs(want).max())))
    assert same_bits(lab, want), c['id']
    assert vmin == float(c['image'].min()) and vmax == float(c['image'].max())
    assert premax == float(np.abs(want).max())


@pytest.mark.parametrize('dtype', ['u8', 'f64'])
def test_batch_of_two_different_images(hip, oracle, dtype):
    """image = blockIdx.z: each image of a batch has its own planes, extremes and premax"""
    from pyimsegm_amd import pipelines as pipe
    from pyimsegm_amd.descriptors import FEATURES_SET_COLOR
    from pyimsegm_amd.graph_cuts import estim_class_model
    from pyimsegm_amd.superpixels import _slic_params
    from pyimsegm_amd.utilities.synthetic import voronoi_image
    shape, sp_size, sp_regul = SHAPES[-1], 12, 0.2
    images = [voronoi_image(shape[0], shape[1], seed=61), voronoi_image(shape[0], shape[1], seed=62)]
    if dtype == 'f64':               # the second one beyond 0 .. 1
        images = [images[0] / 255., images[1] * (1.5 / 255.) - 0.2]
    assert images[0].dtype == images[1].dtype == (np.uint8 if dtype == 'u8' else np.float64)
    np.random.seed(0)
    res = pipe._ResidentImage(images[0], FEATURES_SET_COLOR, sp_size, sp_regul)
    model = estim_class_model(res.features, 3, 'GMM', None, True)
    res.close()
    got = []
    segm = pipe._segment_color2d_batch_call(images, model, FEATURES_SET_COLOR, sp_size, sp_regul, 2.0, 'model',
                                            with_batch=lambda b: got.extend((b.get_lab(i), b.get_pre_scalars(i)) for i in range(2)))
    assert segm is not None and len(got) == 2
    n_seg, compact = _slic_params(shape, sp_size, sp_regul)
    for image, (lab, (vmin, vmax, premax)) in zip(images, got):
        want, _ = oracle_planes(oracle, image, n_seg, compact, 2)
        assert same_bits(lab, want)
        assert vmin == float(image.min()) and vmax == float(image.max())
        assert premax == float(np.abs(want).max())
    assert not np.array_equal(got[0][0], got[1][0])
