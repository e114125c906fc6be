"""csrc/colorspace.hip and what is routed over it: the device's conversion of every case of tests/colorspace_cases.py against the
80-bit reference (hsv bit for bit numpy's, xyz / lab / luv bit for bit the float64 transcription of the kernel, hed within the
tolerance only: the device's ``log`` is no deterministic function of this project), against real scikit-image outputs, the
switch of the statistic entry points to the converted image and back, the feature tables and the pipeline with
``convert_on='device'``, the environment switch and the refusals of ``imsegm_image2d_convert_color``."""
import os
import zlib

import numpy as np
import pytest

import colorspace_cases as CC

pytestmark = pytest.mark.gpu

CASES = CC.cases() if CC.LONGDOUBLE_OK else ()
IDS = [c['id'] for c in CASES]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
BOUND = 1e-5             # the project's descriptor bound (README): 1e-5 x max(1, |expected|)

_RUNS = {}


@pytest.fixture(scope='module')
def hip():
    from pyimsegm_amd import _hip
    _hip.default_context()
    return _hip


def matrix_of(space):
    from pyimsegm_amd.utilities.data_io import _HED_FROM_RGB
    return _HED_FROM_RGB if space == 'hed' else None


def convert(hip, image, spaces=CC.SPACES):
    sess = hip.Image2D(*image.shape[:2])
    try:
        sess.upload(image)
        return {space: sess.convert_color(space, matrix_of(space)).converted() for space in spaces}
    finally:
        sess.close()


def run(hip, c):
    """the five conversions of a case on the device, once per process, read-only"""
    if c['id'] not in _RUNS:
        out = convert(hip, c['image'])
        for arr in out.values():
            arr.setflags(write=False)
        _RUNS[c['id']] = out
    return _RUNS[c['id']]


def voronoi(shape, dtype=np.uint8):
    from pyimsegm_amd.utilities.synthetic import voronoi_image
    image = np.asarray(voronoi_image(shape[0], shape[1]))
    assert image.dtype == np.uint8 and image.shape == shape + (3, )
    return image if dtype == np.uint8 else image.astype(np.float64) / 255


def blocks_map(shape, size=16):
    rows, cols = np.indices(shape) // size
    return (rows * ((shape[1] + size - 1) // size) + cols).astype(np.int64)


@pytest.mark.skipif(not CC.LONGDOUBLE_OK, reason=CC.LONGDOUBLE_REASON)
@pytest.mark.parametrize('space', CC.SPACES)
@pytest.mark.parametrize('c', CASES, ids=IDS)
def test_conversion_against_the_80_bit_reference(hip, c, space):
    ref = CC.reference(c['id'], space)
    got = run(hip, c)[space]
    dev = CC.rel_dev(got, ref['ref'])
    print('%-20s %-3s yardstick %.2e  tolerance %.2e  device %.2e' % (c['id'], space, ref['yardstick'], ref['tol'], dev))
    assert got.shape == c['shape'] + (3, )
    assert dev <= ref['tol'], (c['id'], space, dev, ref['tol'])
    if space == 'hsv':
        assert np.array_equal(got, CC.yardstick64(c['image'], 'hsv'))
    elif space != 'hed':
        assert np.array_equal(got, CC.model64(c['image'], space))


@pytest.mark.parametrize('space', CC.SPACES)
def test_conversion_against_scikit_image(hip, space):
    """the vectors of tests/golden/skimage.npz (real scikit-image 0.18.3), inputs regenerated and CRC-checked as
    tests/test_golden_skimage.py does, within its bound"""
    vec = np.load(os.path.join(GOLDEN, 'skimage.npz'), allow_pickle=False)
    rgb_f = np.random.default_rng(11).random((13, 17, 3))
    rgb_u8 = (np.random.default_rng(12).random((11, 9, 3)) * 255).astype(np.uint8)
    assert [zlib.crc32(rgb_f.tobytes()), zlib.crc32(rgb_u8.tobytes())] == vec['color_crc'].tolist()
    for tag, rgb in (('f64', rgb_f), ('u8', rgb_u8)):
        ref = vec['color_%s_%s' % (space, tag)]
        out = convert(hip, rgb, (space, ))[space]
        scale = max(1.0, float(np.abs(ref).max()))
        assert out.shape == ref.shape and np.max(np.abs(out - ref)) <= 1e-12 * scale, (space, tag, np.max(np.abs(out - ref)))


@pytest.mark.parametrize('dtype', [np.uint8, np.float32, np.float64])
def test_statistics_switch_to_the_converted_image_and_back(hip, dtype):
    rng = np.random.RandomState(CC.SEED)
    shape = (37, 53)
    image = rng.randint(0, 256, shape + (3, )).astype(np.uint8)
    image = image if dtype == np.uint8 else (image / 255.).astype(dtype)
    segm = blocks_map(shape, 8)
    from pyimsegm_amd.descriptors import MAX_SIGNAL_RESPONSE, _select_bank
    batteries, _ = _select_bank('short')

    def everything(sess):
        return list(sess.color_stats()) + [sess.median(), sess.mean_gradient(), sess.features_color()]

    def texture(sess):
        return sess.lm_prepare(150.).lm_features(batteries, MAX_SIGNAL_RESPONSE)

    sess = hip.Image2D(*shape).upload(image).set_labels(segm)
    other = hip.Image2D(*shape)
    try:
        rgb_stats, rgb_texture = everything(sess), texture(sess)
        lab = sess.convert_color('lab').converted()
        assert np.array_equal(lab, convert(hip, image, ('lab', ))['lab'])
        lab_stats = everything(sess)
        assert np.array_equal(texture(sess), rgb_texture)                   # lm_prepare keeps reading the RGB upload
        assert all(np.array_equal(a, b) for a, b in zip(everything(sess), lab_stats))
        other.upload(lab).set_labels(segm)                                  # the same bytes through the same kernels
        expected = everything(other)
        assert len(expected) == len(lab_stats) == 6
        for a, b in zip(lab_stats, expected):
            assert np.array_equal(a, b, equal_nan=True)
        assert not np.array_equal(lab_stats[0], rgb_stats[0])
        sess.convert_color(0)
        for a, b in zip(everything(sess), rgb_stats):
            assert np.array_equal(a, b, equal_nan=True)
        sess.convert_color('hsv')
        sess.upload(image)                                                  # an upload returns to the uploaded image too
        for a, b in zip(everything(sess), rgb_stats):
            assert np.array_equal(a, b, equal_nan=True)
    finally:
        sess.close()
        other.close()


@pytest.mark.parametrize('dtype', ['uint8', 'float64'])
@pytest.mark.parametrize('space', CC.SPACES)
def test_feature_table_of_a_colour_space(hip, space, dtype):
    from pyimsegm_amd.descriptors import NAMES_FEATURE_FLAGS, compute_selected_features_color2d
    image = voronoi((96, 128), np.dtype(dtype))
    segm = blocks_map((96, 128))
    flags = {'color_' + space: NAMES_FEATURE_FLAGS}
    expected, names = compute_selected_features_color2d(image, segm, flags)
    got, got_names = compute_selected_features_color2d(image, segm, flags, convert_on='device')
    assert got_names == names and got.shape == expected.shape == (48, 15)
    print(space, dtype, float(np.max(np.abs(got - expected) / np.maximum(1, np.abs(expected)))))
    if space == 'hsv':
        assert np.array_equal(got, expected)
    else:
        assert np.all(np.abs(got - expected) <= BOUND * np.maximum(1, np.abs(expected)))
    on_host, _ = compute_selected_features_color2d(image, segm, flags, convert_on='host')
    assert np.array_equal(on_host, expected)


def test_resident_table_with_a_colour_space(hip):
    from pyimsegm_amd.descriptors import compute_selected_features_img2d
    from pyimsegm_amd.pipelines import _ResidentImage
    image = voronoi((96, 128))
    feats = {'color_lab': ('mean', 'std'), 'color': ('energy', ), 'tLM_short': ('mean', )}
    res = _ResidentImage(image, feats, 14, 0.2, features_to_host=False, convert_on='device')
    try:
        assert res.resident_features
        expected, names = compute_selected_features_img2d(image, res.slic, feats)
        table = res.features
        assert table.shape == expected.shape == (res.nb_labels, len(names))
        assert [n.split('-')[0] for n in names[:9]] == ['lab'] * 6 + ['rgb'] * 3
        assert np.all(np.abs(table - expected) <= BOUND * np.maximum(1, np.abs(expected)))
        # the RGB statistics are the uploaded image's again
        assert np.array_equal(res.sess.features_color(False, False, True), expected[:, 6:9])
    finally:
        res.close()
    res = _ResidentImage(image, feats, 14, 0.2, features_to_host=False)
    try:
        assert not res.resident_features
    finally:
        res.close()


def _pipeline(image, **kwargs):
    from pyimsegm_amd.pipelines import pipe_color2d_slic_features_model_graphcut
    np.random.seed(0)
    return pipe_color2d_slic_features_model_graphcut(image, 3, {'color_hsv': ('mean', 'std', 'energy')}, sp_size=15, sp_regul=0.2,
                                                     gc_regul=1., **kwargs)


@pytest.fixture(scope='module')
def pipeline_image():
    return voronoi((150, 200))


@pytest.fixture(scope='module')
def pipeline_on_host(hip, pipeline_image):
    segm, soft = _pipeline(pipeline_image)
    segm.setflags(write=False)
    soft.setflags(write=False)
    return segm, soft


def check_pipeline(result, on_host):
    """hsv is converted bit for bit, so the feature table and the fitted model are the host path's, and so are the class map
    and the soft segmentation (measured on the MI355X: largest difference of the soft segmentation 0.0)"""
    segm, soft = result
    print('soft segmentation: max difference', float(np.max(np.abs(soft - on_host[1]))))
    assert np.array_equal(segm, on_host[0])
    assert np.array_equal(soft, on_host[1])


def test_pipeline_with_conversion_on_the_device(pipeline_image, pipeline_on_host):
    check_pipeline(_pipeline(pipeline_image, convert_on='device'), pipeline_on_host)


def test_environment_switch(monkeypatch, pipeline_image, pipeline_on_host):
    from pyimsegm_amd.pipelines import _ResidentImage
    monkeypatch.setenv('IMSEGM_CONVERT_ON', 'device')
    res = _ResidentImage(pipeline_image, {'color_hsv': ('mean', )}, 15, 0.2)
    try:
        assert res.resident_features
    finally:
        res.close()
    check_pipeline(_pipeline(pipeline_image), pipeline_on_host)
    with pytest.raises(ValueError):
        _pipeline(pipeline_image, convert_on='nowhere')
    monkeypatch.setenv('IMSEGM_CONVERT_ON', 'nowhere')
    with pytest.raises(ValueError):
        _pipeline(pipeline_image)


def test_refusals(hip):
    """none of these launches a kernel"""
    image = np.zeros((4, 6, 3), dtype=np.uint8)
    sess = hip.Image2D(4, 6)
    vol = hip.Volume3D(2, 4, 6)
    try:
        with pytest.raises(hip.HipError):
            sess.convert_color('lab')                       # before an upload
        sess.upload(image)
        with pytest.raises(hip.HipError):
            sess.convert_color(9)
        with pytest.raises(hip.HipError):
            sess.convert_color(-1)
        with pytest.raises(hip.HipError):
            sess.convert_color('hed')                       # no matrix
        with pytest.raises(hip.HipError):
            sess.converted()                                # nothing has been converted
        vol.upload(np.zeros((2, 4, 6), dtype=np.uint8))
        with pytest.raises(hip.HipError):
            vol.convert_color('lab')
        sess.convert_color(0)                               # allowed at any time after an upload
    finally:
        sess.close()
        vol.close()
