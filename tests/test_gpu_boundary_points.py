"""The device path of the boundary-point step (csrc/morphology.hip behind ``imsegm_split_background_foreground`` and
``imsegm_boundary_rays``) against the host statement of pyimsegm_amd/ellipse_fitting.py, which
tests/test_boundary_points_reference_host.py ties to the reference's recorded results, to brute-force morphology and to scipy.
Everything up to the rays is integer work and the ray walk repeats the host's float operations in order, so masks, ray tables and
point lists are compared byte for byte."""
import numpy as np
import pytest

import boundary_points_cases as C
import object_shapes_cases as S

pytestmark = pytest.mark.gpu
EDGE = C.edge_cases()
POINT_FUNCTIONS = ('prepare_boundary_points_ray_join', 'prepare_boundary_points_ray_edge', 'prepare_boundary_points_ray_mean',
                   'prepare_boundary_points_ray_dist')


@pytest.fixture(scope='module')
def hip():
    from pyimsegm_amd import _hip
    _hip.default_context()
    return _hip


@pytest.fixture(scope='module')
def ell(hip):
    from pyimsegm_amd import ellipse_fitting
    return ellipse_fitting


@pytest.fixture(scope='module')
def directions():
    from pyimsegm_amd import descriptors
    return descriptors._ray_directions(5.)


@pytest.fixture(scope='module')
def host_results(ell, directions):
    """masks and ray tables of the host statement for every edge map, computed once"""
    results = {}
    for name, case in EDGE.items():
        masks = ell.split_host(case['seg'], case['sel_bg'], case['sel_fg'])
        rays = ell.boundary_rays_host(case['seg'], case['sel_bg'], case['sel_fg'], case['centers'], directions)
        results[name] = masks, rays
    return results


def same_bytes(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def point_call(ell, name, case, centers, on):
    if name.endswith('dist'):
        return lambda: getattr(ell, name)(case['seg'], centers, C.CLOSE_POINTS, case['sel_bg'], case['sel_fg'], on=on)
    return lambda: getattr(ell, name)(case['seg'], centers, C.CLOSE_POINTS, C.MIN_DIAM, case['sel_bg'], case['sel_fg'], on=on)


@pytest.mark.parametrize('name', sorted(EDGE))
def test_masks_equal_the_host_statement(hip, host_results, name):
    case = EDGE[name]
    (want_bg, want_fg), _ = host_results[name]
    seg_bg, seg_fg = hip.split_background_foreground(case['seg'].astype(np.int32), case['sel_bg'], case['sel_fg'])
    assert same_bytes(seg_bg, want_bg.astype(np.uint8)), name
    assert same_bytes(seg_fg, want_fg.astype(np.uint8)), name
    again = hip.split_background_foreground(case['seg'].astype(np.int32), case['sel_bg'], case['sel_fg'])
    assert same_bytes(again[0], seg_bg) and same_bytes(again[1], seg_fg)


@pytest.mark.parametrize('shape', S.SEAM_SHAPES)
@pytest.mark.parametrize('multi', [False, True])
def test_holes_in_rows_of_more_than_one_chunk(hip, ell, shape, multi):
    """maps wider than 256 pixels, inverted so that the objects around the seam between two chunks of a row are the holes"""
    objects = S.seam_map(shape, multi)
    seg = np.where(objects != 0, 0, 1).astype(np.int32)
    seg_bg, seg_fg = hip.split_background_foreground(seg, 0, 0)
    want_bg, want_fg = ell.split_host(seg, 0, 0)
    assert same_bytes(seg_bg, want_bg.astype(np.uint8)) and same_bytes(seg_fg, want_fg.astype(np.uint8))
    # the run lies on the border; the U and the pixel are holes unless column 256 is the border itself
    assert seg_bg[0, 240:257].all() and seg_bg[2:8].any() == (shape[1] == 257)


@pytest.mark.parametrize('name', sorted(EDGE))
def test_rays_equal_the_host_statement(hip, host_results, directions, name):
    case = EDGE[name]
    _, (want_bg, want_fg) = host_results[name]
    seg = case['seg'].astype(np.int32)
    rays_bg, rays_fg = hip.boundary_rays(seg, case['sel_bg'], case['sel_fg'], case['centers'], directions)
    assert same_bytes(rays_bg, want_bg) and same_bytes(rays_fg, want_fg), name
    height, width = seg.shape
    off = [i for i, (row, col) in enumerate(case['centers']) if not (0 <= row < height and 0 <= col < width)]
    assert len(off) == 3 and np.all(rays_bg[off] == -1) and np.all(rays_fg[off] == -1)
    again = hip.boundary_rays(seg, case['sel_bg'], case['sel_fg'], case['centers'], directions)
    assert same_bytes(again[0], rays_bg) and same_bytes(again[1], rays_fg)
    # without the foreground output the foreground is not opened and the background rays stay what they are
    alone, nothing = hip.boundary_rays(seg, case['sel_bg'], case['sel_fg'], case['centers'], directions, with_fg=False)
    assert nothing is None and same_bytes(alone, rays_bg)


@pytest.mark.parametrize('name', sorted(EDGE))
def test_point_lists_equal_the_host_statement(ell, name):
    case = EDGE[name]
    centers = C.inside(case)
    for function in POINT_FUNCTIONS:
        for chosen in (centers, centers[2:3], case['centers']):
            kind, got = C.outcome(point_call(ell, function, case, chosen, 'device'))
            kind_host, want = C.outcome(point_call(ell, function, case, chosen, 'host'))
            assert kind == kind_host, (name, function, got, want)
            if kind == 'points':
                assert len(got) == len(want), (name, function)
                assert all(same_bytes(a, b) for a, b in zip(got, want)), (name, function)
            else:
                assert got == want


def test_public_split_and_golden_points(ell):
    call = dict(C.ELLIPSE_CALL)
    seg = C.ellipse_map()
    points = ell.prepare_boundary_points_ray_dist(seg, call.pop('centers'), call.pop('close_points'), on='device', **call)
    assert len(points) == 1 and np.abs(points[0] - C.golden_points()).max() <= C.ELLIPSE_TOLERANCE
    fixture = C.doctest_fixture()
    for name, example in fixture['examples'].items():
        arguments = {k: v for k, v in example.items() if k not in ('points', 'decimals', 'close_points')}
        got = getattr(ell, name)(fixture['seg'], fixture['centers'], example['close_points'], on='device', **arguments)
        assert np.round(got, example['decimals']).tolist() == example['points'], name
    for name in ('nested', 'labels_above_1_int64', 'seams_w65'):
        case = EDGE[name]
        got = ell.split_segm_background_foreground(case['seg'], case['sel_bg'], case['sel_fg'], on='device')
        want = ell.split_segm_background_foreground(case['seg'], case['sel_bg'], case['sel_fg'], on='host')
        assert same_bytes(got[0], want[0]) and same_bytes(got[1], want[1]) and got[1].dtype == bool


def test_refusals_are_errors_without_a_launch(hip, directions):
    seg = EDGE['nested']['seg']
    centers = EDGE['nested']['centers']
    above = hip.MORPH_MAX_RADIUS + 1
    for sel_bg, sel_fg in ((above, 1), (1, above)):
        with pytest.raises(hip.HipError, match='IMSEGM_MORPH_MAX_RADIUS'):
            hip.split_background_foreground(seg, sel_bg, sel_fg)
        with pytest.raises(hip.HipError, match='IMSEGM_MORPH_MAX_RADIUS'):
            hip.boundary_rays(seg, sel_bg, sel_fg, centers, directions)
    with pytest.raises(hip.HipError, match='IMSEGM_RAY_MAX_ANGLES'):
        hip.boundary_rays(seg, 2, 1, centers, np.tile(directions, (hip.RAY_MAX_ANGLES // len(directions) + 1, 1)))
    with pytest.raises(hip.HipError, match='IMSEGM_RAY_MAX_ANGLES'):
        hip.boundary_rays(seg, 2, 1, centers, directions[:0])
    for shape in ((0, 5), (5, 0)):
        with pytest.raises(hip.HipError, match='positive'):
            hip.split_background_foreground(np.zeros(shape, dtype=np.int32), 1, 1)
        with pytest.raises(hip.HipError, match='positive'):
            hip.boundary_rays(np.zeros(shape, dtype=np.int32), 1, 1, centers, directions)
    # the largest radius is taken, and the library goes on working
    seg_bg, _ = hip.split_background_foreground(seg, hip.MORPH_MAX_RADIUS, 1)
    assert seg_bg.shape == seg.shape
    empty = hip.boundary_rays(seg, 2, 1, np.zeros((0, 2), dtype=np.int32), directions)
    assert empty[0].shape == (0, len(directions)) and empty[1].shape == (0, len(directions))


def test_place_switch(hip, ell, monkeypatch):
    case = EDGE['nested']
    centers = C.inside(case)
    want = ell.prepare_boundary_points_ray_edge(case['seg'], centers, C.CLOSE_POINTS, C.MIN_DIAM, 2, 1, on='device')

    def refuse(*args, **kwargs):
        raise AssertionError('the device was called')

    monkeypatch.setattr(hip, 'boundary_rays', refuse)
    monkeypatch.setattr(hip, 'split_background_foreground', refuse)
    got = ell.prepare_boundary_points_ray_edge(case['seg'], centers, C.CLOSE_POINTS, C.MIN_DIAM, 2, 1, on='host')
    assert all(same_bytes(a, b) for a, b in zip(got, want))
    monkeypatch.setenv('IMSEGM_BOUNDARY_POINTS_ON', 'host')
    got = ell.prepare_boundary_points_ray_edge(case['seg'], centers, C.CLOSE_POINTS, C.MIN_DIAM, 2, 1)
    assert all(same_bytes(a, b) for a, b in zip(got, want))
    ell.split_segm_background_foreground(case['seg'], 2, 1)
    with pytest.raises(AssertionError, match='the device was called'):
        ell.prepare_boundary_points_ray_edge(case['seg'], centers, C.CLOSE_POINTS, C.MIN_DIAM, 2, 1, on='device')
    monkeypatch.delenv('IMSEGM_BOUNDARY_POINTS_ON')
    with pytest.raises(AssertionError, match='the device was called'):
        ell.split_segm_background_foreground(case['seg'], 2, 1)
    # a radius above the device's maximum: the host statement takes over
    above = hip.MORPH_MAX_RADIUS + 1
    ell.split_segm_background_foreground(case['seg'], above, 1)
    # (a disc of that size leaves nothing of this map's background: no ray meets an edge, which is the reference's ValueError)
    assert C.outcome(lambda: ell.prepare_boundary_points_ray_dist(case['seg'], centers[2:3], C.CLOSE_POINTS, above, 1)) == \
        C.outcome(lambda: ell.prepare_boundary_points_ray_dist(case['seg'], centers[2:3], C.CLOSE_POINTS, above, 1, on='host'))
    rays = ell._centre_rays(case['seg'], centers, 1, above, True, None)
    assert rays[0].shape == (len(centers), 72) and rays[1].shape == rays[0].shape
