"""The one ray walk (csrc/raywalk.h) through every entry that instantiates it: ``ray_features_binary2d``, ``ray_features_labels2d``,
``boundary_rays`` and ``object_shapes`` agree with each other and with the one host statement (``descriptors.ray_walk_host``) byte
for byte.  (``RegionGrowing.object_rays`` is held to the same host walk by test_gpu_region_growing.py::test_object_rays.)  Maps of a
single row and column, beside and across a wave; positions on and off the mask, on the image border and outside the image; fewer
angles than lanes, and more."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHAPES = [(1, 97), (97, 1), (61, 67), (64, 130)]
#: angle step -> number of angles
ANGLES = {45: 8, 7: 52, 1: 360}
EDGES = {'up': 1, 'down': -1}


@pytest.fixture(scope='module')
def hip():
    from pyimsegm_amd import _hip
    _hip.default_context()
    return _hip


def discs(shape):
    """(objects, positions): int32 map of a few discs, one value each, some cut by the border of the map; the positions are one on a
    disc, one off them, one on a border pixel of the image and three outside it (row -1, row H, column W)"""
    height, width = shape
    rng = np.random.RandomState(height * 1000 + width)
    rows, cols = np.indices(shape)
    objects = np.zeros(shape, dtype=np.int32)
    centres = [(0, width // 5), (height // 2, width // 2), (height - 1, width - 1), (height // 3, width - 2)]
    for value, (cy, cx) in enumerate(centres, 1):
        ry, rx = rng.randint(3, 2 + max(4, height // 5)), rng.randint(3, 2 + max(4, width // 5))
        objects[((rows - cy) / float(ry))**2 + ((cols - cx) / float(rx))**2 <= 1.] = value
    on = centres[1]
    off = [tuple(p) for p in np.argwhere(objects == 0) if 0 < p[0] < max(height - 1, 1) or 0 < p[1] < max(width - 1, 1)][0]
    assert objects[on] != 0 and objects[off] == 0
    return objects, [on, off, (height - 1, 0), (-1, width // 2), (height, width // 2), (height // 2, width)]


@pytest.mark.parametrize('shape', SHAPES)
@pytest.mark.parametrize('angle_step', sorted(ANGLES))
def test_entries_agree_with_the_host_walk_and_each_other(hip, shape, angle_step):
    from pyimsegm_amd import descriptors, ellipse_fitting
    directions = descriptors._ray_directions(float(angle_step))
    assert len(directions) == ANGLES[angle_step]
    objects, positions = discs(shape)
    seg = (objects != 0).astype(np.int32)                          # the discs with the value 1
    want = {name: descriptors.ray_walk_host(seg == 1, positions, directions, edge) for name, edge in EDGES.items()}
    assert all(w.dtype == np.float32 and w.shape == (6, len(directions)) for w in want.values())
    assert (want['up'][0] == 0).all() and (want['up'][3:] == -1).all() and (want['down'][3:] == -1).all()
    if min(shape) > 1 or 90 % angle_step == 0:                     # (in a single row or column only an axis direction stays inside)
        assert (want['down'][0] > 0).any() and (want['up'][1] > 0).any()

    for name, edge in EDGES.items():
        binary = hip.ray_features_binary2d(seg == 1, positions, directions, edge)
        labels = hip.ray_features_labels2d(seg, [1], positions, directions, edge)
        assert binary.tobytes() == want[name].tobytes(), name
        assert labels.tobytes() == want[name].tobytes(), name

    rays_bg, rays_fg = hip.boundary_rays(seg, 0, 0, positions, directions)
    assert rays_fg.tobytes() == want['down'].tobytes()
    background = ~ellipse_fitting.fill_holes_host(seg > 0)
    assert rays_bg.tobytes() == descriptors.ray_walk_host(background, positions, directions, 1).tobytes()
    assert rays_bg.tobytes() == hip.ray_features_binary2d(background, positions, directions, 1).tobytes()

    count, values, _, centres, rays = hip.object_shapes(objects, directions, 16)
    assert count == len(values) >= 2 and rays.shape == (count, len(directions))
    for value, centre, row in zip(values, centres, rays):
        own = hip.ray_features_binary2d(objects == value, [centre], directions, -1)[0]
        assert row.tobytes() == own.tobytes(), value
        assert row.tobytes() == descriptors.ray_walk_host(objects == value, [centre], directions, -1)[0].tobytes(), value
