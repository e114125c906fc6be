"""CPU checks of tests/boundary3d_cases.py, which tests/test_gpu_boundary3d.py holds the volume kernels (csrc/boundary3d.hip) to,
and of the host side of ``pyimsegm_amd.labeling.compute_boundary_distances`` on 3-D maps: the definitions agree with the brute
force and with shifted comparisons, the stated point counts are those of the generated maps, the host statement of the package
equals the definitions, ``on`` and the routing of what the device does not take behave as documented, and the new source and
symbols are where the build and the header say."""
import os
import re

import numpy as np
import pytest

import boundary3d_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_scipy_is_the_integer_minimum_and_the_mask_is_the_shifted_comparison():
    checked = 0
    for name, seg in C.maps().items():
        mask = C.thick(seg)
        assert mask.dtype == bool and np.array_equal(mask, C.thick_shifted(seg)), name
        if C.brute_fits(mask):
            assert C.same(C.edt(mask), C.edt_brute(mask)), name
            checked += 1
    assert checked >= 50
    # no set voxel: scipy answers with the distance to (slice -1, row 0, column 0); the depth pass restates exactly this
    for shape in ((1, 1, 1), (2, 3, 4), (5, 1, 9), (4, 6, 70)):
        z, y, x = np.indices(shape)
        assert C.same(C.edt(np.zeros(shape, dtype=bool)), np.sqrt(((z + 1)**2 + y**2 + x**2).astype(np.float64))), shape


def test_stated_counts_and_layouts_are_those_of_the_maps():
    maps = C.maps()
    chunk = C.compaction_chunk()
    assert chunk == 2048
    counts = C.COMPACTION_COUNTS
    assert (counts['none'], counts['two'], counts['one_chunk'], counts['one_chunk_and_one'], counts['two_chunks']) == \
        (0, 2, chunk, chunk + 1, 2 * chunk)
    for key, count in counts.items():
        name = C.compaction_name(key)
        assert str(chunk) in name and str(count) in name
        assert int(C.thick(maps[name]).sum()) == count, name
    assert counts['every_voxel'] == maps[C.compaction_name('every_voxel')].size == 4 * 24 * 33 > chunk
    slices = lambda name: C.thick(maps[name]).any(axis=(1, 2)).astype(int).tolist()
    assert slices('middle_slices_9x12x70') == [0, 0, 0, 1, 1, 1, 0, 0, 0]
    assert slices('first_slices_9x12x70') == [1, 1, 0, 0, 0, 0, 0, 0, 0] and slices('last_slices_9x12x70') == [0, 0, 0, 0, 0, 0, 0, 1, 1]
    assert not C.thick(maps['constant_4x6x70']).any() and int(C.thick(maps['far_corner_9x40x300']).sum()) == 4
    for depth in (1, 2):
        name = 'long_row_%dx1x65535' % depth
        largest = 65533**2 + (depth - 1)            # slice 0: set voxels at x = 0 and 1; slice 1: at x = 0, one slice away from (0, 0, 1)
        assert float(C.distance_map(name).max()) == float(np.sqrt(np.float64(largest))) and 2**31 < largest < 2**32 - 1, name
        assert depth**2 + 1 + 65535**2 <= 2**32 - 1
    empty = [len(C.boundary_distances(a, b)[0]) == 0 for a, b in C.pair_cases()]
    assert sum(empty) >= 3 and not all(empty)


def test_host_statement_of_the_package_equals_the_definitions():
    from pyimsegm_amd import labeling
    for ref_name, name in C.small_pair_cases():
        points, dist = labeling.compute_boundary_distances(C.maps()[ref_name], C.maps()[name], on='host')
        want_points, want_dist = C.boundary_distances(ref_name, name)
        assert C.same(points, want_points) and C.same(dist, want_dist), (ref_name, name)
        assert points.shape[1:] == (3, ) and dist.shape == (len(points), )
    assert len(C.small_pair_cases()) >= 60


def test_place_keyword(monkeypatch):
    from pyimsegm_amd import _hip, labeling
    seg = C.maps()['rand_5x6x7_L3']
    monkeypatch.delenv('IMSEGM_BOUNDARY3D_ON', raising=False)
    for bad in ('gpu', 'cpu', '', 1):
        with pytest.raises(ValueError):
            labeling.compute_boundary_distances(seg, seg, on=bad)
    monkeypatch.setenv('IMSEGM_BOUNDARY3D_ON', 'nowhere')
    with pytest.raises(ValueError):
        labeling.compute_boundary_distances(seg, seg)
    monkeypatch.setenv('IMSEGM_BOUNDARY3D_ON', 'host')
    want = C.boundary_distances('rand_5x6x7_L3', 'rand_5x6x7_L3')
    got = labeling.compute_boundary_distances(seg, seg)
    assert C.same(got[0], want[0]) and C.same(got[1], want[1])
    # 'device' without a device raises, as a keyword and from the variable (a machine with a device runs the call instead)
    monkeypatch.setattr(_hip, 'device_count', lambda: 0)
    with pytest.raises(_hip.HipUnavailableError):
        labeling.compute_boundary_distances(seg, seg, on='device')
    monkeypatch.setenv('IMSEGM_BOUNDARY3D_ON', 'device')
    with pytest.raises(_hip.HipUnavailableError):
        labeling.compute_boundary_distances(seg, seg)


def test_what_the_device_does_not_take_goes_to_the_host(monkeypatch):
    """float labels, labels outside int32 and shapes beyond the kernels' limits never reach the device calls: they are replaced by
    ones that fail, and a device is claimed to be present"""
    from pyimsegm_amd import _hip, labeling

    def refuse(*args, **kwargs):
        raise AssertionError('a device call')

    monkeypatch.delenv('IMSEGM_BOUNDARY3D_ON', raising=False)
    monkeypatch.setattr(_hip, 'device_count', lambda: 1)
    monkeypatch.setattr(_hip, 'boundary_distances3d', refuse)
    monkeypatch.setattr(_hip, 'boundary_distances', refuse)
    seg_ref = C.maps()['rand_5x6x7_L3']
    seg = np.resize(C.maps()['rand_4x6x70_L2'], seg_ref.shape)
    want = (np.argwhere(C.thick(seg_ref)).astype(np.int64), C.edt(C.thick(seg))[C.thick(seg_ref)])
    wide = seg.copy()
    wide[wide == 1] = 2**31                          # (one label beyond int32: the mask is that of `seg`)
    for a, b in ((seg_ref.astype(np.float64), seg), (seg_ref, seg.astype(np.float32)), (seg_ref, wide)):
        for on in (None, 'device'):
            points, dist = labeling.compute_boundary_distances(a, b, on=on)
            assert C.same(points, want[0]) and C.same(dist, want[1])
    # four dimensions: the host statement, n x 4 points
    points, dist = labeling.compute_boundary_distances(seg_ref.reshape(5, 6, 7, 1), seg.reshape(5, 6, 7, 1))
    assert points.shape[1] == 4 and C.same(dist, want[1])
    # an int32 pair does go to the device call
    with pytest.raises(AssertionError, match='a device call'):
        labeling.compute_boundary_distances(seg_ref, seg)
    # the limits, on the shape alone: D^2 + H^2 + W^2 <= 2^32 - 1, at most 2^30 voxels, three positive extents
    fits = _hip.boundary3d_fits
    assert fits((1, 1, 1)) and fits((64, 4096, 4096)) and fits((1024, 1024, 1024)) and fits((2, 1, 65535)) and fits((16, 8192, 8192))
    assert not fits((1, 1, 65536)) and not fits((65536, 1, 1)) and not fits((1, 46341, 46341)) and not fits((1025, 1024, 1024))
    assert not fits((65, 4096, 4096)) and not fits((0, 4, 4)) and not fits((4, 4)) and not fits((1, 2, 3, 4))
    assert 1 + 46340**2 + 46340**2 <= 2**32 - 1 < 1 + 46341**2 + 46341**2 and not fits((1, 46340, 46340))       # (2^30 voxels come first)
    assert labeling._device_volume(np.broadcast_to(np.int32(0), (65, 4096, 4096))) is None


def test_new_source_and_symbols_are_declared():
    from pyimsegm_amd import build
    assert 'boundary3d.hip' in build.SOURCES and 'boundary.hip' in build.SOURCES and 'api_boundary.hip' in build.SOURCES
    assert os.path.exists(os.path.join(build.CSRC, 'boundary3d.hip'))
    assert not [flag for flag in build.FLAGS if 'fast' in flag or 'unsafe' in flag or 'approx' in flag or 'finite-math' in flag]
    header = open(os.path.join(ROOT, 'include', 'imsegm_hip.h')).read()
    declared = set(re.findall(r'IMSEGM_API\s+[\w\s\*]*?\b(imsegm_\w+)\s*\(', header))
    wanted = {'imsegm_boundary_mask3d', 'imsegm_distance_map3d', 'imsegm_boundary_distances3d', 'imsegm_volume_boundary_distances'}
    assert wanted <= declared
    from pyimsegm_amd import _hip
    for name in ('boundary_mask3d', 'distance_map3d', 'boundary_distances3d', 'boundary3d_fits'):
        assert callable(getattr(_hip, name)), name
    assert _hip.Volume3D.boundary_distances is not _hip.Image2D.boundary_distances
