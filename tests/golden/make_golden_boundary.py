#!/usr/bin/env python
"""Golden vectors of the scoring functions of the reference's `imsegm/labeling.py` -- contour_binary_map, contour_coords,
compute_distance_map, compute_boundary_distances, compute_labels_overlap_matrix, relabel_max_overlap_unique,
relabel_max_overlap_merge -- from a run of the UNCHANGED reference module under the build container's conda Python 3.9 with the
real scikit-image 0.18.3 and its scipy (build container: /opt/conda/bin/python3.9 tests/golden/make_golden_boundary.py).

The reference module is imported from the reference tree as it is.  It spells its integer dtype `np.int`, an alias numpy 1.24
removed; the interpreter's numpy gets that alias back for this process (`np.int = int`, what it always meant) -- the only
accommodation, and none to the reference.  nibabel / OleFileIO_PL, which `imsegm.utilities.data_io` imports and these functions
never reach, are stubbed as in _reference_env.py.

Inputs are the seeded maps of tests/boundary_cases.py (GOLDEN_MAPS, GOLDEN_PAIRS: at most 64 x 96, the reference walks every pixel
in Python); only outputs are stored, plus the CRC32 of every input so that a drifting generator is noticed.  A relabelling the
reference fails on (its `max_axis` quirk raises IndexError for some label layouts, a reference map of one label ValueError
with keep_bg) has no entry."""
import os
import sys
import types
import warnings
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = '/root/reference'
warnings.filterwarnings('ignore')


def crc(arr):
    return zlib.crc32(np.ascontiguousarray(arr).tobytes())


def main():
    if not hasattr(np, 'int'):
        np.int = int
    for name in ('nibabel', 'OleFileIO_PL', 'planar', 'gco'):
        sys.modules.setdefault(name, types.ModuleType(name))
    os.environ['IMSEGM_REFERENCE'] = ''
    sys.path.insert(0, REF)
    sys.path.insert(1, os.path.join(ROOT, 'tests'))
    import skimage
    import scipy
    import imsegm
    import imsegm.labeling as ref
    assert skimage.__version__.startswith('0.18'), skimage.__version__
    assert os.path.dirname(os.path.abspath(imsegm.__file__)) == os.path.join(REF, 'imsegm'), imsegm.__file__
    import boundary_cases as B
    out = {'versions': np.array('scikit-image %s, scipy %s, numpy %s' % (skimage.__version__, scipy.__version__, np.__version__))}
    for name in B.GOLDEN_MAPS:
        seg = np.array(B.maps()[name])
        out[name + '_crc'] = np.array(crc(seg))
        for flag in (0, 1):
            out['%s_contour%d' % (name, flag)] = np.asarray(ref.contour_binary_map(seg, 1, bool(flag)))
            out['%s_coords%d' % (name, flag)] = np.array(ref.contour_coords(seg, 1, bool(flag)), dtype=np.int64).reshape(-1, 2)
        out[name + '_distance'] = np.asarray(ref.compute_distance_map(seg, 1))
        print(name, seg.shape, int(out[name + '_contour1'].sum()), float(out[name + '_distance'].max()))
    for ref_name, name in B.GOLDEN_PAIRS:
        seg_ref, seg = np.array(B.maps()[ref_name]), np.array(B.maps()[name])
        key = ref_name + '__' + name
        points, dist = ref.compute_boundary_distances(seg_ref, seg)
        out[key + '_points'], out[key + '_dist'] = np.asarray(points), np.asarray(dist)
        out[key + '_overlap'] = np.asarray(ref.compute_labels_overlap_matrix(seg_ref, seg))
        failed = []
        for keep_bg in (0, 1):
            for kind, call in (('unique', ref.relabel_max_overlap_unique), ('merge', ref.relabel_max_overlap_merge)):
                try:
                    out['%s_%s%d' % (key, kind, keep_bg)] = np.asarray(call(seg_ref.copy(), seg.copy(), keep_bg=bool(keep_bg)))
                except (IndexError, ValueError):
                    failed.append('%s%d' % (kind, keep_bg))
        print(key, out[key + '_points'].shape, out[key + '_points'].dtype, out[key + '_overlap'].shape, 'raised:', failed)
    target = os.path.join(HERE, 'boundary.npz')
    np.savez_compressed(target, **out)
    print(target, os.path.getsize(target), 'bytes')


if __name__ == '__main__':
    main()
