#!/usr/bin/env python
"""Time ``labeling.compute_boundary_distances`` on a pair of label volumes -- a blocky supervoxel-like map with ragged edges
against a coarser blocky annotation, 16 x 256 x 256 and 64 x 512 x 512 -- end to end from host memory to host memory, three ways in
one run, alternating:

* ``device``: ``compute_boundary_distances(segm_ref, segm, on='device')``, one ``imsegm_boundary_distances3d`` call (both maps
  are uploaded);
* ``device_session``: the same against the map a ``Volume3D`` session already holds (``imsegm_volume_boundary_distances``, only the
  reference is uploaded);
* ``host``: the same with ``on='host'``, this repository's numpy / scipy statement.

Median of ``--repeats`` runs after ``--warmup`` ones, with minimum and maximum, and whether all gave the same bytes.  The kernels are
not timed one by one.

    python tools/time_boundary_distances3d.py [--out profiles/boundary_distances3d_time.json] [--repeats 5] [--warmup 2]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from time_center_annotation import alternating, same  # noqa: E402


def blocky_pair(shape, seed=7):
    """(annotation, supervoxels): boxes of a quarter of every extent shifted by (1, 5, 7) voxels so that their faces do not lie on
    those of the supervoxels, and boxes of 4 x 16 x 16 voxels of which a tenth of the voxels takes the label of the neighbour to
    the right (ragged faces)"""
    z, y, x = np.indices(shape)
    coarse = [max(1, extent // 4) for extent in shape]
    annot = ((z + 1) // coarse[0]) * 25 + ((y + 5) // coarse[1]) * 5 + (x + 7) // coarse[2]
    step = (4, 16, 16)
    per_row, per_slice = -(-shape[2] // step[2]), -(-shape[1] // step[1]) * -(-shape[2] // step[2])
    segm = (z // step[0]) * per_slice + (y // step[1]) * per_row + x // step[2]
    moved = np.random.default_rng(seed).random(shape) < 0.1
    segm = np.where(moved, np.roll(segm, -1, axis=2), segm)
    return annot.astype(np.int32), segm.astype(np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'boundary_distances3d_time.json'))
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--box', default='one MI355X (gfx950)')
    ap.add_argument('--shapes', nargs='+', default=['16x256x256', '64x512x512'])
    args = ap.parse_args()
    from pyimsegm_amd import _hip, labeling
    _hip.default_context()
    result = {'repeats': args.repeats, 'warmup': args.warmup, 'unit': 'ms', 'box': args.box,
              'note': 'one run on one box; host memory to host memory; device, session and host calls alternate', 'sizes': {}}
    for text in args.shapes:
        shape = tuple(int(extent) for extent in text.split('x'))
        segm_ref, segm = blocky_pair(shape)
        sess = _hip.Volume3D(*shape).upload(np.zeros(shape, dtype=np.uint8)).set_labels(segm)
        try:
            stats, answers = alternating({
                'device': lambda: labeling.compute_boundary_distances(segm_ref, segm, on='device'),
                'device_session': lambda: labeling.compute_boundary_distances(segm_ref, None, _session=sess),
                'host': lambda: labeling.compute_boundary_distances(segm_ref, segm, on='host')}, args.warmup, args.repeats)
        finally:
            sess.close()
        stats['points'] = int(len(answers['host'][0]))
        stats['same_bytes'] = same(answers['device'], answers['host']) and same(answers['device_session'], answers['host'])
        stats['host_over_device'] = stats['host']['median'] / stats['device']['median']
        stats['host_over_device_session'] = stats['host']['median'] / stats['device_session']['median']
        result['sizes'][text] = stats
        print(text, 'device %.2f ms' % stats['device']['median'], 'session %.2f ms' % stats['device_session']['median'],
              'host %.2f ms' % stats['host']['median'], 'same bytes' if stats['same_bytes'] else 'DIFFERENT BYTES', flush=True)
    print(json.dumps(result))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as out:
        json.dump(result, out, indent=1)
        out.write('\n')


if __name__ == '__main__':
    main()
