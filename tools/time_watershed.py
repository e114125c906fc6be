#!/usr/bin/env python
"""Time the egg segmentation by marker watershed on one class map -- 1024 x 768, 12 and 48 synthetic tilted ellipses drawn as
tools/time_cut_objects.py draws them, one centre per ellipse at its centre of mass, the reference's radii 5 and 15 -- end to end
from host memory to host memory, two ways in one run, alternating:

* ``device``: ``segment_watershed(seg, centres, post_morph=True, on='device')``, one ``imsegm_watershed`` call;
* ``host``: the same with ``on='host'``, this repository's numpy / scipy statement.

The stages ``watershed_markers`` (the flood with its distance transform) and ``watershed_post_morph`` (the clean-up) are timed alone
in the same way.  Median of ``--repeats`` runs after ``--warmup`` ones, with minimum and maximum, and whether both gave the same
bytes.  The kernels are not timed one by one.

    python tools/time_watershed.py [--out profiles/watershed_time.json] [--repeats 5] [--warmup 2]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from time_center_annotation import alternating, same  # noqa: E402
from time_object_shapes import make_case  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'watershed_time.json'))
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--height', type=int, default=768)
    ap.add_argument('--width', type=int, default=1024)
    ap.add_argument('--box', default='one MI355X (gfx950)')
    ap.add_argument('--counts', type=int, nargs='+', default=[12, 48], help='numbers of ellipses')
    args = ap.parse_args()
    from pyimsegm_amd import _hip
    from pyimsegm_amd import egg_segmentation as egg
    from pyimsegm_amd.center_annotation import compute_eggs_center_host
    from pyimsegm_amd.ellipse_fitting import fill_holes_host
    _hip.default_context()
    result = {'height': args.height, 'width': args.width, 'radius_close': 5, 'radius_open': 15, 'repeats': args.repeats,
              'warmup': args.warmup, 'unit': 'ms', 'box': args.box,
              'note': 'one run on one box; host memory to host memory; device and host calls alternate', 'sizes': {}}
    for count in args.counts:
        objects = make_case(args.height, args.width, count)
        seg = objects > 0
        centres = [(float(y), float(x)) for x, y in compute_eggs_center_host(objects.astype(np.int32))]
        mask = fill_holes_host(seg)
        markers = np.zeros(seg.shape, dtype=np.int32)
        for i, (row, col) in enumerate(centres):
            markers[int(row), int(col)] = i + 1
        flooded = egg.watershed_markers_host(mask, markers)
        entry = {'centres': len(centres), 'labels_after_flood': int(len(np.unique(flooded)) - 1)}
        calls = {'segment_watershed': lambda on: egg.segment_watershed(seg, centres, True, on=on)[0],
                 'watershed_markers': lambda on: egg.watershed_markers(mask, markers, on=on),
                 'watershed_post_morph': lambda on: egg.watershed_post_morph(flooded, on=on)}
        for name, call in calls.items():
            stats, answers = alternating({'device': lambda: call('device'), 'host': lambda: call('host')}, args.warmup, args.repeats)
            stats['same_bytes'] = same(answers['device'], answers['host'])
            stats['host_over_device'] = stats['host']['median'] / stats['device']['median']
            entry[name] = stats
            print(count, name, 'device %.2f ms' % stats['device']['median'], 'host %.2f ms' % stats['host']['median'],
                  'same bytes' if stats['same_bytes'] else 'DIFFERENT BYTES', flush=True)
        result['sizes'][str(count)] = entry
    print(json.dumps(result))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as out:
        json.dump(result, out, indent=1)
        out.write('\n')


if __name__ == '__main__':
    main()
