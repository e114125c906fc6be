#!/usr/bin/env python
"""Time the centre-level annotation of one map of annotated eggs -- 1024 x 768, 12 and 48 synthetic tilted ellipses drawn as
tools/time_cut_objects.py draws them, the reference's constants (``disk(25)``, ``min_size`` 64, levels 0 / 0.4 / 0.8) -- end to end
from host memory to host memory, two ways in one run, alternating:

* ``device``: ``create_annot_centers(img, on='device')``, one ``imsegm_create_annot_centers`` call;
* ``host``: the same with ``on='host'``, this repository's numpy / scipy statement, object by object.

``correct_segm`` and ``segm_center_levels`` are timed alone in the same way.  Median of ``--repeats`` runs after ``--warmup`` ones,
with minimum and maximum, and whether both gave the same bytes.  The kernels are not timed one by one.

    python tools/time_center_annotation.py [--out profiles/center_annotation_time.json] [--repeats 5] [--warmup 2]
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

from time_object_shapes import make_case  # noqa: E402


def alternating(runs, warmup, repeats):
    """``runs``: name -> callable; one call of each per round, in turn"""
    times, results = {name: [] for name in runs}, {}
    for i in range(warmup + repeats):
        for name, run in runs.items():
            t0 = time.perf_counter()
            results[name] = run()
            if i >= warmup:
                times[name].append((time.perf_counter() - t0) * 1e3)
    stats = {name: {'median': float(np.median(t)), 'min': float(np.min(t)), 'max': float(np.max(t)), 'runs': t} for name, t in times.items()}
    return stats, results


def same(a, b):
    a, b = (a, b) if isinstance(a, tuple) else ((a, ), (b, ))
    return bool(len(a) == len(b) and all(x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a, b)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'center_annotation_time.json'))
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--height', type=int, default=768)
    ap.add_argument('--width', type=int, default=1024)
    ap.add_argument('--box', default='one MI355X (gfx950)')
    ap.add_argument('--counts', type=int, nargs='+', default=[12, 48], help='numbers of ellipses')
    args = ap.parse_args()
    from pyimsegm_amd import _hip
    from pyimsegm_amd import center_annotation as annot
    _hip.default_context()
    result = {'height': args.height, 'width': args.width, 'sel_radius': 25, 'min_size': 64, 'levels': annot.DISTANCE_LEVELS,
              'repeats': args.repeats, 'warmup': args.warmup, 'unit': 'ms', 'box': args.box,
              'note': 'one run on one box; host memory to host memory; device and host calls alternate', 'sizes': {}}
    for count in args.counts:
        img = (make_case(args.height, args.width, count) > 0).astype(np.uint8) * 255
        _, seg_lb = annot.correct_segm_host(img)
        entry = {'labels_after_correction': int(seg_lb.max())}
        calls = {'create_annot_centers': lambda on: annot.create_annot_centers(img, on=on),
                 'correct_segm': lambda on: annot.correct_segm(img, on=on),
                 'segm_center_levels': lambda on: annot.segm_center_levels(seg_lb, on=on)}
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
