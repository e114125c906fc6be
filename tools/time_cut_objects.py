#!/usr/bin/env python
"""Time the cut-out of all annotated eggs of one image -- ``cut_objects`` on a 1024 x 768 RGB uint8 image whose label map holds 12 and
48 non-overlapping tilted ellipses, padding 5, ``use_mask`` on, end to end from host memory to host memory -- two ways in one run:

* ``device``: ``cut_objects(img, segm, on='device')``, one ``imsegm_cut_objects`` call for all objects;
* ``host``: the same with ``on='host'``, the loop of this repository's numpy statement ``cut_object_host`` over the labels.

Median of ``--repeats`` runs after ``--warmup`` ones, with minimum and maximum, and whether both gave the same bytes.

    python tools/time_cut_objects.py [--out profiles/cut_objects_time.json] [--repeats 5] [--warmup 2]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from time_object_shapes import make_case, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'cut_objects_time.json'))
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--height', type=int, default=768)
    ap.add_argument('--width', type=int, default=1024)
    ap.add_argument('--padding', type=int, default=5)
    args = ap.parse_args()
    from pyimsegm_amd import _hip
    from pyimsegm_amd.utilities import data_io
    _hip.default_context()
    result = {'height': args.height, 'width': args.width, 'channels': 3, 'padding': args.padding, 'use_mask': True,
              'repeats': args.repeats, 'warmup': args.warmup, 'unit': 'ms', 'sizes': {}}
    for count in (12, 48):
        segm = make_case(args.height, args.width, count)
        img = np.random.RandomState(count).randint(0, 256, segm.shape + (3, )).astype(np.uint8)
        assert len(np.unique(segm)) == count + 1
        entry, answers = {}, {}
        for name in ('device', 'host'):
            entry[name], answers[name] = timed(lambda: data_io.cut_objects(img, segm, padding=args.padding, use_mask=True, on=name),
                                               args.warmup, args.repeats)
            print(count, name, '%.2f ms' % entry[name]['median'], flush=True)
        entry['same_bytes'] = bool(len(answers['device']) == len(answers['host']) == count and all(
            a.shape == b.shape and a.tobytes() == b.tobytes() for a, b in zip(answers['device'], answers['host'])))
        entry['host_over_device'] = entry['host']['median'] / entry['device']['median']
        result['sizes'][str(count)] = entry
    print(json.dumps(result))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as out:
        json.dump(result, out, indent=1)
        out.write('\n')


if __name__ == '__main__':
    main()
