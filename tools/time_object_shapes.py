#!/usr/bin/env python
"""Time the step from an annotated egg map to the ray vectors of its objects -- ``compute_object_shapes`` on one 1024 x 768 label map
with 12 and with 48 non-overlapping ellipses, ``ray_step`` 5, end to end from host memory to host memory -- three ways in one run:

* ``batched_device``: ``compute_object_shapes([map], on='device')``, one ``imsegm_object_shapes`` call for all objects;
* ``host``: the same with ``on='host'``, this repository's numpy / scipy statement of the same definitions;
* ``parent_loop``: what the repository offered before the batched call, written out here with functions that were there already:
  ``compute_segm_object_shape(map == label, ray_step)`` for every label -- a full-image mask, ``ndimage.center_of_mass`` and one ray
  launch per object.

``rays_device`` / ``rays_host`` time the stage in front of the fill / rotate alone (``object_shape_rays``).  Median of ``--repeats``
runs after ``--warmup`` ones, with minimum and maximum.

    python tools/time_object_shapes.py [--out profiles/object_shapes_time.json] [--repeats 5] [--warmup 2]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_case(height, width, count, seed=0):
    """``count`` ellipses with the labels 1 .. count, one per cell of a grid over the map, each turned and well inside its cell"""
    rng = np.random.RandomState(seed)
    across = int(np.ceil(np.sqrt(count * width / float(height))))
    down = int(np.ceil(count / float(across)))
    cell_h, cell_w = height / float(down), width / float(across)
    rows, cols = np.indices((height, width))
    img = np.zeros((height, width), dtype=np.int32)
    for k in range(count):
        cy, cx = (k // across + 0.5) * cell_h, (k % across + 0.5) * cell_w
        limit = 0.5 * min(cell_h, cell_w) - 2
        a, b = rng.uniform(0.6, 0.95) * limit, rng.uniform(0.4, 0.6) * limit
        theta = rng.uniform(0, np.pi)
        dy, dx = rows - cy, cols - cx
        u, v = dx * np.cos(theta) + dy * np.sin(theta), -dx * np.sin(theta) + dy * np.cos(theta)
        img[(u / a)**2 + (v / b)**2 <= 1.] = k + 1
    return img


def timed(run, warmup, repeats):
    times, result = [], None
    for i in range(warmup + repeats):
        t0 = time.perf_counter()
        result = run()
        if i >= warmup:
            times.append((time.perf_counter() - t0) * 1e3)
    return {'median': float(np.median(times)), 'min': float(np.min(times)), 'max': float(np.max(times)), 'runs': times}, result


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'object_shapes_time.json'))
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--height', type=int, default=768)
    ap.add_argument('--width', type=int, default=1024)
    ap.add_argument('--ray-step', type=int, default=5)
    args = ap.parse_args()
    from pyimsegm_amd import _hip
    from pyimsegm_amd import region_growing as rg
    _hip.default_context()
    result = {'height': args.height, 'width': args.width, 'ray_step': args.ray_step, 'repeats': args.repeats, 'warmup': args.warmup,
              'unit': 'ms', 'sizes': {}}
    for count in (12, 48):
        img = make_case(args.height, args.width, count)
        labels = np.unique(img)[1:]
        assert len(labels) == count

        def parent_loop():
            list_rays, list_shifts = [], []
            for label in labels:
                rays, shift = rg.compute_segm_object_shape(img == label, args.ray_step)
                list_rays.append(rays)
                list_shifts.append(shift)
            return list_rays, list_shifts

        entry, answers = {}, {}
        for name, run in (('batched_device', lambda: rg.compute_object_shapes([img], args.ray_step, on='device')),
                          ('host', lambda: rg.compute_object_shapes([img], args.ray_step, on='host')),
                          ('parent_loop', parent_loop),
                          ('rays_device', lambda: rg.object_shape_rays(img, args.ray_step, on='device')),
                          ('rays_host', lambda: rg.object_shape_rays(img, args.ray_step, on='host'))):
            entry[name], answers[name] = timed(run, args.warmup, args.repeats)
            print(count, name, '%.2f ms' % entry[name]['median'], flush=True)
        entry['same_rays'] = bool(answers['batched_device'][0] == answers['host'][0] == answers['parent_loop'][0])
        entry['same_raw_bytes'] = bool(all(a.tobytes() == b.tobytes() for a, b in zip(answers['rays_device'], answers['rays_host'])))
        entry['host_over_batched_device'] = entry['host']['median'] / entry['batched_device']['median']
        entry['parent_loop_over_batched_device'] = entry['parent_loop']['median'] / entry['batched_device']['median']
        result['sizes'][str(count)] = entry
    print(json.dumps(result))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as out:
        json.dump(result, out, indent=1)
        out.write('\n')


if __name__ == '__main__':
    main()
