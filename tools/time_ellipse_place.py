#!/usr/bin/env python
"""Time the placement of fitted ellipses into a 1024 x 768 label map -- the last step of the egg experiment's three ellipse methods --
with 12 and with 48 synthetic ellipses, end to end from host memory to host memory:

* ``add_overlap_ellipses`` on the device against the host statement (``on='host'``),
* the single-call route (``add_overlap_ellipse`` ellipse by ellipse) on the device against the host statement, with the time of
  every single call by the ``max(segm)`` it met: where the device starts to win is ``SINGLE_CALL_DEVICE_FROM_LABELS``,
* ``ellipse_label_overlaps`` on the device against its host statement.

THE YARDSTICK IS THIS REPOSITORY'S OWN NUMPY STATEMENT (pyimsegm_amd/ellipse_fitting.py ``place_host`` / ``overlaps_host``), which
already counts the overlap from the pixels under the ellipse instead of three full-image passes per label as the reference does.
Median of ``--repeats`` runs after ``--warmup`` ones, with minimum and maximum.

    python tools/time_ellipse_place.py [--out profiles/ellipse_place_time.json] [--repeats 5] [--warmup 2]
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
    """ellipses of egg size scattered over the map: most fit next to each other, some overlap an earlier one"""
    rng = np.random.RandomState(seed)
    scale = np.sqrt(12. / count)
    params = [(int(rng.randint(40, height - 40)), int(rng.randint(40, width - 40)), int(rng.randint(50, 90) * scale) + 1,
               int(rng.randint(70, 130) * scale) + 1, float(rng.uniform(-np.pi, np.pi))) for _ in range(count)]
    return np.zeros((height, width), dtype=int), params


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
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'ellipse_place_time.json'))
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--height', type=int, default=768)
    ap.add_argument('--width', type=int, default=1024)
    ap.add_argument('--thr', type=float, default=0.5)
    args = ap.parse_args()
    from pyimsegm_amd import _hip
    from pyimsegm_amd import ellipse_fitting as ell
    _hip.default_context()
    result = {'height': args.height, 'width': args.width, 'thr_overlap': args.thr, 'repeats': args.repeats, 'warmup': args.warmup,
              'unit': 'ms', 'yardstick': "this repository's own numpy statement (ellipse_fitting.place_host / overlaps_host), not the reference",
              'single_call_device_from_labels': ell.SINGLE_CALL_DEVICE_FROM_LABELS, 'sizes': {}}
    for count in (12, 48):
        segm, params = make_case(args.height, args.width, count)
        labels = list(range(1, count + 1))
        entry, answers = {}, {}

        def batched(on):
            return lambda: ell.add_overlap_ellipses(segm.copy(), params, labels, args.thr, on=on)

        def single(on, steps=None):
            def run():
                out = segm.copy()
                for p, lb in zip(params, labels):
                    top = int(out.max())
                    t0 = time.perf_counter()
                    ell.add_overlap_ellipse(out, p, lb, args.thr, on=on)
                    if steps is not None:
                        steps.setdefault(top, []).append((time.perf_counter() - t0) * 1e3)
                return out
            return run

        for on in ('device', 'host'):
            entry['batched_' + on], answers['batched_' + on] = timed(batched(on), args.warmup, args.repeats)
            steps = {}
            entry['single_' + on], answers['single_' + on] = timed(single(on, steps), args.warmup, args.repeats)
            entry['single_' + on + '_by_max_label'] = {str(top): float(np.median(ms)) for top, ms in sorted(steps.items())}
            print(count, on, 'batched %.2f ms, single %.2f ms' % (entry['batched_' + on]['median'], entry['single_' + on]['median']), flush=True)
        entry['single_default'], answers['single_default'] = timed(single(None), args.warmup, args.repeats)
        placed_map = answers['batched_host'][0]
        for on in ('device', 'host'):
            entry['overlaps_' + on], answers['overlaps_' + on] = timed(lambda: ell.ellipse_label_overlaps(placed_map, params, on=on),
                                                                     args.warmup, args.repeats)
        entry['placed'] = int(answers['batched_host'][1].sum())
        entry['same_bytes'] = bool(all(np.array_equal(answers['batched_host'][0], other) for other in
                                       (answers['batched_device'][0], answers['single_device'], answers['single_host'], answers['single_default']))
                                   and np.array_equal(answers['batched_host'][1], answers['batched_device'][1])
                                   and all(np.array_equal(a, b) for a, b in zip(answers['overlaps_host'], answers['overlaps_device'])))
        for route in ('batched', 'single', 'overlaps'):
            entry[route + '_host_over_device'] = entry[route + '_host']['median'] / entry[route + '_device']['median']
        result['sizes'][str(count)] = entry
    print(json.dumps(result))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as out:
        json.dump(result, out, indent=1)
        out.write('\n')


if __name__ == '__main__':
    main()
