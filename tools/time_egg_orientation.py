#!/usr/bin/env python
"""Time the orientation of the egg cut-outs of one stage -- a synthetic stage of 1 024 cut-outs of 128 x 256 x 3 uint8 (an egg-like
blob that is brighter on one side, noise, every second cut-out turned) -- end to end from host memory to host memory, two ways in one
run, alternating:

* ``device``: ``swap_orientations(images, swap_type, on='device')``, one ``imsegm_orient_stack`` call, transfers included;
* ``host``: the same with ``on='host'``, the numpy statements of this repository (``np.median`` over the stack, the float swap tests
  image by image).

``compute_mean_image`` is timed alone in the same way, and the median kernel alone from the context's event pairs.  Median of
``--repeats`` runs after ``--warmup`` ones, with minimum and maximum, and whether both gave the same flags and bytes.  Exits with an
error when a device run is slower than its host run.

    python tools/time_egg_orientation.py [--out profiles/egg_orientation_time.json] [--repeats 5] [--warmup 2]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from time_center_annotation import alternating  # noqa: E402


def make_stage(count, height, width, seed=0):
    rng = np.random.RandomState(seed)
    rows, cols = np.mgrid[:height, :width]
    images = []
    for i in range(count):
        cy, cx = height / 2. + rng.uniform(-6, 6), width / 2. + rng.uniform(-10, 10)
        inside = ((rows - cy) / (0.42 * height)) ** 2 + ((cols - cx) / (0.45 * width)) ** 2 <= 1
        egg = inside * (60 + 120. * cols / width) + rng.randint(0, 30, (height, width))
        img = np.clip(egg[:, :, None] + rng.randint(0, 20, (height, width, 3)), 0, 255).astype(np.uint8)
        images.append(np.ascontiguousarray(img[::-1, ::-1]) if i % 2 else img)
    return images


def same_answers(a, b):
    return bool(np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and len(a[0]) == len(b[0])
                and all(np.array_equal(x, y) for x, y in zip(a[0], b[0])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'egg_orientation_time.json'))
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--count', type=int, default=1024)
    ap.add_argument('--height', type=int, default=128)
    ap.add_argument('--width', type=int, default=256)
    ap.add_argument('--box', default='one MI355X (gfx950)')
    args = ap.parse_args()
    from pyimsegm_amd import _hip
    from pyimsegm_amd import egg_orientation as egg
    ctx = _hip.default_context()
    images = make_stage(args.count, args.height, args.width)
    result = {'count': args.count, 'height': args.height, 'width': args.width, 'channels': 3, 'repeats': args.repeats,
              'warmup': args.warmup, 'unit': 'ms', 'box': args.box,
              'note': 'one run on one box; host memory to host memory, transfers included; device and host calls alternate'}
    calls = {'swap_orientations_cc': lambda on: egg.swap_orientations(images, 'cc', on=on),
             'swap_orientations_density': lambda on: egg.swap_orientations(images, 'density', on=on),
             'compute_mean_image': lambda on: egg.compute_mean_image(images, on=on)}
    slower = []
    for name, call in calls.items():
        stats, answers = alternating({'device': lambda: call('device'), 'host': lambda: call('host')}, args.warmup, args.repeats)
        if name == 'compute_mean_image':
            stats['same_bytes'] = bool(np.array_equal(answers['device'], answers['host']))
        else:
            stats['same_bytes'] = same_answers(answers['device'], answers['host'])
            stats['swapped'] = int(answers['device'][1].sum())
        stats['host_over_device'] = stats['host']['median'] / stats['device']['median']
        result[name] = stats
        print(name, 'device %.2f ms' % stats['device']['median'], 'host %.2f ms' % stats['host']['median'],
              'same bytes' if stats['same_bytes'] else 'DIFFERENT BYTES', flush=True)
        if stats['device']['median'] > stats['host']['median']:
            slower.append(name)
    # the median kernel alone: the event pair around its launch (profile group 'color_stats' of the context)
    stack = egg._device_stack(images, (args.height, args.width))
    kernel = []
    ctx.profile_enable(True)
    for i in range(args.warmup + args.repeats):
        ctx.profile_reset()
        _hip.stack_median(stack, 0, ctx=ctx)
        ms, launches = ctx.profile_get('color_stats')
        assert launches == 1
        if i >= args.warmup:
            kernel.append(ms)
    ctx.profile_enable(False)
    result['median_kernel'] = {'median': float(np.median(kernel)), 'min': float(np.min(kernel)), 'max': float(np.max(kernel)), 'runs': kernel,
                               'stack_bytes_read': int(2 * args.count * args.height * args.width)}
    print('median kernel alone %.3f ms' % result['median_kernel']['median'], flush=True)
    print(json.dumps(result))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as out:
        json.dump(result, out, indent=1)
        out.write('\n')
    if slower:
        sys.exit('the device run is slower than the host run: %s' % ', '.join(slower))


if __name__ == '__main__':
    main()
