#!/usr/bin/env python
"""Time every public pixel function of ``pyimsegm_amd.annotation`` on the device against its host statement (``on='host'``) on the same
box, end to end from host memory to host memory: painted label maps of 1024 x 768 and 2048 x 2048 pixels with legends of 4 and 32
colours, 20 % of the pixels overwritten with noise that is none of the legend's colours.

THE YARDSTICK IS THIS REPOSITORY'S OWN NUMPY / SCIPY STATEMENT, not the reference.  Median of ``--repeats`` runs after ``--warmup`` ones,
with minimum and maximum.  The host statement of ``quantize_image_nearest_pixel`` (a k-d tree over all exact pixels, asked at every
pixel) takes seconds: it is timed with ``--slow-repeats`` runs after one warm-up, and at 2048 x 2048 only with ``--slow-large``.

The tool exits with an error when ``quantize_image_nearest_pixel`` on the device is not faster than its host statement at 1024 x 768:
that function is the reason for the kernels.  ``host_by_default`` lists the functions whose device median is not below their host
median at 1024 x 768 with either legend; ``annotation.HOST_BY_DEFAULT`` follows it.

    python tools/time_annotation.py [--out profiles/annotation_time.json] [--repeats 5] [--warmup 2]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = ((768, 1024), (2048, 2048))
LEGENDS = (4, 32)


def make_case(height, width, nb_colors, seed=0, noise=0.2):
    """(painted image uint8, clean image uint8, colours, label map): 64 x 64 blocks painted with distinct colours of even blue; the
    noise has an odd blue, so it is none of the legend's colours"""
    rng = np.random.RandomState(seed)
    keys = rng.choice(1 << 23, size=nb_colors, replace=False) * 2
    colors = [(int(k) >> 16, (int(k) >> 8) & 255, int(k) & 255) for k in keys]
    coarse = rng.randint(0, nb_colors, (height // 64 + 1, width // 64 + 1))
    segm = np.repeat(np.repeat(coarse, 64, axis=0), 64, axis=1)[:height, :width].astype(np.int64)
    clean = np.array(colors, dtype=np.uint8)[segm]
    painted = clean.copy()
    spoiled = rng.rand(height, width) < noise
    fill = rng.randint(0, 256, (height, width, 3)).astype(np.uint8)
    fill[:, :, 2] |= 1
    painted[spoiled] = fill[spoiled]
    return painted, clean, colors, segm


def timed(run, warmup, repeats):
    times, result = [], None
    for i in range(warmup + repeats):
        t0 = time.perf_counter()
        result = run()
        if i >= warmup:
            times.append((time.perf_counter() - t0) * 1e3)
    return {'median': float(np.median(times)), 'min': float(np.min(times)), 'max': float(np.max(times)), 'runs': times}, result


def equal(a, b):
    if isinstance(a, np.ndarray):
        return bool(a.dtype == b.dtype and np.array_equal(a, b))
    return a == b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'annotation_time.json'))
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--slow-repeats', type=int, default=1)
    ap.add_argument('--slow-large', action='store_true', help='time the host statement of quantize_image_nearest_pixel at 2048 x 2048 too')
    args = ap.parse_args()
    from pyimsegm_amd import _hip
    from pyimsegm_amd import annotation as ann
    _hip.default_context()
    result = {'repeats': args.repeats, 'warmup': args.warmup, 'slow_repeats': args.slow_repeats, 'unit': 'ms', 'noise': 0.2,
              'yardstick': "this repository's own numpy / scipy statements (on='host'), not the reference", 'cases': {}}
    slower = set()
    for height, width in SIZES:
        for nb_colors in LEGENDS:
            painted, clean, colors, segm = make_case(height, width, nb_colors)
            lut = dict(enumerate(colors))
            calls = {
                'unique_image_colors': lambda on: ann.unique_image_colors(painted, on=on),
                'image_frequent_colors': lambda on: ann.image_frequent_colors(painted, on=on),
                'convert_img_colors_to_labels': lambda on: ann.convert_img_colors_to_labels(clean, lut, on=on),
                'convert_img_colors_to_labels_reverted': lambda on: ann.convert_img_colors_to_labels_reverted(clean, {c: i for i, c in lut.items()}, on=on),
                'convert_img_labels_to_colors': lambda on: ann.convert_img_labels_to_colors(segm, lut, on=on),
                'image_color_2_labels': lambda on: ann.image_color_2_labels(painted, colors, on=on),
                'quantize_image_nearest_color': lambda on: ann.quantize_image_nearest_color(painted, colors, on=on),
                'quantize_image_nearest_pixel': lambda on: ann.quantize_image_nearest_pixel(painted, colors, on=on),
            }
            entry = {'unmatched_share': float(((painted != clean).any(axis=2)).mean())}
            for name, call in calls.items():
                row = {}
                row['device'], on_device = timed(lambda: call('device'), args.warmup, args.repeats)
                slow = name == 'quantize_image_nearest_pixel'
                if slow and height * width > 1024 * 768 and not args.slow_large:
                    row['host'], row['same_bytes'] = None, None
                else:
                    row['host'], on_host = timed(lambda: call('host'), 1 if slow else args.warmup, args.slow_repeats if slow else args.repeats)
                    # (the nearest-pixel answers differ where several exact pixels are equally near: the share that is the same is recorded)
                    row['same_bytes'] = float((on_device == on_host).all(axis=2).mean()) if slow else equal(on_device, on_host)
                    row['host_over_device'] = row['host']['median'] / row['device']['median']
                    if (height, width) == SIZES[0] and row['device']['median'] >= row['host']['median']:
                        slower.add(name)
                entry[name] = row
                print('%4d x %4d, %2d colours, %-40s device %9.2f ms, host %s' % (
                    height, width, nb_colors, name, row['device']['median'], '%9.2f ms' % row['host']['median'] if row['host'] else 'not timed'), flush=True)
            result['cases']['%dx%d_%dcolours' % (height, width, nb_colors)] = entry
    result['host_by_default'] = sorted(slower)
    result['host_by_default_in_module'] = sorted(ann.HOST_BY_DEFAULT)
    print(json.dumps({'host_by_default': result['host_by_default'], 'in_module': result['host_by_default_in_module']}))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as out:
        json.dump(result, out, indent=1)
        out.write('\n')
    if 'quantize_image_nearest_pixel' in slower:
        sys.exit('quantize_image_nearest_pixel is not faster on the device than on the host at 1024 x 768: the kernel is wrong')


if __name__ == '__main__':
    main()
