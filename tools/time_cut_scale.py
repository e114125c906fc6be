#!/usr/bin/env python
"""Time the cut-and-scale step of the egg chain -- a synthetic 1 024 x 768 RGB image with 12 and with 48 ellipses of mixed sizes, so
that cut-outs are both shrunk and enlarged on the way to the normal size of the stage -- end to end from host memory to host memory,
two ways in one run, alternating:

* ``device``: ``extract_ellipse_objects(img, ellipses, norm_size, on='device')``, one ``imsegm_ellipse_cut_scale`` call, transfers
  and both host hooks included;
* ``host``: ``extract_ellipse_objects_host``, the numpy / scipy statements of this repository, ellipse by ellipse.

The resize alone is timed the same way on the host's cut-outs: ``resize_images(cuts, norm_size, as_uint8=True)``.  Median of
``--repeats`` runs after ``--warmup`` ones, with minimum and maximum, and whether both gave the same bytes.  The medians decide the
default place of ``pyimsegm_amd.ellipse_cut_scale``; the tool exits with an error when a device run is slower than its host run.

    python tools/time_cut_scale.py [--out profiles/cut_scale_time.json] [--repeats 5] [--warmup 2]
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


def make_scene(height, width, count, seed=0):
    """an RGB image with texture and a dark border, and ``count`` ellipses (xc, yc, a, b, theta) of mixed sizes inside it"""
    rng = np.random.RandomState(seed)
    rows, cols = np.mgrid[:height, :width].astype(np.float64)
    img = np.empty((height, width, 3), dtype=np.uint8)
    for ch in range(3):
        wave = 110 + 60 * np.sin(rows / (9. + ch)) * np.cos(cols / (11. - ch)) + rng.randint(-50, 51, size=(height, width))
        img[:, :, ch] = np.clip(wave, 0, 255).astype(np.uint8)
        img[:3, :, ch] = img[-3:, :, ch] = 10 + ch
    ellipses = []
    for k in range(count):
        a = rng.uniform(25, 60) * (1, 1.8, 3.2)[k % 3]                # small, medium and large eggs
        b = a * rng.uniform(0.45, 0.75)
        ellipses.append((rng.uniform(a, height - a), rng.uniform(a, width - a), a, b, rng.uniform(-np.pi, np.pi)))
    return img, ellipses


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'cut_scale_time.json'))
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--height', type=int, default=768)
    ap.add_argument('--width', type=int, default=1024)
    ap.add_argument('--box', default='one MI355X (gfx950)')
    args = ap.parse_args()
    from pyimsegm_amd import _hip
    from pyimsegm_amd import ellipse_cut_scale as ecs
    from pyimsegm_amd.utilities.data_io import cut_object_host
    _hip.default_context()
    result = {'height': args.height, 'width': args.width, 'channels': 3, 'repeats': args.repeats, 'warmup': args.warmup, 'unit': 'ms',
              'box': args.box,
              'note': 'one run on one box; host memory to host memory, transfers included; device and host calls alternate'}
    slower = []
    for count in (12, 48):
        img, ellipses = make_scene(args.height, args.width, count)
        norm_size = ecs.stage_norm_size(ellipses)
        bg_color = ecs._bg_color(img)
        cuts = [cut_object_host(img, ecs._ellipse_mask_host(img.shape, ell), 0, use_mask=True, bg_color=bg_color) for ell in ellipses]
        heights, widths = [cut.shape[0] for cut in cuts], [cut.shape[1] for cut in cuts]
        calls = {'extract_ellipse_objects': {'device': lambda: ecs.extract_ellipse_objects(img, ellipses, norm_size, on='device'),
                                             'host': lambda: ecs.extract_ellipse_objects_host(img, ellipses, norm_size)},
                 'resize_images': {'device': lambda: ecs.resize_images(cuts, norm_size, on='device', as_uint8=True),
                                   'host': lambda: ecs.resize_images(cuts, norm_size, on='host', as_uint8=True)}}
        entry = {'ellipses': count, 'norm_size': list(norm_size), 'cut_heights': [min(heights), max(heights)],
                 'cut_widths': [min(widths), max(widths)]}
        for name, pair in calls.items():
            stats, answers = alternating(pair, args.warmup, args.repeats)
            stats['same_bytes'] = bool(np.array_equal(answers['device'], answers['host']))
            stats['host_over_device'] = stats['host']['median'] / stats['device']['median']
            entry[name] = stats
            print(count, 'ellipses', name, 'device %.2f ms' % stats['device']['median'], 'host %.2f ms' % stats['host']['median'],
                  'same bytes' if stats['same_bytes'] else 'DIFFERENT BYTES', flush=True)
            if stats['device']['median'] > stats['host']['median'] or not stats['same_bytes']:
                slower.append('%s with %d ellipses' % (name, count))
        result['ellipses_%d' % count] = entry
    print(json.dumps(result))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as out:
        json.dump(result, out, indent=1)
        out.write('\n')
    if slower:
        sys.exit('the device run is slower than the host run, or differs: %s' % ', '.join(slower))


if __name__ == '__main__':
    main()
