#!/usr/bin/env python
"""Time the centre detection end to end from host memory to host memory, device and host calls alternating in one run:

* ``cluster_center_candidates`` at 200 and at 1258 random integer points in 1024 x 768 with ``eps=50``, ``min_samples=1`` -- the
  reference's settings; 1258 is the map over 25^2 pixels per superpixel -- ``on='device'`` (one ``imsegm_dbscan_points`` call) against
  ``on='host'`` (this repository's numpy statement); scikit-learn's ``DBSCAN`` with the reference's means is timed next to them;
* ``cluster_center_candidates_batch`` on 16 such sets;
* the row loop of ``shift_ray_features`` against ``shift_ray_features_rows`` on 1258 x 24 rays (both on the host);
* ``detect_centers`` at 1024 x 768 on the synthetic ellipse image of tools/time_object_shapes.py with a 20-tree forest, the clustering
  on the device and on the host.

Median of ``--repeats`` runs after ``--warmup`` ones, with minimum and maximum, and whether both gave the same bytes.  The kernels
are not timed one by one.

    python tools/time_center_detection.py [--out profiles/center_detection_time.json] [--repeats 5] [--warmup 2]
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
from time_object_shapes import make_case  # noqa: E402


def same(a, b):
    return bool(len(a) == len(b) and all(np.asarray(x).dtype == np.asarray(y).dtype and np.array_equal(x, y) for x, y in zip(a, b)))


def sklearn_clustering(points, eps, min_samples):
    from sklearn import cluster
    labels = cluster.DBSCAN(eps=eps, min_samples=min_samples).fit(points).labels_.copy()
    return np.array([np.mean(points[labels == i], axis=0) for i in range(max(labels) + 1)]), labels


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'center_detection_time.json'))
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--height', type=int, default=768)
    ap.add_argument('--width', type=int, default=1024)
    ap.add_argument('--box', default='one MI355X (gfx950)')
    ap.add_argument('--sizes', type=int, nargs='+', default=[200, 1258], help='points of a set')
    ap.add_argument('--sets', type=int, default=16, help='sets of the batch')
    ap.add_argument('--eggs', type=int, default=12, help='ellipses of the image')
    args = ap.parse_args()
    from sklearn.ensemble import RandomForestClassifier
    from pyimsegm_amd import _hip, center_annotation, descriptors
    from pyimsegm_amd import center_detection as detection
    _hip.default_context()
    eps, min_samples = detection.CLUSTER_PARAMS['DBSCAN_max_dist'], detection.CLUSTER_PARAMS['DBSCAN_min_samples']
    result = {'height': args.height, 'width': args.width, 'eps': eps, 'min_samples': min_samples, 'repeats': args.repeats,
              'warmup': args.warmup, 'unit': 'ms', 'box': args.box,
              'note': 'one run on one box; host memory to host memory; the calls of an entry alternate', 'cluster_center_candidates': {}}
    rng = np.random.RandomState(0)

    def scatter(count):
        return np.stack([rng.randint(0, args.height, count), rng.randint(0, args.width, count)], axis=1).astype(np.float64)

    def report(name, stats, answers):
        stats['same_bytes'] = same(answers['device'], answers['host'])
        stats['host_over_device'] = stats['host']['median'] / stats['device']['median']
        print(name, ' '.join('%s %.2f ms' % (k, v['median']) for k, v in stats.items() if isinstance(v, dict)),
              'same bytes' if stats['same_bytes'] else 'DIFFERENT BYTES', flush=True)
        return stats

    for count in args.sizes:
        points = scatter(count)
        stats, answers = alternating({'device': lambda: detection.cluster_center_candidates(points, eps, min_samples, on='device'),
                                      'host': lambda: detection.cluster_center_candidates(points, eps, min_samples, on='host'),
                                      'scikit_learn': lambda: sklearn_clustering(points, eps, min_samples)}, args.warmup, args.repeats)
        stats['clusters'] = int(len(answers['host'][0]))
        stats['same_as_scikit_learn'] = same(answers['host'], answers['scikit_learn'])
        result['cluster_center_candidates'][str(count)] = report('cluster %i' % count, stats, answers)

    sets = [scatter(args.sizes[-1]) for _ in range(args.sets)]

    def flat(pairs):
        return [part for pair in pairs for part in pair]

    stats, answers = alternating({'device': lambda: flat(detection.cluster_center_candidates_batch(sets, eps, min_samples, on='device')),
                                  'host': lambda: flat(detection.cluster_center_candidates_batch(sets, eps, min_samples, on='host')),
                                  'scikit_learn': lambda: flat([sklearn_clustering(s, eps, min_samples) for s in sets])},
                                 args.warmup, args.repeats)
    stats['sets'], stats['points_per_set'] = args.sets, args.sizes[-1]
    result['cluster_center_candidates_batch'] = report('batch of %i' % args.sets, stats, answers)

    rays = rng.randint(0, 400, (args.sizes[-1], 24)).astype(np.float32)

    def loop():
        shifted = [descriptors.shift_ray_features(row) for row in rays]
        return np.array([row for row, _ in shifted]), np.array([shift for _, shift in shifted])

    def rows():
        table, shifts = descriptors.shift_ray_features_rows(rays)
        return table, np.array(shifts)

    stats, answers = alternating({'rows': rows, 'loop': loop}, args.warmup, args.repeats)
    stats['same_bytes'] = same(answers['rows'], answers['loop'])
    stats['loop_over_rows'] = stats['loop']['median'] / stats['rows']['median']
    stats['shape'] = list(rays.shape)
    result['shift_ray_features'] = stats
    print('shift rows %.2f ms loop %.2f ms' % (stats['rows']['median'], stats['loop']['median']),
          'same bytes' if stats['same_bytes'] else 'DIFFERENT BYTES', flush=True)

    eggs = make_case(args.height, args.width, args.eggs)
    img = np.where((eggs > 0)[:, :, None], np.array([200, 150, 90]), np.array([40, 40, 60])).astype(np.float64)
    img = np.clip(img + rng.normal(0, 6, img.shape), 0, 255).astype(np.uint8)
    levels, _ = center_annotation.create_annot_centers((eggs > 0).astype(np.uint8) * 255)
    segm = levels.astype(np.int64)
    params = dict(detection.CENTER_PARAMS, **detection.CLUSTER_PARAMS)
    _, _, points, features, _ = detection.estim_points_compute_features('', img, segm, params)
    target = (np.asarray(detection.label_close_points(levels, points, params)) >= 2).astype(int)
    classif = RandomForestClassifier(n_estimators=20, random_state=0, n_jobs=1).fit(features, target)

    def detect(on):
        found = detection.detect_centers(img, segm, classif, on=on, classif_on='device')
        return found['slic'], found['features'], found['labels'], found['candidates'], found['clust_labels'], found['centres']

    stats, answers = alternating({'device': lambda: detect('device'), 'host': lambda: detect('host')}, args.warmup, args.repeats)
    stats.update({'points': len(points), 'candidates': int(len(answers['host'][3])), 'centres': int(len(answers['host'][5])),
                  'eggs': args.eggs, 'trees': 20})
    result['detect_centers'] = report('detect_centers', stats, answers)
    print(json.dumps(result))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as out:
        json.dump(result, out, indent=1)
        out.write('\n')


if __name__ == '__main__':
    main()
