#!/usr/bin/env python
"""Time the scoring functions of ``pyimsegm_amd.classification`` on the device against their host statement (``on='host'``) on the same
box, alternating, end to end from host memory to the returned result: ``compute_stat_per_image`` on one 2048 x 2048 pair with 4
classes and on eight 647 x 1024 pairs, with ``relabel`` off and on, int32 and uint8 maps; ``compute_classif_metrics`` and
``compute_tp_tn_fp_fn`` on the single pair (two classes for the latter); ``_hip.score_pairs`` alone (uploads, three kernels, download),
the same call with every label dropped (the counting pass returns at once), and the transfers alone: the same arrays copied to the
device from pageable memory by torch, one copy per array, then a synchronise.

THE YARDSTICK IS THIS REPOSITORY'S OWN HOST STATEMENT, not the reference.  Median of ``--repeats`` runs after ``--warmup`` ones, with
minimum and maximum.  ``host_by_default`` lists the functions whose device median is not below their host median in some case;
``classification.HOST_BY_DEFAULT`` follows it.

    python tools/time_scoring.py [--out profiles/scoring_time.json] [--repeats 5] [--warmup 2]

For the two pixel kernels' own durations run ``rocprofv3 --kernel-trace --stats -- python tools/time_scoring.py --kernels-only`` (a run of
its own: ten ``score_pairs`` calls per case and nothing else) and set them against the bytes they must move, 8 B per pixel and pass for
int32 and 2 B for uint8 (``bytes_per_pass`` in the file).
"""
import argparse
import json
import os
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_pairs(count, height, width, classes, dtype, seed=0):
    """blocky annotations over ``classes`` labels and segmentations that agree on 85 % of the pixels"""
    rng = np.random.RandomState(seed)
    pairs = []
    for _ in range(count):
        coarse = rng.randint(0, classes, (height // 16 + 1, width // 16 + 1))
        annot = np.repeat(np.repeat(coarse, 16, axis=0), 16, axis=1)[:height, :width]
        segm = np.where(rng.rand(height, width) < 0.85, annot, rng.randint(0, classes, (height, width)))
        pairs.append((annot.astype(dtype), segm.astype(dtype)))
    return pairs


def timed_alternating(runs, warmup, repeats):
    """``runs``: place -> callable; the places take turns so that drifts of the box hit both"""
    times, results = {place: [] for place in runs}, {}
    for i in range(warmup + repeats):
        for place, run in runs.items():
            t0 = time.perf_counter()
            results[place] = run()
            if i >= warmup:
                times[place].append((time.perf_counter() - t0) * 1e3)
    return {place: {'median': float(np.median(t)), 'min': float(np.min(t)), 'max': float(np.max(t)), 'runs': t} for place, t in times.items()}, results


def same(a, b):
    if hasattr(a, 'to_dict'):
        a, b = a.to_dict('index'), b.to_dict('index')
    if isinstance(a, dict):
        return list(a) == list(b) and all(same(a[key], b[key]) for key in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if isinstance(a, float):
        return (a != a and b != b) or abs(a - b) <= 1e-12 * abs(b)
    return a == b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'scoring_time.json'))
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--kernels-only', action='store_true', help='ten score_pairs calls per case and nothing else, for a kernel trace')
    args = ap.parse_args()
    warnings.filterwarnings('ignore')
    import torch
    from pyimsegm_amd import _hip
    from pyimsegm_amd import classification as clf
    _hip.default_context()
    layouts = {'1x2048x2048_4classes': (1, 2048, 2048, 4), '8x647x1024_4classes': (8, 647, 1024, 4)}
    if args.kernels_only:
        for count, height, width, classes in layouts.values():
            for dtype in (np.int32, np.uint8):
                pairs = make_pairs(count, height, width, classes, dtype)
                for _ in range(10):
                    _hip.score_pairs([a.ravel() for a, _ in pairs], [s.ravel() for _, s in pairs])
        return
    result = {'repeats': args.repeats, 'warmup': args.warmup, 'unit': 'ms',
              'yardstick': "this repository's own host statement (on='host': scikit-learn and numpy on the vectors), same box, alternating",
              'cases': {}}
    slower = set()
    for layout, (count, height, width, classes) in layouts.items():
        for dtype in (np.int32, np.uint8):
            pairs = make_pairs(count, height, width, classes, dtype)
            annots, segms = [a for a, _ in pairs], [s for _, s in pairs]
            flat = [a.ravel() for a in annots], [s.ravel() for s in segms]
            pixels = count * height * width
            entry = {'pixels': pixels, 'bytes_per_pass': 2 * pixels * np.dtype(dtype).itemsize}
            calls = {'compute_stat_per_image': lambda on: clf.compute_stat_per_image(segms, annots, on=on),
                     'compute_stat_per_image_relabel': lambda on: clf.compute_stat_per_image(segms, annots, relabel=True, on=on)}
            if count == 1:
                binary = (annots[0] > 1).astype(dtype), (segms[0] > 1).astype(dtype)
                calls['compute_classif_metrics'] = lambda on: clf.compute_classif_metrics(flat[0][0], flat[1][0], on=on)
                calls['compute_tp_tn_fp_fn'] = lambda on: clf.compute_tp_tn_fp_fn(binary[0], binary[1], on=on)
            for name, call in calls.items():
                row, results = timed_alternating({'device': lambda: call('device'), 'host': lambda: call('host')}, args.warmup, args.repeats)
                row['same_result'] = bool(same(results['device'], results['host']))
                row['host_over_device'] = row['host']['median'] / row['device']['median']
                if row['device']['median'] >= row['host']['median']:
                    slower.add(name.replace('_relabel', ''))
                entry[name] = row
                print('%-22s %-6s %-32s device %9.2f ms, host %9.2f ms' % (layout, np.dtype(dtype).name, name, row['device']['median'],
                                                                           row['host']['median']), flush=True)
            def upload():
                held = [torch.from_numpy(vector).to('cuda') for vector in flat[0] + flat[1]]
                torch.cuda.synchronize()
                return len(held)

            row, _ = timed_alternating({'score_pairs': lambda: _hip.score_pairs(flat[0], flat[1]),
                                        'score_pairs_all_dropped': lambda: _hip.score_pairs(flat[0], flat[1], list(range(classes))),
                                        'transfers': upload}, args.warmup, args.repeats)
            entry['score_pairs'] = row
            print('%-22s %-6s %-32s %9.2f ms, every label dropped %9.2f ms' % (layout, np.dtype(dtype).name, 'score_pairs', row['score_pairs']['median'],
                                                                              row['score_pairs_all_dropped']['median']), flush=True)
            print('%-22s %-6s %-32s %9.2f ms' % (layout, np.dtype(dtype).name, 'transfers alone (torch)', row['transfers']['median']), flush=True)
            result['cases']['%s_%s' % (layout, np.dtype(dtype).name)] = entry
    result['host_by_default'] = sorted(slower)
    result['host_by_default_in_module'] = sorted(clf.HOST_BY_DEFAULT)
    print(json.dumps({'host_by_default': result['host_by_default'], 'in_module': result['host_by_default_in_module']}))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as out:
        json.dump(result, out, indent=1)
        out.write('\n')


if __name__ == '__main__':
    main()
