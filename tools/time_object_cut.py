#!/usr/bin/env python
"""Time ``object_segmentation_graphcut_pixels`` at the size and parameters of the egg experiment's ``GC_pixels-shape`` method
(1024 x 768, 12 centres, seed_size=10, coef_shape=0.1, gc_regul=3): once on the device path, once as the route it replaces -- the
numpy statement in front of pyGCO's edge list in numpy and ``cut_general_graph`` (what ``cut_grid_graph`` did before).  Median of
``--repeats`` runs after ``--warmup`` ones, with the split into building the terms and the topology versus the cut (the cut's
kernel time from the context's profiler).

    python tools/time_object_cut.py [--out profiles/object_cut_time.json] [--repeats 5] [--warmup 2] [--height 768 --width 1024]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_case(height, width, n_centres, seed=0):
    rng = np.random.RandomState(seed)
    rows, cols = np.indices((height, width))
    centres = [(int(rng.randint(40, height - 40)), int(rng.randint(40, width - 40))) for _ in range(n_centres)]
    segm = np.zeros((height, width), dtype=int)
    for i, (r, c) in enumerate(centres):
        segm[(rows - r)**2 + (cols - c)**2 <= (30 + 3 * i)**2] = 1 + i % 2
    noise = rng.rand(height, width) < 0.02
    segm[noise] = rng.randint(0, 3, int(noise.sum()))
    return segm, centres


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'object_cut_time.json'))
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--height', type=int, default=768)
    ap.add_argument('--width', type=int, default=1024)
    ap.add_argument('--centres', type=int, default=12)
    args = ap.parse_args()
    from pyimsegm_amd import _hip
    from pyimsegm_amd import region_growing as rg
    segm, centres = make_case(args.height, args.width, args.centres)
    kwargs = dict(labels_fg_prob=(0.1, 0.9, 0.7), gc_regul=3., seed_size=10, coef_shape=0.1, shape_mean_std=(50., 10.))
    ctx = _hip.default_context()
    ctx.profile_enable(True)

    def cut_ms():
        return sum(ctx.profile_get(group)[0] for group in ('graphcut', ))

    def device():
        t0 = time.perf_counter()
        labels = rg.object_segmentation_graphcut_pixels(segm, centres, on='device', **kwargs)
        total = (time.perf_counter() - t0) * 1e3
        return labels, total, None

    def parent():
        t0 = time.perf_counter()
        rounded = [np.round(c).astype(int) for c in centres]
        tables = rg._object_tables(kwargs['labels_fg_prob'], kwargs['coef_shape'], kwargs['shape_mean_std'],
                                   rg._max_centre_distance(segm.shape, rounded))
        unary = rg._object_pixels_unary(segm, rounded, tables, kwargs['coef_shape'], kwargs['seed_size'])
        height, width, n_labels = unary.shape
        pairwise = (1 - np.eye(n_labels)) * kwargs['gc_regul']
        index = np.arange(height * width, dtype=np.int32).reshape(height, width)
        edges = np.concatenate([np.stack([index[:-1].ravel(), index[1:].ravel()], axis=1),
                                np.stack([index[:, :-1].ravel(), index[:, 1:].ravel()], axis=1)], axis=0)
        weights = np.ones(len(edges))
        front = (time.perf_counter() - t0) * 1e3
        labels = _hip.cut_general_graph(edges, weights, unary.reshape(height * width, n_labels), pairwise, n_iter=999)
        total = (time.perf_counter() - t0) * 1e3
        return labels.reshape(segm.shape), total, front

    result = {'height': args.height, 'width': args.width, 'centres': args.centres, 'parameters': {k: v for k, v in kwargs.items()},
              'repeats': args.repeats, 'warmup': args.warmup, 'unit': 'ms', 'routes': {}}
    answers = {}
    for name, run in (('device', device), ('parent', parent)):
        totals, cuts, fronts = [], [], []
        for i in range(args.warmup + args.repeats):
            ctx.profile_reset()
            labels, total, front = run()
            cut = cut_ms()
            if i >= args.warmup:
                totals.append(total)
                cuts.append(cut)
                fronts.append(front)
            print(name, 'run', i, 'total %.1f ms, cut kernels %.1f ms' % (total, cut), flush=True)
        answers[name] = labels
        entry = {'total': totals, 'total_median': float(np.median(totals)), 'cut_kernels': cuts, 'cut_kernels_median': float(np.median(cuts)),
                 'front_median': float(np.median(np.array(totals) - np.array(cuts)))}
        if fronts[0] is not None:
            entry['numpy_statement_and_edges_median'] = float(np.median(fronts))
        result['routes'][name] = entry
    result['same_labels'] = bool(np.array_equal(answers['device'], answers['parent']))
    print(json.dumps(result))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as out:
        json.dump(result, out, indent=1)
        out.write('\n')


if __name__ == '__main__':
    main()
