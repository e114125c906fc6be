#!/usr/bin/env python
"""Times a region growing in the egg-segmentation driver's setting (run_ovary_egg-segmentation.py:548-639): a synthetic 1024 x 647
class map, superpixels of size 15 (staggered squares, ~3000), ~20 centres, a 'set_cdfs' model of 5 tables of 72 angles;
``region_growing_shape_slic_greedy`` with greedy_tol=1e-1, nb_iter=1000, then ``region_growing_shape_slic_graphcut`` with
nb_iter=250.  ``on='device'`` against ``on='host'`` of the same build, alternating, medians of 7 after a warm-up.  It also times a
stand-in for the per-iteration traffic of the device path (K labels up, K / 4 candidate triples down, once per iteration, through a
scratch buffer of its own): an estimate of what the copies cost, not the growth's own copies timed apart.

THE YARDSTICK IS THIS REPOSITORY'S OWN NUMPY STATEMENT (pyimsegm_amd/region_growing.py, on='host'), NOT the reference: the
reference (one ``interp2d`` object per superpixel and object) cannot run where the GPU is, and the parent commit has no such
function.  The cut of the graph-cut variant runs on the device on both sides.

    python tools/time_region_growing.py [--out profiles/region_growing_time.json] [--repeats 7] [--greedy-iter 1000] [--graphcut-iter 250]

Exits non-zero when the device path is slower than the host statement in either variant, or when the two return other labels."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HEIGHT, WIDTH, STEP, NB_ANGLES, NB_TABLES = 647, 1024, 15, 72, 5


class NearestMeans(object):
    """a mixture with unit covariances around the mean ray vectors: ``predict_proba`` as the growth calls it"""

    def __init__(self, means):
        self.means_ = np.asarray(means, dtype=np.float64)

    def predict_proba(self, samples):
        score = -0.5 * np.sum((np.asarray(samples, dtype=np.float64)[:, None, :] - self.means_[None])**2, axis=2)
        score = np.exp(score - score.max(axis=1, keepdims=True))
        return score / score.sum(axis=1, keepdims=True)


def scene(seed=0):
    """(slic, slic_prob_fg, centres, shape_model): 4 x 5 eggs, squares of 15 pixels with every other row shifted by half a square"""
    rng = np.random.default_rng(seed)
    rows, cols = np.indices((HEIGHT, WIDTH))
    band = rows // STEP
    per_row = WIDTH // STEP + 2
    slic = band * per_row + (cols + (band % 2) * (STEP // 2)) // STEP
    slic = np.unique(slic, return_inverse=True)[1].reshape(HEIGHT, WIDTH)
    segm = np.zeros((HEIGHT, WIDTH), dtype=bool)
    centres = []
    for row in range(4):
        for col in range(5):
            cy, cx = 90 + 155 * row + rng.normal(0, 8), 110 + 200 * col + rng.normal(0, 8)
            a, b, theta = rng.uniform(45, 60), rng.uniform(60, 85), rng.uniform(-1.5, 1.5)
            r, c = rows - cy, cols - cx
            segm |= ((r * np.cos(theta) + c * np.sin(theta)) / a)**2 + ((r * np.sin(theta) - c * np.cos(theta)) / b)**2 <= 1
            centres.append((int(cy + rng.integers(-10, 11)), int(cx + rng.integers(-10, 11))))
    inside = np.bincount(slic.ravel(), segm.ravel(), int(slic.max()) + 1) / np.bincount(slic.ravel())
    prob = np.where(inside > 0.5, 0.9, 0.1)
    model = []
    for k in range(NB_TABLES):
        nb_dists = 80 + 10 * k
        radius = (45 + 7 * k) * (1 + 0.25 * np.cos(2 * np.linspace(0, 2 * np.pi, NB_ANGLES, endpoint=False)))
        table = 1. / (1. + np.exp((np.arange(nb_dists)[None, :] - radius[:, None]) / 5.))
        model.append((radius.tolist(), np.round(table, 3)))
    return slic, prob, centres, (NearestMeans([m for m, _ in model]), model)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'region_growing_time.json'))
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--greedy-iter', type=int, default=1000)
    ap.add_argument('--graphcut-iter', type=int, default=250)
    args = ap.parse_args()
    from pyimsegm_amd import _hip
    from pyimsegm_amd import region_growing as rg
    slic, prob, centres, shape_model = scene()
    nb_labels = int(slic.max()) + 1
    variants = {
        'greedy': lambda on, history=None: rg.region_growing_shape_slic_greedy(
            slic, prob, centres, shape_model, 'set_cdfs', coef_shape=5., coef_pairwise=15., greedy_tol=1e-1, nb_iter=args.greedy_iter,
            debug_history=history, on=on),
        'graphcut': lambda on, history=None: rg.region_growing_shape_slic_graphcut(
            slic, prob, centres, shape_model, 'set_cdfs', coef_shape=5., coef_pairwise=15., nb_iter=args.graphcut_iter,
            debug_history=history, on=on),
    }
    result = {'what': 'region growing of %d centres on %d superpixels (map %d x %d, size %d), set_cdfs of %d tables x %d angles' %
                      (len(centres), nb_labels, WIDTH, HEIGHT, STEP, NB_TABLES, NB_ANGLES),
              'yardstick': "this repository's own numpy statement (region_growing on='host'), not the reference",
              'repeats': args.repeats, 'nb_iter': {'greedy': args.greedy_iter, 'graphcut': args.graphcut_iter}}
    ctx = _hip.default_context()
    slower = False
    for name, grow in variants.items():
        history = {}
        device = grow('device', history)                                    # (the warm-up of both sides, and the comparison)
        host = grow('host')
        iterations = len(history['labels'])
        times = {'device': [], 'host': []}
        for _ in range(args.repeats):
            for on in ('device', 'host'):
                start = time.perf_counter()
                grow(on)
                times[on].append((time.perf_counter() - start) * 1e3)
        # a stand-in for what an iteration moves: K labels up, the (object, superpixel, change) triples of K / 4 candidates down
        up, down = nb_labels * 4, (nb_labels // 4) * 16
        staging = np.zeros(max(up, down), dtype=np.uint8)
        scratch = _hip.C.c_void_p()
        _hip._check(_hip.load_library().imsegm_device_alloc(ctx.device, len(staging), _hip.C.byref(scratch)))
        moves = []
        for _ in range(args.repeats + 1):
            start = time.perf_counter()
            for _ in range(iterations):
                ctx.copy(scratch.value, staging.ctypes.data, up)
                ctx.copy(staging.ctypes.data, scratch.value, down)
            moves.append((time.perf_counter() - start) * 1e3)
        _hip.load_library().imsegm_device_free(scratch)
        result[name] = {'iterations': iterations, 'labels_equal': bool(np.array_equal(device, host)),
                        'device_ms_median': float(np.median(times['device'])), 'host_ms_median': float(np.median(times['host'])),
                        'traffic_stand_in_ms_median': float(np.median(moves[1:])), 'device_ms': times['device'], 'host_ms': times['host']}
        slower |= result[name]['device_ms_median'] > result[name]['host_ms_median'] or not result[name]['labels_equal']
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as fp:
        json.dump(result, fp, indent=1)
    print(json.dumps({k: ({kk: vv for kk, vv in v.items() if not kk.endswith('_ms')} if isinstance(v, dict) else v)
                      for k, v in result.items()}))
    return 1 if slower else 0


if __name__ == '__main__':
    sys.exit(main())
