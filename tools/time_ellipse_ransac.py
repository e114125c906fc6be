#!/usr/bin/env python
"""Times the RANSAC scoring of ellipse trials in the egg-segmentation driver's setting (250 trials, residual threshold 25,
min_samples 0.35) on a synthetic 1024 x 647 class map with ~20 centres: ``imsegm_ellipse_ransac`` on the device against
``score_trials_host``, alternating, medians of 7 after a warm-up, with the transfers of the device call timed alone.

THE YARDSTICK IS THIS REPOSITORY'S OWN NUMPY STATEMENT of the three definitions (pyimsegm_amd/ellipse_fitting.py, on='host'), NOT
the reference: the reference (scikit-image's per-point ``leastsq``) cannot run where the GPU is, and the parent commit has no such
call.  Sampling and the estimates are the same host code on both sides and are reported once.

    python tools/time_ellipse_ransac.py [--out profiles/ellipse_ransac_time.json]

Exits non-zero when the device is slower than the host statement."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HEIGHT, WIDTH, STEP, EGGS, TRIALS, THRESHOLD, MIN_SAMPLES, POINTS, REPEATS = 647, 1024, 15, 20, 250, 25., 0.35, 72, 7


def scene(seed=0):
    """~20 eggs on a grid of the map, superpixel-like centres every 15 pixels (~2900), 72 boundary points per egg, a fifth outliers"""
    rng = np.random.default_rng(seed)
    centres = np.stack(np.meshgrid(np.arange(STEP // 2, HEIGHT, STEP), np.arange(STEP // 2, WIDTH, STEP), indexing='ij'), axis=-1)
    centres = (centres.reshape(-1, 2) + rng.integers(-3, 4, (centres.shape[0] * centres.shape[1], 2))).astype(np.float64)
    labels = np.zeros(len(centres), dtype=np.int64)
    list_points = []
    for row in range(4):
        for col in range(5):
            true = (90 + 155 * row + rng.normal(0, 8), 110 + 200 * col + rng.normal(0, 8), rng.uniform(45, 65), rng.uniform(60, 90),
                    rng.uniform(-1.5, 1.5))
            r, c = centres[:, 0] - true[0], centres[:, 1] - true[1]
            inside = ((r * np.cos(true[4]) + c * np.sin(true[4])) / true[2]) ** 2 + ((r * np.sin(true[4]) - c * np.cos(true[4])) / true[3]) ** 2 <= 1
            labels[inside] = 1 + (rng.uniform(size=inside.sum()) < 0.5)
            t = rng.uniform(0, 2 * np.pi, POINTS)
            points = np.stack([true[0] + true[2] * np.cos(true[4]) * np.cos(t) - true[3] * np.sin(true[4]) * np.sin(t),
                               true[1] + true[2] * np.sin(true[4]) * np.cos(t) + true[3] * np.cos(true[4]) * np.sin(t)], axis=1)
            points += rng.normal(0, 1.5, points.shape)
            points[:POINTS // 5] += rng.normal(0, 40, (POINTS // 5, 2))
            list_points.append(points)
    weights = rng.integers(150, 300, len(centres))
    return list_points[:EGGS], centres, weights, labels, [[0.01, 0.7, 0.95], [0.99, 0.3, 0.05]]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'ellipse_ransac_time.json'))
    args = ap.parse_args()
    from pyimsegm_amd import _hip
    from pyimsegm_amd import ellipse_fitting as ell
    list_points, centres, weights, labels, table_prob = scene()
    np.random.seed(0)
    t0 = time.perf_counter()
    nb = int(MIN_SAMPLES * POINTS)
    drawn = [np.array([np.random.choice(POINTS, nb, replace=False) for _ in range(TRIALS)]) for _ in list_points]
    t1 = time.perf_counter()
    fits = [ell.estimate_stack(points[idx]) for points, idx in zip(list_points, drawn)]
    t2 = time.perf_counter()
    params, success = np.concatenate([f[0] for f in fits]), np.concatenate([f[1] for f in fits]).astype(np.uint8)
    job = (np.arange(len(list_points) + 1, dtype=np.int32) * POINTS, np.concatenate(list_points), params, success,
           np.repeat(np.arange(len(list_points), dtype=np.int32), TRIALS), centres, ell.point_values(centres, weights, labels, table_prob),
           THRESHOLD)
    ctx = _hip.default_context()
    nbytes = sum(np.asarray(a).nbytes for a in job[:7])
    staging = np.zeros(nbytes, dtype=np.uint8)

    def transfers():
        # what the call moves, alone: its inputs up and its results (two indices per egg, one byte per point, one double per
        # trial) down, through the same scratch
        ctx.copy(ctx_scratch, staging.ctypes.data, nbytes)
        ctx.copy(staging.ctypes.data, ctx_scratch, len(list_points) * 8 + len(job[1]) + len(params) * 8)

    scratch = _hip.C.c_void_p()
    _hip._check(_hip.load_library().imsegm_device_alloc(ctx.device, nbytes, _hip.C.byref(scratch)))
    ctx_scratch = scratch.value
    device = _hip.ellipse_ransac(*job)
    host = ell.score_trials_host(*job)
    same = all(np.array_equal(a, b) for a, b in zip(device[:3], host[:3]))
    transfers()
    times = {'device': [], 'host': [], 'transfers': []}
    for _ in range(REPEATS):
        for name, call in (('device', lambda: _hip.ellipse_ransac(*job)), ('host', lambda: ell.score_trials_host(*job)),
                           ('transfers', transfers)):
            start = time.perf_counter()
            call()
            times[name].append((time.perf_counter() - start) * 1e3)
    _hip.load_library().imsegm_device_free(scratch)
    result = {
        'what': 'RANSAC scoring of %d eggs x %d trials, %d points per egg, %d centres, threshold %g (map %d x %d)' % (
            len(list_points), TRIALS, POINTS, len(centres), THRESHOLD, WIDTH, HEIGHT),
        'yardstick': "this repository's own numpy statement (ellipse_fitting.score_trials_host), not the reference",
        'device_ms_median': float(np.median(times['device'])), 'host_ms_median': float(np.median(times['host'])),
        'transfers_alone_ms_median': float(np.median(times['transfers'])), 'device_ms': times['device'], 'host_ms': times['host'],
        'sampling_ms_once': (t1 - t0) * 1e3, 'estimates_ms_once': (t2 - t1) * 1e3, 'successful_trials': int(success.sum()),
        'best_kept_mask_equal': bool(same), 'repeats': REPEATS,
    }
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as fp:
        json.dump(result, fp, indent=1)
    print(json.dumps({k: v for k, v in result.items() if not k.endswith('_ms')}))
    return 0 if result['device_ms_median'] <= result['host_ms_median'] else 1


if __name__ == '__main__':
    sys.exit(main())
