"""Time the class model's fit on the host against the device fit (graph_cuts.estim_class_model, fit_on='host' / 'device') on one
box, alternating, median of the runs after a warm-up, for the two sizes the pipelines meet: the 1954 x 9 table of a 2048 x 2048
image and the 298 116 x 3 table of a 64 x 4096 x 4096 volume (seeded synthetic tables of three overlapping Gaussians); the
device fit is also split into seeding, Lloyd and EM (each with its read-back).  ``--wide`` times the wide device fit
(fit_on='device_wide') instead, on the 1954 x 180 Leung-Malik table of tests/golden/reference_c3.npz (standardised once, outside
the timing); ``--device-only`` runs the device leg alone (for a kernel trace).

    python tools/time_mixture_fit.py [--runs 7] [--out profiles/mixture_fit_time.json]
    python tools/time_mixture_fit.py --wide [--device-only] [--out profiles/mixture_fit_wide_time.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def table_of(n_rows, n_features, seed=20261016):
    rng = np.random.RandomState(seed)
    means = rng.uniform(-3, 3, (3, n_features))
    scales = rng.uniform(.6, 1.3, (3, n_features))
    which = rng.randint(0, 3, n_rows)
    raw = means[which] + rng.standard_normal((n_rows, n_features)) * scales[which]
    return np.ascontiguousarray((raw - raw.mean(axis=0)) / raw.std(axis=0))


def golden_wide_table():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    raw = np.asarray(np.load(os.path.join(root, 'tests', 'golden', 'reference_c3.npz'))['features'], dtype=np.float64)
    return np.ascontiguousarray((raw - raw.mean(axis=0)) / raw.std(axis=0))


def median_ms(values):
    return round(float(np.median(values)) * 1e3, 3)


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--runs', type=int, default=7)
    parser.add_argument('--out', default=None)
    parser.add_argument('--wide', action='store_true')
    parser.add_argument('--device-only', action='store_true')
    args = parser.parse_args()
    from pyimsegm_amd import _hip, graph_cuts
    out_path = args.out or os.path.join('profiles', 'mixture_fit_wide_time.json' if args.wide else 'mixture_fit_time.json')
    device = 'device_wide' if args.wide else 'device'
    kmeans_lloyd, mixture_em = (_hip.kmeans_lloyd_wide, _hip.mixture_em_wide) if args.wide else (_hip.kmeans_lloyd, _hip.mixture_em)
    result = {'runs': args.runs, 'n_init': 9, 'n_classes': 3, 'sizes': []}
    for n_rows, n_features in ((1954, 180), ) if args.wide else ((1954, 9), (298116, 3)):
        table = golden_wide_table() if args.wide else table_of(n_rows, n_features)
        whole = {'host': [], 'device': []}
        for run in range(args.runs + 1):
            for where in ('device', ) if args.device_only else ('host', 'device'):
                np.random.seed(run)
                start = time.perf_counter()
                graph_cuts.estim_class_model(table, 3, use_scaler=False, fit_on=device if where == 'device' else where)
                whole[where].append(time.perf_counter() - start)
        # --wide: the device fit again without a host fit in between (the alternating figure starts from a device that sat idle for the
        # length of a host fit, and from caches the host fit has filled)
        back_to_back = []
        for run in range(args.runs + 1 if args.wide else 0):
            np.random.seed(run)
            start = time.perf_counter()
            graph_cuts.estim_class_model(table, 3, use_scaler=False, fit_on=device)
            back_to_back.append(time.perf_counter() - start)
        parts = {'seeding': [], 'lloyd': [], 'em': []}
        for run in range(args.runs + 1):
            t0 = time.perf_counter()
            seeds = graph_cuts.device_fit_seeds(table, 3, 9, np.random.RandomState(run))
            t1 = time.perf_counter()
            lloyd = kmeans_lloyd(table, seeds, 300, 1e-4 * np.mean(np.var(table, axis=0)), want_labels=False)
            t2 = time.perf_counter()
            fit = mixture_em(9, 3, n_features, tol=1e-3, max_iter=99)
            t3 = time.perf_counter()
            parts['seeding'].append(t1 - t0)
            parts['lloyd'].append(t2 - t1)
            parts['em'].append(t3 - t2)
        entry = {'rows': n_rows, 'features': n_features,
                 'host_ms': median_ms(whole['host'][1:]) if whole['host'] else None, 'device_ms': median_ms(whole['device'][1:]),
                 'device_parts_ms': {key: median_ms(values[1:]) for key, values in parts.items()},
                 'lloyd_iterations': lloyd['n_iter'].tolist(), 'em_iterations': fit['n_iter'].tolist()}
        if back_to_back:
            entry['device_back_to_back_ms'] = median_ms(back_to_back[1:])
        print(json.dumps(entry), flush=True)
        result['sizes'].append(entry)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, 'w') as out:
        json.dump(result, out, indent=1)


if __name__ == '__main__':
    main()
