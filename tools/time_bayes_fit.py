"""Time the Bayesian class model's fit on the host against the device fit (graph_cuts.estim_class_model(table, 3, 'BGM'),
fit_on='host' / 'device': nine restarts, max_iter=99) on one box, alternating, median of the runs after the warm-ups, on two tables
of tests/mixture_fit_cases.py: ``synthetic_300k`` (300 000 x 3, the size of a 64 x 4096 x 4096 volume's table) and
``reference_2048`` (1954 x 9).  The device fit is also split into seeding, Lloyd and the variational iterations (each with its
read-back; the last is the kernel time alone), and the iterations of every restart are recorded on both sides: the device's, and
scikit-learn's own loop from the same seeds (``--no-host-iterations`` leaves that out: it costs a host fit).

    python tools/time_bayes_fit.py [--runs 5] [--warmup 2] [--out profiles/bayes_fit_time.json]
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
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def median_ms(values):
    return round(float(np.median(values)) * 1e3, 3)


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--runs', type=int, default=5)
    parser.add_argument('--warmup', type=int, default=2)
    parser.add_argument('--out', default=os.path.join('profiles', 'bayes_fit_time.json'))
    parser.add_argument('--no-host-iterations', action='store_true')
    args = parser.parse_args()
    import bayes_fit_cases as BC
    import mixture_fit_cases as MC
    from sklearn.mixture import BayesianGaussianMixture
    from pyimsegm_amd import _hip, graph_cuts
    warnings.simplefilter('ignore')
    result = {'runs': args.runs, 'warmup': args.warmup, 'n_init': 9, 'n_classes': 3, 'max_iter': 99, 'tables': []}
    for name in ('synthetic_300k', 'reference_2048'):
        table = MC.load_table(name)
        n_rows, n_features = table.shape
        whole = {'host': [], 'device': []}
        for run in range(args.warmup + args.runs):
            for where in ('host', 'device'):
                np.random.seed(run)
                start = time.perf_counter()
                model = graph_cuts.estim_class_model(table, 3, 'BGM', use_scaler=False, fit_on=where)
                whole[where].append(time.perf_counter() - start)
                print(name, where, 'run', run, '%.1f ms' % (whole[where][-1] * 1e3), 'iterations of the winner',
                      model.steps[-1][1].n_iter_, flush=True)
        own = BayesianGaussianMixture(n_components=3)
        own._check_parameters(table)
        priors = (own.weight_concentration_prior_type, own.weight_concentration_prior_, own.mean_precision_prior_, own.mean_prior_,
                  own.degrees_of_freedom_prior_, own.covariance_prior_)
        parts = {'seeding': [], 'lloyd': [], 'variational': []}
        for run in range(args.warmup + args.runs):
            t0 = time.perf_counter()
            seeds = graph_cuts.device_fit_seeds(table, 3, 9, np.random.RandomState(run))
            t1 = time.perf_counter()
            lloyd = _hip.kmeans_lloyd(table, seeds, 300, 1e-4 * np.mean(np.var(table, axis=0)), want_labels=False)
            t2 = time.perf_counter()
            fit = _hip.bayes_mixture_em(9, 3, n_features, *priors, tol=1e-3, max_iter=99)
            t3 = time.perf_counter()
            parts['seeding'].append(t1 - t0)
            parts['lloyd'].append(t2 - t1)
            parts['variational'].append(t3 - t2)
        entry = {'table': name, 'rows': n_rows, 'features': n_features,
                 'host_ms': median_ms(whole['host'][args.warmup:]), 'device_ms': median_ms(whole['device'][args.warmup:]),
                 'device_parts_ms': {key: median_ms(values[args.warmup:]) for key, values in parts.items()},
                 'lloyd_iterations': lloyd['n_iter'].tolist(), 'device_iterations': fit['n_iter'].tolist()}
        if not args.no_host_iterations:      # scikit-learn's loop from the seeds of the last run above
            labels = MC.reference_lloyd(table, seeds)[0]
            entry['host_iterations'] = [BC.reference_bayes_em(table, lab, 1e-3, 99, BC.PROCESS, n_components=3)['n_iter'] for lab in labels]
        print(json.dumps(entry), flush=True)
        result['tables'].append(entry)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as out:
        json.dump(result, out, indent=1)


if __name__ == '__main__':
    main()
