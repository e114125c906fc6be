#!/usr/bin/env python
"""Time ``predict_proba`` of the reference's random forest (20 trees, ``min_samples_leaf=2``, ``min_samples_split=3`` behind a
``StandardScaler``) on the device against scikit-learn on the same box, alternating in one process:

* host table -> host probabilities through ``imsegm_forest_proba`` (``_hip.forest_proba``: uploads, three kernels, download) against
  ``model.predict_proba`` with ``n_jobs=1`` and with ``n_jobs=-1``, on tables of 2 025 x 9, 1 954 x 180 and 298 116 x 3 rows x columns
  (the superpixel tables of benchmark configurations 2 and 3 and the supervoxels of configuration 5; seeded random values);
* the fused supervised step (``segment_color2d_slic_features_model_graphcut`` with a trained forest) on one 2048 x 2048 image with
  ``classif_on='device'`` against ``'host'`` -- the resident form of the evaluation is inside that step.

Median of ``--repeats`` runs after ``--warmup`` ones, with minimum and maximum; every device result is compared with the host's
bytes before it is timed.  No ratio is asserted: the record says what was measured, and where the device loses.

    python tools/time_forest_proba.py [--out profiles/forest_proba_time.json] [--repeats 5] [--warmup 2] [--size 2048]
"""
import argparse
import json
import os
import platform
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TABLES = ((2025, 9), (1954, 180), (298116, 3))


def timed(fn):
    start = time.perf_counter()
    fn()
    return (time.perf_counter() - start) * 1e3


def alternate(variants, repeats, warmup):
    """{name: {'median', 'min', 'max', 'runs'}} in ms: the variants take turns, ``warmup`` rounds are dropped"""
    runs = {name: [] for name in variants}
    for turn in range(warmup + repeats):
        for name, fn in variants.items():
            ms = timed(fn)
            if turn >= warmup:
                runs[name].append(ms)
    return {name: {'median': float(np.median(r)), 'min': min(r), 'max': max(r), 'runs': r} for name, r in runs.items()}


def fit_forest(rows, columns, seed):
    from sklearn.ensemble import RandomForestClassifier
    from sklearn.pipeline import Pipeline
    from sklearn.preprocessing import StandardScaler
    rng = np.random.RandomState(seed)
    table = rng.randn(rows, columns) * 3. + 1.
    labels = (np.abs(table[:, 0] * 1.7 + table[:, -1]) * 1.3).astype(int) % 3
    train = rng.choice(rows, min(rows, 2500), replace=False)
    model = Pipeline([('scaler', StandardScaler()),
                      ('classif', RandomForestClassifier(n_estimators=20, min_samples_leaf=2, min_samples_split=3, n_jobs=1, random_state=0))])
    return model.fit(table[train], labels[train]), table


def time_tables(repeats, warmup):
    from pyimsegm_amd import _hip
    cases = {}
    for rows, columns in TABLES:
        model, table = fit_forest(rows, columns, seed=rows)
        forest = _hip.DeviceForest(model)
        expected = model.predict_proba(table)
        assert np.array_equal(_hip.forest_proba(forest, table), expected), 'the device result differs from scikit-learn'

        def host(jobs):
            def run():
                model.set_params(classif__n_jobs=jobs)
                model.predict_proba(table)
            return run

        record = alternate({'device': lambda: _hip.forest_proba(forest, table), 'host_n_jobs_1': host(1), 'host_n_jobs_all': host(-1)},
                           repeats, warmup)
        model.set_params(classif__n_jobs=1)
        sizes = np.diff(forest.tree_start)
        record.update(rows=rows, columns=columns, trees=forest.n_trees, nodes_per_tree_max=int(sizes.max()), nodes=int(sizes.sum()),
                      device_over_host_n_jobs_1=record['device']['median'] / record['host_n_jobs_1']['median'])
        cases['%dx%d' % (rows, columns)] = record
    return cases


def time_step(size, repeats, warmup):
    from pyimsegm_amd import pipelines as pipe
    from pyimsegm_amd.utilities.synthetic import voronoi_image
    features = {'color': ['mean', 'std', 'energy']}
    small, annot = voronoi_image(512, 512, return_classes=True)
    np.random.seed(0)
    model = pipe.train_classif_color2d_slic_features([small], [annot], features, sp_size=30, sp_regul=0.2, pca_coef=None)[0]
    model.set_params(classif__n_jobs=1)
    image = voronoi_image(size, size)

    def step(place):
        return lambda: pipe.segment_color2d_slic_features_model_graphcut(image, model, features, sp_size=30, sp_regul=0.2, classif_on=place)

    on_host, on_device = step('host')(), step('device')()
    assert np.array_equal(on_host[0], on_device[0]) and np.array_equal(on_host[1], on_device[1]), 'the step differs between the places'
    record = alternate({'classif_on_device': step('device'), 'classif_on_host': step('host')}, repeats, warmup)
    record.update(image='%dx%d' % (size, size), classes=int(on_host[1].shape[2]),
                  device_over_host=record['classif_on_device']['median'] / record['classif_on_host']['median'])
    return record


def main():
    parser = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    parser.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'forest_proba_time.json'))
    parser.add_argument('--repeats', type=int, default=5)
    parser.add_argument('--warmup', type=int, default=2)
    parser.add_argument('--size', type=int, default=2048)
    args = parser.parse_args()
    import sklearn
    import torch

    from pyimsegm_amd import _hip
    if _hip.device_count() < 1:
        raise SystemExit('no HIP device: nothing is measured without one')
    record = {'repeats': args.repeats, 'warmup': args.warmup, 'unit': 'ms',
              'box': {'gpu': torch.cuda.get_device_name(0), 'cpu': platform.processor() or platform.machine(),
                      'cpus_usable': len(os.sched_getaffinity(0)), 'sklearn': sklearn.__version__, 'numpy': np.__version__},
              'forest': 'StandardScaler + RandomForestClassifier(n_estimators=20, min_samples_leaf=2, min_samples_split=3)',
              'tables': time_tables(args.repeats, args.warmup),
              'fused_supervised_step': time_step(args.size, args.repeats, args.warmup)}
    print(json.dumps(record, indent=1))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as out:
        json.dump(record, out, indent=1)


if __name__ == '__main__':
    main()
