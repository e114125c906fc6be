#!/usr/bin/env python
"""Golden vectors of the reference's `compute_object_shapes`, `compute_cumulative_distrib` and its six `transform_rays_model_*`
functions (`imsegm/region_growing.py:259-588`), all run UNCHANGED under the build container's conda Python 3.9 with its scipy and
scikit-learn (/opt/conda/bin/python3.9 tests/golden/make_golden_object_shapes.py, through `_reference_env.ReferenceEnv` like the
other generators).  Only numbers are stored, plus the seeds.

* `shapes_<case>_*` for the seeded maps of tests/object_shapes_cases.py: the rays and shifts `compute_object_shapes` returned and,
  per object in call order (captured by wrapping `compute_segm_object_shape` and `compute_ray_features_segm_2d` as
  make_golden_region_growing.py does), the rounded centre of mass and the raw 'down' rays; the labels are `np.unique(map)[1:]`, or
  1 .. n for a map of at most two values, checked against every mask.
* `model_<function>_<table>_*`: the fitted scikit-learn attributes of the reference's run on the doctest's ray list and on a
  seeded table, the `max_dist` it handed to `compute_cumulative_distrib`, and the tables it returned.
* `histograms_*`, `cumulative_*`: `transform_rays_model_cdf_histograms` and `compute_cumulative_distrib` on the doctest inputs and
  on two seeded tables.

Conditions asserted, which concern the reference alone (the generator re-seeds a map until they hold):

* no centre-of-mass coordinate lies within 1e-9 of a rounding tie unless it is exactly one;
* every case has at least one object;
* at least one stored object has a ray of -1."""
import os
import sys

import numpy as np

from _reference_env import HERE, ROOT, ReferenceEnv

sys.path.insert(0, os.path.join(ROOT, 'tests'))


class Rejected(Exception):
    pass


def run_shapes(ref, cases, name, seed):
    from scipy import ndimage
    img, ray_step = cases.case(name, seed)
    calls, raw = [], [None]
    originals = ref.compute_segm_object_shape, ref.compute_ray_features_segm_2d

    def rays_2d(*args, **kwargs):
        raw[0] = np.array(originals[1](*args, **kwargs), dtype=np.float32)
        return raw[0].copy()

    def object_shape(img_object, *args, **kwargs):
        mass = ndimage.center_of_mass(img_object)
        for c in mass:
            frac = c - np.floor(c)
            if c * 2 != np.floor(c * 2) and abs(frac - 0.5) <= 1e-9:
                raise Rejected('a centre coordinate next to a rounding tie')
        result = originals[0](img_object, *args, **kwargs)
        calls.append((np.array(img_object), [int(round(c)) for c in mass], raw[0].copy()))
        return result

    ref.compute_segm_object_shape, ref.compute_ray_features_segm_2d = object_shape, rays_2d
    try:
        list_rays, list_shifts = ref.compute_object_shapes([img], ray_step=ray_step)
    finally:
        ref.compute_segm_object_shape, ref.compute_ray_features_segm_2d = originals
    if not calls:
        raise Rejected('no object')
    values = np.unique(img)
    labels = np.arange(1, len(calls) + 1) if len(values) <= 2 else values[1:]
    assert len(labels) == len(calls) == len(list_rays)
    if len(values) > 2:
        for label, (mask, _, _) in zip(labels, calls):
            assert np.array_equal(mask, img == label)
    return {'seed': seed, 'labels': np.asarray(labels, dtype=np.int64), 'centres': np.array([c[1] for c in calls], dtype=np.int32),
            'rays_raw': np.array([c[2] for c in calls], dtype=np.float32), 'rays': np.array(list_rays, dtype=np.float64),
            'shifts': np.array(list_shifts, dtype=np.float64)}


def run_models(ref, table_name, list_rays, out):
    """the five scikit-learn variants: attributes of the estimators the reference fitted, max_dist, tables"""
    handed = []
    original = ref.compute_cumulative_distrib

    def cumulative(means, stds, weights, max_dist):
        handed.append(float(max_dist))
        return original(means, stds, weights, max_dist)

    ref.compute_cumulative_distrib = cumulative
    try:
        def store(function, **values):
            values['max_dist'] = np.array(handed)
            del handed[:]
            out.update({'model_%s_%s_%s' % (function, table_name, key): np.asarray(value) for key, value in values.items()})

        np.random.seed(0)
        mm, cdist = ref.transform_rays_model_cdf_mixture(list_rays)
        store('cdf_mixture', means=mm.means_, covariances=mm.covariances_, weights=mm.weights_, n_components=mm.n_components,
              table=cdist)
        np.random.seed(0)
        mm, pairs = ref.transform_rays_model_sets_mean_cdf_mixture(list_rays, 2)
        store('sets_mean_cdf_mixture', means=mm.means_, covariances=mm.covariances_, table_means=[p[0] for p in pairs],
              **{'table%d' % i: p[1] for i, p in enumerate(pairs)})
        np.random.seed(0)
        km, pairs = ref.transform_rays_model_sets_mean_cdf_kmeans(list_rays, 2)
        store('sets_mean_cdf_kmeans', centres=km.cluster_centers_, labels=km.labels_, table_means=[p[0] for p in pairs],
              **{'table%d' % i: p[1] for i, p in enumerate(pairs)})
        np.random.seed(0)
        sc, cdist = ref.transform_rays_model_cdf_spectral(list_rays, 3)
        store('cdf_spectral', labels=sc.labels_, table=cdist)
        np.random.seed(0)
        km, cdist = ref.transform_rays_model_cdf_kmeans(list_rays)
        store('cdf_kmeans', centres=km.cluster_centers_, labels=km.labels_, table=cdist)
        np.random.seed(0)
        km, cdist = ref.transform_rays_model_cdf_kmeans(list_rays, nb_components=2)
        store('cdf_kmeans2', centres=km.cluster_centers_, labels=km.labels_, table=cdist)
    finally:
        ref.compute_cumulative_distrib = original


def main():
    with ReferenceEnv() as env:
        for name in ('int', 'float', 'bool'):
            if not hasattr(np, name):
                setattr(np, name, {'int': int, 'float': float, 'bool': bool}[name])
        if not hasattr(np, 'Inf'):
            np.Inf = np.inf
        import imsegm.region_growing as ref
        import object_shapes_cases as cases
        out = {'versions': env.versions}
        with_hole = 0
        for name in cases.CASES:
            for seed in range(1, 200):
                try:
                    case = run_shapes(ref, cases, name, seed)
                    break
                except Rejected as why:
                    print(name, 'seed', seed, 'rejected:', why)
            else:
                raise SystemExit('no seed of %s meets the conditions' % name)
            with_hole += int((case['rays_raw'] == -1).any())
            print(name, 'seed', seed, 'objects', len(case['labels']), 'centres', case['centres'].tolist())
            out.update({'shapes_%s_%s' % (name, key): np.asarray(value) for key, value in case.items()})
        assert with_hole >= 1, 'no stored object has a ray of -1'
        for table_name, list_rays in (('doctest', cases.DOCTEST_RAYS), ('seeded0', cases.ray_table(0))):
            run_models(ref, table_name, list_rays, out)
        for table_name, list_rays, nb_bins in (('doctest', cases.DOCTEST_RAYS, 5), ('seeded0', cases.ray_table(0), 10),
                                               ('seeded1', cases.ray_table(1), 7)):
            out['histograms_' + table_name] = np.array(ref.transform_rays_model_cdf_histograms(list_rays, nb_bins=nb_bins))
        out['cumulative_doctest'] = ref.compute_cumulative_distrib(np.array([[1, 2]]), np.array([[1.5, 0.5], [0.5, 1]]), np.array([0.5]), 6)
        for seed in (0, 1):
            out['cumulative_seeded%d' % seed] = ref.compute_cumulative_distrib(*cases.cumulative_inputs(seed))
    target = os.path.join(HERE, 'object_shapes.npz')
    np.savez_compressed(target, **out)
    print(target, os.path.getsize(target), 'bytes')
    import inspect
    import json
    names = sorted(n for n, f in inspect.getmembers(ref, inspect.isfunction) if f.__module__ == ref.__name__ and not n.startswith('_'))
    with open(os.path.join(HERE, 'region_growing_names.json'), 'w') as fp:
        json.dump(names, fp, indent=1)
        fp.write('\n')
    print(len(names), 'public functions')


if __name__ == '__main__':
    main()
