#!/usr/bin/env python
"""Golden vectors of the reference's `imsegm/region_growing.py` -- `compute_shape_prior_table_cdf` (with its `interp2d`) on a grid
of (point, centre, shift, table), and three whole growths each of the UNCHANGED `region_growing_shape_slic_greedy` and
`region_growing_shape_slic_graphcut` with their `debug_history` -- from a run of the reference module under the build container's
conda Python 3.9 with its scipy (which still has `interp2d`) and scikit-learn (build container: /opt/conda/bin/python3.9
tests/golden/make_golden_region_growing.py, through `_reference_env.ReferenceEnv` like the other generators).

Inputs are the seeded cases of tests/region_growing_cases.py; only numbers are stored, plus the seed and the CRC32 of the inputs.

* `shape_prior`: the reference's value per grid entry, next to it the bilinear value in long double.  `shape_prior_tol` = 10 x
  max |reference - long double| (floor 1e-12); the generator asserts that it is below 1e-9 -- the pin that `interp2d` on a
  2 x 2 cell is bilinear.
* `greedy_<case>_*`, `graphcut_<case>_*` for the cases of `GROWTH_CASES`: labels, criteria, centres and shifts of every iteration,
  `lut_data_cost`, the first and the last `lut_shape_cost`, the returned labels.  For the 'set_cdfs' case also, per call of
  `compute_segm_object_shape` (every object in every cost update, in call order): the rounded centre of mass, the raw 'down' rays
  and the rays it returned (interpolated where a ray left the image, then shifted); and the arrays of the fitted two-component
  `GaussianMixture`.
* THE CUT of the graph-cut cases is answered by this repository's CPU oracle (`orc_cut_general_graph`) through `ReferenceEnv`'s
  bridge: `ReferenceEnv` puts the bridge in the place of the `gco` module.  Everything around the cut is the reference's.  The only
  vectors from the real gco are the criteria and label maps the reference's docstrings print (tests/doctests/region_growing.py).

Conditions asserted per case, so that a test cannot hide a failure (the generator re-seeds until they hold; they concern the
reference alone):

* no `angle_norm` evaluated in the `dist >= D - 1` branch lies within 1e-6 of a half-integer; no in-range `angle_norm` or `dist`
  lies within 1e-9 of an integer unless it is exactly one (every call of `compute_shape_prior_table_cdf` a growth makes);
* in every greedy iteration the best change against 0, each `(best - score) / best` against `greedy_tol` and each `score` against 0
  is exactly at its limit or more than 1e-6 relative away (changes against 0: relative to the criterion they
  are differences of); two accepted changes of the same superpixel, whose order in the sort decides the label, are equal or differ by more than 1e-9 relative;
* every threshold test on centre, shift and volume has a margin of 1e-6 (centre and shift compare integers unless the
  `centre_init` clamp acts, which is asserted not to), no `rad2deg(theta)` lies within 1e-6 of a rounding tie, and no
  centre coordinate does unless it is a tie exactly (the mean of an even number of integer points is k + 0.5 in every arithmetic,
  and `np.round` then takes the even neighbour: a growth of two superpixels cannot avoid it);
* no raw ray of the stored 'set_cdfs' objects is -1, in both growths that have such a model (the greedy and the graph-cut one)."""
import os
import sys

import numpy as np

from _reference_env import HERE, ROOT, ReferenceEnv

sys.path.insert(0, os.path.join(ROOT, 'tests'))
LD = np.longdouble


class Rejected(Exception):
    pass


def off_tie(value, tie_at_half):
    """distance of value from the nearest integer (or half-integer)"""
    frac = value - np.floor(value)
    return abs(frac - 0.5) if tie_at_half else min(frac, 1 - frac)


def check_prior_margins(point, table_shape, centre, shift):
    nb_angles, nb_dists = table_shape
    dx, dy = point[0] - centre[0], point[1] - centre[1]
    dist = np.sqrt(dx**2 + dy**2)
    angle_norm = (((2 * 360) + 90 - np.rad2deg(np.arctan2(dy, dx)) - shift) % 360) / (360. / nb_angles)
    if dist >= nb_dists - 1:
        if off_tie(angle_norm, True) <= 1e-6:
            raise Rejected('an angle at a half-integer in the far branch')
        return
    for value in (angle_norm, dist):
        if value != np.floor(value) and off_tie(value, False) <= 1e-9:
            raise Rejected('an angle or a distance next to an integer')
    if dist != nb_dists - 1 and abs(dist - (nb_dists - 1)) <= 1e-9:
        raise Rejected('a distance next to D - 1')


def shape_prior_fixture(ref, C, out):
    values, wide, rows = [], [], 0
    for points, centre, shift, table in C.shape_prior_grid():
        for point in points:
            check_prior_margins(point, table.shape, centre, shift)           # (the grid is fixed: a rejection here is an error)
            values.append(float(ref.compute_shape_prior_table_cdf(point, table, centre, shift)))
        wide.append(C.shape_prior_longdouble(points, table, centre, shift))
        rows += len(points)
    values, wide = np.array(values), np.concatenate(wide)
    spread = float(np.max(np.abs(values.astype(LD) - wide)))
    tol = max(10 * spread, 1e-12)
    assert tol < 1e-9, ('interp2d on a 2 x 2 cell is not bilinear', spread)
    print('shape prior:', rows, 'values, max |reference - long double|', spread, 'tol', tol)
    out.update(shape_prior=values, shape_prior_longdouble=wide.astype(np.float64), shape_prior_tol=tol)


class Recorder(object):
    """wraps the functions of the reference module a growth calls, records what the conditions and the fixture need, and puts the
    originals back"""
    NAMES = ('compute_shape_prior_table_cdf', 'compute_rg_crit', 'enforce_center_labels', 'compute_centre_moment_points',
             'compute_segm_object_shape', 'compute_ray_features_segm_2d', 'update_shape_costs_points')

    def __init__(self, ref):
        self.ref, self.originals = ref, {name: getattr(ref, name) for name in self.NAMES}
        self.crits, self.shapes, self.raw = [], [], None

    def __enter__(self):
        ref, orig = self.ref, self.originals

        def prior(point, cum_distribution, centre, angle_shift=0):
            check_prior_margins(point, np.shape(cum_distribution), centre, angle_shift)
            return orig['compute_shape_prior_table_cdf'](point, cum_distribution, centre, angle_shift)

        def crit(*args):
            value = orig['compute_rg_crit'](*args)
            self.crits[-1].append(value)
            return value

        def enforce(*args):
            self.crits.append([])                                            # an iteration begins
            return orig['enforce_center_labels'](*args)

        def moment(points):
            points = np.asarray(points)
            mean = np.mean(points, axis=0)
            if any(c * 2 != np.floor(c * 2) and off_tie(c, True) <= 1e-6 for c in mean):
                raise Rejected('a centre coordinate at a rounding tie')
            if len(points) > 1:
                evals, evecs = np.linalg.eig(np.cov((points - mean).T))
                evec = evecs[:, np.argmax(evals)]
                if off_tie(np.rad2deg(np.arctan2(evec[0], evec[1])), True) <= 1e-6:
                    raise Rejected('an orientation at a rounding tie')
            return orig['compute_centre_moment_points'](points)

        def rays_2d(*args, **kwargs):
            self.raw = np.array(orig['compute_ray_features_segm_2d'](*args, **kwargs), dtype=np.float64)
            return self.raw.copy()

        def object_shape(img_object, *args, **kwargs):
            from scipy import ndimage
            centre = [int(round(c)) for c in ndimage.center_of_mass(img_object)]
            rays, shift = orig['compute_segm_object_shape'](img_object, *args, **kwargs)
            self.shapes.append((centre, self.raw.copy(), np.array(rays, dtype=np.float64)))
            return rays, shift

        def update(lut_shape_cost, slic, points, labels, init_centres, centres, shifts, volumes, shape_model, shape_type,
                   selected_idx=None, swap_shift=False, dict_thresholds=None):
            for i in range(len(init_centres)):
                if shape_type == 'set_cdfs' and volumes[i] != 0:
                    diff = np.abs(np.sum(labels == i + 1) - volumes[i]) / float(volumes[i])
                    if abs(diff - dict_thresholds['volume']) <= 1e-6:
                        raise Rejected('a volume change at its threshold')
                mean = np.mean(points[labels == i + 1], axis=0)
                if np.sum((np.round(mean) - init_centres[i])**2) > dict_thresholds['centre_init']**2:
                    raise Rejected('the centre_init clamp acts: centres are no integers')
            return orig['update_shape_costs_points'](lut_shape_cost, slic, points, labels, init_centres, centres, shifts, volumes,
                                                     shape_model, shape_type, selected_idx, swap_shift, dict_thresholds)

        wrapped = dict(zip(self.NAMES, (prior, crit, enforce, moment, object_shape, rays_2d, update)))
        for name in self.NAMES:
            setattr(ref, name, wrapped[name])
        return self

    def __exit__(self, *exc):
        for name in self.NAMES:
            setattr(self.ref, name, self.originals[name])
        return False


def away(value, limit, rel):
    return value == limit or abs(value - limit) > rel * max(abs(value), abs(limit), 1e-300)


def check_greedy_margins(ref, rec, history, slic, greedy_tol):
    """the decisions of every greedy iteration from the criteria the reference computed: [recorded, current, one per candidate]"""
    _, edges = ref.make_graph_segm_connect_grid2d_conn4(slic)
    neighbours = ref.get_neighboring_segments(edges)
    for it, crits in enumerate(rec.crits):
        labels = history['labels'][it]
        superpixels = []
        for i in range(history['centres'][0].shape[0]):
            superpixels += ref.get_neighboring_candidates(neighbours, labels, i + 1, True)
        assert len(crits) == 2 + len(superpixels), (it, len(crits), len(superpixels))
        changes = crits[1] - np.array(crits[2:])
        if not len(changes):
            continue
        best = changes.max()
        scale = abs(crits[1])                                                # (changes are differences of sums of this size)
        if best != 0 and abs(best) <= 1e-6 * scale:
            raise Rejected('the best change next to 0')
        ratio = (best - changes) / best
        if np.any((ratio != greedy_tol) & (np.abs(ratio - greedy_tol) <= 1e-6 * greedy_tol)):
            raise Rejected('a change next to the greedy tolerance')
        if np.any((changes != 0) & (np.abs(changes) <= 1e-6 * scale)):
            raise Rejected('a score next to 0')
        accepted = (ratio < greedy_tol) & (changes > 0)
        for s in set(np.asarray(superpixels)[accepted].tolist()):
            vals = changes[accepted & (np.asarray(superpixels) == s)]
            for a in range(len(vals)):
                for b in range(a + 1, len(vals)):
                    if not away(vals[a], vals[b], 1e-9):
                        raise Rejected('two accepted changes of a superpixel next to a tie')


def run_growth(ref, C, method, name, seed, model):
    slic, prob, centres, shape_model, shape_type = C.growth_case(name, seed, model)
    history, kw = {}, C.GROWTH_KW[method]
    with Recorder(ref) as rec:
        if method == 'greedy':
            returned = ref.region_growing_shape_slic_greedy(slic, prob, centres, shape_model, shape_type, debug_history=history, **kw)
        else:
            returned = ref.region_growing_shape_slic_graphcut(slic, prob, centres, shape_model, shape_type, debug_history=history, **kw)
    if len(history['labels']) < 3 or len(history['labels']) >= kw['nb_iter']:
        raise Rejected('fewer than three iterations, or no convergence')
    if set(np.unique(returned)) != set(range(len(centres) + 1)):
        raise Rejected('an object vanished')
    if method == 'greedy':
        check_greedy_margins(ref, rec, history, slic, kw['greedy_tol'])
    case = {'seed': seed, 'crc': C.input_crc(slic, prob, centres, shape_model), 'labels': np.array(history['labels']),
            'criteria': np.array(history['criteria'], dtype=np.float64), 'centres': np.array(history['centres'], dtype=np.float64),
            'shifts': np.array(history['shifts'], dtype=np.float64), 'lut_data_cost': history['lut_data_cost'],
            'lut_shape_first': history['lut_shape_cost'][0], 'lut_shape_last': history['lut_shape_cost'][-1],
            'returned': np.asarray(returned)}
    if shape_type == 'set_cdfs':
        case.update(mass_centres=np.array([s[0] for s in rec.shapes]), rays_raw=np.array([s[1] for s in rec.shapes]),
                    rays=np.array([s[2] for s in rec.shapes]))
        weights = model.predict_proba(case['rays'])
        mine = C.ArrayMixture(model.weights_, model.means_, model.precisions_cholesky_).predict_proba(case['rays'])
        assert np.max(np.abs(weights - mine)) <= 1e-12, 'the mixture from its arrays differs from scikit-learn'
    print(method, name, 'seed', seed, 'iterations', len(history['labels']), 'criteria', np.round(case['criteria'][[0, -1]], 3),
          'objects', np.bincount(returned).tolist())
    return case


def mixture_model(means, seed=0):
    """a fitted two-component ``GaussianMixture`` around the given ray vectors"""
    from sklearn import mixture
    rng = np.random.RandomState(seed)
    means = np.asarray(means, dtype=np.float64)
    samples = np.vstack([m + rng.randn(40, means.shape[1]) for m in means])
    return mixture.GaussianMixture(len(means), random_state=0, means_init=means).fit(samples)


def main():
    with ReferenceEnv() as env:
        for name in ('int', 'float', 'bool'):
            if not hasattr(np, name):
                setattr(np, name, {'int': int, 'float': float, 'bool': bool}[name])
        if not hasattr(np, 'Inf'):
            np.Inf = np.inf
        import imsegm.region_growing as ref
        import region_growing_cases as C
        segments = ref.get_neighboring_segments
        # (the reference indexes np.array(list of lists): ragged arrays need dtype=object in this numpy)
        ref.get_neighboring_segments = lambda edges: (lambda near: np.array(near + [None], dtype=object)[:-1])(list(segments(edges)))
        out = {'versions': env.versions}
        shape_prior_fixture(ref, C, out)
        model = mixture_model(C.MIXTURE_MEANS)
        out.update(gmm_weights=model.weights_, gmm_means=model.means_, gmm_precisions_cholesky=model.precisions_cholesky_)
        clean_rays = 0
        for method in ('greedy', 'graphcut'):
            for name in C.GROWTH_CASES:
                for seed in range(11, 60):
                    try:
                        case = run_growth(ref, C, method, name, seed, model)
                        break
                    except Rejected as why:
                        print(method, name, 'seed', seed, 'rejected:', why)
                else:
                    raise SystemExit('no seed of %s %s meets the conditions' % (method, name))
                if 'rays_raw' in case:
                    clean_rays += int((case['rays_raw'] != -1).all())
                out.update({'%s_%s_%s' % (method, name, key): np.asarray(value) for key, value in case.items()})
        assert clean_rays >= 2, 'a stored set_cdfs growth has a ray that left the image'
    target = os.path.join(HERE, 'region_growing.npz')
    np.savez_compressed(target, **out)
    print(target, os.path.getsize(target), 'bytes')


if __name__ == '__main__':
    main()
