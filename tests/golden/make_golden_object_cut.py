#!/usr/bin/env python
"""Golden vectors of the reference's `object_segmentation_graphcut_pixels` and `object_segmentation_graphcut_slic`
(`imsegm/region_growing.py:42-256`), both run UNCHANGED under the build container's conda Python 3.9 with its scikit-image and scipy
(/opt/conda/bin/python3.9 tests/golden/make_golden_object_cut.py, through `_reference_env.ReferenceEnv` like the other generators).

Inputs are the seeded cases of tests/object_cut_cases.py; only numbers are stored, plus the seed.

* THE CUT is answered by this repository's CPU oracle.  `ReferenceEnv` installs its general-graph bridge under the name
  `cut_grid_graph` too, whose signature does not fit; this generator therefore sets `cut_grid_graph` and `cut_general_graph` of the
  imported reference module to bridges of its own, which record their arguments.  The grid bridge hands the oracle the general graph
  pyGCO builds (vertical edges, then horizontal ones).  With `add_neighbours=True` the reference passes edges (0, 0): a self-edge
  adds w * V(l, l) = 0 to every labelling, but pyGCO takes its scaling maximum over all weights before GCO sees an edge -- the
  bridge converts to pyGCO's integers with all weights, drops the self-edges and cuts the integer problem.  What gco itself does
  with a self-edge is not verified here.
* Per case: the recorded float unary costs, weights and pairwise matrix, their pyGCO integers, the returned labels.

Conditions asserted per case (the generator re-seeds until they hold; they concern the reference alone):

* every (u / dwf) * 100000 and (w / dwf) * 1000 is exactly an integer or more than 1e-6 away from one;
* no seed disc leaves the image;
* every label has at least one pixel / superpixel in the result."""
import ctypes as C
import os
import sys

import numpy as np

from _reference_env import HERE, ROOT, ReferenceEnv

sys.path.insert(0, os.path.join(ROOT, 'tests'))


class Rejected(Exception):
    pass


def pygco_integers(unary, weights, pairwise):
    """gco/pygco.py cut_general_graph: down_weight_factor and the truncation of GCO._convert_*"""
    mu, mw, mp = np.max(np.abs(unary)), (np.max(np.abs(weights)) if len(weights) else 0.), np.max(pairwise)
    dwf = (mw * mp if len(weights) and mw * mp > mu else mu) + 1e-10
    for scaled in ((unary / dwf) * 100000, (weights / dwf) * 1000):
        off = np.abs(scaled - np.rint(scaled))
        if np.any((off != 0) & (off <= 1e-6)):
            raise Rejected('a scaled cost next to an integer')
    return ((unary / dwf) * 100000).astype(np.int32), ((weights / dwf) * 1000).astype(np.int32), (pairwise * 100).astype(np.int32), dwf


def make_bridges(recorded):
    lib = C.CDLL(os.path.join(ROOT, 'oracle', 'liboracle.so'))
    lib.orc_alpha_expansion_int.restype = C.c_int64
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731

    def cut(edges, weights, unary, pairwise, n_iter):
        edges = np.ascontiguousarray(edges, dtype=np.int32).reshape(-1, 2)
        weights, unary, pairwise = (np.ascontiguousarray(a, dtype=np.float64) for a in (weights, unary, pairwise))
        ui, wi, si, dwf = pygco_integers(unary, weights, pairwise)
        recorded.update(edges=edges.copy(), weights=weights.copy(), unary=unary.copy(), pairwise=pairwise.copy(), unary_int=ui,
                        weights_int=wi, pairwise_int=si, dwf=dwf)
        keep = edges[:, 0] != edges[:, 1]
        kept, wk = np.ascontiguousarray(edges[keep]), np.ascontiguousarray(wi[keep])
        labels = np.zeros(unary.shape[0], dtype=np.int32)
        recorded['energy'] = lib.orc_alpha_expansion_int(ptr(kept), C.c_int(len(kept)), ptr(wk), ptr(ui), C.c_int(unary.shape[0]),
                                                         C.c_int(unary.shape[1]), ptr(si), C.c_int(n_iter), ptr(labels))
        return labels

    def cut_general_graph(edges, edge_weights, unary_cost, pairwise_cost, n_iter=-1, algorithm='expansion', **kw):
        return cut(edges, edge_weights, unary_cost, pairwise_cost, n_iter)

    def cut_grid_graph(unary_cost, pairwise_cost, cost_v, cost_h, n_iter=-1, algorithm='expansion', **kw):
        height, width, n_labels = unary_cost.shape
        index = np.arange(height * width, dtype=np.int32).reshape(height, width)
        edges = np.concatenate([np.stack([index[:-1].ravel(), index[1:].ravel()], axis=1),
                                np.stack([index[:, :-1].ravel(), index[:, 1:].ravel()], axis=1)], axis=0)
        weights = np.concatenate([np.asarray(cost_v, dtype=np.float64).ravel(), np.asarray(cost_h, dtype=np.float64).ravel()])
        return cut(edges, weights, np.asarray(unary_cost, dtype=np.float64).reshape(height * width, n_labels), pairwise_cost, n_iter)

    return cut_general_graph, cut_grid_graph


def stored(recorded, labels, seed):
    keys = ('edges', 'weights', 'unary', 'pairwise', 'unary_int', 'weights_int', 'pairwise_int', 'dwf', 'energy')
    return dict({key: np.asarray(recorded[key]) for key in keys}, labels=np.asarray(labels), seed=seed)


def run_pixels(ref, cases, recorded, name, seed):
    segm, centres, kwargs = cases.pixel_case(name, seed)
    size = kwargs.get('seed_size', 0)
    for r, c in centres:
        if r - size < 0 or c - size < 0 or r + size >= segm.shape[0] or c + size >= segm.shape[1]:
            raise Rejected('a seed disc leaves the image')
    labels = ref.object_segmentation_graphcut_pixels(segm, centres, **kwargs)
    if set(np.unique(labels)) != set(range(len(centres) + 1)):
        raise Rejected('a label without a pixel')
    return stored(recorded, labels, seed)


def run_slic(ref, cases, recorded, name, seed):
    slic, segm, centres = cases.slic_case(seed)
    labels = ref.object_segmentation_graphcut_slic(slic, segm, centres, labels_fg_prob=cases.LABELS_FG_PROB, **cases.SLIC_CASES[name])
    if set(np.unique(labels)) != set(range(len(centres) + 1)):
        raise Rejected('a label without a superpixel')
    return stored(recorded, labels, seed)


def main():
    with ReferenceEnv() as env:
        for name in ('int', 'float', 'bool'):
            if not hasattr(np, name):
                setattr(np, name, {'int': int, 'float': float, 'bool': bool}[name])
        import imsegm.region_growing as ref
        import object_cut_cases as cases
        recorded = {}
        ref.cut_general_graph, ref.cut_grid_graph = make_bridges(recorded)
        out = {'versions': env.versions}
        for kind, names, run in (('pixels', cases.PIXEL_CASES, run_pixels), ('slic', cases.SLIC_CASES, run_slic)):
            for name in names:
                for seed in range(1, 200):
                    try:
                        case = run(ref, cases, recorded, name, seed)
                        break
                    except Rejected as why:
                        print(kind, name, 'seed', seed, 'rejected:', why)
                else:
                    raise SystemExit('no seed of %s %s meets the conditions' % (kind, name))
                print(kind, name, 'seed', seed, 'sites', len(case['labels'].ravel()), 'energy', int(case['energy']),
                      'labels', np.bincount(case['labels'].ravel()).tolist()[:8])
                out.update({'%s_%s_%s' % (kind, name, key): value for key, value in case.items()})
    target = os.path.join(HERE, 'object_cut.npz')
    np.savez_compressed(target, **out)
    print(target, os.path.getsize(target), 'bytes')


if __name__ == '__main__':
    main()
