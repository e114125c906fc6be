#!/usr/bin/env python
"""Golden results of the reference's scoring functions (`imsegm/classification.py:305-471, 635-655, 1265-1366`), run UNCHANGED with
the installed Python, numpy and scikit-learn (python tests/golden/make_golden_scoring.py).  The reference is found through
`_reference_env.py` (its `REF`); `classification.py` and `labeling.py` are loaded from their paths.  What they import from the rest of
the package and cannot be loaded here comes from stand-in modules made here: `imsegm.utilities` (`ImageDimensionError`),
`imsegm.utilities.data_io` (`get_image2d_boundary_color`, never called), `imsegm.utilities.experiments` (`WrapExecuteSequence` as a
plain loop, `get_nb_workers`), and `scipy.interp`, which scipy has dropped, is numpy's.  Only numbers and names are stored:

* `scoring.json`: what `compute_classif_stat_segm_annot` returns with `relabel` off and on for the `GOLDEN` cases of
  tests/scoring_cases.py, `compute_classif_metrics` with all four averages, `compute_tp_tn_fp_fn` and the two ratios, and the values of
  the module's doctests;
* `scoring_names.json`: the eight names this project defines, with the signatures of the functions.
"""
import importlib.util
import inspect
import json
import os
import sys
import types
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from _reference_env import REF  # noqa: E402

NAMES = ('METRIC_AVERAGES', 'relabel_sequential', 'compute_classif_metrics', 'compute_classif_stat_segm_annot', 'compute_stat_per_image',
         'compute_tp_tn_fp_fn', 'compute_metric_fpfn_tpfn', 'compute_metric_tpfp_tpfn')


def load(name):
    spec = importlib.util.spec_from_file_location('imsegm.' + name, os.path.join(REF, 'imsegm', name + '.py'))
    module = importlib.util.module_from_spec(spec)
    sys.modules['imsegm.' + name] = module
    spec.loader.exec_module(module)
    return module


def load_reference():
    import scipy

    class ImageDimensionError(TypeError):
        pass

    def sequence(function, iterable, nb_workers=1, desc=''):
        return (function(item) for item in iterable)

    package, utilities = types.ModuleType('imsegm'), types.ModuleType('imsegm.utilities')
    data_io, experiments = types.ModuleType('imsegm.utilities.data_io'), types.ModuleType('imsegm.utilities.experiments')
    package.__path__, utilities.__path__ = [], []
    utilities.ImageDimensionError = ImageDimensionError
    data_io.get_image2d_boundary_color = None
    experiments.WrapExecuteSequence, experiments.get_nb_workers = sequence, lambda ratio: 1
    sys.modules.update({'imsegm': package, 'imsegm.utilities': utilities, 'imsegm.utilities.data_io': data_io,
                        'imsegm.utilities.experiments': experiments})
    if not hasattr(scipy, 'interp'):
        scipy.interp = np.interp
    try:
        import skimage.segmentation  # noqa: F401
    except ImportError:               # (labeling.py imports it for functions that are not called here)
        sys.modules.update({'skimage': types.ModuleType('skimage'), 'skimage.segmentation': types.ModuleType('skimage.segmentation')})
    load('labeling')
    return load('classification')


def plain(value):
    """results as JSON: numpy scalars as Python numbers, NaN as the string 'nan'"""
    if isinstance(value, dict):
        return {key: plain(item) for key, item in value.items()}
    if isinstance(value, (list, tuple)):
        return [plain(item) for item in value]
    if isinstance(value, np.generic):
        value = value.item()
    if isinstance(value, float) and value != value:
        return 'nan'
    return value


def attempt(call):
    try:
        return plain(call())
    except Exception as ex:
        return {'raises': type(ex).__name__}


def main():
    import sklearn
    import scoring_cases as cases
    warnings.filterwarnings('ignore')
    ref = load_reference()
    out = {'versions': 'numpy %s, scikit-learn %s, Python %s' % (np.__version__, sklearn.__version__, sys.version.split()[0]), 'cases': {}}
    for name in cases.GOLDEN:
        annot, segm, drop = cases.CASES[name]
        y_true, y_pred = cases.kept(annot, segm, drop)
        out['cases'][name] = {
            'stat': attempt(lambda: ref.compute_classif_stat_segm_annot((annot, segm, name), drop_labels=drop, relabel=False)),
            'stat_relabel': attempt(lambda: ref.compute_classif_stat_segm_annot((annot, segm, name), drop_labels=drop, relabel=True)),
            'metrics': attempt(lambda: ref.compute_classif_metrics(y_true, y_pred, metric_averages=cases.AVERAGES)),
            'tp_tn_fp_fn': attempt(lambda: ref.compute_tp_tn_fp_fn(y_true, y_pred)),
            'fpfn_tpfn': attempt(lambda: ref.compute_metric_fpfn_tpfn(y_true, y_pred)),
            'tpfp_tpfn': attempt(lambda: ref.compute_metric_tpfp_tpfn(y_true, y_pred)),
        }
    # the doctests of the module (:313-328, :382-397, :436-458, :642-643, :1273-1289, :1321-1329, :1348-1358)
    doc = out['doctests'] = {}
    np.random.seed(0)
    y_true, y_pred = np.random.randint(0, 3, 25) * 2, np.random.randint(0, 2, 25) * 2
    doc['metrics_same'] = plain(ref.compute_classif_metrics(y_true, y_true))
    doc['metrics'] = plain(ref.compute_classif_metrics(y_true, y_pred))
    doc['metrics_pred'] = plain(ref.compute_classif_metrics(y_pred, y_pred))
    np.random.seed(0)
    annot, segm = np.random.randint(0, 2, (5, 10)), np.random.randint(0, 2, (5, 10))
    doc['stat_same'] = plain(ref.compute_classif_stat_segm_annot((annot, annot, 'ttt'), relabel=True, drop_labels=[5]))
    doc['stat'] = plain(ref.compute_classif_stat_segm_annot((annot, segm, 'ttt'), relabel=True, drop_labels=[5]))
    doc['stat_shifted'] = plain(ref.compute_classif_stat_segm_annot((annot, segm + 1, 'ttt'), relabel=False, drop_labels=[0]))
    np.random.seed(0)
    img_true, img_pred = np.random.randint(0, 3, (50, 100)), np.random.randint(0, 2, (50, 100))
    doc['per_image_same'] = plain(ref.compute_stat_per_image([img_true], [img_true], nb_workers=2, relabel=True).iloc[0].to_dict())
    doc['per_image'] = plain(ref.compute_stat_per_image([img_true], [img_pred], drop_labels=[-1]).iloc[0].to_dict())
    doc['relabel_sequential'] = plain(ref.relabel_sequential([0, 0, 0, 5, 5, 5, 0, 5]))
    np.random.seed(0)
    annot, segm = np.random.randint(0, 2, (5, 7)) * 9, np.random.randint(0, 2, (5, 7)) * 9
    doc['cells_same'] = plain(ref.compute_tp_tn_fp_fn(annot, annot))
    doc['cells'] = plain(ref.compute_tp_tn_fp_fn(annot, segm))
    doc['cells_ones'] = plain(ref.compute_tp_tn_fp_fn(annot, np.ones((5, 7))))
    doc['cells_zeros'] = plain(ref.compute_tp_tn_fp_fn(np.zeros((5, 7)), np.zeros((5, 7))))
    np.random.seed(0)
    annot, segm = np.random.randint(0, 2, (50, 75)) * 3, np.random.randint(0, 2, (50, 75)) * 3
    doc['fpfn_tpfn'] = [plain(ref.compute_metric_fpfn_tpfn(annot, other)) for other in (segm, annot, np.ones((50, 75)))]
    doc['tpfp_tpfn'] = [plain(ref.compute_metric_tpfp_tpfn(annot, other)) for other in (segm, annot, np.ones((50, 75)), np.zeros((50, 75)))]
    with open(os.path.join(HERE, 'scoring.json'), 'w') as fp:
        json.dump(out, fp, indent=1)
        fp.write('\n')
    names = {'constants': {'METRIC_AVERAGES': list(ref.METRIC_AVERAGES)}, 'functions': {}}
    for name in NAMES[1:]:
        parameters = inspect.signature(getattr(ref, name)).parameters
        names['functions'][name] = [[key, None if p.default is inspect.Parameter.empty else plain(p.default)] for key, p in parameters.items()]
    with open(os.path.join(HERE, 'scoring_names.json'), 'w') as fp:
        json.dump(names, fp, indent=1)
        fp.write('\n')
    print(os.path.getsize(os.path.join(HERE, 'scoring.json')), 'bytes;', len(out['cases']), 'cases')


if __name__ == '__main__':
    main()
