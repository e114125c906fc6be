#!/usr/bin/env python
"""Golden vectors of the reference's `experiments_ovary_centres/run_create_annotation.py`, run UNCHANGED under the build container's
conda Python 3.9 with its scipy 1.7.1 and scikit-image 0.18.3 (/opt/conda/bin/python3.9
tests/golden/make_golden_center_annotation.py, through `_reference_env.ReferenceEnv` like the other generators) on the inputs of
tests/center_annotation_cases.py.  Only numbers are stored.

* `load_correct_segm` reads a temporary PNG of every `CORRECT_CASES` input: `<name>_img`, `<name>_seg`, `<name>_seg_lb`.  Its two
  constants -- `disk(25)` and the default `min_size` of `remove_small_objects` -- are the case's `sel_radius` and `min_size`: the
  module's name `morphology` is wrapped for the call, the function itself runs as it is.  Then `segm_set_center_levels` and
  `compute_eggs_center` on its label map: `<name>_levels`, `<name>_centres`.
* `segm_set_center_levels` writes a temporary PNG for every `LEVEL_CASES` / `HOST_ONLY` input, which is read back: `<name>_seg`
  (the input), `<name>_levels`; `compute_eggs_center`: `<name>_centres` (X, Y).
* `sample_*`: the same chain with the reference's constants on a crop of its own `annot_eggs` sample.

pandas 2 has no `DataFrame.append`, which `compute_eggs_center` calls: it is given back for the run, as `np.int` is."""
import os
import sys
import tempfile
import types

import numpy as np

from _reference_env import HERE, REF, ROOT, ReferenceEnv

sys.path.insert(0, os.path.join(ROOT, 'tests'))

SAMPLE = os.path.join(REF, 'data-images', 'drosophila_ovary_slice', 'annot_eggs', 'insitu7545.png')
SAMPLE_CROP = (slice(150, 470), slice(180, 620))


def correct(ref, tmp, img, sel_radius, min_size):
    from skimage import morphology
    path = os.path.join(tmp, 'in.png')
    ref.tl_data.io_imsave(path, img)
    wrapped = types.SimpleNamespace(binary_opening=morphology.binary_opening,
                                    disk=lambda radius: morphology.disk(sel_radius if radius == 25 else radius),
                                    remove_small_objects=lambda ar: morphology.remove_small_objects(ar, min_size=min_size))
    ref.morphology = wrapped
    try:
        seg, seg_lb = ref.load_correct_segm(path)
    finally:
        ref.morphology = morphology
    return seg, seg_lb


def levels_of(ref, tmp, seg, levels):
    ref.segm_set_center_levels('out.png', seg, tmp, levels)
    return np.asarray(ref.tl_data.io_imread(os.path.join(tmp, 'out.png')))


def centres_of(ref, seg):
    table = ref.compute_eggs_center(seg)
    return np.asarray(table[['X', 'Y']], dtype=np.float64) if len(table) else np.zeros((0, 2), dtype=np.float64)


def main():
    with ReferenceEnv() as env, tempfile.TemporaryDirectory() as tmp:
        for alias in ('int', 'float', 'bool'):
            if not hasattr(np, alias):
                setattr(np, alias, {'int': int, 'float': float, 'bool': bool}[alias])
        import pandas as pd
        if not hasattr(pd.DataFrame, 'append'):
            pd.DataFrame.append = lambda self, row, ignore_index=False: pd.concat([self, pd.DataFrame([row])], ignore_index=ignore_index)
        sys.path.insert(0, os.path.join(REF, 'experiments_ovary_centres'))
        import run_create_annotation as ref
        import center_annotation_cases as cases
        import scipy
        out = {'versions': np.array('%s, scipy %s' % (env.versions, scipy.__version__))}
        for name in list(cases.LEVEL_CASES) + list(cases.HOST_ONLY):
            inputs = cases.level_case(name)
            out[name + '_seg'] = inputs['seg']
            out[name + '_levels'] = levels_of(ref, tmp, inputs['seg'], inputs['levels'])
            out[name + '_centres'] = centres_of(ref, inputs['seg'])
            print(name, inputs['seg'].shape, np.bincount(out[name + '_levels'].ravel()).tolist())
        table = {name: cases.correct_case(name) for name in cases.CORRECT_CASES}
        sample = np.asarray(ref.tl_data.io_imread(SAMPLE))
        assert sample.ndim == 2, sample.shape
        table['sample'] = dict(img=np.ascontiguousarray(sample[SAMPLE_CROP]), sel_radius=25, min_size=64)
        for name, inputs in table.items():
            seg, seg_lb = correct(ref, tmp, inputs['img'], inputs['sel_radius'], inputs['min_size'])
            out[name + '_img'], out[name + '_seg'], out[name + '_seg_lb'] = inputs['img'], seg, seg_lb
            out[name + '_levels'] = levels_of(ref, tmp, seg_lb, cases.LEVELS)
            out[name + '_centres'] = centres_of(ref, seg_lb)
            print(name, inputs['img'].shape, seg_lb.dtype, int(seg_lb.max()), np.bincount(out[name + '_levels'].ravel()).tolist())
    target = os.path.join(HERE, 'center_annotation.npz')
    np.savez_compressed(target, **out)
    print(target, os.path.getsize(target), 'bytes')


if __name__ == '__main__':
    main()
