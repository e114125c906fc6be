"""Writes tests/golden/forest_proba.npz: for the fits ``forest_cases.GOLDEN`` the packed forest (``_hip.DeviceForest``), the table and
``model.predict_proba(table)`` of scikit-learn with ``n_jobs=1`` -- so that the GPU tests compare with scikit-learn's bytes without
a fit, whatever scikit-learn is installed where they run.  scikit-learn only; run from the repository root:

    python tests/golden/make_golden_forest.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))]

PARTS = ('threshold', 'word', 'tree_start', 'leaf_values', 'scaler_mean', 'scaler_scale', 'classes', 'table', 'expected')


def main():
    import sklearn

    import forest_cases as FC
    from pyimsegm_amd import _hip
    out = {'sklearn_version': np.array(sklearn.__version__)}
    for name in FC.GOLDEN:
        case = FC.fit_by_name(name)
        model, table = FC.fit_model(case), FC.fit_table(case)
        packed = _hip.DeviceForest(model)
        empty = np.zeros(0)
        parts = (packed.nodes['threshold'], packed.nodes['word'], packed.tree_start, packed.leaf_values,
                 empty if packed.scaler_mean is None else packed.scaler_mean,
                 empty if packed.scaler_scale is None else packed.scaler_scale, packed.classes, table, model.predict_proba(table))
        out.update({'%s/%s' % (name, part): value for part, value in zip(PARTS, parts)})
    np.savez_compressed(os.path.join(HERE, 'forest_proba.npz'), **out)


if __name__ == '__main__':
    main()
