#!/usr/bin/env python
"""Golden vectors of the egg orientation step from the REAL reference: ``correlation_coefficient``, ``condition_swap_correl``,
``condition_swap_density`` and ``compute_mean_image`` of its ``experiments_ovary_detect/run_egg_swap_orientation.py`` are lifted out
of the script with ``ast`` (as tests/golden/make_golden.py lifts) -- the script itself imports drivers and reads files -- and run on
the case stacks of tests/egg_orientation_cases.py.  The loader and ``WrapExecuteSequence`` are stubs that hand the arrays through.
No reference text is held here.

    python tests/golden/make_egg_orientation_golden.py <directory that holds the reference's experiments_ovary_detect/>

Per case, into tests/golden/egg_orientation.npz: ``<name>_crc`` (of the inputs: a drifting case builder is noticed),
``<name>_template`` (float64: the reference's median, or the given template), ``<name>_cc`` / ``<name>_cc_swap`` (float64 [N]: the
two coefficients of every image cropped to the template as ``perform_orientation_swap`` crops it), ``<name>_swap_cc`` and
``<name>_swap_density`` (bool [N]: the decisions of the two conditions).
"""
import ast
import os
import sys
import types
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
NAMES = ('IMAGE_CHANNEL', 'correlation_coefficient', 'condition_swap_correl', 'condition_swap_density', 'compute_mean_image')


def lift(path, names, namespace):
    """exec the named top-level functions / assignments of a reference file inside `namespace`"""
    tree = ast.parse(open(path).read())
    picked = [node for node in tree.body
              if (isinstance(node, ast.FunctionDef) and node.name in names)
              or (isinstance(node, ast.Assign) and any(isinstance(t, ast.Name) and t.id in names for t in node.targets))]
    missing = set(names) - {getattr(n, 'name', None) or n.targets[0].id for n in picked}
    assert not missing, missing
    exec(compile(ast.Module(body=picked, type_ignores=[]), path, 'exec'), namespace)
    return namespace


def main():
    import egg_orientation_cases as cases
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    root = sys.argv[1]
    script = os.path.join(root, 'experiments_ovary_detect', 'run_egg_swap_orientation.py')
    ref = lift(script, NAMES, {
        'np': np,
        'tl_data': types.SimpleNamespace(load_image_2d=lambda img: (img, None)),
        'tl_expt': types.SimpleNamespace(WrapExecuteSequence=lambda func, items, **_: [func(item) for item in items]),
    })
    warnings.filterwarnings('ignore')
    out = {}
    for name in cases.CASES:
        images, template = cases.case(name)
        out[name + '_crc'] = np.array(cases.crc(name), dtype=np.uint32)
        if template is None:
            template = ref['compute_mean_image'](images)
        n = len(images)
        cc, cc_swap = np.zeros(n), np.zeros(n)
        swap_cc, swap_density = np.zeros(n, dtype=bool), np.zeros(n, dtype=bool)
        for i, img in enumerate(images):
            img = img[:template.shape[0], :template.shape[1]]           # (perform_orientation_swap :50-51)
            cc[i] = ref['correlation_coefficient'](img[:, :, ref['IMAGE_CHANNEL']], template)
            cc_swap[i] = ref['correlation_coefficient'](img[::-1, ::-1, ref['IMAGE_CHANNEL']], template)
            swap_cc[i] = ref['condition_swap_correl'](img, template)
            swap_density[i] = ref['condition_swap_density'](img)
            assert swap_cc[i] == (cc[i] < cc_swap[i])
        out[name + '_template'] = np.asarray(template, dtype=np.float64)
        out[name + '_cc'], out[name + '_cc_swap'] = cc, cc_swap
        out[name + '_swap_cc'], out[name + '_swap_density'] = swap_cc, swap_density
        close = np.abs(cc - cc_swap) <= 1e-12
        print('%-22s N %5d template %-9r swaps cc %5d density %5d |cc - cc_swap| <= 1e-12: %d' % (
            name, n, template.shape, swap_cc.sum(), swap_density.sum(), close.sum()))
    np.savez_compressed(os.path.join(HERE, 'egg_orientation.npz'), **out)


if __name__ == '__main__':
    main()
