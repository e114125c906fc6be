#!/usr/bin/env python
"""Golden vectors of the reference's `imsegm/annotation.py`, run UNCHANGED with the installed Python and numpy 2.x
(python tests/golden/make_golden_annotation.py).  Only that one file of the reference is loaded, from its path: the two names it imports
from `imsegm.utilities` (`ImageDimensionError`, `io_imread`) come from stand-in modules made here, and the two numpy aliases it uses
that numpy has dropped are set here (`np.int = int`, `np.product = np.prod`).  Only numbers and names are stored:

* `annotation.npz`: the results of every pixel function on the seeded inputs of tests/annotation_cases.py, the names of the
  exceptions the reference raises, and the values of its doctests;
* `annotation_names.json`: the public functions and constants of the module.
"""
import importlib.util
import inspect
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get('IMSEGM_REFERENCE', '/root/reference')
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def load_reference():
    class ImageDimensionError(TypeError):
        pass

    def io_imread(path):
        from PIL import Image
        return np.asarray(Image.open(path))

    package, utilities, data_io = types.ModuleType('imsegm'), types.ModuleType('imsegm.utilities'), types.ModuleType('imsegm.utilities.data_io')
    package.__path__, utilities.__path__ = [], []
    utilities.ImageDimensionError, data_io.io_imread = ImageDimensionError, io_imread
    sys.modules.update({'imsegm': package, 'imsegm.utilities': utilities, 'imsegm.utilities.data_io': data_io})
    np.int, np.product = int, np.prod
    spec = importlib.util.spec_from_file_location('imsegm.annotation', os.path.join(REF, 'imsegm', 'annotation.py'))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


def raised(call):
    try:
        call()
    except Exception as ex:
        return np.array(type(ex).__name__)
    return np.array('')


def frequent(ref, img, threshold):
    found = ref.image_frequent_colors(img, threshold)
    return np.array(list(found.keys()), dtype=np.int64).reshape(-1, 3), np.array(list(found.values()), dtype=np.int64)


def main():
    import scipy
    import PIL
    import annotation_cases as cases
    ref = load_reference()
    out = {'versions': np.array('numpy %s, scipy %s, Pillow %s, Python %s' % (np.__version__, scipy.__version__, PIL.__version__,
                                                                            sys.version.split()[0]))}
    for name in cases.PAINTED:
        image, colors, segm, kept = cases.painted(name)
        out[name + '_color_2_labels'] = ref.image_color_2_labels(image, colors)
        out[name + '_color_2_labels_default'] = ref.image_color_2_labels(image)
        out[name + '_default_colors'] = np.array(list(ref.image_frequent_colors(image).keys()), dtype=np.int64).reshape(-1, 3)
        out[name + '_nearest_color'] = ref.quantize_image_nearest_color(image, colors)
        out[name + '_nearest_pixel'] = ref.quantize_image_nearest_pixel(image, colors)
        out[name + '_unique_sorted'] = np.array(sorted(ref.unique_image_colors(image)), dtype=np.int64)
        out[name + '_frequent_keys'], out[name + '_frequent_counts'] = frequent(ref, image, 1e-3)
        # a threshold that sits exactly at the count of one colour: n * (count / n) >= count has to keep it
        counts = np.sort(out[name + '_frequent_counts'])
        at = float(counts[len(counts) // 2]) / float(image.shape[0] * image.shape[1])
        out[name + '_frequent_at'] = np.array(at)
        out[name + '_frequent_at_keys'], out[name + '_frequent_at_counts'] = frequent(ref, image, at)
        out[name + '_reverted_error'] = raised(lambda: ref.convert_img_colors_to_labels_reverted(image, {c: i for i, c in enumerate(colors)}))
        labels = np.where(kept, segm, np.nan)
        out[name + '_inpaint'] = ref.image_inpaint_pixels(labels, kept)
        share = float(cases.ambiguous_mask(segm, kept).mean())
        assert share <= cases.AMBIGUOUS_CAP, (name, share)
        print(name, image.shape, 'ambiguous share %.3f' % share, 'colours', len(out[name + '_unique_sorted']))
        clean, lut, segm = cases.clean(name)
        out[name + '_to_labels'] = ref.convert_img_colors_to_labels(clean, lut)
        out[name + '_to_labels_reverted'] = ref.convert_img_colors_to_labels_reverted(clean, {c: i + 5 for i, c in enumerate(colors)})
        out[name + '_to_colors'] = ref.convert_img_labels_to_colors(segm, lut)
        shifted, shifted_lut = cases.shifted_labels(name)
        out[name + '_to_colors_shifted'] = ref.convert_img_labels_to_colors(shifted, shifted_lut)
        out[name + '_to_colors_error'] = raised(lambda: ref.convert_img_labels_to_colors(segm, {k: v for k, v in lut.items() if k != 1}))
    # what the reference does with an image that has none of the colours, and with a shape mismatch
    none_of_them = np.full((4, 5, 3), 7, dtype=np.uint8)
    out['all_invalid_error'] = raised(lambda: ref.quantize_image_nearest_pixel(none_of_them, [(0, 0, 0), (1, 1, 1)]))
    out['inpaint_shape_error'] = raised(lambda: ref.image_inpaint_pixels(np.zeros((3, 4)), np.ones((4, 3), dtype=bool)))
    # the doctests of the module (annotation.py:52-56, :79-88, :135-144, :171-178, :233-241, :259-267, :296-304)
    np.random.seed(0)
    out['doctest_unique_sorted'] = np.array(sorted(ref.unique_image_colors(np.random.randint(0, 2, (50, 50, 3)))), dtype=np.int64)
    np.random.seed(0)
    seg = np.random.randint(0, 2, (5, 7))
    img = np.array([(0.2, 0.2, 0.2), (0.9, 0.9, 0.9)])[seg]
    out['doctest_to_labels'] = ref.convert_img_colors_to_labels(img, {0: (0.2, 0.2, 0.2), 1: (0.9, 0.9, 0.9)})
    out['doctest_to_labels_reverted'] = ref.convert_img_colors_to_labels_reverted(img, {(0.2, 0.2, 0.2): 0, (0.9, 0.9, 0.9): 1})
    out['doctest_to_colors'] = ref.convert_img_labels_to_colors(seg, {0: (0.2, 0.2, 0.2), 1: (0.9, 0.9, 0.9)})
    np.random.seed(0)
    out['doctest_frequent_keys'], out['doctest_frequent_counts'] = frequent(ref, np.random.randint(0, 2, (50, 50, 3)).astype(np.uint8), 1e-3)
    np.random.seed(0)
    rand = np.random.randint(0, 2, (5, 7)).astype(np.uint8)
    gray = np.rollaxis(np.array([rand] * 3), 0, 3)
    out['doctest_color_2_labels'] = ref.image_color_2_labels(gray)
    out['doctest_color_2_labels_colors'] = np.array(list(ref.image_frequent_colors(gray).keys()), dtype=np.int64).reshape(-1, 3)
    np.random.seed(0)
    img = np.random.randint(0, 2, (5, 7, 3)).astype(np.uint8)
    out['doctest_nearest_color'] = ref.quantize_image_nearest_color(img, [(0, 0, 0), (1, 1, 1)])
    out['doctest_nearest_pixel'] = ref.quantize_image_nearest_pixel(img, [(0, 0, 0), (1, 1, 1)])
    target = os.path.join(HERE, 'annotation.npz')
    np.savez_compressed(target, **out)
    print(target, os.path.getsize(target), 'bytes')
    functions = sorted(n for n, f in inspect.getmembers(ref, inspect.isfunction) if f.__module__ == ref.__name__ and not n.startswith('_'))
    constants = sorted(n for n in vars(ref) if n.isupper() and not n.startswith('_'))
    with open(os.path.join(HERE, 'annotation_names.json'), 'w') as fp:
        json.dump({'functions': functions, 'constants': constants}, fp, indent=1)
        fp.write('\n')
    print(len(functions), 'public functions,', len(constants), 'constants; errors:',
          {k: str(v) for k, v in out.items() if k.endswith('_error')})


if __name__ == '__main__':
    main()
