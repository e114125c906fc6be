#!/usr/bin/env python
"""Golden vectors of the cut-and-scale step (`experiments_ovary_detect/run_ellipse_cut_scale.py` of the reference), made ONCE under
the build container's conda Python 3.9 with scikit-image 0.18.3 and scipy 1.7.1 (/opt/conda/bin/python3.9
tests/golden/make_golden_cut_scale.py) on the generated inputs of tests/cut_scale_cases.py.  The tests never import this file.
Only numbers are stored, plus the CRC of every input.

Per resize case `<name>_crc` (of the input), `<name>_blurred` (what scikit-image's `resize` got back from
`ndi.gaussian_filter`: uint8), `<name>_resized` (`skimage.transform.resize(img, shape)`: float64) and `<name>_exported`
(`(img / float(img.max()) * 255).astype(np.uint8)`, the array half of the reference's `export_image`).

Per full-chain case `<name>_crc` and, per ellipse k, `<name>_resized<k>` and `<name>_exported<k>`: lines 62-72 of
`extract_ellipse_object` with the reference's own `add_overlap_ellipse`, `cut_object`, `transform.resize` and `export_image`
(written as PNG into a temporary folder and read back).

`max_float_diff`: the largest |pyimsegm_amd.ellipse_cut_scale.resize_image_host - skimage| over all cases, which the host test
multiplies by 16 for its bound; `README_cut_scale.md` repeats it."""
import os
import sys
import tempfile
import types
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = '/root/reference'
warnings.filterwarnings('ignore')
sys.path.insert(0, os.path.join(ROOT, 'tests'))

README = """# cut_scale.npz

`make_golden_cut_scale.py` (conda Python 3.9, %(versions)s) stores numbers only, on the generated inputs of
`tests/cut_scale_cases.py` (their CRCs are pinned in the file):

* per resize case what scikit-image's `resize` got back from `ndi.gaussian_filter` (uint8), its result (float64) and the bytes the
  array half of the reference's `export_image` makes of it;
* per full-chain case and ellipse the result of the reference's own `add_overlap_ellipse`, `cut_object`, `transform.resize` and
  `export_image` (lines 62-72 of `extract_ellipse_object`).

The largest |`resize_image_host` - scikit-image| over all cases when the file was made: **%(diff).3e** (`max_float_diff` in the
file).  `tests/test_cut_scale_reference_host.py` allows 16 times that: the margin covers the least-squares scale factors of
`AffineTransform.estimate` on other LAPACK builds, and the bound stays ten orders below one grey level.

Exported bytes: a pixel may differ from the golden by exactly 1 where the golden's own stretched float value lies within 1e-9 of
an integer.  Largest share of such pixels on a re-scaling case when the file was made: %(share).4f %% (allowed: 1 %%).  The same-size
case(s) %(same)s are checked by the float bound and the by-one rule only: every stretched value sits on an integer there and the
reference's own bytes depend on 1e-16 of noise.
"""


def main():
    for alias in ('int', 'float', 'bool'):
        if not hasattr(np, alias):
            setattr(np, alias, {'int': int, 'float': float, 'bool': bool}[alias])
    for name in ('nibabel', 'planar', 'gco', 'OleFileIO_PL'):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules['planar'].line = types.ModuleType('planar.line')
    sys.path.insert(0, REF)
    sys.path.insert(1, ROOT)
    import scipy
    import skimage
    from PIL import Image
    from scipy import ndimage
    from skimage import transform

    import cut_scale_cases as cases
    import imsegm.ellipse_fitting as ell_fit
    import imsegm.utilities.data_io as tl_data
    from pyimsegm_amd import ellipse_cut_scale as ecs

    versions = 'scikit-image %s, scipy %s, numpy %s' % (skimage.__version__, scipy.__version__, np.__version__)
    out = {'versions': np.array(versions)}
    original_filter = ndimage.gaussian_filter
    seen = []

    def gaussian_filter(image, *args, **kwargs):
        result = original_filter(image, *args, **kwargs)
        seen.append(result.copy())
        return result

    worst, share = 0., 0.

    def compare(name, img, shape, resized, exported):
        nonlocal worst, share
        mine = ecs.resize_image_host(img, shape)
        worst = max(worst, float(np.abs(mine - resized).max()))
        differ = ecs.export_image_array(mine) != exported
        if name not in cases.SAME_SIZE_CASES:
            share = max(share, 100. * differ.sum() / differ.size)
        print(name, img.shape, '->', resized.shape, 'float diff %.3e' % np.abs(mine - resized).max(), 'bytes differing', int(differ.sum()),
              'of', differ.size)

    ndimage.gaussian_filter = gaussian_filter
    try:
        for name in cases.RESIZE_CASES:
            img, shape = cases.resize_case(name)
            del seen[:]
            resized = transform.resize(img, shape)
            assert len(seen) == 1 and seen[0].dtype == np.uint8 and seen[0].shape == img.shape
            exported = (resized / float(resized.max()) * 255).astype(np.uint8)
            out.update({name + '_crc': np.int64(cases.crc(img)), name + '_blurred': seen[0], name + '_resized': resized,
                        name + '_exported': exported})
            assert np.array_equal(ecs.blur_image_host(img, shape), seen[0]), name
            compare(name, img, shape, resized, exported)
        with tempfile.TemporaryDirectory() as tmp:
            for name in cases.CHAIN_CASES:
                img, ellipses, norm_size = cases.chain_case(name)
                out[name + '_crc'] = np.int64(cases.crc(img))
                for k, ell in enumerate(ellipses):
                    mask = ell_fit.add_overlap_ellipse(np.zeros(img.shape[:2], dtype=int), list(ell), 1)
                    img_cut = tl_data.cut_object(img, mask, 0, use_mask=True, bg_color=None)
                    img_norm = transform.resize(img_cut, norm_size)
                    path = tl_data.export_image(os.path.join(tmp, '%s_%d' % (name, k)), img_norm)
                    exported = np.array(Image.open(path))
                    assert exported.dtype == np.uint8 and exported.shape == img_norm.shape
                    out['%s_resized%d' % (name, k)] = img_norm
                    out['%s_exported%d' % (name, k)] = exported
                    compare('%s[%d]' % (name, k), img_cut, norm_size, img_norm, exported)
    finally:
        ndimage.gaussian_filter = original_filter
    out['max_float_diff'] = np.float64(worst)
    target = os.path.join(HERE, 'cut_scale.npz')
    np.savez_compressed(target, **out)
    with open(os.path.join(HERE, 'README_cut_scale.md'), 'w') as handle:
        handle.write(README % {'versions': versions, 'diff': worst, 'share': share, 'same': ', '.join(cases.SAME_SIZE_CASES)})
    print(target, os.path.getsize(target), 'bytes; max float diff %.3e; largest share of differing bytes %.4f %%' % (worst, share))


if __name__ == '__main__':
    main()
