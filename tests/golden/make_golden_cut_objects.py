#!/usr/bin/env python
"""Golden vectors of the reference's `cut_object` (`imsegm/utilities/data_io.py:1060-1128`), run UNCHANGED under the build
container's conda Python 3.9 with its scipy 1.7.1 and scikit-image 0.18.3 (/opt/conda/bin/python3.9
tests/golden/make_golden_cut_objects.py, through `_reference_env.ReferenceEnv` like the other generators) on the seeded inputs of
tests/cut_objects_cases.py.  Only numbers are stored, plus the seeds.

Per case `<name>_seed` and, per label k in the order of the case, `<name>_crop<k>` (what `cut_object` returned), and the rows of
`<name>_centroids` (regionprops centroid of the mask), `<name>_angles` (degrees, what `ndimage.rotate` was handed; 0 without rotation)
and `<name>_boxes` (regionprops bbox of the turned mask on its canvas, half open) -- captured by wrapping `measure.regionprops` and
`ndimage.rotate` of the reference's module.

Conditions asserted, which concern the reference alone (a 'seeded' case is re-seeded until they hold):

* stability: the crop is unchanged when the angle handed to `ndimage.rotate` is moved by +1e-9 and by -1e-9 degrees -- last-bit
  differences between scikit-image's float moments and integer moments stay away from rounding ties;
* conditioning: |a - c| + |b| of the inertia tensor is above 1e-6 (a + c) in every turned 'seeded' case;
* at least one stored crop has pixels from outside the source, and at least one is clipped by `add_padding` at a canvas edge."""
import os
import sys

import numpy as np

from _reference_env import HERE, ROOT, ReferenceEnv

sys.path.insert(0, os.path.join(ROOT, 'tests'))


class Rejected(Exception):
    pass


def run_object(ref, img, mask, kwargs, seeded):
    """one call of the reference with its regionprops and rotate calls recorded, and twice more with the angle moved"""
    from scipy import ndimage
    from skimage import measure
    original_props, original_rotate = measure.regionprops, ndimage.rotate
    seen = {'props': [], 'angles': [], 'outside': False}
    nudge = [0.]

    def regionprops(label_image, *args, **kw):
        props = original_props(label_image, *args, **kw)
        if props:
            seen['props'].append((props[0].centroid, props[0].bbox, tuple(props[0].inertia_tensor.flat), label_image.shape))
        return props

    def rotate(arr, angle, *args, **kw):
        if arr.ndim == 2:
            seen['angles'].append(float(angle))
        return original_rotate(arr, angle + nudge[0], *args, **kw)

    ref.measure.regionprops, ref.ndimage.rotate = regionprops, rotate
    try:
        crop = ref.cut_object(img.copy(), mask.copy(), **kwargs)
        recorded = {key: list(value) if isinstance(value, list) else value for key, value in seen.items()}
        if kwargs['allow_rotate']:
            for nudge[0] in (1e-9, -1e-9):
                moved = ref.cut_object(img.copy(), mask.copy(), **kwargs)
                if moved.shape != crop.shape or not np.array_equal(moved, crop):
                    raise Rejected('the crop changes with the angle moved by %g degrees' % nudge[0])
    finally:
        ref.measure.regionprops, ref.ndimage.rotate = original_props, original_rotate
    # calls of regionprops: the horizontal segment, the mask, the (turned) mask
    (centroid, _, tensor, _), (_, box, _, canvas) = recorded['props'][1], recorded['props'][2]
    angle = recorded['angles'][0] if kwargs['allow_rotate'] else 0.
    a, b, _, c = tensor
    if kwargs['allow_rotate'] and seeded and not abs(a - c) + abs(b) > 1e-6 * (a + c):
        raise Rejected('an ill-conditioned orientation')
    return crop, centroid, angle, box, canvas


def run_case(ref, cases, name, seed, kind):
    inputs = cases.case(name, seed)
    kwargs = {key: inputs[key] for key in ('padding', 'use_mask', 'bg_color', 'allow_rotate')}
    out, crops, centroids, angles, boxes = {'seed': np.int64(seed)}, [], [], [], []
    flags = {'outside': 0, 'clipped': 0}
    for k, (label, mask) in enumerate(cases.masks_of(name, inputs)):
        crop, centroid, angle, box, canvas = run_object(ref, inputs['img'], mask, kwargs, kind == 'seeded')
        out['crop%d' % k] = crop
        centroids.append(centroid)
        angles.append(angle)
        boxes.append(box)
        padded = ref.add_padding(canvas, kwargs['padding'], *box)
        wanted = (box[0] - kwargs['padding'], box[1] - kwargs['padding'], box[2] + kwargs['padding'], box[3] + kwargs['padding'])
        flags['clipped'] += int(tuple(padded) != wanted)
        if kwargs['allow_rotate'] and inputs['img'].dtype == np.uint8 and not kwargs['use_mask']:
            # pixels from outside the source are 0 in a uint8 image: count crops the same call on an all-255 image leaves a 0 in
            white = ref.cut_object(np.full_like(inputs['img'], 255), mask.copy(), **kwargs)
            flags['outside'] += int((white == 0).any())
    out.update(centroids=np.array(centroids, dtype=np.float64), angles=np.array(angles, dtype=np.float64),
               boxes=np.array(boxes, dtype=np.int64))
    return out, flags


def main():
    with ReferenceEnv() as env:
        for alias in ('int', 'float', 'bool'):
            if not hasattr(np, alias):
                setattr(np, alias, {'int': int, 'float': float, 'bool': bool}[alias])
        import imsegm.utilities.data_io as ref
        import cut_objects_cases as cases
        import scipy
        out = {'versions': np.array('%s, scipy %s' % (env.versions, scipy.__version__))}
        totals = {'outside': 0, 'clipped': 0}
        for table in (cases.CASES, cases.INT_MASK_CASES):
            for name, (kind, _) in table.items():
                for seed in range(1, 200):
                    try:
                        result, flags = run_case(ref, cases, name, seed, kind)
                        break
                    except Rejected as why:
                        if kind == 'fixed':
                            raise SystemExit('%s: %s' % (name, why))
                        print(name, 'seed', seed, 'rejected:', why)
                else:
                    raise SystemExit('no seed of %s meets the conditions' % name)
                for key in totals:
                    totals[key] += flags[key]
                print(name, 'seed', seed, 'angles', np.round(result['angles'], 3).tolist(), 'shapes',
                      [result['crop%d' % k].shape for k in range(len(result['angles']))], flags)
                out.update({'%s_%s' % (name, key): np.asarray(value) for key, value in result.items()})
        # a label that is absent: the reference's error
        inputs = cases.case('rgb_p0', 1)
        try:
            ref.cut_object(inputs['img'], inputs['segm'] == 77, 0)
            raise SystemExit('the reference cut an absent label')
        except IndexError:
            pass
        assert totals['outside'] >= 1, 'no stored crop has pixels from outside the source'
        assert totals['clipped'] >= 1, 'no stored crop is clipped by add_padding'
    target = os.path.join(HERE, 'cut_objects.npz')
    np.savez_compressed(target, **out)
    print(target, os.path.getsize(target), 'bytes', totals)


if __name__ == '__main__':
    main()
