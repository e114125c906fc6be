"""Time the centre-candidate point descriptors on the benchmark image: its 2048 x 2048 class map (SLIC -> colour features -> GMM ->
GraphCut with bench.py's parameters) and its SLIC centres, the default radii (10 .. 50) and ``angle_step=5``.

Two formulations of the same tables, alternating in one process, median of the runs after a warm-up:

* ``batched``: ``compute_label_histograms_positions`` (one launch, every window read once) and ``compute_ray_features_positions`` with
  ``smooth_ray`` (mask and smoothing inside the kernel);
* ``composed``: what the package offered before -- ``compute_label_hist_positions`` once per radius, and
  ``hip_ray_features_positions`` on a mask built on the host followed by ``scipy.ndimage.gaussian_filter1d`` per position.

The results are compared before anything is timed (rings bit for bit, rays within one float32 spacing).  Every call ends in a
download, so the host clock measures finished work.  The exit status is 1 when either batched call is slower than its composition.

    python tools/time_point_descriptors.py [--runs 7] [--size 2048] [--out profiles/point_descriptors_time.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SP_SIZE, SP_REGUL, NB_CLASSES, GC_REGUL, EDGE_TYPE = 46, 0.2, 3, 2.0, 'model'         # bench.py
SMOOTH_RAY, ANGLE_STEP, BORDER_LABELS = 1.0, 5, [0]


def class_map_and_centres(size):
    from pyimsegm_amd import pipelines as pipe
    from pyimsegm_amd import superpixels
    from pyimsegm_amd.descriptors import FEATURES_SET_COLOR
    from pyimsegm_amd.graph_cuts import estim_class_model
    from pyimsegm_amd.utilities.synthetic import voronoi_image
    image = voronoi_image(size, size, seed=1)
    sp_size = max(int(round(SP_SIZE * size / 2048.)), 4)
    np.random.seed(0)
    resident = pipe._ResidentImage(image, FEATURES_SET_COLOR, sp_size, SP_REGUL)
    try:
        model = estim_class_model(resident.features, NB_CLASSES, 'GMM', None, True)
        segm, _ = resident.segment(None, GC_REGUL, EDGE_TYPE, classes=getattr(model, 'classes_', None), to_host=True, want_soft=False,
                                   model=model)
    finally:
        resident.close()
    slic = superpixels.segment_slic_img2d(image, sp_size=sp_size, relative_compact=SP_REGUL)
    centres = np.round(np.asarray(superpixels.superpixel_centers(slic))).astype(int)
    return np.asarray(segm), centres


def composed_rings(descriptors, segm, centres, radii, nb_labels):
    per_disc = [descriptors.compute_label_hist_positions(segm, centres, descriptors._disc(r), nb_labels) for r in radii]
    hist, size = np.stack([h for h, _ in per_disc], axis=1), np.stack([s for _, s in per_disc], axis=1)
    hist_last = np.concatenate([np.zeros_like(hist[:, :1]), hist[:, :-1]], axis=1)
    inter_size = size - np.concatenate([np.zeros_like(size[:, :1]), size[:, :-1]], axis=1)
    return ((hist - hist_last) / inter_size[:, :, None]).reshape(len(centres), -1)


def composed_rays(descriptors, segm, centres):
    from scipy import ndimage
    rays = descriptors.hip_ray_features_positions(np.isin(segm, BORDER_LABELS), centres, ANGLE_STEP, 'up')
    return np.array([ndimage.gaussian_filter1d(row, SMOOTH_RAY) for row in rays])


def median_ms(values):
    return round(float(np.median(values)) * 1e3, 3)


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--runs', type=int, default=7)
    parser.add_argument('--size', type=int, default=2048)
    parser.add_argument('--out', default=os.path.join('profiles', 'point_descriptors_time.json'))
    args = parser.parse_args()
    from pyimsegm_amd import descriptors
    segm, centres = class_map_and_centres(args.size)
    radii, nb_labels = list(descriptors.HIST_CIRCLE_DIAGONALS), int(segm.max()) + 1

    def batched_rings():
        return descriptors.compute_label_histograms_positions(segm, centres, radii, nb_labels)[0]

    def batched_rays():
        return descriptors.compute_ray_features_positions(segm, centres, ANGLE_STEP, border_labels=BORDER_LABELS, smooth_ray=SMOOTH_RAY,
                                                          shifting=False)[0]

    calls = {'rings_batched': batched_rings, 'rings_composed': lambda: composed_rings(descriptors, segm, centres, radii, nb_labels),
             'rays_batched': batched_rays, 'rays_composed': lambda: composed_rays(descriptors, segm, centres)}
    first = {name: call() for name, call in calls.items()}                      # the warm-up, and the comparison
    assert np.array_equal(first['rings_batched'], first['rings_composed'])
    assert np.all(np.abs(first['rays_batched'].astype(np.float64) - first['rays_composed']) <= np.spacing(np.abs(first['rays_composed'])))
    times = {name: [] for name in calls}
    for _ in range(args.runs):
        for name, call in calls.items():
            start = time.perf_counter()
            call()
            times[name].append(time.perf_counter() - start)
    result = {'size': args.size, 'positions': int(len(centres)), 'labels': nb_labels, 'radii': radii, 'angle_step': ANGLE_STEP,
              'smooth_ray': SMOOTH_RAY, 'border_labels': BORDER_LABELS, 'runs': args.runs}
    for name in calls:
        result[name + '_ms'] = median_ms(times[name])
        result[name + '_ms_min_max'] = [median_ms([min(times[name])]), median_ms([max(times[name])])]
    result['rings_not_slower'] = bool(result['rings_batched_ms'] <= result['rings_composed_ms'])
    result['rays_not_slower'] = bool(result['rays_batched_ms'] <= result['rays_composed_ms'])
    print(json.dumps(result), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as out:
        json.dump(result, out, indent=1)
    return 0 if result['rings_not_slower'] and result['rays_not_slower'] else 1


if __name__ == '__main__':
    sys.exit(main())
