"""Time ``segment_color2d_slic_features_model_graphcut`` on the bench's 2048 x 2048 image with a class model that has a PCA step
(``estim_class_model(..., pca_coef=0.95)`` on ``{'color': mean, std, energy}``): the device model (k_pca_project + k_gmm_proba in
the one call) against the path this model took before the device evaluated it -- ``pipelines._device_gmm`` answering None: feature
table down, scikit-learn's ``predict_proba`` on the host, probabilities up.  Same process, same build, the two variants alternating
(ABAB...), medians over the repeats; writes profiles/reduced_model_time.json and exits with an error when the device model is the
slower one.  No speed-up is promised anywhere: the file holds what was measured.

This is NOT a comparison with the parent commit's build: both variants run in this build, so whatever the change costs the shared
path (larger scratch, wider kernel arguments) falls on both sides.  The output file names that under 'comparison'.

    python tools/time_reduced_model.py [--repeats 15] [--size 2048] [--out profiles/reduced_model_time.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FEATURES = {'color': ['mean', 'std', 'energy']}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--repeats', type=int, default=15)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--size', type=int, default=2048)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'reduced_model_time.json'))
    args = ap.parse_args(argv)
    import bench
    from pyimsegm_amd import _hip
    from pyimsegm_amd import pipelines as pipe
    from pyimsegm_amd.graph_cuts import estim_class_model
    from pyimsegm_amd.utilities.synthetic import voronoi_image

    image = voronoi_image(args.size, args.size, seed=1)
    res = pipe._ResidentImage(image, FEATURES, bench.SP_SIZE, bench.SP_REGUL)
    try:
        table = np.array(res.features)
    finally:
        res.close()
    np.random.seed(0)
    model = estim_class_model(table, bench.NB_CLASSES, 'GMM', pca_coef=0.95)
    gmm = pipe._device_gmm(model)
    if gmm is None:
        raise SystemExit('the device does not take this model')
    device_gmm = pipe._device_gmm

    def run(on_device):
        pipe._device_gmm = device_gmm if on_device else (lambda model: None)
        try:
            t0 = time.perf_counter()
            segm, _ = pipe.segment_color2d_slic_features_model_graphcut(image, model, FEATURES, bench.SP_SIZE, bench.SP_REGUL,
                                                                        bench.GC_REGUL, bench.EDGE_TYPE)
            _hip.default_context().synchronize()
            return time.perf_counter() - t0, np.asarray(segm)
        finally:
            pipe._device_gmm = device_gmm

    for _ in range(args.warmup):
        _, on_dev = run(True)
        _, on_host = run(False)
    times = {True: [], False: []}
    for _ in range(args.repeats):
        for variant in (True, False):
            times[variant].append(run(variant)[0])
    med = {k: float(np.median(v)) for k, v in times.items()}
    out = {
        'what': 'segment_color2d_slic_features_model_graphcut, %d x %d, model with pca_coef=0.95 (%d -> %d columns, %d classes)'
                % (args.size, args.size, gmm.n_inputs, gmm.n_features, gmm.n_classes),
        'comparison': 'device model against the host-evaluated route of the SAME build (pipelines._device_gmm answering None: the '
                      'route the parent commit takes for this model); not a run of the parent commit\'s build -- costs of the change '
                      'on the shared path fall on both sides',
        'repeats': args.repeats, 'order': 'alternating device, host',
        'device_model_median_s': med[True], 'host_model_median_s': med[False],
        'device_model_min_s': float(np.min(times[True])), 'host_model_min_s': float(np.min(times[False])),
        'device_model_all_s': times[True], 'host_model_all_s': times[False],
        'pixels_differing': int(np.sum(on_dev != on_host)),
    }
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as fp:
        json.dump(out, fp, indent=1)
    print(json.dumps({k: v for k, v in out.items() if not k.endswith('_all_s')}))
    if med[True] > med[False]:
        raise SystemExit('the device model is slower than the host-evaluated path: %.4f s against %.4f s' % (med[True], med[False]))


if __name__ == '__main__':
    main()
