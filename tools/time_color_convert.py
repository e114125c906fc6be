"""Time the 'color_<space>' descriptor groups of ``descriptors.compute_selected_features_color2d`` on the 2048 x 2048 benchmark
image (``voronoi_image``, the generator of bench.py's config 2) with its SLIC map held fixed: ``convert_on='host'`` -- numpy's
conversion and a second upload of the float64 result, what the call does by default -- against ``convert_on='device'`` (the
conversion kernel of csrc/colorspace.hip on the session that holds the RGB image), for ``{'color_lab': ('mean', 'std',
'energy')}`` and for all five spaces together.  The two alternate on one box after a warm-up; the median of the runs counts.  The
conversion kernel's own duration comes from stream events (the context's profiler) over the same image, per space, with the bytes
it must move for a uint8 image (3 B read + 24 B written per pixel).  The tables are compared before anything is timed (1e-5 x
max(1, |expected|), the descriptor bound).  The exit status is 1 when the device path is slower than the host path of the same
run, for either feature set.

    python tools/time_color_convert.py [--runs 7] [--size 2048] [--out profiles/color_convert_time.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SPACES = ('hsv', 'luv', 'lab', 'hed', 'xyz')
STATS = ('mean', 'std', 'energy')
FEATURE_SETS = {'lab': {'color_lab': STATS}, 'all_five': {'color_' + space: STATS for space in SPACES}}
BYTES_PER_PIXEL = 27


def median_ms(values):
    return round(float(np.median(values)) * 1e3, 3)


def kernel_times(image, runs):
    """{space: microseconds of one conversion kernel}, median of ``runs`` launches timed by stream events"""
    from pyimsegm_amd import _hip
    from pyimsegm_amd.utilities.data_io import _HED_FROM_RGB
    ctx = _hip.default_context()
    sess = _hip.Image2D(*image.shape[:2], ctx=ctx).upload(image)
    out = {}
    try:
        ctx.profile_enable(True)
        for space in SPACES:
            matrix = _HED_FROM_RGB if space == 'hed' else None
            sess.convert_color(space, matrix)           # warm-up: the buffer, the code object
            ctx.synchronize()
            samples = []
            for _ in range(runs):
                ctx.profile_reset()
                sess.convert_color(space, matrix)
                ctx.synchronize()
                ms, count = ctx.profile_get('color_stats')
                assert count == 1
                samples.append(ms)
            out[space] = round(float(np.median(samples)) * 1e3, 2)
    finally:
        ctx.profile_enable(False)
        sess.close()
    return out


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--runs', type=int, default=7)
    parser.add_argument('--size', type=int, default=2048)
    parser.add_argument('--out', default=os.path.join('profiles', 'color_convert_time.json'))
    args = parser.parse_args()
    from pyimsegm_amd import superpixels
    from pyimsegm_amd.descriptors import compute_selected_features_color2d
    from pyimsegm_amd.utilities.synthetic import voronoi_image
    size = args.size
    image = voronoi_image(size, size, seed=1)           # the image of bench.py's 2048 x 2048 line, its superpixel size and regularity
    slic = superpixels.segment_slic_img2d(image, sp_size=max(int(round(46 * size / 2048.)), 4), relative_compact=0.2)
    result = {'size': size, 'dtype': str(image.dtype), 'superpixels': int(slic.max()) + 1, 'runs': args.runs, 'feature_sets': {}}
    for name, flags in FEATURE_SETS.items():
        want, want_names = compute_selected_features_color2d(image, slic, flags, convert_on='host')
        got, got_names = compute_selected_features_color2d(image, slic, flags, convert_on='device')
        assert got_names == want_names and np.all(np.abs(got - want) <= 1e-5 * np.maximum(1, np.abs(want)))
        times = {'host': [], 'device': []}
        for _ in range(args.runs + 1):
            for where in ('host', 'device'):
                start = time.perf_counter()
                compute_selected_features_color2d(image, slic, flags, convert_on=where)
                times[where].append(time.perf_counter() - start)
        entry = {'columns': int(want.shape[1]), 'host_ms': median_ms(times['host'][1:]), 'device_ms': median_ms(times['device'][1:])}
        entry['host_over_device'] = round(entry['host_ms'] / entry['device_ms'], 2)
        entry['device_not_slower_than_host'] = bool(entry['device_ms'] <= entry['host_ms'])
        result['feature_sets'][name] = entry
    kernel_us = kernel_times(image, args.runs)
    moved = BYTES_PER_PIXEL * size * size
    result['kernel_us'] = kernel_us
    result['kernel_bytes'] = moved
    result['kernel_gb_per_s'] = {space: round(moved / (us * 1e-6) / 1e9, 1) for space, us in kernel_us.items()}
    result['device_not_slower_than_host'] = all(e['device_not_slower_than_host'] for e in result['feature_sets'].values())
    print(json.dumps(result), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as out:
        json.dump(result, out, indent=1)
    # the yardstick: not slower than the host path measured in the same run
    return 0 if result['device_not_slower_than_host'] else 1


if __name__ == '__main__':
    sys.exit(main())
