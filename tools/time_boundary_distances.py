"""Time ``labeling.compute_boundary_distances`` on a 2048 x 2048 pair -- the SLIC map of the benchmark image at K = 2025 against a
block annotation -- on the device and as the numpy + scipy statement of the same definition (shifted comparisons for the thick
boundaries, ``scipy.ndimage.distance_transform_edt``), alternating on one box, median of the runs after a warm-up.  The device is
timed in its stateless form (both maps uploaded) and in its session form (the SLIC map already resident, only the annotation
uploaded); the share of the transfers is the time of the same host <-> device copies alone (two int32 maps up, the points down).
The results are compared bit for bit before anything is timed.  The exit status is 1 when the device (stateless form) is slower
than the host formulation of the same run.

    python tools/time_boundary_distances.py [--runs 7] [--size 2048] [--out profiles/boundary_distances_time.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def host_boundary_distances(segm_ref, segm):
    from scipy import ndimage

    def thick(seg):
        out = np.zeros(seg.shape, dtype=bool)
        out[:-1, :] |= seg[:-1, :] != seg[1:, :]
        out[1:, :] |= seg[1:, :] != seg[:-1, :]
        out[:, :-1] |= seg[:, :-1] != seg[:, 1:]
        out[:, 1:] |= seg[:, 1:] != seg[:, :-1]
        return out
    on_ref = thick(segm_ref)
    return np.argwhere(on_ref), ndimage.distance_transform_edt(~thick(segm))[on_ref]


def median_ms(values):
    return round(float(np.median(values)) * 1e3, 3)


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--runs', type=int, default=7)
    parser.add_argument('--size', type=int, default=2048)
    parser.add_argument('--out', default=os.path.join('profiles', 'boundary_distances_time.json'))
    args = parser.parse_args()
    from pyimsegm_amd import _hip, labeling, superpixels
    from pyimsegm_amd.utilities.synthetic import voronoi_image
    size = args.size
    image = voronoi_image(size, size, seed=1)           # the image of bench.py's 2048 x 2048 line, its superpixel size and regularity
    slic = superpixels.segment_slic_img2d(image, sp_size=max(int(round(46 * size / 2048.)), 4), relative_compact=0.2)
    rows, cols = np.indices((size, size))
    annot = ((rows // (size // 6 + 1)) * 6 + cols // (size // 5 + 1)).astype(np.int64)
    got, want = labeling.compute_boundary_distances(annot, slic), host_boundary_distances(annot, slic)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[1].dtype == want[1].dtype
    session = _hip.Image2D(size, size).set_labels(slic)
    with_session = labeling.compute_boundary_distances(annot, None, _session=session)
    assert np.array_equal(with_session[0], want[0]) and np.array_equal(with_session[1], want[1])
    ctx = _hip.default_context()
    up = np.ascontiguousarray(slic, dtype=np.int32)
    device_buf = _hip.C.c_void_p()
    _hip._check(_hip.load_library().imsegm_device_alloc(ctx.device, up.nbytes, _hip.C.byref(device_buf)))
    down = np.empty(len(want[0]) * 2, dtype=np.float64)
    times = {'host': [], 'device': [], 'device_session': [], 'transfers': []}
    for _ in range(args.runs + 1):
        start = time.perf_counter()
        host_boundary_distances(annot, slic)
        times['host'].append(time.perf_counter() - start)
        start = time.perf_counter()
        labeling.compute_boundary_distances(annot, slic)
        times['device'].append(time.perf_counter() - start)
        start = time.perf_counter()
        labeling.compute_boundary_distances(annot, None, _session=session)
        times['device_session'].append(time.perf_counter() - start)
        start = time.perf_counter()
        ctx.copy(device_buf.value, up.ctypes.data, up.nbytes)
        ctx.copy(device_buf.value, up.ctypes.data, up.nbytes)
        ctx.copy(down.ctypes.data, device_buf.value, down.nbytes)
        times['transfers'].append(time.perf_counter() - start)
    _hip.load_library().imsegm_device_free(device_buf)
    session.close()
    result = {'size': size, 'superpixels': int(slic.max()) + 1, 'annotation_labels': int(annot.max()) + 1, 'points': int(len(want[0])),
              'runs': args.runs, 'host_ms': median_ms(times['host'][1:]), 'device_ms': median_ms(times['device'][1:]),
              'device_session_ms': median_ms(times['device_session'][1:]), 'transfers_ms': median_ms(times['transfers'][1:])}
    result['transfer_share_of_device'] = round(result['transfers_ms'] / result['device_ms'], 3)
    result['device_not_slower_than_host'] = bool(result['device_ms'] <= result['host_ms'])
    print(json.dumps(result), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as out:
        json.dump(result, out, indent=1)
    # the yardstick: not slower than the host formulation measured in the same run
    return 0 if result['device_not_slower_than_host'] else 1


if __name__ == '__main__':
    sys.exit(main())
