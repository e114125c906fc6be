"""Time ``ellipse_fitting.prepare_boundary_points_ray_edge`` with its default discs (15 / 5) and 32 centres on a 2048 x 2048 class map
of synthetic eggs (ellipses of class 1 with a yolk of class 2 and a few pinholes, on background 0) on the device and as the scipy /
numpy statement of the same definitions (``on='host'``), alternating on one box, median of the runs after a warm-up.  The share of
the transfers is the time of the same host <-> device copies alone (the int32 class map up, the two ray tables down).  The point
lists are compared byte for byte before anything is timed.  The exit status is 1 when the device is slower than the host statement
of the same run.

    python tools/time_boundary_points.py [--runs 7] [--size 2048] [--centres 32] [--out profiles/boundary_points_time.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def egg_map(size, centres, seed=3):
    """class map and the centres of its eggs: ellipses on a jittered grid"""
    rng = np.random.RandomState(seed)
    seg = np.zeros((size, size), dtype=np.int32)
    per_side = int(np.ceil(np.sqrt(centres)))
    cell = size / float(per_side)
    rows, cols = np.mgrid[:size, :size]
    positions = []
    for index in range(centres):
        row = (index // per_side + 0.5 + rng.uniform(-0.1, 0.1)) * cell
        col = (index % per_side + 0.5 + rng.uniform(-0.1, 0.1)) * cell
        a, b, theta = cell * rng.uniform(0.25, 0.4), cell * rng.uniform(0.18, 0.3), rng.uniform(0, np.pi)
        u = (rows - row) * np.cos(theta) + (cols - col) * np.sin(theta)
        v = (rows - row) * np.sin(theta) - (cols - col) * np.cos(theta)
        seg[(u / a) ** 2 + (v / b) ** 2 < 1] = 1
        seg[(u / (0.4 * a)) ** 2 + (v / (0.4 * b)) ** 2 < 1] = 2
        positions.append((int(row), int(col)))
    speckle = rng.rand(size, size)
    seg[speckle < 0.002] = 0                                     # pinholes the hole filling closes
    seg[(speckle > 0.99995) & (seg == 0)] = 1                    # specks the opening removes
    return seg, positions


def median_ms(values):
    return round(float(np.median(values)) * 1e3, 3)


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--runs', type=int, default=7)
    parser.add_argument('--size', type=int, default=2048)
    parser.add_argument('--centres', type=int, default=32)
    parser.add_argument('--out', default=os.path.join('profiles', 'boundary_points_time.json'))
    args = parser.parse_args()
    from pyimsegm_amd import _hip
    from pyimsegm_amd import ellipse_fitting as ell
    seg, centres = egg_map(args.size, args.centres)
    got = ell.prepare_boundary_points_ray_edge(seg, centres, on='device')
    want = ell.prepare_boundary_points_ray_edge(seg, centres, on='host')
    assert len(got) == len(want) and all(a.tobytes() == b.tobytes() for a, b in zip(got, want))
    ctx = _hip.default_context()
    device_buf = _hip.C.c_void_p()
    _hip._check(_hip.load_library().imsegm_device_alloc(ctx.device, seg.nbytes, _hip.C.byref(device_buf)))
    down = np.empty(2 * len(centres) * 72, dtype=np.float32)
    times = {'host': [], 'device': [], 'transfers': []}
    for _ in range(args.runs + 1):
        start = time.perf_counter()
        ell.prepare_boundary_points_ray_edge(seg, centres, on='host')
        times['host'].append(time.perf_counter() - start)
        start = time.perf_counter()
        ell.prepare_boundary_points_ray_edge(seg, centres, on='device')
        times['device'].append(time.perf_counter() - start)
        start = time.perf_counter()
        ctx.copy(device_buf.value, seg.ctypes.data, seg.nbytes)
        ctx.copy(down.ctypes.data, device_buf.value, down.nbytes)
        times['transfers'].append(time.perf_counter() - start)
    _hip.load_library().imsegm_device_free(device_buf)
    result = {'size': args.size, 'centres': len(centres), 'sel_bg': ell.STRUC_ELEM_BG, 'sel_fg': ell.STRUC_ELEM_FG,
              'points': int(sum(len(p) for p in want)), 'runs': args.runs, 'host_ms': median_ms(times['host'][1:]),
              'device_ms': median_ms(times['device'][1:]), 'transfers_ms': median_ms(times['transfers'][1:])}
    result['transfer_share_of_device'] = round(result['transfers_ms'] / result['device_ms'], 3)
    result['device_not_slower_than_host'] = bool(result['device_ms'] <= result['host_ms'])
    print(json.dumps(result), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as out:
        json.dump(result, out, indent=1)
    # the yardstick: not slower than the host statement measured in the same run
    return 0 if result['device_not_slower_than_host'] else 1


if __name__ == '__main__':
    sys.exit(main())
