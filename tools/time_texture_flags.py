#!/usr/bin/env python
"""Time the Leung-Malik texture statistics on the device: the full bank on the 2048 x 2048 image of BASELINE config 3 (its
SLIC superpixels) with mean / std / energy (the fused lm_features call) and with all five statistics (battery by battery:
median and mean gradient of every response), then the short bank with all five on a gray volume.  Wall clock around the
device-synchronised calls, warm-up first, median of N runs; one JSON line out (and into OUT when given).

    python tools/time_texture_flags.py [--runs N] [--size S] [--volume D H W] [OUT]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pyimsegm_amd import _hip  # noqa: E402
from pyimsegm_amd import descriptors as D  # noqa: E402
from pyimsegm_amd.superpixels import _open_session, _run_slic  # noqa: E402
from pyimsegm_amd.utilities.synthetic import ellipsoid_volume, voronoi_image  # noqa: E402

SUMS = ('mean', 'std', 'energy')
FIVE = D.NAMES_FEATURE_FLAGS


def timed(fn, runs):
    ctx = _hip.default_context()
    fn()                                    # warm-up: library load, buffers, kernel code objects
    times = []
    for _ in range(runs):
        ctx.synchronize()
        t0 = time.perf_counter()
        out = fn()
        ctx.synchronize()
        times.append(time.perf_counter() - t0)
    return out, float(np.median(times)) * 1e3, [round(t * 1e3, 3) for t in times]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--size', type=int, default=2048)
    ap.add_argument('--volume', type=int, nargs=3, default=(16, 512, 512))
    ap.add_argument('out', nargs='?')
    args = ap.parse_args()
    result = {'runs': args.runs}
    img = voronoi_image(args.size, args.size)
    sess, mode = _open_session(img)
    _run_slic(sess, mode, 46, 0.2)
    filters, names = D._select_bank('normal')
    result['image'] = dict(shape=list(img.shape), n_labels=int(sess.n_labels), batteries=len(filters))
    for tag, flags in (('image_sums', SUMS), ('image_five', FIVE)):
        fts, ms, all_ms = timed(lambda: D._texture_desc_lm_device(img, None, flags, filters, names, sess=sess), args.runs)
        result[tag] = dict(flags=list(flags), columns=int(fts[0].shape[1]), median_ms=round(ms, 3), runs_ms=all_ms)
    sess.close()
    vol = ellipsoid_volume(tuple(args.volume), seed=3).astype(np.float64)
    steps = (4, 24, 24)
    seg = np.ravel_multi_index(tuple(g // s for g, s in zip(np.indices(vol.shape), steps)),
                               tuple(-(-n // s) for n, s in zip(vol.shape, steps))).astype(np.int32)
    fts, ms, all_ms = timed(lambda: D.compute_texture_desc_lm_img3d_val(vol, seg, FIVE, bank_type='short'), args.runs)
    result['volume_five'] = dict(shape=list(vol.shape), n_labels=int(seg.max()) + 1, bank='short', flags=list(FIVE),
                                 columns=int(fts[0].shape[1]), median_ms=round(ms, 3), runs_ms=all_ms)
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()
