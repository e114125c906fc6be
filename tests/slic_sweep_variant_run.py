#!/usr/bin/env python
"""One child process of tests/test_gpu_slic_sweeps.py::test_shipped_variants_read_once_per_process: the library reads
IMSEGM_ASSIGN_UNITS and IMSEGM_DEBUG_ASSIGN once per process, so every setting gets a fresh interpreter.  Runs the cases of
slic_sweep_cases.VARIANT_CASES at max_iter 1, 2, 3 and 10 and prints one line ``CRC <case> <max_iter> <crc>`` each: labels, the
centroid rows with a non-empty window and all windows (slic_sweep_cases.crc_of)."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]


def main():
    import slic_sweep_cases as S
    from pyimsegm_amd import _hip as hip
    for cid in S.VARIANT_CASES:
        c = S.case(cid)
        sess = hip.Image2D(*c['image'].shape[:2])
        try:
            for m in S.SWEEPS:
                sess.upload(c['image'])
                sess.slic(c['n_segments'], c['compactness'], sigma=c['sigma'], normalize=c['normalize'], max_iter=m,
                          enforce_connectivity=False, max_candidates=c['max_candidates'], slic_zero=c['slic_zero'])
                rows, windows = sess.get_centroids()
                live = (windows[:, 1] > windows[:, 0]) & (windows[:, 3] > windows[:, 2])
                print('CRC %s %d %d' % (cid, m, S.crc_of(sess.get_nearest(), rows, windows, live)), flush=True)
        finally:
            sess.close()


if __name__ == '__main__':
    main()
