"""The 2-D SLIC sweeps (csrc/slic.hip) sweep by sweep on the cases of tests/slic_sweep_cases.py: labels AND the centroid table
(``Image2D.get_centroids()``) after max_iter = 1, 2, 3 and 10, against the oracle and against the independent definition of a
centroid -- the mean of the pixels that carry its label.

The oracle (``orc_slic_iterate``) updates its table once more after its last sweep, the device does not: the table the device
holds after ``max_iter`` sweeps is compared with the oracle's table of the run with ONE SWEEP FEWER (the grid with colour 0 for
max_iter = 1), ``slic_sweep_cases.table_into``.  A row that is dead in the oracle (NaN) must have an empty window on the device;
the live windows are the restated ``search_window`` of the oracle's rows.

Colour bound of the independent check: every pixel enters the sums as trunc(v * 2^f) (common.h), f = 46 - e, 2^e > premax, so a
sum of n pixels is short of the true sum by less than n * 2^-f and the mean by less than 2^-f; the canonical split, the scaling
by 2^-f (exact) and the division round twice more: 2^-f + 2^-51 * |mean|.  Positions: integer sums, exact; one rounding in the
division -- equality."""
import os
import subprocess
import sys

import numpy as np
import pytest

import slic_sweep_cases as S

pytestmark = pytest.mark.gpu

CASES = S.cases()
IDS = [c['id'] for c in CASES]
HERE = os.path.dirname(os.path.abspath(__file__))
PLACEMENTS = ('default', 'IMSEGM_FUSE_FINALIZE', 'IMSEGM_SEPARATE_FINALIZE')
LD = np.longdouble


@pytest.fixture(scope='module')
def hip():
    from pyimsegm_amd import _hip
    _hip.default_context()
    return _hip


def device_run(hip, c, max_iter, sess=None):
    """(nearest, rows, windows, planes, premax) of one run with enforce_connectivity=False (start_label 0)"""
    own = sess is None
    if own:
        sess = hip.Image2D(*c['image'].shape[:2])
    try:
        sess.upload(c['image'])
        sess.slic(c['n_segments'], c['compactness'], sigma=c['sigma'], normalize=c['normalize'], max_iter=max_iter,
                  enforce_connectivity=False, max_candidates=c['max_candidates'], slic_zero=c['slic_zero'])
        rows, windows = sess.get_centroids()
        return sess.get_nearest(), rows, windows, sess.get_lab(), sess.get_pre_scalars()[2]
    finally:
        if own:
            sess.close()


def check_against_oracle(c, max_iter, nearest, rows, windows):
    geo = S.geometry_of(c)
    assert np.array_equal(nearest, S.oracle_run(c, max_iter)[0]), '%s: labels after %d sweeps' % (c['id'], max_iter)
    table = S.table_into(c, max_iter)
    live = S.live_rows(table)
    assert rows.shape == table.shape and windows.shape == (geo['K'], 4)
    assert np.array_equal(rows[live].view(np.uint64), np.ascontiguousarray(table[live]).view(np.uint64)), \
        '%s: centroid rows going into sweep %d' % (c['id'], max_iter)
    assert np.array_equal(windows, S.search_windows(table, geo)), '%s: windows going into sweep %d' % (c['id'], max_iter)
    assert (windows[~live] == 0).all()


def check_against_the_means(c, max_iter, previous_nearest, rows, windows, lab, premax):
    """rows of the table after ``max_iter`` sweeps against the pixels labelled k in the map of ``max_iter - 1`` sweeps"""
    H, W = previous_nearest.shape
    K = len(rows)
    flat = previous_nearest.ravel()
    ok = flat >= 0
    n = np.bincount(flat[ok], minlength=K)
    y, x = np.mgrid[0:H, 0:W]
    sy = np.bincount(flat[ok], weights=y.ravel()[ok].astype(np.float64), minlength=K)        # (integers < 2^53: exact)
    sx = np.bincount(flat[ok], weights=x.ravel()[ok].astype(np.float64), minlength=K)
    live = n > 0
    assert np.array_equal(live, (windows[:, 1] > windows[:, 0]) & (windows[:, 3] > windows[:, 2]))
    assert np.array_equal(rows[live, 0], sy[live] / n[live]) and np.array_equal(rows[live, 1], sx[live] / n[live])
    e = int(np.frexp(premax)[1]) if premax > 0 else 1
    f = 46 - e
    worst = 0.0
    for ch in range(3):
        sums = np.zeros(K, dtype=LD)
        np.add.at(sums, flat[ok], lab[ch].ravel()[ok].astype(LD))
        mean = sums[live] / n[live].astype(LD)
        err = np.abs(rows[live, 2 + ch].astype(LD) - mean)
        bound = LD(2.0) ** -f + LD(2.0) ** -51 * np.abs(mean)
        worst = max(worst, float((err / bound).max()))
        assert (err <= bound).all(), '%s: colour %d going into sweep %d: %.3g of the bound' % (c['id'], ch, max_iter, worst)
    return worst


@pytest.mark.parametrize('c', CASES, ids=IDS)
def test_labels_and_centroids_sweep_by_sweep(hip, c):
    runs = {m: device_run(hip, c, m) for m in S.ORACLE_SWEEPS}
    worst = 0.0
    for m in S.ORACLE_SWEEPS:
        nearest, rows, windows, lab, premax = runs[m]
        check_against_oracle(c, m, nearest, rows, windows)
        if m - 1 in runs:
            worst = max(worst, check_against_the_means(c, m, runs[m - 1][0], rows, windows, lab, premax))
    grid = S.grid_table(S.geometry_of(c))
    assert np.array_equal(runs[1][1], grid)
    print('%-34s largest colour error: %.3g of the bound' % (c['id'], worst))


@pytest.mark.parametrize('c', CASES, ids=IDS)
def test_every_placement_of_the_update(hip, monkeypatch, c):
    """default, IMSEGM_FUSE_FINALIZE, IMSEGM_SEPARATE_FINALIZE: the same bytes; an image whose tiles all overflow is handed back
    exactly once by the fused update (where a sweep is fused at all: fast32, default list capacity, no SLICO)"""
    geo = S.geometry_of(c)
    for m in S.SWEEPS:
        got = {}
        for place in PLACEMENTS:
            if place != 'default':
                monkeypatch.setenv(place, '1')
            before = hip.slic_sweep_runs()[1]
            got[place] = device_run(hip, c, m)
            handed_back = hip.slic_sweep_runs()[1] - before
            if place != 'default':
                monkeypatch.delenv(place)
            if place == 'IMSEGM_SEPARATE_FINALIZE':
                assert handed_back == 0
            if place == 'IMSEGM_FUSE_FINALIZE' and (c.get('all_tiles_overflow') or c.get('step_one')):
                fused = geo['fast32'] and not c['slic_zero'] and (m >= 3 or (m == 2 and S.grid_covers(geo)))
                assert handed_back == (1 if fused else 0), (c['id'], m, handed_back)
        check_against_oracle(c, m, *got['default'][:3])
        for place in PLACEMENTS[1:]:
            for a, b in zip(got[place][:3], got['default'][:3]):
                assert a.tobytes() == b.tobytes(), (c['id'], m, place)


def test_smaller_case_after_a_larger_one_and_after_poison(hip):
    big, small = S.case('dead-96x128'), S.case('tile-noise-33x65-n33')
    sess_big = hip.Image2D(96, 128)
    try:
        for m in S.SWEEPS:
            check_against_oracle(big, m, *device_run(hip, big, m, sess_big)[:3])
            tiny = S.case('tile-ramp-96x128-n2')
            check_against_oracle(tiny, m, *device_run(hip, tiny, m, sess_big)[:3])        # K = 2 in a table that held 192
        sess_big.poison(0x7F7F7F7F)
        with pytest.raises(hip.HipError):
            sess_big.get_centroids()
        check_against_oracle(big, 10, *device_run(hip, big, 10, sess_big)[:3])
    finally:
        sess_big.close()
    sess = hip.Image2D(33, 65)
    try:
        for c in (S.case('slico-noise-33x65'), small, S.case('tie-constant-33x65-corners'), small):
            check_against_oracle(c, 3, *device_run(hip, c, 3, sess)[:3])
    finally:
        sess.close()


@pytest.mark.parametrize('cid', [c['id'] for c in CASES if c['id'].startswith(('massdeath-', 'uncovered-'))])
def test_start_labels_with_connectivity(hip, oracle, cid):
    """start_label 1 needs the connectivity stage: the raw assignment carries no offset, the label map is the oracle's"""
    c = S.case(cid)
    img = c['image']
    sess = hip.Image2D(*img.shape[:2])
    try:
        sess.upload(img)
        sess.slic(c['n_segments'], c['compactness'], sigma=c['sigma'], normalize=c['normalize'], start_label=c['start_label'])
        nearest, labels = sess.get_nearest(), sess.get_labels()
        rows, windows = sess.get_centroids()
    finally:
        sess.close()
    check_against_oracle(c, 10, nearest, rows, windows)
    want = oracle.slic(np.array(img), c['n_segments'], c['compactness'], sigma=c['sigma'], normalize=(float(img.min()), float(img.max())),
                       start_label=c['start_label'])
    assert np.array_equal(labels, want)


def test_batch_of_three_33x65_images(hip, oracle):
    """tie, noise and ramp as float64 through Batch2D in one call: each superpixel map equals its single run and the oracle's"""
    from test_gpu_batch import _batched, _model
    images = [np.array(S.case('tie-constant-33x65-corners')['image']),
              np.ascontiguousarray(S.case('tile-noise-33x65-n33')['image'].astype(np.float64) / 255.0),
              np.array(S.case('tile-ramp-33x65-n33')['image'])]
    from pyimsegm_amd.utilities.synthetic import voronoi_image
    model = _model([voronoi_image(120, 160, seed=3).astype(np.float64) / 255.], 14, 0.25)      # (any class model: the maps are compared)
    maps = []
    _batched(images, model, 8, 0.3, keep=lambda b: maps.extend(b.get_labels(i) for i in range(3)))
    from pyimsegm_amd.superpixels import segment_slic_img2d
    for i, img in enumerate(images):
        assert np.array_equal(maps[i], np.asarray(segment_slic_img2d(img, 8, 0.3))), i
        assert np.array_equal(maps[i], oracle.segment_slic_img2d(img, 8, 0.3)), i


VARIANT_SETTINGS = ('IMSEGM_ASSIGN_UNITS=2', 'IMSEGM_DEBUG_ASSIGN=16', 'IMSEGM_DEBUG_ASSIGN=32', 'IMSEGM_DEBUG_ASSIGN=48')


def test_shipped_variants_read_once_per_process():
    """two units per wave, k_slic_assign<*, false> with its fp32 pre-selection instead of the dot form (16), k_slic_assign<*, FIRST>
    instead of the closed-form first sweep (32), both (48): one fresh child process each, one after the other, each with its own
    time limit; the first child that does not exit 0 (or runs out of time: subprocess.run kills it and raises) ends the test, so
    nothing more is started on the device behind it.  Every child is compared before the next one starts."""
    want = {}
    for cid in S.VARIANT_CASES:
        c = S.case(cid)
        geo = S.geometry_of(c)
        for m in S.SWEEPS:
            table = S.table_into(c, m)
            want[(cid, str(m))] = S.crc_of(S.oracle_run(c, m)[0], table, S.search_windows(table, geo), S.live_rows(table))
    for setting in VARIANT_SETTINGS:
        name, value = setting.split('=')
        env = dict(os.environ)
        env[name] = value
        try:
            done = subprocess.run([sys.executable, os.path.join(HERE, 'slic_sweep_variant_run.py')], env=env, stdout=subprocess.PIPE,
                                  stderr=subprocess.PIPE, universal_newlines=True, timeout=120)
        except subprocess.TimeoutExpired as ex:
            pytest.fail('%s: the child ran past its time limit and was killed; nothing more is started.  stderr: %s'
                        % (setting, (ex.stderr or '')[-2000:]))
        assert done.returncode == 0, (setting, done.returncode, done.stderr[-2000:])
        got = dict((tuple(line.split()[1:3]), int(line.split()[3])) for line in done.stdout.splitlines() if line.startswith('CRC '))
        assert got == want, (setting, sorted(k for k in want if got.get(k) != want[k]))
