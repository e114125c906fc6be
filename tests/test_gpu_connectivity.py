"""``_enforce_label_connectivity_cython`` (scikit-image 0.18, the second native call inside ``skimage.segmentation.slic``;
/root/reference/imsegm/superpixels.py:61-63) on crafted label maps, HIP against the oracle AND against the outputs of the real
scikit-image 0.18.3 (``tests/golden/connectivity.npz``), bit for bit.

The 2-D tile path of ``csrc/connectivity.hip`` has hand-over points (more than 256 local components in a tile, a BFS
frontier of more than 64 cells, bounding boxes beyond the LDS tiles, oversize components); every case below is built to
cross one of them.
"""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def hip():
    from pyimsegm_amd import _hip
    _hip.default_context()
    return _hip


HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location('make_golden_connectivity', os.path.join(HERE, 'golden', 'make_golden_connectivity.py'))
GEN = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(GEN)
_salted = GEN.salted

#: the crafted maps of tests/golden/make_golden_connectivity.py (outputs of the real scikit-image 0.18.3 in connectivity.npz)
#: plus one that only the oracle covers
CASES = [(name, (lambda name=name: GEN.make(name)), GEN.CASES[name][1], GEN.CASES[name][2])
         for name in GEN.CASES if name != 'volume'] + [
    ('tiny', lambda: GEN.blocks(4, 4, 2, 2), 2, 100),
]

import connectivity_cases as CC  # noqa: E402

GOLDEN = np.load(os.path.join(HERE, 'golden', 'connectivity.npz'))

#: which path has to finish the case: the tile path (incl. its own hand-overs to the 128 K tile and the LDS-frontier kernel), or
#: the general one (None: either)
PATH = {'blocks_ragged': 'tile', 'salt_1pct': 'tile', 'comb_frontier_75': 'tile', 'diagonal_100': 'tile', 'diagonal_200': 'tile',
        'one_row': 'tile', 'one_column': 'tile', 'tiny': 'tile', 'noise': 'general', 'oversize': 'general',
        'salt_10pct': 'tile',            # at most 240 of the 256 slots of a tile are taken
        'everything_small': 'general'}   # 465 local components in a tile
#: the stage of the tile path that has to finish the small components: (CNT_FB, CNT_FB2) = how many the 16 K tile hands to the
#: 128 K tile, and that one to the LDS-frontier kernel.  From the code: the comb's BFS walks along its spine, its widest level
#: holds 5 cells whatever the number of teeth (never more than the 64 of k_small_bfs_reg), its box has 1 848 cells; the
#: diagonals have one-cell frontiers and boxes of 10 920 (first stage) and 41 820 cells (second stage)
STAGE = {'comb_frontier_75': (0, 0), 'diagonal_100': (0, 0), 'diagonal_200': (1, 0)}


@pytest.mark.parametrize('name,make,min_size,max_size', CASES, ids=[c[0] for c in CASES])
@pytest.mark.parametrize('start_label', [0, 1])
def test_enforce_connectivity_bit_exact(hip, oracle, name, make, min_size, max_size, start_label):
    lab = make() + start_label          # (as slic hands it over: no pixel carries the mask label start_label - 1)
    want = oracle.enforce_connectivity(lab, min_size, max_size, start_label)
    im = hip.Image2D(lab.shape[0], lab.shape[1])
    general_runs = hip.load_library().imsegm_debug_conn_general_runs
    try:
        before = general_runs()
        got = im.enforce_connectivity(lab, min_size, max_size, start_label)
        took_general = general_runs() - before
        assert got.shape == lab.shape and np.array_equal(got, want), '%d pixels differ' % int((got != want).sum())
        key = '%s_start%d' % (name, start_label)
        if key in GOLDEN:                              # ... and with the real scikit-image 0.18.3
            assert np.array_equal(got, GOLDEN[key])
        if PATH.get(name) == 'tile':
            assert took_general == 0, 'left the tile path'
            last = hip.conn_last()
            assert last['general'] is None and last['tile']['flag'] == 0
            if name in STAGE:
                assert (last['tile']['fb'], last['tile']['fb2']) == STAGE[name]
        elif PATH.get(name) == 'general':
            assert took_general == 1
        # session reuse: a second, different map on the same buffers
        lab2 = np.ascontiguousarray(lab[::-1])
        assert np.array_equal(im.enforce_connectivity(lab2, min_size, max_size, start_label),
                              oracle.enforce_connectivity(lab2, min_size, max_size, start_label))
    finally:
        im.close()


@pytest.mark.parametrize('case', CC.TABLE, ids=[c['name'] for c in CC.TABLE])
@pytest.mark.parametrize('start_label', [0, 1])
def test_enforce_connectivity_at_every_hand_over(hip, oracle, monkeypatch, case, start_label):
    """the table of tests/connectivity_cases.py: bit for bit the oracle, and finished by the kernels the table names -- read
    from the counters the host holds anyway (imsegm_debug_conn_last).

    Start label 1 with a first segment below min_size (comb_up_h3_d2, corners, the tile_box_* and general_box_* maps, ...): the
    reference writes 0 over it, the mask label there, and seeds its voxels again; k_small_rescan replays that."""
    lab = case['make']() + start_label
    min_size, max_size = case['min_size'], case['max_size']
    want = oracle.enforce_connectivity(lab, min_size, max_size, start_label)
    if case['closed_form']:
        assert np.array_equal(want, case['closed_form'](case['make'](), start_label))
    if case['force_general']:
        monkeypatch.setenv('IMSEGM_CONN_GENERAL', '1')
    session = hip.Image2D(*lab.shape) if lab.ndim == 2 else hip.Volume3D(*lab.shape)
    try:
        got = session.enforce_connectivity(lab, min_size, max_size, start_label)
        last = hip.conn_last()
        assert got.shape == want.shape and got.dtype == want.dtype
        assert np.array_equal(got, want), '%d voxels differ' % int((got != want).sum())
        _check_stage(case, lab, last)
        # session reuse: the flipped map on the same buffers
        lab2 = np.ascontiguousarray(lab[::-1] if lab.ndim == 2 else lab[:, ::-1, ::-1])
        assert np.array_equal(session.enforce_connectivity(lab2, min_size, max_size, start_label),
                              oracle.enforce_connectivity(lab2, min_size, max_size, start_label))
    finally:
        session.close()


def _check_stage(case, lab, last):
    must = case['must']
    tile_tried = lab.ndim == 2 and not case['force_general']
    assert (last['tile'] is not None) == tile_tried
    if lab.size > CC.RESTATE_MAX_VOXELS:                    # the closed-form block maps: path and kept count
        assert (last['general'] is None) == (must['path'] == 'tile')
        assert (last['general'] or last['tile'])['kept'] == must['kept']
        return
    e = CC.expected_stage(case)                             # (the facts belong to start label 0; they do not depend on it)
    assert e['path'] == must.get('path', e['path'])
    assert (last['general'] is None) == (e['path'] == 'tile'), (last, e)
    if tile_tried:
        t = last['tile']
        assert bool(t['flag']) == e['tile']['flag'], (last, e)
        if not e['tile']['flag']:
            assert bool(t['over']) == e['tile']['over'], (last, e)
            if not e['tile']['over']:
                assert (t['fb'], t['fb2'], t['fallback']) == (e['tile']['fb'], e['tile']['fb2'], e['tile']['fallback']), (last, e)
                if e['path'] == 'tile':
                    assert t['kept'] == e['kept']
    if e['path'] == 'general':
        g = last['general']
        n = lab.size
        assert g['kept'] == e['kept'] and last['oversize_rounds'] == e['oversize_rounds'], (last, e)
        assert g['small'] == CC.facts(case)['small']
        assert (g['small'] > n // CC.LIMITS['TABLE_DIV']) == e['general']['all_to_thread']
        assert (g['big'], g['fallback']) == (e['general']['big'], e['general']['fallback']), (last, e)   # CNT_FALLBACK: the thread BFS


def test_enforce_connectivity_randomised(hip, oracle):
    rng = np.random.RandomState(7)
    for _ in range(12):
        h, w = int(rng.randint(5, 300)), int(rng.randint(5, 300))
        bh, bw = int(rng.randint(3, 40)), int(rng.randint(3, 40))
        lab = _salted(h, w, bh, bw, float(rng.choice([0.0, 0.002, 0.02, 0.1])), int(rng.randint(1 << 30)))
        seg = h * w / float(lab.max() + 1)
        min_size, max_size = int(0.5 * seg), int(3 * seg)
        im = hip.Image2D(h, w)
        try:
            got = im.enforce_connectivity(lab, min_size, max_size, 0)
        finally:
            im.close()
        assert np.array_equal(got, oracle.enforce_connectivity(lab, min_size, max_size, 0)), (h, w, bh, bw)


def test_enforce_connectivity_volume_golden(hip):
    """the volume of the golden set (real scikit-image 0.18.3), both start labels"""
    _, min_size, max_size = GEN.CASES['volume']
    for start_label in (0, 1):
        lab = GEN.make('volume') + start_label
        vol = hip.Volume3D(*lab.shape)
        try:
            got = vol.enforce_connectivity(lab, min_size, max_size, start_label)
        finally:
            vol.close()
        assert np.array_equal(got, GOLDEN['volume_start%d' % start_label])


def test_enforce_connectivity_volume(hip, oracle):
    """3-D label maps (6 neighbours, z first) take the general path through the same entry point"""
    rng = np.random.RandomState(11)
    for shape, b in (((6, 40, 50), 10), ((12, 33, 21), 7), ((1, 64, 64), 16)):
        zz, yy, xx = np.mgrid[0:shape[0], 0:shape[1], 0:shape[2]]
        lab = ((zz // max(1, shape[0] // 2)) * 100 + (yy // b) * 10 + xx // b).astype(np.int32)
        m = rng.rand(*shape) < 0.03
        lab[m] = rng.randint(0, 40, m.sum())
        seg = lab.size / float(len(np.unique(lab)))
        want = oracle.enforce_connectivity(lab, int(0.5 * seg), int(3 * seg), 0)
        vol = hip.Volume3D(*shape)
        try:
            got = vol.enforce_connectivity(lab, int(0.5 * seg), int(3 * seg), 0)
        finally:
            vol.close()
        assert np.array_equal(got, want), shape


def test_slic_of_benchmark_like_images_stays_on_the_tile_path(hip):
    """SLIC label maps of the synthetic benchmark images (configs 2 and 4) must not need the general connectivity path"""
    from pyimsegm_amd import superpixels as S
    from pyimsegm_amd.utilities.synthetic import voronoi_image
    general_runs = hip.load_library().imsegm_debug_conn_general_runs
    before = general_runs()
    for shape, sp, seed in (((647, 1024), 35, 100), ((647, 1024), 35, 101), ((1024, 1024), 46, 1)):
        S.segment_slic_img2d(voronoi_image(shape[0], shape[1], seed=seed), sp, 0.2)
    assert general_runs() == before
