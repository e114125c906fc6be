"""Every claim of tests/slic_sweep_cases.py against the oracle, on the CPU: a case that no longer reaches its edge fails here.  The
check names follow the groups of cases: tile geometry, step 1 and candidate overflow, K > 4096, exact ties, the fast32 switch,
colour scale, dead centroids, SLICO; the restated helpers are held against the oracle's own grid and steps on all cases."""
import numpy as np
import pytest

import slic_sweep_cases as S

CASES = S.cases()


def group(name):
    return [c for c in CASES if c['group'] == name]


def ids(cs):
    return [c['id'] for c in cs]


@pytest.mark.parametrize('c', CASES, ids=ids(CASES))
def test_restated_grid_steps_and_windows_are_the_oracles(oracle, c):
    """K, the integer steps and the float step of the oracle's own run; the windows of the grid table as orc_slic_iterate forms them:
    the first sweep of the oracle must label exactly the pixels the restated windows of the grid cover"""
    geo = S.geometry_of(c)
    H, W = c['image'].shape[:2]
    _, info = oracle.slic(np.array(c['image']), c['n_segments'], c['compactness'], sigma=0., max_iter=1, enforce_connectivity=False,
                          return_internals=True)
    assert info['K'] == geo['K'] and info['steps'][1:] == [geo['step_y'], geo['step_x']] and float(np.float32(info['step'])) == geo['step']
    cent, _ = oracle.grid_centroids((1, H, W), c['n_segments'])
    assert np.array_equal(cent[:, 1:], S.grid_table(geo)[:, :2])
    win = S.search_windows(S.grid_table(geo), geo)
    assert np.array_equal(S.covered_mask(win, (H, W)), S.oracle_run(c, 1)[0] >= 0)
    if S.grid_covers(geo):
        assert (S.oracle_run(c, 1)[0] >= 0).all()


@pytest.mark.parametrize('c', group('tile'), ids=ids(group('tile')))
def test_tile_geometry_cases_reach_their_shapes(c):
    H, W = c['image'].shape[:2]
    assert (H, W) in S.TILE_SIZES and c['n_segments'] in (1, 2, 3, max(1, H * W // 64))
    geo = S.geometry_of(c)
    assert geo['K'] >= 1
    if H * W <= c['n_segments']:
        assert geo['grid_dy'] == geo['grid_dx'] == 1 and geo['step_y'] == geo['step_x'] == 1      # regular_grid returned slice(None)


def test_tile_geometry_sizes_straddle_the_workgroup_and_the_bin_tile():
    sizes = {c['image'].shape[:2] for c in group('tile')}
    assert sizes == set(S.TILE_SIZES)
    assert {h for h, w in sizes} >= {1, 15, 16, 17, 31, 32, 33} and {w for h, w in sizes} >= {1, 63, 64, 65}


@pytest.mark.parametrize('c', group('overflow'), ids=ids(group('overflow')))
def test_step_one_and_candidate_overflow(c):
    geo = S.geometry_of(c)
    if c.get('step_one'):
        assert geo['K'] == geo['H'] * geo['W'] and geo['step_y'] == geo['step_x'] == geo['grid_dy'] == geo['grid_dx'] == 1
    counts = {m: [len(t) for t in S.tile_candidates(S.search_windows(S.table_into(c, m), geo), geo)] for m in S.SWEEPS}
    if c.get('all_tiles_overflow') or c.get('step_one'):
        assert all(min(v) > S.MAXC for v in counts.values()), counts       # whole-table scan, leftover list, hand-back
    if c.get('has_lists'):
        assert all(min(v) <= S.MAXC for v in counts.values())
    if c.get('forced_overflow'):
        assert c['max_candidates'] == 3 and all(min(v) > 3 for v in counts.values())
        assert not S.geometry(c['image'].shape[:2], c['n_segments'], c['compactness'], c['normalize'], -1)['fast32']


@pytest.mark.parametrize('c', group('bigk'), ids=ids(group('bigk')))
def test_more_than_4096_centroids_on_the_full_scan(c):
    geo = S.geometry_of(c)
    assert geo['K'] > S.BIN_MAX_K_LDS
    full, behind = [], []
    for m in range(1, 11):
        table = S.table_into(c, m)
        if S.local_predicate(geo, S.drift_of(table, geo)):
            continue
        full.append(m)
        tiles = S.tile_candidates(S.search_windows(table, geo), geo)
        if any(1 <= len(t) <= S.MAXC and (t >= S.BIN_MAX_K_LDS).any() for t in tiles):
            behind.append(m)
    assert full, 'no sweep scans the whole table'
    assert behind, 'no tile lists a centroid read from s.win[k] behind the LDS copy'
    assert set(S.SWEEPS) & set(behind), (full, behind)


@pytest.mark.parametrize('c', group('tie'), ids=ids(group('tie')))
def test_exact_ties_beyond_the_first_sweep(c):
    geo = S.geometry_of(c)
    assert geo['fast32'] == bool(c.get('fast32', False))
    if c['normalize'] == 0:
        assert not geo['fast32']
    if c['id'] == 'tie-constant-96x128-exact':
        assert float(c['image'].min()) == float(c['image'].max()) == 0.5
    lab = S.oracle_run(c, 1)[2]
    assert c['tie_sweeps']
    for m in (1, 2, 3):
        b1, b2 = S.two_smallest(lab, S.table_into(c, m), geo)
        frac = float((b1 == b2).mean())
        print('%s: %.4f of the pixels on an exact tie going into sweep %d' % (c['id'], frac, m))
        if m in c['tie_sweeps']:
            assert frac > 0 and frac >= c.get('tie_fraction', 0.0), (c['id'], m, frac)


def test_exact_ties_beyond_the_first_sweep_on_the_exact_path():
    c = S.case('tie-checkerboard-72x90-exact')
    assert not S.geometry_of(c)['fast32'] and c['tie_sweeps'] == (2, 3)
    assert np.array_equal(S.oracle_run(c, 1)[2], S.oracle_run(S.case('tie-checkerboard-72x90'), 1)[2])


def test_the_numpy_distances_pick_the_oracles_labels():
    """two_smallest is the contract's arithmetic: where the smallest distance is unique ... the oracle's label has it"""
    c = S.case('tie-checkerboard-72x90')
    geo = S.geometry_of(c)
    table, lab = S.table_into(c, 2), S.oracle_run(c, 1)[2]
    b1, _ = S.two_smallest(lab, table, geo)
    near = S.oracle_run(c, 2)[0]
    y, x = np.mgrid[0:geo['H'], 0:geo['W']]
    k = near
    d = ((table[k, 0] - y) * (table[k, 0] - y) + (table[k, 1] - x) * (table[k, 1] - x)) * geo['sw']
    col = (lab[0] - table[k, 2]) ** 2
    col = col + (lab[1] - table[k, 3]) ** 2
    col = col + (lab[2] - table[k, 4]) ** 2
    assert np.array_equal(d + col, b1)


@pytest.mark.parametrize('c', group('fast32'), ids=ids(group('fast32')))
def test_fast32_switch(c):
    geo = S.geometry_of(c)
    assert geo['fast32'] == c['fast32']
    comp = c['compactness']
    if comp in (0.02640, 0.02639):
        assert (geo['M'] < 4096.0) == (comp == 0.02640) and geo['kappa'] < np.float32(1e-2)
    if comp in (0.00894, 0.00892):
        # (kappa < 1e-2 alone never decides: kappa reaches 1e-2 at M of about 12100, where M < 4096 has long failed -- both runs
        # take the exact path; the pair pins the restated kappa on the two sides of its threshold)
        assert (geo['kappa'] < np.float32(1e-2)) == (comp == 0.00894) and geo['M'] >= 4096.0 and not geo['fast32']


def test_fast32_cases_sit_on_both_sides_of_both_thresholds():
    comps = sorted(c['compactness'] for c in group('fast32'))
    assert comps == [0.00892, 0.00894, 0.02639, 0.0264, 0.09, 400.0]


@pytest.mark.parametrize('c', group('scale'), ids=ids(group('scale')))
def test_colour_scale(c):
    img = c['image']
    if img.dtype == np.float64:
        assert float(img.min()) == -3.0 and float(img.max()) == 7.0
        assert S.geometry_of(c)['fast32'] == (c['normalize'] != 0)
    else:
        assert img.dtype == np.uint8 and c['sigma'] in (0.0, 1.0)
    assert {c['normalize'] for c in group('scale') if c['image'].dtype == np.float64} == {0, 1, 2}


@pytest.mark.parametrize('c', [c for c in CASES if c.get('dead')], ids=ids([c for c in CASES if c.get('dead')]))
def test_dead_centroids(c):
    """some label of 0..K-1 is absent after a sweep m < 10 and still absent after sweep 10; its row is dead in the table"""
    geo = S.geometry_of(c)
    first = None
    for m in (1, 2, 3, 9):
        absent = np.setdiff1d(np.arange(geo['K']), S.oracle_run(c, m)[0])
        if len(absent):
            first = (m, absent)
            break
    assert first is not None
    m, absent = first
    assert not np.isin(absent, S.oracle_run(c, 10)[0]).any()
    assert not S.live_rows(S.table_into(c, m + 1))[absent].any()
    assert (S.search_windows(S.table_into(c, m + 1), geo)[absent] == 0).all()


@pytest.mark.parametrize('c', group('uncovered'), ids=ids(group('uncovered')))
def test_uncovered_pixels(c):
    """going into sweep ``uncovered_into`` >= 2 at least one pixel lies in no window of the oracle's table; it had a label before
    and keeps it: the oracle's map after that sweep has the label of the sweep before at every such pixel"""
    geo = S.geometry_of(c)
    m = c['uncovered_into']
    assert 2 <= m <= 10 and c['start_label'] in (0, 1)
    hole = ~S.covered_mask(S.search_windows(S.table_into(c, m), geo), c['image'].shape[:2])
    assert hole.any()
    before, after = S.oracle_run(c, m - 1)[0], S.oracle_run(c, m)[0]
    assert (before[hole] >= 0).all() and np.array_equal(after[hole], before[hole])
    assert (before[hole] != S.oracle_run(c, 1)[0][hole]).any() or m > 2          # (not simply the label of the first sweep's cell)
    assert {k['start_label'] for k in group('uncovered') if k['image'].shape == c['image'].shape} == {0, 1}


@pytest.mark.parametrize('c', group('slico'), ids=ids(group('slico')))
def test_slico_cases(c):
    assert c['slic_zero']
    plain = dict(c, id=c['id'] + '-plain', slic_zero=False)
    assert not np.array_equal(S.oracle_run(c, 10)[0], S.oracle_run(plain, 10)[0])      # the division by the maxima matters


def test_variant_cases_exist():
    for cid in S.VARIANT_CASES:
        S.case(cid)
