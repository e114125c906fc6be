"""The cases of ``tests/connectivity_cases.py`` on the host: the oracle (``oracle/imsegm_oracle.c``) against the plain Python
restatement and against the closed forms, the restatement against the real scikit-image 0.18.3 (``tests/golden/connectivity.npz``)
on the golden cases it can take, the recorded facts of every case against the limits of ``csrc/connectivity.hip`` they are aimed
at, and seeded defects of the restatement, each of which at least one case has to see (7 of 7 are seen).

Run with ``-s`` to get, per case, its facts against the limits and the cases that see each defect.
"""
import os

import numpy as np
import pytest

import connectivity_cases as CC

L = CC.LIMITS
SMALL = [c for c in CC.TABLE if c['make']().size <= CC.RESTATE_MAX_VOXELS]
LARGE = [c for c in CC.TABLE if c['make']().size > CC.RESTATE_MAX_VOXELS]
GOLDEN = np.load(os.path.join(CC.HERE, 'golden', 'connectivity.npz'))


def test_only_closed_form_cases_are_beyond_the_restatement():
    assert LARGE and all(c['closed_form'] is not None for c in LARGE)
    assert max(c['make']().size for c in CC.TABLE) <= 1024 * 514


@pytest.mark.parametrize('case', SMALL, ids=[c['name'] for c in SMALL])
@pytest.mark.parametrize('start_label', [0, 1])
def test_oracle_equals_restatement(oracle, case, start_label):
    lab = case['make']() + start_label
    want = CC.restate(lab, case['min_size'], case['max_size'], start_label)
    got = oracle.enforce_connectivity(lab, case['min_size'], case['max_size'], start_label)
    assert got.shape == want.shape and np.array_equal(got, want)
    key = '%s_start%d' % (case['name'], start_label)
    if key in GOLDEN:                                       # the real scikit-image 0.18.3
        assert np.array_equal(want, GOLDEN[key])


@pytest.mark.parametrize('case', [c for c in CC.TABLE if c['closed_form']], ids=[c['name'] for c in CC.TABLE if c['closed_form']])
@pytest.mark.parametrize('start_label', [0, 1])
def test_oracle_equals_closed_form(oracle, case, start_label):
    lab = case['make']() + start_label
    got = oracle.enforce_connectivity(lab, case['min_size'], case['max_size'], start_label)
    assert np.array_equal(got, case['closed_form'](case['make'](), start_label))


def test_golden_volume_through_the_restatement():
    _, mn, mx = CC.GEN.CASES['volume']
    for start_label in (0, 1):
        assert np.array_equal(CC.restate(CC.GEN.make('volume') + start_label, mn, mx, start_label), GOLDEN['volume_start%d' % start_label])


@pytest.mark.parametrize('case', SMALL, ids=[c['name'] for c in SMALL])
def test_case_lies_on_the_intended_side_of_its_limit(case):
    f, e, must = CC.facts(case), CC.expected_stage(case), case['must']
    shape3 = f['shape3']
    n = int(np.prod(shape3))
    boxes_g = [CC.cells_general(s['box'], shape3) for s in f['smalls']]
    boxes_t = [CC.cells_tile(s['box']) for s in f['smalls']]
    widest = max([s['widest'] for s in f['smalls']], default=0)
    print('\n%-22s %-14s kept %5d small %5d (table %5d) rounds %d | small boxes: general <= %6d (1024 / 8192), tile <= %6d (16384 / '
          '131072), widest level %4d (64 / 2048) | roots per 256 x 16 tile %3d..%4d (64) | tile-local <= %s (256) -> %s %s'
          % (case['name'], 'x'.join(map(str, shape3)), f['kept'], f['small'], n // L['TABLE_DIV'], f['oversize_rounds'],
             max(boxes_g, default=0), max(boxes_t, default=0), widest, min(f['roots_per_size_tile']), max(f['roots_per_size_tile']),
             max(f['tile_local']) if f['tile_local'] else '-', e['path'], e.get('tile') or ''))
    if 'path' in must:
        assert e['path'] == must['path']
    for key in ('kept', 'small'):
        if key in must:
            assert f[key] == must[key]
    if 'small_is' in must:
        assert f['small'] == must['small_is'] and e['general']['all_to_thread'] == must['all_to_thread']
        assert (f['small'] > n // L['TABLE_DIV']) == must['all_to_thread']
    if 'rounds' in must:
        assert f['oversize_rounds'] == must['rounds']
    if 'hash_tiles' in must:
        assert min(f['roots_per_size_tile']) == must['hash_tiles'][0] == L['FS_SLOTS'] and max(f['roots_per_size_tile']) >= must['hash_tiles'][1]
        assert shape3[2] % 4 == 0
    if 'hash_min' in must:
        assert min(f['roots_per_size_tile']) >= must['hash_min'] and shape3[2] % 4 == 0
    if 'box_general' in must:
        assert max(boxes_g) == must['box_general']
        assert e['general']['big'] >= must['big'] and (max(boxes_g) > L['ORDER_BIG']) == bool(must['big'])
        assert e['general']['fallback'] == must['thread'] and (max(boxes_g) > L['WAVE_CELLS']) == bool(must['thread'])
    if 'box_tile' in must:
        assert max(boxes_t) == must['box_tile']
    if 'widest' in must:
        assert widest == must['widest']
    if 'fb' in must:
        assert e['tile']['fb'] == must['fb'] and e['tile']['fb2'] == must['fb2']
    if 'tile_local' in must:
        assert max(f['tile_local']) == must['tile_local']
        if must['tile_local'] > L['CT_SLOTS']:
            assert sum(1 for c in f['tile_local'] if c > L['CT_SLOTS']) == 1


def test_row_segment_cases_cross_every_segment_border():
    """a run of one label over x = 62, 124, 186 and 248, and rows in groups that are no multiple of CR_ROWS = 4 or of 16"""
    crossed = set()
    for c in SMALL:
        if c['name'].startswith(('row_w', 'run_edges', 'comb_up', 'width_')):
            lab = c['make']()
            lab3 = lab[None] if lab.ndim == 2 else lab
            for b in (62, 124, 186, 248):
                if lab3.shape[2] > b and (lab3[:, :, b - 1] == lab3[:, :, b]).any():
                    crossed.add(b)
    assert crossed == {62, 124, 186, 248}
    assert {CC.BY_NAME['comb_up_h%d_d2' % h]['make']().shape[1] for h in (1, 3, 4, 5, 17)} == {1, 3, 4, 5, 17}
    assert {CC.BY_NAME['width_%dx3_d2' % w]['make']().size % 4 for w in (249, 250, 251)} == {1, 2, 3}


def test_seeded_defects_are_seen():
    seen = {}
    names = ['corners', 'run_edges_d2', 'sizes_exact', 'joined_behind_d2', 'l_shape', 'touching', 'row_w63_d2', 'stripes_d2', 'hash_noise']
    for defect in CC.DEFECTS:
        seen[defect] = []
        for name in names:
            c = CC.BY_NAME[name]
            for start_label in (0, 1):
                lab = c['make']() + start_label
                good = CC.restate(lab, c['min_size'], c['max_size'], start_label)
                bad = CC.restate(lab, c['min_size'], c['max_size'], start_label, defect=defect)
                if not np.array_equal(good, bad):
                    seen[defect].append('%s/start%d' % (name, start_label))
    for defect, where in seen.items():
        print('\ndefect %-22s seen by %d: %s' % (defect, len(where), ', '.join(where)))
    n_seen = sum(1 for where in seen.values() if where)
    print('\n%d of %d seeded defects seen' % (n_seen, len(CC.DEFECTS)))
    assert n_seen == len(CC.DEFECTS), [d for d, where in seen.items() if not where]
