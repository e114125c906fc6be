"""Label maps aimed at the capacity limits and kernel hand-overs of ``pyimsegm_amd/csrc/connectivity.hip``, and a second, plain
restatement of ``_enforce_label_connectivity_cython`` (scikit-image 0.18 ``_slic.pyx``) that records, while it runs, the facts
those limits are about.  ``tests/test_connectivity_reference_host.py`` holds the restatement against the oracle, the golden file
and the closed forms, and checks that every case lies on the intended side of its limit; ``tests/test_gpu_connectivity.py`` runs
the table on the device and asks the library which kernels finished each case.

The restatement shares no code with ``oracle/imsegm_oracle.c`` or ``tests/test_oracle_slic.py``: flat indices, Python lists.
It is slow (about a second per 10^5 voxels), so only the kept-capacity block maps are larger; those have a closed form.
"""
import importlib.util
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location('make_golden_connectivity', os.path.join(HERE, 'golden', 'make_golden_connectivity.py'))
GEN = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(GEN)
blocks, salted, comb, diagonal = GEN.blocks, GEN.salted, GEN.comb, GEN.diagonal

#: the limits of csrc/connectivity.hip, with the lines that state them
LIMITS = {
    'CR_SPAN': 62,              # :102  voxels of a row per wave (k_ccl_init_rows / k_ccl_merge_rows)
    'CR_GROUP': 248,            # :109  four segments per workgroup
    'CR_ROWS': 4,               # :126  rows per wave of the merge
    'FS_SLOTS': 64,             # :236  roots of a 256 x 16 tile in the LDS size table
    'FS_TILE': (16, 256),       # :261-262
    'SCAN_BLOCK': 4096,         # :390  voxels per workgroup of k_kept_scan
    'TABLE_DIV': 12,            # :918  bounding-box table: n / 12 small components
    'ORDER_BIG': 1024,          # :935  k_small_order: boxes beyond this many cells first
    'WAVE_CELLS': 8192,         # :936  k_small_bfs_wave<8192, 2048, .>
    'WAVE_FRONT': 2048,
    'CT_TILE': (32, 64),        # :968  tile of the 2-D path (rows, columns)
    'CT_SLOTS': 256,            # :968
    'CONN_KEPT_CAP': 65536,     # :969
    'CONN_FB_CAP': 4096,        # :969
    'KR_BUCKETS': 1024,         # :1239
    'KR_SORTED_LDS': 2048,      # :1239
    'BR_CELLS': 16384,          # :1302
    'BR_CELLS_BIG': 131072,     # :1303
    'REG_FRONT': 64,            # :1412 frontier of k_small_bfs_reg (one wave)
}

RESTATE_MAX_VOXELS = 150000

DEFECTS = ('neighbour_order', 'adjacent_first', 'min_size_le', 'max_size_late', 'no_z', 'start_label_ignored', 'segment_border_size')


def restate(labels, min_size, max_size, start_label=0, defect=None, record=None):
    """``_enforce_label_connectivity_cython`` from its definition: raster scan; every voxel not yet labelled seeds a BFS over the
    voxels of its label that are still unlabelled, neighbours in the order +x, -x, +y, -y, +z, -z, stopped when ``max_size`` voxels
    are collected; ``adjacent`` is the label of the last labelled voxel of another segment the BFS looked at (0 if none); a segment
    below ``min_size`` takes ``adjacent``, any other the next number from ``start_label``.  ``defect`` seeds one deliberate mistake;
    ``record`` (a dict) receives the facts of the run."""
    lab = np.ascontiguousarray(labels)
    shape = lab.shape
    D, H, W = (1, ) + shape if lab.ndim == 2 else shape
    n, HW = D * H * W, H * W
    seg = lab.ravel().tolist()
    mask = start_label - 1
    out = [mask] * n
    order = (0, 1, 2, 3, 4, 5)
    if defect == 'neighbour_order':
        order = (2, 3, 0, 1, 4, 5)
    if defect == 'no_z':
        order = (0, 1, 2, 3)
    current = start_label
    gen = [0] * n if record is not None else None           # how many truncated segments a voxel was left over by
    kept = small = rounds = 0
    smalls = []
    for p in range(n):
        if out[p] >= start_label:
            continue
        label = seg[p]
        adjacent = 0
        adjacent_set = False
        out[p] = current
        queue = [p]
        depth = [0]
        size = 1
        v = 0
        limit = max_size + 1 if defect == 'max_size_late' else max_size
        while v < size < limit:
            q = queue[v]
            x = q % W
            y = (q // W) % H
            z = q // HW
            for d in order:
                if d == 0:
                    if x + 1 >= W: continue
                    t = q + 1
                elif d == 1:
                    if x == 0: continue
                    t = q - 1
                elif d == 2:
                    if y + 1 >= H: continue
                    t = q + W
                elif d == 3:
                    if y == 0: continue
                    t = q - W
                elif d == 4:
                    if z + 1 >= D: continue
                    t = q + HW
                else:
                    if z == 0: continue
                    t = q - HW
                o = out[t]
                if seg[t] == label and o == mask:
                    out[t] = current
                    queue.append(t)
                    depth.append(depth[v] + 1)
                    size += 1
                    if size >= limit:
                        break
                elif o >= start_label and o != current:
                    if not (defect == 'adjacent_first' and adjacent_set):
                        adjacent = o
                        adjacent_set = True
            v += 1
        counted = size
        if defect == 'segment_border_size':                 # a voxel lost where a run crosses x = 62
            counted -= sum(1 for q in queue if q % W == 62 and seg[q - 1] == label) > 0
        is_small = counted <= min_size if defect == 'min_size_le' else counted < min_size
        if record is not None:
            if size >= max_size:
                g = gen[p] + 1
                rounds = max(rounds, g)
                _mark_left_over(queue, seg, out, mask, gen, g, D, H, W)
            if is_small:
                small += 1
                xs, ys, zs = [q % W for q in queue], [(q // W) % H for q in queue], [q // HW for q in queue]
                smalls.append({'root': p, 'size': size, 'box': (min(zs), max(zs), min(ys), max(ys), min(xs), max(xs)),
                               'widest': int(np.bincount(depth).max())})
            else:
                kept += 1
        if is_small:
            for q in queue:
                out[q] = adjacent
        else:
            current += 1
    if record is not None:
        record.update(kept=kept, small=small, smalls=smalls, oversize_rounds=rounds)
    res = np.array(out, dtype=np.int64).reshape(shape)
    if defect == 'start_label_ignored':                     # the kept segments numbered from 0
        res = np.where(res >= start_label, res - start_label, res)
    return res


def _mark_left_over(members, seg, out, mask, gen, g, D, H, W):
    """the voxels a truncated BFS left behind (same label, still unlabelled, connected to it): generation g"""
    HW = H * W
    label = seg[members[0]]
    stack = list(members)
    seen = set()
    while stack:
        q = stack.pop()
        x, y, z = q % W, (q // W) % H, q // HW
        for ok, t in ((x + 1 < W, q + 1), (x > 0, q - 1), (y + 1 < H, q + W), (y > 0, q - W), (z + 1 < D, q + HW), (z > 0, q - HW)):
            if ok and seg[t] == label and out[t] == mask and t not in seen:
                seen.add(t)
                gen[t] = g
                stack.append(t)


def components(lab3):
    """ids of the 6-connected sets of equal labels (the smallest flat index of each set), plain union-find over numpy passes"""
    D, H, W = lab3.shape
    idx = np.arange(lab3.size).reshape(lab3.shape)
    parent = idx.copy().ravel()
    pairs = []
    for ax in range(3):
        a = [slice(None)] * 3
        b = [slice(None)] * 3
        a[ax], b[ax] = slice(1, None), slice(None, -1)
        same = lab3[tuple(a)] == lab3[tuple(b)]
        pairs.append(np.stack([idx[tuple(a)][same], idx[tuple(b)][same]], 1))
    pairs = np.concatenate(pairs)
    while True:                                             # min-label propagation with pointer jumping
        before = parent.copy()
        if len(pairs):
            m = np.minimum(parent[pairs[:, 0]], parent[pairs[:, 1]])
            np.minimum.at(parent, pairs[:, 0], m)
            np.minimum.at(parent, pairs[:, 1], m)
            np.minimum.at(parent, before[pairs[:, 0]], m)
            np.minimum.at(parent, before[pairs[:, 1]], m)
        parent = parent[parent]
        if np.array_equal(parent, before):
            return parent.reshape(lab3.shape)


def tile_counts(lab, tile, local):
    """per tile of (rows, columns) of every slice: the number of components inside the tile alone (local) or of distinct
    components of the whole map that reach into it; returns the list over all tiles"""
    lab3 = lab[None] if lab.ndim == 2 else lab
    th, tw = tile
    whole = None if local else components(lab3)
    counts = []
    for z in range(lab3.shape[0]):
        for y in range(0, lab3.shape[1], th):
            for x in range(0, lab3.shape[2], tw):
                if local:
                    counts.append(len(np.unique(components(lab3[z:z + 1, y:y + th, x:x + tw]))))
                else:
                    counts.append(len(np.unique(whole[z, y:y + th, x:x + tw])))
    return counts


def cells_general(box, shape3):
    """cells k_small_order / k_small_bfs_wave stage: the bounding box plus one ring, clipped to the volume (:579-582, :616-621)"""
    D, H, W = shape3
    z0, z1, y0, y1, x0, x1 = box
    return ((min(x1 + 1, W - 1) - max(x0 - 1, 0) + 1) * (min(y1 + 1, H - 1) - max(y0 - 1, 0) + 1) *
            (min(z1 + 1, D - 1) - max(z0 - 1, 0) + 1))


def cells_tile(box):
    """cells k_small_bfs_reg stages: the bounding box plus two rings, not clipped (:1337-1339)"""
    _, _, y0, y1, x0, x1 = box
    return (x1 - x0 + 5) * (y1 - y0 + 5)


def facts(case):
    """the facts of a case the limits are about (start label 0), cached"""
    if 'facts' in case:
        return case['facts']
    lab = case['make']()
    shape3 = (1, ) + lab.shape if lab.ndim == 2 else lab.shape
    f = {}
    restate(lab, case['min_size'], case['max_size'], 0, record=f)
    f['shape3'] = shape3
    f['first_sizes'] = np.bincount(components(lab.reshape(shape3)).ravel())
    f['roots_per_size_tile'] = tile_counts(lab, LIMITS['FS_TILE'], False)
    f['tile_local'] = tile_counts(lab, LIMITS['CT_TILE'], True) if shape3[0] == 1 else None
    case['facts'] = f
    return f


def expected_stage(case):
    """what the kernels' limits make of the recorded facts: the path that finishes the case and the counters it leaves"""
    f = facts(case)
    shape3 = f['shape3']
    n = shape3[0] * shape3[1] * shape3[2]
    L = LIMITS
    e = {'kept': f['kept'], 'oversize_rounds': f['oversize_rounds'], 'tile': None}
    oversize = bool((f['first_sizes'] >= case['max_size']).any())
    tile_tried = shape3[0] == 1 and not case['force_general']
    if tile_tried:
        wide = [s for s in f['smalls'] if s['widest'] > L['REG_FRONT']]
        fb = sum(1 for s in f['smalls'] if cells_tile(s['box']) > L['BR_CELLS'] or s['widest'] > L['REG_FRONT'])
        fb2 = sum(1 for s in f['smalls'] if cells_tile(s['box']) > L['BR_CELLS_BIG'] or s['widest'] > L['REG_FRONT'])
        left = sum(1 for s in f['smalls'] if (cells_tile(s['box']) > L['BR_CELLS_BIG'] or s in wide) and
                   (cells_general(s['box'], shape3) > L['WAVE_CELLS'] or s['widest'] > L['WAVE_FRONT']))
        flag = max(f['tile_local']) > L['CT_SLOTS']
        e['tile'] = {'flag': flag, 'over': oversize, 'fb': fb, 'fb2': fb2, 'fallback': left}
        e['path'] = 'general' if flag or oversize or left or f['kept'] > L['CONN_KEPT_CAP'] or fb > L['CONN_FB_CAP'] else 'tile'
    else:
        e['path'] = 'general'
    if e['path'] == 'general':
        all_to_thread = f['small'] > n // L['TABLE_DIV']
        big = [s for s in f['smalls'] if cells_general(s['box'], shape3) > L['ORDER_BIG']]
        thread = [s for s in f['smalls'] if cells_general(s['box'], shape3) > L['WAVE_CELLS'] or s['widest'] > L['WAVE_FRONT']]
        e['general'] = {'small': f['small'], 'all_to_thread': all_to_thread, 'big': 0 if all_to_thread else len(big),
                        'fallback': 0 if all_to_thread else len(thread)}
    return e


# ---- builders -------------------------------------------------------------------------------------------------------------------
def stack(maps, step):
    """slices of a volume: map i carries its labels + i * step (step 0: the slices join along z)"""
    return np.stack([m + i * step for i, m in enumerate(maps)]).astype(np.int32)


def whole_rows(w, d):
    """one label across a whole row, three rows per slice"""
    one = (np.arange(3)[:, None] * np.ones((1, w), int)).astype(np.int32)
    return one if d == 1 else stack([one] * d, 3)


#: where a run ends and the next begins
EDGES = (61, 62, 63, 247, 248, 249)


def run_edges(d):
    """rows of 300: a run [0, b) and a run [b, 300) for every edge b; the slices of a volume carry the rows in reverse"""
    one = np.zeros((len(EDGES), 300), np.int32)
    for r, b in enumerate(EDGES):
        one[r, :b], one[r, b:] = 2 * r, 2 * r + 1
    return one if d == 1 else stack([one, one[::-1]][:d], 20)


def comb_up(h, w, d):
    """teeth in the even columns that join only through row 0 (h = 1: the row alone); a volume repeats it under other labels"""
    one = np.zeros((h, w), np.int32)
    one[0, :] = 1
    one[1:, ::2] = 1
    return one if d == 1 else stack([one] * d, 2)


def joined_behind(d, w=130):
    """slice 0 is one label; the runs of the slices behind it carry that label and touch one another only through slice 0"""
    vol = np.zeros((d, 2, w), np.int32)
    for z in range(1, d):
        vol[z, :, 59 + z:64 + z] = z                        # the gap crosses x = 62
        vol[z, :, 120:126] = 7 + z                          # ... and x = 124
        vol[z, 1, :] = 20 + z                               # the runs of row 0 do not meet in row 1 either
    return vol


def widths(w, h, d, seed):
    """blocks with a little salt on rows of w voxels"""
    one = [salted(h, w, 2, 50, 0.02, seed + z) for z in range(d)]
    return one[0] if d == 1 else stack(one, 0)


def stripes(d):
    """16 rows of 512: stripes four voxels wide in the first 256 columns (64 roots in that tile), two wide in the rest (128)"""
    x = np.arange(512)
    row = np.where(x < 256, x // 4, 64 + (x - 256) // 2)
    one = np.tile(row, (16, 1)).astype(np.int32)
    return one if d == 1 else stack([one] * d, 0)


def lattice(extra):
    """24 x 24 x 3 = 1728 voxels, one component with 144 = 1728 // 12 isolated voxels inside (slice 1, odd rows and columns),
    `extra` more in slice 0"""
    vol = np.zeros((3, 24, 24), np.int32)
    vol[1, 1::2, 1::2] = 1
    for i in range(extra):
        vol[0, 2, 2 + 2 * i] = 1
    return vol


def sliver_l(H, W, y0, x0, h, w, bs=16):
    """a one-voxel L (down, then right) with the tight bounding box h x w at (y0, x0) on blocks of bs x bs"""
    lab = blocks(H, W, bs, bs) + 1
    lab[y0:y0 + h, x0] = 0
    lab[y0 + h - 1, x0:x0 + w] = 0
    return lab


def wedge(k, long_side):
    """a filled k x long_side rectangle whose corner is its first voxel: the widest BFS level holds k cells"""
    lab = blocks(k + 76, long_side + 76, 200, 200) + 1         # (one kept component around it)
    lab[6:6 + k, 6:6 + long_side] = 0
    return lab


def corners():
    """components of 1, 2 and min_size - 1 = 4 voxels in the corners and on the edges and faces of a 6 x 8 x 10 volume"""
    vol = (np.arange(6)[:, None, None] // 3 * 4 + blocks(8, 10, 4, 5)[None]).astype(np.int32)
    vol[0, 0:2, 0] = 50; vol[0, 0, 1] = 50; vol[1, 0, 0] = 50       # the first voxel of the volume, 4 voxels over three axes
    vol[5, 7, 9] = 51                                                # the last voxel, alone
    vol[5, 7, 0:2] = 52                                              # a corner, 2 voxels
    vol[0, 7, 9] = 53; vol[1, 7, 9] = 53                             # a corner, 2 voxels along z
    vol[3, 0, 3:7] = 54                                              # an edge of a slice, 4 voxels
    vol[2:4, 4, 9] = 55                                              # a face, 2 voxels along z
    vol[0, 3, 4] = 56                                                # a face, alone
    vol[5, 2:4, 5] = 57
    return vol


def sizes_exact(w=51):
    """components of max_size + 1, max_size, 1, max_size - 1 and 2 = min_size voxels with max_size = w - 1"""
    lab = np.zeros((3, w), np.int32)
    lab[0, :] = 1
    lab[1, :w - 1], lab[1, w - 1:] = 2, 3
    lab[2, :w - 2], lab[2, w - 2:] = 4, 5
    return lab


def l_shape():
    """a one-voxel L of 3 * 40 + 5 voxels on blocks of 25: with max_size 40 its left-over is oversize twice more"""
    lab = blocks(70, 75, 5, 5) + 1
    lab[3:63, 4] = 0
    lab[62, 4:70] = 0
    return lab


def touching():
    """two components of 60 voxels side by side, max_size 40"""
    lab = blocks(12, 20, 3, 5) + 2
    lab[2:8, 0:10], lab[2:8, 10:20] = 0, 1
    return lab


def kept_blocks(h, w):
    return blocks(h, w, 2, 4)


def closed_form_blocks(lab, start_label):
    """every 4 x 2 block is kept at min_size = 8 and numbered in raster order"""
    return lab.astype(np.int64) + start_label


def column_stripes():
    """500 one-pixel columns of 1025 rows: every kept root lies in row 0, that is in bucket 0 of the 1024 of kept_rank_block.
    (All roots in one bucket AND more than KR_SORTED_LDS = 2048 of them needs 2049 * 1024 pixels: beyond half a megapixel.)"""
    return np.tile(np.arange(500, dtype=np.int32), (1025, 1))


def scan_line(n, along_z):
    row = blocks(1, n, 1, 37)
    return row.reshape(n, 1, 1) if along_z else row.reshape(1, 1, n)


def _case(name, make, min_size, max_size, force_general=False, closed_form=None, **must):
    return {'name': name, 'make': make, 'min_size': min_size, 'max_size': max_size, 'force_general': force_general,
            'closed_form': closed_form, 'must': must}


def _table():
    t = []
    # ---- row segments: volumes, and single slices with the general path forced
    for d in (2, 1):
        fg = d == 1
        sfx = '_d%d' % d
        for w in (62, 63, 124, 125, 248, 249, 497):
            t.append(_case('row_w%d%s' % (w, sfx), lambda w=w, d=d: whole_rows(w, d), w, 10 * w, fg, path='general', kept=3 * d))
        t.append(_case('run_edges' + sfx, lambda d=d: run_edges(d), 62, 1000, fg, path='general', small=4 * d))
        for h in (1, 3, 4, 5, 17):
            t.append(_case('comb_up_h%d%s' % (h, sfx), lambda h=h, d=d: comb_up(h, 130, d), 4, 100000, fg, path='general'))
        for w, h, dd in ((249, 3, 3), (250, 3, 3), (251, 3, 3), (250, 2, 2), (252, 3, 2)):
            dd = 1 if d == 1 else dd
            t.append(_case('width_%dx%d%s' % (w, h, sfx), lambda w=w, h=h, dd=dd: widths(w, h, dd, w), 30, 4000, fg, path='general'))
    for d in (2, 3):
        t.append(_case('joined_behind_d%d' % d, lambda d=d: joined_behind(d), 100, 100000, path='general'))
    # ---- the LDS size table of k_ccl_flatten_sizes_rows
    for d in (2, 1):
        t.append(_case('stripes_d%d' % d, lambda d=d: stripes(d), 64 * d, 100000, d == 1, path='general', hash_tiles=(64, 65)))
    t.append(_case('hash_noise', lambda: np.random.RandomState(5).randint(0, 6, (2, 32, 256)).astype(np.int32), 20, 400,
                   path='general', hash_min=200))
    # ---- the bounding-box table
    t.append(_case('table_full', lambda: lattice(0), 2, 100000, path='general', small_is=144, all_to_thread=False))
    t.append(_case('table_over', lambda: lattice(1), 2, 100000, path='general', small_is=145, all_to_thread=True))
    # ---- order, wave BFS and thread BFS of the general path (single slices forced there, and a volume)
    for cells, (h, w) in ((1024, (30, 30)), (1025, (23, 39)), (8192, (62, 126)), (8193, (1, 2729))):
        # (the sliver is small, the blocks around it are kept: one block for the longest sliver)
        t.append(_case('general_box_%d' % cells, lambda h=h, w=w: sliver_l(h + 12, w + 12, 6, 6, h, w, 16 if w < 2000 else 4096), h + w,
                       100000, True,
                       path='general', box_general=cells, big=int(cells > 1024), thread=int(cells > 8192)))
    t.append(_case('corners', corners, 5, 100000, path='general'))
    # ---- k_kept_scan blocks
    for n in (1, 3, 4095, 4096, 4097, 8193):
        t.append(_case('scan_x_%d' % n, lambda n=n: scan_line(n, False), 20, 100, True, path='general'))
        t.append(_case('scan_z_%d' % n, lambda n=n: scan_line(n, True), 20, 100, n == 1, path='general'))
    # ---- oversize rounds
    t.append(_case('sizes_exact', sizes_exact, 2, 50, path='general', rounds=1))
    t.append(_case('sizes_exact_d2', lambda: stack([sizes_exact()] * 2, 10), 2, 50, path='general', rounds=1))
    t.append(_case('sizes_exact_d5', lambda: stack([sizes_exact()] * 5, 0), 2, 50, path='general'))
    t.append(_case('l_shape', l_shape, 10, 40, path='general', rounds=3))
    t.append(_case('l_shape_d2', lambda: stack([l_shape()] * 2, 1000), 10, 40, path='general', rounds=3))
    t.append(_case('touching', touching, 10, 40, path='general', rounds=1))
    t.append(_case('touching_d5', lambda: stack([touching()] * 5, 100), 10, 40, path='general', rounds=1))
    t.append(_case('max_size_is_n', lambda: blocks(8, 12, 4, 4), 10, 96, path='tile', rounds=0))
    t.append(_case('max_size_is_n_d2', lambda: stack([blocks(8, 12, 4, 4)] * 2, 0), 10, 192, path='general', rounds=0))
    t.append(_case('min_size_beyond_n', lambda: blocks(8, 12, 4, 4), 97, 1000, path='tile', kept=0))
    t.append(_case('min_size_beyond_n_d2', lambda: stack([blocks(8, 12, 4, 4)] * 2, 6), 193, 2000, path='general', kept=0))
    # ---- slots of a tile (2-D path)
    t.append(_case('slots_64x32', lambda: kept_blocks(32, 64), 8, 1000, closed_form=closed_form_blocks, path='tile', tile_local=256))
    t.append(_case('slots_128x64', lambda: kept_blocks(64, 128), 8, 1000, closed_form=closed_form_blocks, path='tile', tile_local=256))

    def one_more():
        lab = kept_blocks(64, 128)
        lab[40, 70] = 5000                                  # splits nothing: the corner pixel of a block, which stays connected
        return lab
    t.append(_case('slots_257', one_more, 7, 1000, path='general', tile_local=257))
    t.append(_case('slots_65x33', lambda: kept_blocks(33, 65), 4, 1000, path='tile'))
    t.append(_case('slots_63x31', lambda: kept_blocks(31, 63), 4, 1000, path='tile'))
    # ---- ranking of the kept roots (closed form; only these are larger than the restatement can take)
    for w, h, path in ((128, 128, 'tile'), (128, 130, 'tile'), (1024, 512, 'tile'), (1024, 514, 'general')):
        t.append(_case('kept_%d' % (w * h // 8), lambda w=w, h=h: kept_blocks(h, w), 8, 1000, closed_form=closed_form_blocks,
                       path=path, kept=w * h // 8))
    t.append(_case('kept_bucket0', column_stripes, 1025, 100000, closed_form=lambda lab, s: lab.astype(np.int64) + s, path='tile',
                   kept=500))
    # ---- the three small-component stages of the tile path
    for cells, (h, w) in ((16384, (124, 124)), (16385, (109, 141)), (131072, (252, 508)), (131075, (241, 531))):
        # (131073 = 3 * 43691 and 131074 = 2 * 65537 are no product of two sides >= 5: 131075 = 245 * 535 is the first box beyond)
        t.append(_case('tile_box_%d' % cells, lambda h=h, w=w: sliver_l(h + 8, w + 8, 4, 4, h, w, 64), 1000, 100000,
                       path='general' if cells > 131072 else 'tile', box_tile=cells, fb=int(cells > 16384), fb2=int(cells > 131072)))
    for k in (64, 65):
        t.append(_case('wedge_%d' % k, lambda k=k: wedge(k, 70), 5000, 100000, path='tile', widest=k, fb=int(k > 64), fb2=int(k > 64)))
        # (a comb's BFS walks along the spine: its widest level is about its depth, whatever the number of teeth)
        t.append(_case('comb_teeth_%d' % k, lambda k=k: comb(64, 400, 4, k, 7), 1000, 100000, path='tile', fb=0, fb2=0))
    # ---- the crafted maps of the golden file, with their stages
    for name, (_, mn, mx) in GEN.CASES.items():
        if name != 'volume':
            t.append(_case(name, lambda name=name: GEN.make(name), mn, mx))
    return t


TABLE = _table()
BY_NAME = {c['name']: c for c in TABLE}
assert len(BY_NAME) == len(TABLE)
#: A BFS level of 2 048 / 2 049 cells inside a box of at most 8 192 cells (k_small_bfs_wave<8192, 2048, .>) is not built: level L
#: of a BFS on the grid holds at most 4 L^2 + 2 cells, all within L steps of the seed, and the seed is the first voxel of its
#: component in raster order, so half of that shell at best -- 2 048 cells need L >= 32 and a box that holds a half shell of that
#: radius, about 65 x 65 x 33 cells.  A comb does not help: its BFS walks along the spine (comb_teeth_64: widest level 5).
#: more than CONN_FB_CAP = 4096 components in the second list: every one of them needs a bounding box of more than 16 384 cells
#: (or a frontier of more than 64), hence at least 124 + 124 - 1 pixels of its own inside a box no other such component's pixels
#: may fill up; 4 097 of them need > 10^6 pixels of slivers alone.  Not built.
