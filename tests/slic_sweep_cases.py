"""Cases of the 2-D SLIC sweeps (csrc/slic.hip) at their tile, grid, tie and dead-centroid edges, and the facts each case claims.

A case is ``(image, n_segments, compactness, sigma, normalize, slic_zero, max_candidates)`` (plus ``start_label`` where a case is
about it); images are built from seeds in numpy.  Besides the cases this file restates, from ``oracle.regular_grid`` and
``oracle.grid_centroids``, what the launcher derives from the sizes -- each helper names the lines it restates -- so that
tests/test_slic_sweep_cases_host.py can hold every claim ("this case reaches the full scan of k_slic_bin", "these pixels lie in no
window") against the oracle on the CPU: a case that stops reaching its edge fails there, not silently on the device.
tests/test_gpu_slic_sweeps.py runs the cases on the device.

The oracle (``orc_slic_iterate``) updates its centroid table after EVERY sweep, the last one included; the device does not update
after its last sweep.  The table that goes INTO sweep ``m`` (1-based) is therefore the oracle's table after a run of ``m - 1``
sweeps (the grid with colour 0 for ``m == 1``): :func:`table_into`.

Where the cases differ from the list they were drawn up from:

* K > 4096: a second case at 832 x 832, n_segments 4761 (step 12), where a tile holds at most 64 candidates without any centroid
  dying, does not reach the full scan of k_slic_bin: `local` turns false there only at a drift of 76 pixels.  Tried at that size:
  uint8 noise at compactness 0.05 (drift 40 after ten sweeps), and the two-colour image that makes 272 x 272 work, with cells of
  12 pixels at compactness 0.05 (3187 centroids die, drift 43) and cells of 24 at 0.02 (2485 die, drift 42).  ``bigk-272x272-step4`` is the smallest case found that reaches both edges: two thirds
  of its centroids die in sweep 2, which leaves tiles of 15 to 64 candidates, some with an index >= 4096, while the whole table is
  scanned from sweep 4 on.
* exact ties: a constant image ties only going into sweep 1 (on the grid).  After the first update the first column and row of
  cells are 9 pixels wide and the others 8, so no pixel lies half way between two centroids: the constant image with two corner
  pixels keeps a handful of tied pixels into sweep 2 and none later, the plain constant image none.  Stripes and a checkerboard
  at 96 x 128 with step 8 lose their ties the same way; the two layouts used (45 x 63 step 8, 72 x 90 step 5 phase 2), found by a
  search over sizes, steps and phases, keep more than 1 % of their pixels on exact ties going into sweeps 2 and 3.  The
  checkerboard also runs with ``normalize=0`` (same planes: its extremes are 0 and 1), which is the exact fp64 path of k_slic_assign.
* the child processes of the shipped variants (``VARIANT_CASES``) run the 72 x 90 checkerboard as their tie case, because no
  96 x 128 image keeps its ties.
* pixels that no window covers going into a sweep >= 2: random images do not get there (a centroid keeps pixels within two steps
  of itself, so its next window reaches about as far: 491 of the 768 centroids of ``massdeath-96x128`` die in sweep 2 and every
  pixel stays covered).  The two ``uncovered-*`` images are one-row images of seven palette colours found by a hill climb on
  "left edge of the leftmost live window" over the oracle's tables, and are kept as their palette indices: the first centroids
  die, the one that owns pixel 0 is pulled right by the rest of its pixels, and pixel 0 lies in no window going into sweep 6
  (1 x 96, step 6) resp. sweep 8 (1 x 192, step 16).  It keeps its previous label there.  Both run with both start labels."""
import zlib

import numpy as np

from oracle import oracle as orc

TILE_X, TILE_Y, MAXC = 64, 32, 64          # slic.h: SLIC_TILE_X, SLIC_TILE_Y, SLIC_MAXC
BIN_MAX_K_LDS, BIN_LOCAL_MAX = 4096, 512   # slic.hip: k_slic_bin
SWEEPS = (1, 2, 3, 10)                     # max_iter of the device tests
ORACLE_SWEEPS = (1, 2, 3, 9, 10)           # ... and the runs their tables come from


# ---- what the launcher derives ---------------------------------------------------------------------------------------------
def geometry(shape, n_segments, compactness, normalize, max_candidates=0):
    """api_image2d.hip slic_geometry (lines 13-50): grid starts and steps, K, step_y / step_x, spatial weight, M, kappa, fast32"""
    H, W = shape
    (_, _), (y0, dy), (x0, dx) = orc.regular_grid((1, H, W), n_segments)
    ys = np.arange(y0, H, dy if dy is not None else 1)
    xs = np.arange(x0, W, dx if dx is not None else 1)
    K = len(ys) * len(xs)
    cent, fsteps = orc.grid_centroids((1, H, W), n_segments)
    assert cent.shape[0] == K
    step = np.float32(max(fsteps))                                                  # line 27: float step
    (_, _), (_, sy), (_, sx) = orc.regular_grid((1, H, W), K)                        # lines 28-33: the steps of _slic.pyx
    step_y, step_x = int(sy) if sy is not None else 1, int(sx) if sx is not None else 1
    sw = 1.0 / (float(step) * float(step))                                          # line 34
    u = 2.0 ** -24                                                                  # lines 40-46
    M = 108.0 * (1.0 / compactness) * 1.001
    R = 2.0 * max(step_y, step_x) + 1.0
    E = 3.0 * R + 64.0
    G = np.sqrt(2.0 * sw) * E + np.sqrt(3.0) * 4.0 * M + 16.0
    kappa = np.float32(2.0 * u * (G + 1.0) * 1.0001)
    fast32 = bool(normalize != 0 and max_candidates >= 0 and kappa < np.float32(1e-2) and M < 4096.0)
    return dict(H=H, W=W, K=K, ny=len(ys), nx=len(xs), grid_y0=int(y0), grid_x0=int(x0),
                grid_dy=int(dy) if dy is not None else 1, grid_dx=int(dx) if dx is not None else 1,      # regular_grid3: `all` has step 1
                step_y=step_y, step_x=step_x, step=float(step), sw=sw, M=M, kappa=kappa, fast32=fast32,
                n_tiles=-(-W // TILE_X) * -(-H // TILE_Y), tiles_x=-(-W // TILE_X))


def grid_table(geo):
    """k_centroid_init (slic.hip lines 59-65): K rows (cy, cx, 0, 0, 0), k = iy * nx + ix"""
    k = np.arange(geo['K'])
    t = np.zeros((geo['K'], 5))
    t[:, 0] = geo['grid_y0'] + (k // geo['nx']) * geo['grid_dy']
    t[:, 1] = geo['grid_x0'] + (k % geo['nx']) * geo['grid_dx']
    return t


def live_rows(table):
    return ~np.isnan(table[:, 0])


def search_windows(table, geo):
    """search_window (slic.hip lines 20-36) for every row: K x 4 int32 (y0, y1, x0, x1); a dead row (NaN) has the empty window of
    centroid_finalize_one (line 84)"""
    live = live_rows(table)
    cy, cx = np.where(live, table[:, 0], 0.0), np.where(live, table[:, 1], 0.0)
    out = np.zeros((len(table), 4), dtype=np.int32)
    for col, c, st, size in ((0, cy, geo['step_y'], geo['H']), (2, cx, geo['step_x'], geo['W'])):
        a = c - float(2 * st)
        out[:, col] = np.trunc(np.where(a > 0, a, 0.0))
        a = (c + float(2 * st)) + 1.0
        out[:, col + 1] = np.trunc(np.where(a < size, a, float(size)))
    out[~live] = 0
    return out


def grid_covers(geo):
    """launch_slic_iterations (slic.hip lines 1241-1247): every pixel lies in the window of its nearest grid node"""
    reach_y = max(geo['grid_y0'], geo['H'] - 1 - (geo['grid_y0'] + (geo['ny'] - 1) * geo['grid_dy']), geo['grid_dy'] // 2 + 1)
    reach_x = max(geo['grid_x0'], geo['W'] - 1 - (geo['grid_x0'] + (geo['nx'] - 1) * geo['grid_dx']), geo['grid_dx'] // 2 + 1)
    return reach_y <= 2 * geo['step_y'] and reach_x <= 2 * geo['step_x']


def drift_of(table, geo):
    """centroid_finalize_one (slic.hip lines 96-99): the largest distance, per axis and rounded up, of a live centroid from its
    grid node -- what the k_slic_bin of the sweep this table goes into reads from its drift slot (0 for the grid itself)"""
    live = live_rows(table)
    if not live.any():
        return 0
    g = grid_table(geo)
    d = np.maximum(np.abs(table[live, 0] - g[live, 0]), np.abs(table[live, 1] - g[live, 1]))
    return int(np.ceil(d.max()))


def local_predicate(geo, drift):
    """`local` of k_slic_bin (slic.hip lines 140-142): only the grid nodes within reach of a tile are looked at; false: the whole
    table is scanned (through the LDS copy of the first BIN_MAX_K_LDS windows, s.win[k] behind it)"""
    reach_y, reach_x = 2 * geo['step_y'] + 1 + drift, 2 * geo['step_x'] + 1 + drift
    return (geo['grid_dy'] > 0 and geo['grid_dx'] > 0 and
            (2 * reach_y + TILE_Y + 2 * geo['grid_dy']) * (2 * reach_x + TILE_X + 2 * geo['grid_dx']) <=
            BIN_LOCAL_MAX * geo['grid_dy'] * geo['grid_dx'])


def tile_candidates(windows, geo):
    """the hit test of k_slic_bin (slic.hip line 178) for every 64 x 32 tile: list of index arrays, ascending k"""
    out = []
    for tile in range(geo['n_tiles']):
        tx0, ty0 = (tile % geo['tiles_x']) * TILE_X, (tile // geo['tiles_x']) * TILE_Y
        tx1, ty1 = min(tx0 + TILE_X, geo['W']), min(ty0 + TILE_Y, geo['H'])
        hit = (windows[:, 0] < ty1) & (windows[:, 1] > ty0) & (windows[:, 2] < tx1) & (windows[:, 3] > tx0)
        out.append(np.flatnonzero(hit))
    return out


def covered_mask(windows, shape):
    """pixels that lie in at least one window"""
    H, W = shape
    cov = np.zeros((H + 1, W + 1), dtype=np.int64)
    w = windows[(windows[:, 1] > windows[:, 0]) & (windows[:, 3] > windows[:, 2])]
    np.add.at(cov, (w[:, 0], w[:, 2]), 1)
    np.add.at(cov, (w[:, 1], w[:, 3]), 1)
    np.add.at(cov, (w[:, 0], w[:, 3]), -1)
    np.add.at(cov, (w[:, 1], w[:, 2]), -1)
    return cov.cumsum(0).cumsum(1)[:H, :W] > 0


def two_smallest(lab, table, geo):
    """per pixel the two smallest fp64 distances over the windows that cover it, in the operation order documented above
    k_slic_assign (slic.hip lines 279-281): (dy*dy + dx*dx) * sw; ((dL*dL) + da*da) + db*db; their sum.  numpy rounds every
    operation once (no fused multiply-add), like the contract"""
    H, W = geo['H'], geo['W']
    b1, b2 = np.full((H, W), np.inf), np.full((H, W), np.inf)
    win = search_windows(table, geo)
    for k in np.flatnonzero(live_rows(table)):
        y0, y1, x0, x1 = win[k]
        if y1 <= y0 or x1 <= x0:
            continue
        ty = (table[k, 0] - np.arange(y0, y1, dtype=np.float64))[:, None]
        tx = (table[k, 1] - np.arange(x0, x1, dtype=np.float64))[None, :]
        d = (ty * ty + tx * tx) * geo['sw']
        t0, t1, t2 = (lab[c, y0:y1, x0:x1] - table[k, 2 + c] for c in range(3))
        col = t0 * t0
        col = col + t1 * t1
        col = col + t2 * t2
        d = d + col
        s1, s2 = b1[y0:y1, x0:x1], b2[y0:y1, x0:x1]
        lt = d < s1
        s2[...] = np.where(lt, s1, np.minimum(s2, d))
        s1[...] = np.where(lt, d, s1)
    return b1, b2


# ---- the oracle ------------------------------------------------------------------------------------------------------------
def scaled(normalize, vmin, vmax):
    """imsegm_hip.h: minmax_normalize 1 = always, 0 = never, 2 = unless min == 0 and max == 1"""
    return normalize == 1 or (normalize == 2 and not (vmin == 0 and vmax == 1))


_ORACLE = {}


def oracle_run(c, max_iter):
    """(nearest H x W int32, table K x 5 after the update that follows sweep ``max_iter``, planes 3 x H x W) -- once per process,
    read-only; ``max_iter == 0``: the grid"""
    key = (c['id'], max_iter)
    if key not in _ORACLE:
        img = c['image']
        vmin, vmax = float(img.min()), float(img.max())
        norm = (vmin, vmax) if scaled(c['normalize'], vmin, vmax) else None
        _, info = orc.slic(np.array(img), c['n_segments'], c['compactness'], sigma=c['sigma'], normalize=norm, max_iter=max(max_iter, 1),
                           enforce_connectivity=False, return_internals=True, slic_zero=c['slic_zero'])
        geo = geometry_of(c)
        assert info['K'] == geo['K']
        if max_iter == 0:
            nearest, table = np.full(img.shape[:2], -1, dtype=np.int32), grid_table(geo)
        else:
            nearest, table = info['nearest'][0].astype(np.int32), np.array(info['segments'][:, 1:6])
        pre = info['pre'].reshape((3, ) + img.shape[:2])
        for a in (nearest, table, pre):
            a.setflags(write=False)
        _ORACLE[key] = nearest, table, pre
    return _ORACLE[key]


def table_into(c, sweep):
    """the centroid table that goes into sweep ``sweep`` (1-based): what the device holds after ``max_iter = sweep`` sweeps"""
    return oracle_run(c, sweep - 1)[1]


def geometry_of(c):
    return geometry(c['image'].shape[:2], c['n_segments'], c['compactness'], c['normalize'], c['max_candidates'])


def crc_of(nearest, rows, windows, live):
    """what a child process of the shipped-variant test prints: labels, live centroid rows and all windows in one CRC"""
    crc = zlib.crc32(np.ascontiguousarray(nearest, dtype=np.int32).tobytes())
    crc = zlib.crc32(np.ascontiguousarray(rows[live], dtype=np.float64).tobytes(), crc)
    return zlib.crc32(np.ascontiguousarray(windows, dtype=np.int32).tobytes(), crc)


# ---- images ----------------------------------------------------------------------------------------------------------------
def block_noise(shape, seed, block=3, levels=256):
    """uint8 colour noise in ``block`` x ``block`` blocks of one colour"""
    H, W = shape
    rng = np.random.default_rng(seed)
    small = rng.integers(0, levels, (-(-H // block), -(-W // block), 3)) * (255 // (levels - 1))
    return np.ascontiguousarray(np.kron(small, np.ones((block, block, 1), dtype=np.int64))[:H, :W].astype(np.uint8))


def ramp(shape):
    """smooth float64 ramp inside (0, 1), the three channels different"""
    H, W = shape
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    return np.ascontiguousarray(np.stack([0.1 + 0.8 * (0.6 * y / H + 0.3 * x / W + 0.1 * ch / 3.0) for ch in range(3)], axis=-1))


def piecewise(shape, seed):
    """float64 image of a few flat rectangles with a little noise, values in [0, 1] with both ends taken"""
    H, W = shape
    rng = np.random.default_rng(seed)
    img = np.zeros((H, W, 3))
    for _ in range(12):
        y0, x0 = rng.integers(0, H), rng.integers(0, W)
        img[y0:y0 + rng.integers(4, H), x0:x0 + rng.integers(4, W)] = rng.random(3)
    img = np.clip(img + 0.02 * rng.standard_normal(img.shape), 0.0, 1.0)
    img[0, 0], img[-1, -1] = 0.0, 1.0
    return np.ascontiguousarray(img)


def two_colour_cells(shape, seed, cell, flat_blocks=0):
    """uint8 noise of two colours whose mixing ratio is drawn per ``cell`` x ``cell`` square, optionally with blocks of flat colour.
    At low compactness the pixels of one colour all go to the few centroids within reach that hold most of that colour: the
    others lose every pixel (dead centroids), the winners wander, and holes open that no window covers"""
    H, W = shape
    rng = np.random.default_rng(seed)
    frac = np.kron(rng.random((-(-H // cell), -(-W // cell))), np.ones((cell, cell)))[:H, :W]
    pick = rng.random((H, W)) < frac
    img = np.where(pick[..., None], np.array([230, 40, 60]), np.array([30, 200, 120])).astype(np.uint8)
    for _ in range(flat_blocks):
        y0, x0 = rng.integers(0, max(H - 20, 1)), rng.integers(0, max(W - 28, 1))
        img[y0:y0 + 20, x0:x0 + 28] = rng.integers(0, 256, 3)
    return np.ascontiguousarray(img)


PALETTE = np.array([[128, 128, 128], [150, 150, 150], [230, 40, 60], [30, 200, 120], [20, 30, 220], [0, 0, 0], [255, 255, 255]], dtype=np.uint8)
UNCOVERED_1X96 = '126441326556606444111112463555441111111110133333111333333333363311333331333444564422234333335565'
UNCOVERED_1X192 = ('301241060465666263666364214520131444226136636111621420542031401101611155555542211233262223333333'
                   '354612213066200021635032265645130613332244444000000214301231500164340132251105533553111110554265')


def palette_row(indices):
    """one-row uint8 image from a string of PALETTE indices"""
    return np.ascontiguousarray(PALETTE[np.array([int(ch) for ch in indices])][None])


def constant_image(shape, corners):
    img = np.full(shape + (3, ), 0.5)
    if corners:
        img[0, 0], img[-1, -1] = 0.0, 1.0
    return img


def stripes(shape, period, phase=0):
    """horizontal stripes, ``period`` rows each way, float64 in {0.25, 0.75} with the ends 0 and 1 in two corners"""
    H, W = shape
    img = np.empty((H, W, 3))
    img[...] = np.where(((np.arange(H) + phase) // period) % 2 == 0, 0.25, 0.75)[:, None, None]
    img[0, 0], img[-1, -1] = 0.0, 1.0
    return img


def checkerboard(shape, period, phase=0):
    H, W = shape
    y, x = np.mgrid[0:H, 0:W]
    img = np.empty((H, W, 3))
    img[...] = np.where((((y + phase) // period) + ((x + phase) // period)) % 2 == 0, 0.25, 0.75)[..., None]
    img[0, 0], img[-1, -1] = 0.0, 1.0
    return img


# ---- the cases -------------------------------------------------------------------------------------------------------------
TILE_SIZES = ((1, 1), (1, 200), (200, 1), (7, 5), (15, 64), (16, 64), (17, 64), (31, 63), (32, 64), (33, 65), (96, 128))


def _case(cid, group, image, n_segments, compactness, sigma=0.0, normalize=2, slic_zero=False, max_candidates=0, start_label=0, **claims):
    image = np.ascontiguousarray(image)
    image.setflags(write=False)
    c = dict(id=cid, group=group, image=image, n_segments=int(n_segments), compactness=float(compactness), sigma=float(sigma),
             normalize=int(normalize), slic_zero=bool(slic_zero), max_candidates=int(max_candidates), start_label=int(start_label))
    c.update(claims)
    return c


def _build():
    out = []
    # tile geometry: images below one bin tile / one workgroup, one row, one column, one pixel into the next tile
    for (H, W) in TILE_SIZES:
        for n_seg in sorted({1, 2, 3, max(1, (H * W) // 64)}):
            out.append(_case('tile-noise-%dx%d-n%d' % (H, W, n_seg), 'tile', block_noise((H, W), 1000 + H * 7 + W), n_seg, 10.0, sigma=0.0))
            out.append(_case('tile-ramp-%dx%d-n%d' % (H, W, n_seg), 'tile', ramp((H, W)), n_seg, 0.5, sigma=1.0, normalize=1))
    # step 1 and candidate overflow: every pixel a centroid (regular_grid returns slice(None)); superpixels of 3 pixels
    for (H, W) in ((12, 20), (40, 70)):
        for mult in (1, 2):
            out.append(_case('step1-%dx%d-x%d' % (H, W, mult), 'overflow', block_noise((H, W), 2000 + H), mult * H * W, 1.0, sigma=1.0,
                             step_one=True, all_tiles_overflow=(H, W) == (40, 70)))
    out.append(_case('overflow-96x128-sp3', 'overflow', block_noise((96, 128), 2100), (96 * 128) // 9, 1.0, sigma=1.0, all_tiles_overflow=True))
    out.append(_case('lists-96x128-sp8', 'overflow', block_noise((96, 128), 2100), (96 * 128) // 64, 1.0, sigma=1.0, has_lists=True))
    out.append(_case('lists-96x128-sp8-maxcand3', 'overflow', block_noise((96, 128), 2100), (96 * 128) // 64, 1.0, sigma=1.0, max_candidates=3,
                     forced_overflow=True))
    # K > BIN_MAX_K_LDS on the full scan of k_slic_bin
    out.append(_case('bigk-272x272-step4', 'bigk', two_colour_cells((272, 272), 3001, 4), 4624, 0.05, sigma=0.0, big_k=True))
    # exact ties beyond sweep 1
    out.append(_case('tie-constant-96x128-exact', 'tie', constant_image((96, 128), False), 192, 1.0, sigma=0.0, normalize=0, tie_sweeps=(1, )))
    out.append(_case('tie-constant-96x128-corners', 'tie', constant_image((96, 128), True), 192, 1.0, sigma=0.0, normalize=2, tie_sweeps=(1, 2), fast32=True))
    # stripes and a checkerboard whose period is the grid step: on 96 x 128 with step 8 the ties are gone after sweep 2 (the first
    # column of cells is 9 pixels wide, the others 8: no pixel is half way between two centroids); these two layouts, found by a
    # search over sizes, steps and phases, keep more than 1 % of their pixels on exact ties going into sweeps 2 and 3
    out.append(_case('tie-stripes-45x63', 'tie', stripes((45, 63), 8), (45 * 63) // 64, 10.0, sigma=0.0, tie_sweeps=(2, 3), tie_fraction=0.01, fast32=True))
    out.append(_case('tie-checkerboard-72x90', 'tie', checkerboard((72, 90), 5, 2), (72 * 90) // 25, 1.0, sigma=0.0, tie_sweeps=(2, 3), tie_fraction=0.01,
                     fast32=True))
    out.append(_case('tie-checkerboard-72x90-exact', 'tie', checkerboard((72, 90), 5, 2), (72 * 90) // 25, 1.0, sigma=0.0, normalize=0,
                     tie_sweeps=(2, 3), tie_fraction=0.01))
    out.append(_case('tie-constant-33x65-corners', 'tie', constant_image((33, 65), True), 32, 1.0, sigma=0.0, tie_sweeps=(1, 2), fast32=True))
    # the fast32 switch: M = 108 / compactness * 1.001 on both sides of 4096, kappa on both sides of 1e-2
    pw = piecewise((64, 96), 4001)
    for comp, fast in ((0.02640, True), (0.02639, False), (0.00894, False), (0.00892, False), (0.09, True), (400.0, True)):
        out.append(_case('fast32-64x96-c%g' % comp, 'fast32', pw, 96, comp, sigma=1.0, fast32=fast))
    # colour scale
    wide = np.ascontiguousarray(np.random.default_rng(5001).random((40, 70, 3)) * 10.0 - 3.0)
    wide[0, 0, 0], wide[-1, -1, 2] = -3.0, 7.0
    for norm in (0, 1, 2):
        out.append(_case('scale-wide-40x70-norm%d' % norm, 'scale', wide, 40, 5.0, sigma=1.0, normalize=norm))
    for sigma in (0.0, 1.0):
        out.append(_case('scale-u8-40x70-sigma%g' % sigma, 'scale', block_noise((40, 70), 5002, block=2), 40, 8.0, sigma=sigma))
    # dead centroids and pixels no window covers
    dead = two_colour_cells((96, 128), 6001, 8, flat_blocks=3)
    out.append(_case('dead-96x128', 'dead', dead, 192, 0.05, sigma=0.0, dead=True))
    # (no case with a pixel that NO window covers going into a sweep >= 2 was found: a centroid keeps the pixels it was given, all of
    # them within two steps of it, so its next window still reaches about as far; 491 of the 768 centroids of this image die in sweep
    # 2 and every pixel stays covered.  The image runs with both start labels.)
    hole = two_colour_cells((96, 128), 6002, 4)
    for start in (0, 1):
        out.append(_case('massdeath-96x128-start%d' % start, 'dead', hole, 768, 0.05, sigma=0.0, start_label=start, dead=True))
    # pixels that no window covers (they keep their previous label), with both start labels
    for start in (0, 1):
        out.append(_case('uncovered-1x96-start%d' % start, 'uncovered', palette_row(UNCOVERED_1X96), 16, 0.02, sigma=0.0, start_label=start,
                         uncovered_into=6))
        out.append(_case('uncovered-1x192-start%d' % start, 'uncovered', palette_row(UNCOVERED_1X192), 12, 0.02, sigma=0.0, start_label=start,
                         uncovered_into=8))
    # SLICO
    out.append(_case('slico-tie-72x90', 'slico', checkerboard((72, 90), 5, 2), (72 * 90) // 25, 1.0, sigma=0.0, slic_zero=True))
    out.append(_case('slico-dead-96x128', 'slico', dead, 192, 0.05, sigma=0.0, slic_zero=True))
    out.append(_case('slico-noise-33x65', 'slico', block_noise((33, 65), 1000 + 33 * 7 + 65), 33, 10.0, sigma=0.0, slic_zero=True))
    return out


_CASES = None


def cases():
    global _CASES
    if _CASES is None:
        _CASES = _build()
        assert len({c['id'] for c in _CASES}) == len(_CASES)
    return _CASES


def case(cid):
    return next(c for c in cases() if c['id'] == cid)


#: what a child process of the shipped-variant test runs, and what goes through Batch2D in one call
VARIANT_CASES = ('tile-noise-33x65-n33', 'tie-checkerboard-72x90', 'dead-96x128')
