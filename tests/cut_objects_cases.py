"""Seeded inputs (``CASES``) and edge inputs built from plain arrays (``RUN_MAPS``, ``EDGE_CASES``) of the cut_object / cut_objects tests
(tests/test_cut_objects_reference_host.py, tests/test_gpu_cut_objects.py, tests/test_gpu_cut_objects_edges.py) and of
tests/golden/make_golden_cut_objects.py, which runs the reference's ``cut_object`` on the seeded ones and picks the seeds.  Ellipses are
painted with the package's own ``ellipse_pixels_host``; no scikit-image is needed.

A case is ``case(name, seed) -> dict(img, segm, labels, padding, use_mask, bg_color, allow_rotate)``: the reference is called once
per label with the boolean mask ``segm == label``.  ``kind`` of ``CASES``: 'fixed' inputs do not depend on the seed beyond the image
noise; 'seeded' ones are re-seeded by the generator until the reference's result is stable (see the generator)."""
import contextlib
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden', 'cut_objects.npz')


def _noise(rng, shape, channels):
    return rng.randint(0, 256, tuple(shape) + ((channels, ) if channels else ())).astype(np.uint8)


def _paint(segm, label, r, c, r_radius, c_radius, orientation):
    from pyimsegm_amd.ellipse_fitting import ellipse_pixels_host
    rr, cc = ellipse_pixels_host(r, c, r_radius, c_radius, orientation, segm.shape)
    segm[rr, cc] = label


def _three_ellipses(rng, shape=(61, 83)):
    segm = np.zeros(shape, dtype=np.int32)
    for label, (r, c) in enumerate(((17, 20), (40, 44), (20, 64)), 1):
        _paint(segm, label, r + rng.uniform(-2, 2), c + rng.uniform(-2, 2), rng.uniform(9, 13), rng.uniform(4, 6.5),
               rng.uniform(0.15, np.pi - 0.15))
    return segm


def _ellipses(channels, padding, use_mask, allow_rotate=True, bg_color=None):
    def make(seed):
        rng = np.random.RandomState(seed)
        segm = _three_ellipses(rng)
        return dict(img=_noise(rng, segm.shape, channels), segm=segm, labels=[1, 2, 3], padding=padding, use_mask=use_mask,
                    bg_color=bg_color, allow_rotate=allow_rotate)
    return make


def _doctest(kwargs, dtype):
    def make(seed):
        img = np.ones((10, 20), dtype=dtype)
        img[3:7, 4:16] = 2
        segm = np.zeros((10, 20), dtype=np.int32)
        segm[4:6, 5:15] = 1
        return dict(img=img, segm=segm, labels=[1], padding=2, use_mask=kwargs.get('use_mask', False), bg_color=None,
                    allow_rotate=kwargs.get('allow_rotate', True))
    return make


def _border(seed):
    """ellipses that leave the map on three sides: the shift brings zeros in and the crops reach beyond the turned frame"""
    rng = np.random.RandomState(seed)
    segm = np.zeros((61, 83), dtype=np.int32)
    _paint(segm, 1, 3 + rng.uniform(-1, 1), 30, 11, 5, rng.uniform(0.3, 1.2))
    _paint(segm, 2, 40, 80 + rng.uniform(-1, 1), 12, 6, rng.uniform(1.9, 2.8))
    _paint(segm, 3, 57 + rng.uniform(-1, 1), 4, 10, 4.5, rng.uniform(0.3, 1.2))
    return dict(img=_noise(rng, segm.shape, 3), segm=segm, labels=[1, 2, 3], padding=3, use_mask=False, bg_color=None, allow_rotate=True)


def _two_pieces(seed):
    """one label in two pieces (one region for regionprops), beside a second label"""
    rng = np.random.RandomState(seed)
    segm = np.zeros((61, 83), dtype=np.int32)
    _paint(segm, 5, 15, 18, 8, 4, rng.uniform(0.2, 1.3))
    _paint(segm, 5, 44, 60, 9, 5, rng.uniform(1.8, 2.9))
    _paint(segm, 2, 45, 20, 7, 4, rng.uniform(0.2, 2.9))
    return dict(img=_noise(rng, segm.shape, 3), segm=segm, labels=[2, 5], padding=2, use_mask=True, bg_color=None, allow_rotate=True)


def _axis_aligned(seed):
    """a level and an upright rectangle and a single row, centroids exact in binary: angles of exactly 0 and +-90 degrees"""
    rng = np.random.RandomState(seed)
    segm = np.zeros((40, 50), dtype=np.int32)
    segm[5:9, 6:26] = 1
    segm[14:36, 34:40] = 2
    segm[30, 4:21] = 3
    return dict(img=_noise(rng, segm.shape, 3), segm=segm, labels=[1, 2, 3], padding=1, use_mask=True, bg_color=(7, 8, 9), allow_rotate=True)


def _one_pixel(seed):
    rng = np.random.RandomState(seed)
    segm = np.zeros((21, 30), dtype=np.int32)
    segm[13, 22] = 4
    segm[0, 0] = 9
    return dict(img=_noise(rng, segm.shape, 0), segm=segm, labels=[4, 9], padding=2, use_mask=False, bg_color=None, allow_rotate=False)


def _sparse33(seed):
    """33 small tilted ellipses on a grid, label values with gaps and above 1000"""
    rng = np.random.RandomState(seed)
    segm = np.zeros((97, 155), dtype=np.int32)          # (odd: the canvas centre is no rounding tie)
    labels = sorted(rng.choice(np.arange(3, 5000), 33, replace=False).tolist())
    for k, label in enumerate(labels):
        r, c = 8 + 16 * (k // 7), 11 + 22 * (k % 7)
        _paint(segm, label, r + rng.uniform(-1, 1), c + rng.uniform(-1, 1), rng.uniform(7, 9.5), rng.uniform(2.5, 4.5),
               rng.uniform(0.15, np.pi - 0.15))
    return dict(img=_noise(rng, segm.shape, 3), segm=segm, labels=labels, padding=1, use_mask=False, bg_color=None, allow_rotate=True)


def _large(seed):
    """130 x 70: the object spans more than one tile of every kernel in both directions"""
    rng = np.random.RandomState(seed)
    segm = np.zeros((130, 70), dtype=np.int32)
    _paint(segm, 1, 64 + rng.uniform(-2, 2), 35 + rng.uniform(-2, 2), 55, 24, rng.uniform(0.2, 0.6))
    return dict(img=_noise(rng, segm.shape, 3), segm=segm, labels=[1], padding=4, use_mask=True, bg_color=None, allow_rotate=True)


#: name -> (kind, builder)
CASES = {
    'doctest_u8': ('fixed', _doctest({}, np.uint8)),
    'doctest_u8_mask': ('fixed', _doctest({'use_mask': True, 'allow_rotate': False}, np.uint8)),
    'rgb_p0': ('seeded', _ellipses(3, 0, False)),
    'rgb_p4_mask': ('seeded', _ellipses(3, 4, True)),
    'gray_p0_mask': ('seeded', _ellipses(0, 0, True)),
    'gray_p4': ('seeded', _ellipses(0, 4, False)),
    'rgba_p4_mask_bg': ('seeded', _ellipses(4, 4, True, bg_color=(1, 2, 3, 4))),
    'rgb_p60_mask': ('seeded', _ellipses(3, 60, True)),          # the crop is the whole canvas, corners outside the turned frame included
    'no_rotate': ('seeded', _ellipses(3, 4, True, allow_rotate=False)),
    'border': ('seeded', _border),
    'two_pieces': ('seeded', _two_pieces),
    'axis_aligned': ('fixed', _axis_aligned),
    'one_pixel': ('fixed', _one_pixel),
    'sparse33': ('seeded', _sparse33),
    'large': ('seeded', _large),
}

#: cases whose MASK is handed over as int64 (host statement only): the doctest's own dtypes, and a turned object under use_mask
INT_MASK_CASES = {
    'doctest_int': ('fixed', _doctest({}, np.int64)),
    'doctest_int_mask': ('fixed', _doctest({'use_mask': True, 'allow_rotate': False}, np.int64)),
    'int_mask_turned': ('seeded', _ellipses(3, 60, True)),
}


def case(name, seed):
    table = CASES if name in CASES else INT_MASK_CASES
    return table[name][1](int(seed))


def masks_of(name, inputs):
    """the masks the reference is called with, one per label: boolean, or int64 for the INT_MASK_CASES"""
    for label in inputs['labels']:
        mask = inputs['segm'] == label
        yield label, (mask.astype(np.int64) if name in INT_MASK_CASES else mask)


def load_golden():
    return np.load(GOLDEN, allow_pickle=False)


def golden_crops(golden, name, count):
    return [golden['%s_crop%d' % (name, k)] for k in range(count)]


# ------------------------------------------------------------------------------------------------
# edge cases from plain arrays: no seed, no generator, no golden file -- the expectations are int64 numpy sums and scipy's own
# ``ndimage.shift`` / ``ndimage.rotate``, evaluated in the tests
# ------------------------------------------------------------------------------------------------

#: the run rule of k_cut_moments / ca_runs / k_ca_sizes: a wave holds 64 consecutive pixels of a row, a workgroup 256
WAVE, CHUNK = 64, 256
RUN_WIDTHS = (64, 65, 128, 256, 257, 320, 513)
#: the maps hold the ids 0 .. 3 (for ``center_levels``: background and the labels 1 .. 3); for cutting an id stands for one of these
#: values -- a negative one, 0 and the largest int32 are listed, the id 3 is a value that is NOT in the list
RUN_CUT_VALUES = np.array([0, -3, 2 ** 31 - 1, 5], dtype=np.int32)
RUN_UNLISTED_ID = 3


def _run_whole(width):
    return np.full((3, width), 2, dtype=np.int32)


def _run_alternate(width):
    rows, cols = np.indices((4, width))
    return (1 + (rows + cols) % 2).astype(np.int32)


def _run_exact(width):
    """runs of exactly 64 and 256 pixels from column 0 and from column 1, where the row is long enough"""
    seg = np.zeros((4, width), dtype=np.int32)
    for row, (start, length) in enumerate(((0, 64), (1, 64), (0, 256), (1, 256))):
        if start + length <= width:
            seg[row, start:start + length] = 1
    return seg


def _run_to_end(width):
    seg = np.zeros((3, width), dtype=np.int32)
    for row, start in enumerate((63, 255, 319)):
        seg[row, start:] = 2
    return seg


def _run_pixel63(width):
    seg = np.zeros((3, width), dtype=np.int32)
    seg[1, 63] = 1
    return seg


def _run_unlisted_between(width):
    seg = np.zeros((3, width), dtype=np.int32)
    seg[:, 3:13], seg[:, 13:23], seg[:, 23:33] = 1, RUN_UNLISTED_ID, 2
    seg[2, 13:23] = 0
    return seg


def _run_full_row(width):
    seg = (2 * ((np.indices((5, width))[1] // 7) % 2)).astype(np.int32)
    seg[2, :] = 1
    return seg


def _run_corner(width):
    seg = np.full((6, width), 1, dtype=np.int32)
    seg[5, width - 1] = 2
    return seg


RUN_LAYOUTS = {'whole': _run_whole, 'alternate': _run_alternate, 'exact': _run_exact, 'to_end': _run_to_end, 'pixel63': _run_pixel63,
               'unlisted_between': _run_unlisted_between, 'full_row': _run_full_row, 'corner': _run_corner}
#: (width, layout) -> builder of the id map
RUN_MAPS = {(width, layout): (lambda w=width, f=builder: f(w)) for width in RUN_WIDTHS for layout, builder in RUN_LAYOUTS.items()}


def run_map(width, layout):
    return RUN_MAPS[(width, layout)]()


def run_branches(seg, listed=None):
    """which branches of the run rule the map reaches, by the rule restated row by row: a lane opens a run where its value differs
    from its left neighbour's or where a wave begins.  ``listed``: the ids whose runs a kernel adds (None: all)."""
    height, width = seg.shape
    reached = set()
    if -(-width // CHUNK) > 1:
        reached.add('chunks > 1')
    if width % WAVE == 0:
        reached.add('no invalid lane')
    if width % CHUNK == 0:
        reached.add('no invalid lane in a workgroup')
    for row in seg:
        for start in range(0, width, WAVE):
            wave = row[start:start + WAVE]
            heads = [0] + [i for i in range(1, len(wave)) if wave[i] != wave[i - 1]]
            if len(heads) == WAVE:
                reached.add('64 heads')
            if WAVE - 1 in heads:
                reached.add('head at lane 63')
            if len(wave) == WAVE and heads[-1] == WAVE - 1 and start + WAVE == width:
                reached.add('head at lane 63, last of the row')
            if len(heads) == 1 and len(wave) == WAVE and start + WAVE < width and row[start + WAVE] == wave[0]:
                reached.add('run of 64 goes on in the next ' + ('workgroup' if (start + WAVE) % CHUNK == 0 else 'wave'))
            if listed is not None:
                ids = [wave[i] for i in heads]
                if any(ids[i] not in listed and ids[i - 1] in listed and ids[i + 1] in listed for i in range(1, len(ids) - 1)):
                    reached.add('unlisted between listed')
    return reached


#: what every layout has to reach, at the widths named (None: at every width)
RUN_REACH = {
    'whole': [('run of 64 goes on in the next wave', (128, 256, 257, 320, 513)), ('run of 64 goes on in the next workgroup', (257, 320, 513))],
    'alternate': [('64 heads', None), ('head at lane 63', None), ('head at lane 63, last of the row', (64, 128, 256))],
    'exact': [('run of 64 goes on in the next wave', (128, 256, 257, 320, 513)), ('run of 64 goes on in the next workgroup', (257, 320, 513))],
    'to_end': [('head at lane 63', None), ('head at lane 63, last of the row', (64, )), ('run of 64 goes on in the next workgroup', (513, ))],
    'pixel63': [('head at lane 63', None), ('head at lane 63, last of the row', (64, ))],
    'unlisted_between': [('unlisted between listed', None)],
    'full_row': [('run of 64 goes on in the next wave', (128, 256, 257, 320, 513))],
    'corner': [('head at lane 63, last of the row', (64, 128, 256))],
}
RUN_REACH_ALWAYS = [('chunks > 1', (257, 320, 513)), ('no invalid lane', (64, 128, 256, 320)), ('no invalid lane in a workgroup', (256, ))]


def run_cut_inputs(width, layout):
    """the id map as a map of ``RUN_CUT_VALUES`` with a one-channel image: (img, segm, listed labels ascending, listed ids)"""
    ids = run_map(width, layout)
    segm = RUN_CUT_VALUES[ids]
    listed_ids = [i for i in np.unique(ids).tolist() if i != RUN_UNLISTED_ID]
    labels = sorted(int(RUN_CUT_VALUES[i]) for i in listed_ids)
    img = ((np.arange(ids.size, dtype=np.int64) * 37 + 11) % 251).astype(np.uint8).reshape(ids.shape)
    return img, segm, labels, listed_ids


@contextlib.contextmanager
def orientation_forced(orientation):
    """inside: ``data_io._cut_geometry`` -- still the one place the geometry is formed -- is handed ``orientation`` (radians) for every
    object, which reaches the turns no region's own orientation gives (it lies in (-pi / 2, pi / 2]: turns of [0, 180) degrees).
    None: nothing is changed."""
    from pyimsegm_amd.utilities import data_io
    if orientation is None:
        yield
        return
    saved = data_io._orientation
    data_io._orientation = lambda moments: orientation
    try:
        yield
    finally:
        data_io._orientation = saved


#: turn in degrees (what ``ndimage.rotate`` is handed) -> the orientation that gives it; None: the object's own
TURNS = {0: None, 90: None, -90: np.pi, 180: -np.pi / 2}


def _frame(shape, boxes, padding, turn, allow_rotate=True):
    segm = np.zeros(shape, dtype=np.int32)
    for label, (r0, r1, c0, c1) in enumerate(boxes, 1):
        segm[r0:r1, c0:c1] = label
    return dict(segm=segm, labels=list(range(1, len(boxes) + 1)), padding=padding, turn=turn, allow_rotate=allow_rotate)


def _edge_frames():
    """level and upright rectangles with even sides (centroids at k + 0.5 on both axes), a single row and a single column, on
    frames with an even and an odd side: (name, frame)"""
    out = {}
    for shape in ((20, 24), (20, 25), (21, 24)):
        tag = '%dx%d' % shape
        level = [(3, 7, 2, 12), (12, 13, 4, 20)]              # 4 x 10 at (4.5, 6.5); the row 12, columns 4 .. 19
        upright = [(2, 14, 15, 19), (5, 17, 3, 4)]            # 12 x 4 at (7.5, 16.5); the column 3, rows 5 .. 16
        out['level_%s' % tag] = _frame(shape, level, 1, 0)
        out['upright_%s' % tag] = _frame(shape, upright, 1, 90)
        out['level_%s_back' % tag] = _frame(shape, level, 2, 180)
        out['upright_%s_down' % tag] = _frame(shape, upright, 0, -90)
    return out


def _all_borders(shape=(20, 24)):
    """one object that touches all four borders: the frame without its corners"""
    segm = np.ones(shape, dtype=np.int32)
    segm[0, 0] = segm[0, -1] = segm[-1, 0] = segm[-1, -1] = 0
    return dict(segm=segm, labels=[1], padding=2, turn=0, allow_rotate=True)


def _tile_crop(width, height):
    """a level rectangle of width x height pixels, padding 0: the crop is that rectangle -- 64 x 16 is one tile of k_cut_write"""
    shape = (height + 8, width + 12)                     # (both shifts are -1.5)
    return dict(_frame(shape, [(3, 3 + height, 5, 5 + width)], 0, 0), crop=(height, width))


EDGE_CASES = dict(_edge_frames())
EDGE_CASES['all_borders'] = _all_borders()
EDGE_CASES['all_borders_back'] = dict(_all_borders((21, 24)), turn=180)
for _w, _h in ((64, 16), (65, 17), (129, 33)):
    EDGE_CASES['crop_%dx%d' % (_w, _h)] = _tile_crop(_w, _h)
    EDGE_CASES['crop_%dx%d_fixed' % (_w, _h)] = dict(_tile_crop(_w, _h), allow_rotate=False)

#: (tag, image shape suffix): one channel as H x W and as H x W x 1, then 2, 3 and 4 channels
EDGE_CHANNELS = (('gray', None), ('c1', 1), ('c2', 2), ('c3', 3), ('c4', 4))
#: a background whose bytes all differ
EDGE_BG = (201, 17, 94, 153)


def edge_image(shape, channels):
    """every byte of the image is a function of its place: no two neighbours, rows or channels alike"""
    rows, cols = np.indices(shape)
    planes = [((rows * 29 + cols * 13 + ch * 71 + 5) % 199 + 1).astype(np.uint8) for ch in range(channels or 1)]
    return planes[0] if channels is None else np.stack(planes, axis=2)


def edge_variants(name):
    """the case with every image layout, ``use_mask`` on and off: dicts of the keys of ``case`` plus ``turn``"""
    base = EDGE_CASES[name]
    for tag, channels in EDGE_CHANNELS:
        bg = EDGE_BG[0] if channels is None else EDGE_BG[:channels]
        for use_mask in (False, True):
            yield '%s-%s' % (tag, 'mask' if use_mask else 'all'), dict(base, img=edge_image(base['segm'].shape, channels), use_mask=use_mask,
                                                                   bg_color=bg)


def edge_geometry(name, moments, shape, allow_rotate=True):
    """``_cut_geometry``'s dictionary for the turn of the case (the geometry hook of the edge tests)"""
    from pyimsegm_amd.utilities import data_io
    with orientation_forced(TURNS[EDGE_CASES[name]['turn']]):
        return data_io._hook_geometry(moments, shape, allow_rotate)


def edge_host_crop(name, inputs, label):
    """``cut_object_host`` on the case, the turn of the case given"""
    from pyimsegm_amd.utilities import data_io
    with orientation_forced(TURNS[EDGE_CASES[name]['turn']]):
        return data_io.cut_object_host(inputs['img'], inputs['segm'] == label, inputs['padding'], inputs['use_mask'], inputs['bg_color'],
                                       inputs['allow_rotate'])


def edge_scipy_crop(name, inputs, label):
    """the reference's ``cut_object`` statement by statement with scipy's own resamplings; angle and shift from ``_cut_geometry``, the
    padding from ``add_padding``.  (regionprops' box of the turned mask is the box of its set pixels.)"""
    from scipy import ndimage
    from pyimsegm_amd.utilities import data_io
    img, mask = inputs['img'], inputs['segm'] == label
    bg_color = inputs['bg_color']
    if inputs['allow_rotate']:
        geometry = edge_geometry(name, data_io._region_moments(mask), mask.shape)
        shift = np.append(geometry['shift'], np.zeros(img.ndim - mask.ndim))
        mask = ndimage.shift(mask, -shift[:mask.ndim], order=0)
        mask = ndimage.rotate(mask, geometry['angle'], order=0, reshape=True, mode='constant', cval=np.nan)
        img = ndimage.shift(img, -shift[:img.ndim], order=0)
        img = ndimage.rotate(img, geometry['angle'], order=0, reshape=True, mode='constant', cval=np.nan)
    img_cut = img.copy()
    rows, cols = np.nonzero(mask)
    min_row, min_col, max_row, max_col = data_io.add_padding(img_cut.shape, inputs['padding'], rows.min(), cols.min(), rows.max() + 1,
                                                             cols.max() + 1)
    img_cut = img_cut[min_row:max_row, min_col:max_col, ...]
    if inputs['use_mask']:
        img_cut[~mask[min_row:max_row, min_col:max_col], ...] = bg_color
    return img_cut


def edge_ties(name, label):
    """the coordinates of the case that sit on a rounding tie or on the last pixel: (shift coordinates at k + 0.5, rotation
    coordinates at k + 0.5, rotation coordinates equal to n - 1)"""
    from pyimsegm_amd.utilities import data_io
    base = EDGE_CASES[name]
    height, width = base['segm'].shape
    geometry = edge_geometry(name, data_io._region_moments(base['segm'] == label), (height, width))
    shifted = [np.arange(n) + s for n, s in zip((height, width), geometry['shift'])]
    i = np.arange(geometry['canvas'][0], dtype=np.float64)[:, None]
    j = np.arange(geometry['canvas'][1], dtype=np.float64)[None, :]
    matrix, offset = geometry['matrix'], geometry['offset']
    turned = [((0. + i * matrix[a, 0]) + j * matrix[a, 1]) + offset[a] for a in range(2)]
    half = lambda x: int(np.count_nonzero(x - np.floor(x) == 0.5))
    return (sum(half(x) for x in shifted), sum(half(x) for x in turned),
            sum(int(np.count_nonzero(x == n - 1)) for x, n in zip(turned, (height, width))))
