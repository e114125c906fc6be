"""Shared cases of the centre-detection tests (tests/test_center_detection_reference_host.py, tests/test_gpu_center_detection.py):
plain arrays, each tiny and named for the branch of the clustering it reaches.  ``CASES[name]()`` gives ``(points, eps,
min_samples)``; :func:`facts` says -- from the definition alone, in plain numpy -- what a case contains, so that a test can assert
that the branch in its name really occurs."""
import numpy as np

#: ``IMSEGM_DBSCAN_MAX_POINTS``
CAP = 4096


def _scatter(count, seed, kind='int', near=4.0, eps=50.0):
    """``count`` points in a square in which a point has about ``near`` others within ``eps``"""
    rng = np.random.RandomState(seed)
    side = max(np.sqrt(count * np.pi * eps * eps / near), 4.0)
    if kind == 'int':
        return rng.randint(0, int(side) + 1, (count, 2)).astype(np.float64)
    if kind == 'half':
        return rng.randint(0, 2 * int(side) + 1, (count, 2)) / 2.0
    return rng.uniform(0, side, (count, 2))


def _sized(count):
    return lambda: (_scatter(count, 100 + count), 50.0, 3)


def _line(step, min_samples):
    return lambda: (np.stack([np.arange(300) * float(step), np.full(300, 7.0)], axis=1), 50.0, min_samples)


def _triangles():
    # consecutive points 3-4-5 apart: at eps exactly; and the same figure in half steps
    whole = np.array([[0, 0], [3, 4], [6, 8], [6, 13], [10, 16], [30, 30], [33, 34]], dtype=np.float64)
    return whole, 5.0, 2


def _half_triangles():
    whole, _, _ = _triangles()
    return whole / 2.0, 2.5, 2


def _duplicates():
    points = np.array([[5, 5]] * 4 + [[9, 9]] * 2 + [[5, 6], [40, 40], [40, 40], [40, 40], [80, 80]], dtype=np.float64)
    return points, 1.0, 3


# Two clusters of four core points each and one point between them that is near one core point of either.  (With min_samples = 3 no
# such point exists: a point near two others has three near points with itself and is core.  min_samples = 4 is the smallest
# value at which a border point can lie near the core points of two clusters.)
_BETWEEN = np.array([[4, 0]], dtype=np.float64)
_LEFT = np.array([[0, 0], [1, 0], [2, 0], [1, 1]], dtype=np.float64)
_RIGHT = np.array([[6, 0], [7, 0], [8, 0], [7, 1]], dtype=np.float64)


def _border_between():
    return np.concatenate([_BETWEEN, _RIGHT, _LEFT]), 2.0, 4


def _border_between_reversed():
    return np.concatenate([_BETWEEN, _RIGHT, _LEFT])[::-1].copy(), 2.0, 4


CASES = {'size_%i' % count: _sized(count) for count in (1, 2, 63, 64, 65, 1023, 1024, 1025)}
CASES.update({
    'size_cap': _sized(CAP),
    'size_cap_plus_1': _sized(CAP + 1),                  # takes the host route
    'line_at_eps': _line(50, 1),                         # one cluster through a chain of unions of the largest depth
    'line_at_eps_min_2': _line(50, 2),
    'line_beyond_eps': _line(51, 1),                     # 300 clusters
    'line_beyond_eps_min_2': _line(51, 2),               # all noise
    'triangles_3_4_5': _triangles,                       # near includes equality
    'triangles_half_steps': _half_triangles,
    'duplicates': _duplicates,
    'border_between_two': _border_between,               # takes the lower number
    'border_between_two_reversed': _border_between_reversed,
    'min_samples_above_size': lambda: (_scatter(40, 7), 50.0, 41),      # all noise, centres of shape (0,)
    'half_integer': lambda: (_scatter(400, 8, 'half'), 50.0, 3),
    'uniform_float': lambda: (_scatter(400, 9, 'float'), 50.0, 3),
    'reference_settings': lambda: (_scatter(200, 10, near=12.0), 50.0, 1),
})
#: the sets of the mixed batch: empty sets first, in the middle and last
BATCH = ['empty', 'size_1', 'size_65', 'empty', 'size_1024', 'border_between_two', 'empty']
BATCH_SETTINGS = (50.0, 3)


def case(name):
    if name == 'empty':
        return np.zeros((0, 2), dtype=np.float64), 50.0, 3
    return CASES[name]()


def facts(points, eps, min_samples, labels):
    """what the definition sees in a case, given its labels: the numbers of core, border and noise points, of clusters, and of
    pairs of different points that lie at ``eps`` exactly"""
    points = np.asarray(points, dtype=np.float64)
    count = len(points)
    at_eps, near_count = 0, np.zeros(count, dtype=np.int64)
    for start in range(0, count, 512):
        dx = points[start:start + 512, None, 0] - points[None, :, 0]
        dy = points[start:start + 512, None, 1] - points[None, :, 1]
        dist2 = dx * dx + dy * dy
        near_count[start:start + 512] = (dist2 <= eps * eps).sum(axis=1)
        at_eps += int((dist2 == eps * eps).sum())
    core = near_count >= min_samples
    labels = np.asarray(labels)
    return {'core': int(core.sum()), 'border': int((~core & (labels >= 0)).sum()), 'noise': int((labels < 0).sum()),
            'clusters': int(labels.max()) + 1 if count else 0, 'at_eps': at_eps // 2}


def same(a, b):
    """equal dtype, shape and bytes"""
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ------------------------------------------------------------------------------------------------
# the synthetic image of the end-to-end test: six well-separated ellipses on 256 x 384
# ------------------------------------------------------------------------------------------------

ELLIPSES_SHAPE = (256, 384)


def ellipse_eggs(shape=ELLIPSES_SHAPE, seed=3):
    """label map with six turned ellipses, one per cell of a 2 x 3 grid, each well inside its cell"""
    rng = np.random.RandomState(seed)
    height, width = shape
    cell_h, cell_w = height / 2.0, width / 3.0
    rows, cols = np.indices(shape)
    eggs = np.zeros(shape, dtype=np.int32)
    for k in range(6):
        cy, cx = (k // 3 + 0.5) * cell_h, (k % 3 + 0.5) * cell_w
        limit = 0.5 * min(cell_h, cell_w) - 6
        a, b = rng.uniform(0.8, 0.95) * limit, rng.uniform(0.6, 0.75) * limit
        theta = rng.uniform(0, np.pi)
        dy, dx = rows - cy, cols - cx
        u, v = dx * np.cos(theta) + dy * np.sin(theta), -dx * np.sin(theta) + dy * np.cos(theta)
        eggs[(u / a) ** 2 + (v / b) ** 2 <= 1.] = k + 1
    return eggs


def ellipse_image(eggs, seed=4):
    """an RGB image of the eggs: two flat colours and a little noise"""
    rng = np.random.RandomState(seed)
    img = np.where((eggs > 0)[:, :, None], np.array([200, 150, 90]), np.array([40, 40, 60])).astype(np.float64)
    return np.clip(img + rng.normal(0, 6, img.shape), 0, 255).astype(np.uint8)
