"""Region growing with a ray shape prior on superpixels: the growth loop of the reference's ``imsegm/region_growing.py``
(``region_growing_shape_slic_greedy``, ``region_growing_shape_slic_graphcut`` and what they call) with the per-iteration work on
the device.

* The host keeps the iteration (``list_swap_shift`` and its shaking rule, ``enforce_center_labels``, ``debug_history``, the
  threshold tests on centre, shift and volume, the stable sort and the apply loop of the greedy variant), centre and orientation
  of an object (``np.cov`` + ``np.linalg.eig``: the sign of LAPACK's eigenvector decides between theta and theta + 180), the
  mixture weights and the mixing of the cdf tables, and the assembly of the graph that is cut.
* ``on='device'`` keeps a resident state (``_hip.RegionGrowing``, csrc/region_growing.hip) on the label session: the shape cost of
  every (object, superpixel) pair, the ray distances of every object's mask, the candidates of an iteration with their energy
  changes, and the criterion.  Per iteration K labels go up and the candidates come down.
* ``on='host'`` evaluates the same definitions in numpy (:class:`_HostState`) -- the CPU statement the kernels are tested against.
  The cut of the graph-cut variant always runs on the device (``graph_cuts.cut_general_graph``).

Definitions ("Region growing"): the shape prior is bilinear on the 2 x 2 cell where the reference builds an
``interp2d`` object; the energy change of a candidate is the delta of the criterion, not the difference of two full sums.
"""
import numpy as np
from scipy import ndimage, stats
from sklearn import cluster, mixture

from pyimsegm_amd import _hip
from pyimsegm_amd.descriptors import _ray_directions, interpolate_ray_dist, ray_walk_host, shift_ray_features
from pyimsegm_amd.graph_cuts import MAX_PAIRWISE_COST, compute_spatial_dist, cut_general_graph, cut_grid_graph, get_vertexes_edges
from pyimsegm_amd.labeling import histogram_regions_labels_norm

#: stands in for an infinite cost wherever a cost table or a graph-cut term would hold one
GC_REPLACE_INF = 1e5
#: added to every shape prior before its logarithm: a prior of 0 still has a finite cost
MIN_SHAPE_PROB = 0.01
#: the largest probability a unary term may express (its cost is never below -log of this)
MAX_UNARY_PROB = 1 - 0.01
#: when the shape cost of an object is computed anew during a growth, and how far its centre may wander
RG2SP_THRESHOLDS = {
    'centre': 30,           # pixels between the centre and the one its cost column was computed for
    'shift': 15,            # degrees between the orientation and the one of the column
    'volume': 0.1,          # relative change of the number of superpixels since the column ('set_cdfs')
    'centre_init': 50,      # pixels: the radius around the initial centre within which a centre is kept
}


def _place(on, variable='IMSEGM_RG_ON'):
    """'host' or 'device': ``_hip.resolve_place`` on IMSEGM_RG_ON (``variable``)"""
    return _hip.resolve_place(on, variable, False)[0]


def _replace_inf(values):
    values[np.isinf(values)] = GC_REPLACE_INF
    return values


def _penalties(prob_label_trans):
    """-log of the two transition probabilities with inf replaced (``compute_rg_crit`` :1130-1131)"""
    with np.errstate(divide='ignore'):
        pen = _replace_inf(-np.log(np.asarray(prob_label_trans[:2], dtype=np.float64)))
    return float(pen[0]), float(pen[1])


# ------------------------------------------------------------------------------------------------
# the definitions the kernels implement, in numpy
# ------------------------------------------------------------------------------------------------


def shape_prior_points(points, cum_distribution, centre, angle_shift=0):
    """:func:`compute_shape_prior_table_cdf` for points [N, 2] at once: the numpy statement of ``k_rg_shape_cost``, operation by
    operation.  Row A of the table is row 0 again; a modulus that rounds to 360.0 itself takes row 0 with weight 0."""
    table = np.asarray(cum_distribution, dtype=np.float64)
    nb_angles, nb_dists = table.shape
    points = np.asarray(points, dtype=np.float64).reshape(-1, 2)
    dx, dy = points[:, 0] - float(centre[0]), points[:, 1] - float(centre[1])
    dist = np.sqrt(dx * dx + dy * dy)
    angle = np.rad2deg(np.arctan2(dy, dx))
    angle = np.mod((810.0 - angle) - float(angle_shift), 360.0)
    angle_norm = angle / (360. / nb_angles)
    prior = np.empty(len(points))
    far = dist >= (nb_dists - 1)
    row = np.rint(angle_norm[far]).astype(int)
    row[row >= nb_angles] = 0
    prior[far] = table[row, nb_dists - 1]
    near = ~far
    if near.any():
        a_norm, d = angle_norm[near], dist[near]
        a0 = np.floor(a_norm).astype(int)
        ta = a_norm - a0
        wrapped = a0 >= nb_angles
        a0[wrapped], ta[wrapped] = 0, 0.
        a1 = np.where(a0 + 1 >= nb_angles, 0, a0 + 1)
        d0 = np.floor(d).astype(int)
        td = d - d0
        low = table[a0, d0] + (table[a0, d0 + 1] - table[a0, d0]) * td
        high = table[a1, d0] + (table[a1, d0 + 1] - table[a1, d0]) * td
        prior[near] = low + (high - low) * ta
    return prior


def compute_shape_prior_table_cdf(point, cum_distribution, centre, angle_shift=0):
    """shape prior of one point: the cumulative table read at the point's distance from ``centre`` and at its direction turned by
    ``angle_shift`` degrees (reference :591-652); :func:`shape_prior_points` for a single point.  The reference's examples are in
    tests/doctests/region_growing.py.

    :param tuple(int,int) point: (row, col)
    :param cum_distribution: table [angles, distances]
    :param tuple(float,float) centre: (row, col) of the object
    :param float angle_shift: orientation of the object in degrees
    :return float:
    """
    return shape_prior_points([point], cum_distribution, centre, angle_shift)[0]


def _shape_cost(prior):
    with np.errstate(divide='ignore', invalid='ignore'):
        return _replace_inf(-np.log(prior + MIN_SHAPE_PROB))


def ray_distances_down(mask, position, directions):
    """``computeRayFeaturesBinary2d(mask, position, edge='down')`` in numpy, all angles at once: float32 [A], the one-position call
    of ``descriptors.ray_walk_host``"""
    return ray_walk_host(mask, [(int(position[0]), int(position[1]))], directions, -1)[0]


def _delta_scores(objects, superpixels, labels, weights, lut_data, lut_shape, nb_off, nb_flat, coef_data, coef_shape, coef_pairwise,
                  pen_bg, pen_fg):
    """energy change of every candidate in its delta form: the numpy statement of ``k_rg_scores``"""
    old = labels[superpixels]
    unary = (coef_data * (lut_data[superpixels, old] - lut_data[superpixels, objects])
             + coef_shape * (lut_shape[superpixels, old] - lut_shape[superpixels, objects]))
    change = weights[superpixels].astype(np.float64) * unary
    if coef_pairwise > 0:
        def penalty(own, other):
            return np.where(own == other, 0., np.where((own == 0) | (other == 0), pen_bg, pen_fg))

        pair = np.zeros(len(objects))
        degree = nb_off[superpixels + 1] - nb_off[superpixels]
        for step in range(int(degree.max()) if len(degree) else 0):              # neighbour after neighbour, in list order
            has = np.nonzero(degree > step)[0]
            other = labels[nb_flat[nb_off[superpixels[has]] + step]]
            pair[has] += penalty(old[has], other) - penalty(objects[has], other)
        change = change + coef_pairwise * pair
    return change


def _tree_sum(values):
    """the fixed tree of ``k_rg_crit``: lane i adds entries i, i + 256, ... in order, the 64 lanes of a wave meet in an xor
    butterfly, the four waves as (w0 + w1) + (w2 + w3)"""
    values = np.asarray(values, dtype=np.float64)
    lanes = np.zeros(256)
    for start in range(0, len(values), 256):
        chunk = values[start:start + 256]
        lanes[:len(chunk)] += chunk
    waves = lanes.reshape(4, 64)
    for off in (32, 16, 8, 4, 2, 1):
        waves = waves + waves[:, np.arange(64) ^ off]
    return (waves[0, 0] + waves[1, 0]) + (waves[2, 0] + waves[3, 0])


class _HostState(object):
    """what ``_hip.RegionGrowing`` keeps on the device, in numpy, with the same methods"""

    def __init__(self, slic, n_objects):
        slic = np.asarray(slic)
        self.slic, self.n_objects = slic, int(n_objects)
        self.n_labels = int(slic.max()) + 1
        rows, cols = np.indices(slic.shape)
        count = np.bincount(slic.ravel(), minlength=self.n_labels)
        self._sums = np.stack([count, np.bincount(slic.ravel(), rows.ravel(), self.n_labels).astype(np.int64),
                               np.bincount(slic.ravel(), cols.ravel(), self.n_labels).astype(np.int64)], axis=1).astype(np.int64)
        with np.errstate(invalid='ignore', divide='ignore'):
            centres = np.where(count[:, None] > 0, self._sums[:, 1:] / count[:, None].astype(np.float64), -1.)
        self._points = np.round(centres).astype(np.int32)
        pairs = np.vstack([np.stack([slic[:, :-1].ravel(), slic[:, 1:].ravel()], axis=1),
                           np.stack([slic[:-1, :].ravel(), slic[1:, :].ravel()], axis=1)])
        pairs = np.sort(pairs[pairs[:, 0] != pairs[:, 1]], axis=1)
        codes = np.unique(pairs[:, 0] + self.n_labels * pairs[:, 1].astype(np.int64))
        self.edges = np.stack([codes % self.n_labels, codes // self.n_labels], axis=1).astype(np.int32)      # ordered by (b, a)
        self.lut_data = self.lut_shape = None
        self._labels = np.zeros(self.n_labels, dtype=int)

    def close(self):
        pass

    def sums(self):
        return self._sums

    def points(self):
        return self._points

    def attach(self, nb_off, nb_flat):
        self.nb_off, self.nb_flat = nb_off, nb_flat

    def set_costs(self, lut_data=None, lut_shape=None):
        if lut_data is not None:
            self.lut_data = np.array(lut_data, dtype=np.float64)
        if lut_shape is not None:
            self.lut_shape = np.array(lut_shape, dtype=np.float64)

    def shape_costs(self):
        return self.lut_shape.copy()

    def update_shape_costs(self, objects, centres, shifts, tables, with_proba=False):
        proba = np.empty((len(objects), self.n_labels))
        for j, obj in enumerate(objects):
            proba[j] = shape_prior_points(self._points, tables[j], centres[j], shifts[j])
            self.lut_shape[:, obj + 1] = _shape_cost(proba[j])
        return proba if with_proba else None

    def object_rays(self, labels, positions, directions):
        self._labels = np.asarray(labels if labels is not None else self._labels)
        segm = self._labels[self.slic]
        return np.array([ray_distances_down(segm == i + 1, positions[i], directions) for i in range(self.n_objects)],
                        dtype=np.float32).reshape(self.n_objects, len(directions))

    def greedy_step(self, labels, allow_obj_swap, coef_data, coef_shape, coef_pairwise, pen_bg, pen_fg, with_scores=True):
        labels = self._labels = np.asarray(labels if labels is not None else self._labels)
        owner = np.repeat(np.arange(self.n_labels), np.diff(self.nb_off))
        objects, superpixels = [], []
        for obj in range(1, self.n_objects + 1):
            touched = np.zeros(self.n_labels, dtype=bool)
            touched[owner[labels[self.nb_flat] == obj]] = True
            near = np.nonzero(touched & ((labels != obj) if allow_obj_swap else (labels == 0)))[0]
            superpixels.append(near)
            objects.append(np.full(len(near), obj))
        objects, superpixels = np.concatenate(objects).astype(np.int32), np.concatenate(superpixels).astype(np.int32)
        if not with_scores:
            return objects, superpixels, None
        return objects, superpixels, _delta_scores(objects, superpixels, labels, self._sums[:, 0], self.lut_data, self.lut_shape,
                                                   self.nb_off, self.nb_flat, coef_data, coef_shape, coef_pairwise, pen_bg, pen_fg)

    def criterion(self, labels, coef_data, coef_shape, coef_pairwise, pen_bg, pen_fg):
        labels = self._labels = np.asarray(labels if labels is not None else self._labels)
        every = np.arange(len(labels))
        crit = _tree_sum(self._sums[:, 0].astype(np.float64)
                         * (coef_data * self.lut_data[every, labels] + coef_shape * self.lut_shape[every, labels]))
        if coef_pairwise > 0:
            first, second = labels[self.edges[:, 0]], labels[self.edges[:, 1]]
            pen = np.where(first == second, 0., np.where((first == 0) | (second == 0), pen_bg, pen_fg))
            crit = crit + coef_pairwise * _tree_sum(pen)
        return float(crit)


class _DeviceState(object):
    """the resident state of csrc/region_growing.hip behind the methods of :class:`_HostState`"""

    def __init__(self, slic, n_objects):
        from pyimsegm_amd.superpixels import _session_for_labels
        self.sess = _session_for_labels(np.asarray(slic))
        try:
            self.edges = self.sess.graph()[0]
            self.rg = _hip.RegionGrowing(self.sess, self.edges, n_objects)
        except Exception:
            self.sess.close()
            raise
        self.n_objects, self.n_labels = int(n_objects), self.rg.n_labels
        for name in ('sums', 'points', 'set_costs', 'shape_costs', 'update_shape_costs', 'object_rays', 'greedy_step', 'criterion'):
            setattr(self, name, getattr(self.rg, name))

    def attach(self, nb_off, nb_flat):
        pass

    def close(self):
        self.rg.close()
        self.sess.close()


# ------------------------------------------------------------------------------------------------
# the small functions of the reference
# ------------------------------------------------------------------------------------------------


def compute_segm_prob_fg(slic, segm, labels_prob):
    """foreground probability of every superpixel: ``labels_prob`` of the class of ``segm`` that covers most of it (reference
    :1136-1152; the histogram on the device)

    :param ndarray slic: superpixel map
    :param ndarray segm: class map of the same shape
    :param list(float) labels_prob: foreground probability of every class
    :return ndarray: one probability per superpixel
    """
    majority = np.argmax(histogram_regions_labels_norm(slic, segm), axis=1)
    return np.asarray(labels_prob)[majority]


def compute_centre_moment_points(points):
    """mean of a point set and the direction of its largest spread in whole degrees, 0 .. 359 (reference :704-747).  ``np.cov`` and
    ``np.linalg.eig`` are called on the centred points as the reference calls them: the sign LAPACK gives the eigenvector decides
    between an angle and the opposite one.

    :param points: [N, 2] (row, col)
    :return tuple(ndarray,float): mean, angle
    """
    coords = np.asarray(points)
    mean = np.mean(coords, axis=0)
    degrees = 0.
    if len(coords) > 1:
        values, vectors = np.linalg.eig(np.cov((coords - mean).T))
        main = vectors[:, np.argmax(values)]
        degrees = np.rad2deg(np.arctan2(main[0], main[1]))
    return mean, float((360 + round(degrees)) % 360)


def compute_segm_object_shape(img_object, ray_step=5, interp_order=3, smooth_coef=0, shift_method='phase'):
    """ray distances of the one object in a binary image, cast from its rounded centre of mass to where the object ends; rays that
    leave the image are filled in, the vector is optionally smoothed and then rotated to its main phase (reference :259-286; the
    rays on the device)

    :return tuple(list(float),float): rays, rotation
    """
    from pyimsegm_amd.descriptors import compute_ray_features_segm_2d
    start = [int(round(c)) for c in ndimage.center_of_mass(img_object)]
    return _finish_rays(compute_ray_features_segm_2d(img_object, start, ray_step, 0, edge='down'), interp_order, smooth_coef,
                        shift_method)


def _finish_rays(rays, interp_order=3, smooth_coef=0, shift_method='phase', shift_rays=shift_ray_features):
    """what follows the ray walk of :func:`compute_segm_object_shape`: fill, smooth, rotate (by ``shift_rays``)"""
    if interp_order is not None and np.any(np.asarray(rays) == -1):
        rays = interpolate_ray_dist(rays, interp_order)
    if smooth_coef > 0:
        from scipy.ndimage import gaussian_filter1d
        rays = gaussian_filter1d(rays, smooth_coef)
    rays, rotation = shift_rays(rays, shift_method)
    return rays.tolist(), rotation


def _shift_rays_double(ray_dist, method='phase'):
    """``shift_ray_features`` for the float32 rays of the walk with the spectrum in float64: numpy before 2.0 transformed a float32
    vector in double -- the answers recorded from the reference, and the ``45.`` of its doctest -- where numpy 2 keeps single
    precision, which moves the phase by some 1e-6 degrees.  The mean is taken off in float32 first, as both do."""
    ray_dist = np.asarray(ray_dist)
    if method != 'phase' or ray_dist.dtype != np.float32:
        return shift_ray_features(ray_dist, method)
    periods = np.hstack([ray_dist] * 5)
    half = len(periods) // 2
    spectrum = np.fft.fft((periods - np.mean(periods)).astype(np.float64)) / float(len(periods))
    strongest = np.argmax(np.abs(spectrum)[:half])
    shift = np.rad2deg(-np.angle(spectrum)[:half][strongest])
    shift = (360 + shift) if shift < 0 else shift
    steps = int(round(shift / (360 / len(ray_dist))))
    return np.array(ray_dist[steps:].tolist() + ray_dist[:steps].tolist()), shift


# ------------------------------------------------------------------------------------------------
# ray shape models from annotated label maps (reference :289-588)
# ------------------------------------------------------------------------------------------------


#: objects of one map ``imsegm_object_shapes`` is given room for; a map with more is evaluated on the host
OBJECT_SHAPES_CAPACITY = 1024


def _int32_map(img):
    """the map as a C-contiguous int32 array where that holds every value exactly (integers, booleans, floats with integral
    values), else None"""
    img = np.asarray(img)
    if img.ndim != 2 or img.size == 0 or img.dtype.kind not in 'iubf':
        return None
    if img.dtype.kind == 'f' and not (np.all(np.isfinite(img)) and np.all(img == np.rint(img))):
        return None
    info = np.iinfo(np.int32)
    if img.dtype.kind == 'b' or (info.min <= img.min() and img.max() <= info.max):
        return np.ascontiguousarray(img, dtype=np.int32)
    return None


def _object_shape_rays_host(img, directions):
    """the numpy / scipy statement of ``imsegm_object_shapes`` (csrc/object_shapes.hip): the objects of a map as the reference's
    ``compute_object_shapes`` takes them (:320-326) -- the components of ``ndimage.label`` for a map of at most two values, else the
    values -- without the first, each with its exact pixel count, row sum and column sum, the rounded centre of mass of
    ``compute_segm_object_shape`` (:278-279) and the raw 'down' rays from there"""
    values = np.unique(img)
    if len(values) <= 2:
        img, _ = ndimage.label(img)
        values = np.unique(img)
    labels = values[1:]
    rows, cols = np.indices(img.shape)
    moments = np.zeros((len(labels), 3), dtype=np.int64)
    centres = np.zeros((len(labels), 2), dtype=np.int32)
    rays = np.zeros((len(labels), len(directions)), dtype=np.float32)
    for k, label in enumerate(labels):
        mask = img == label
        count, row_sum, col_sum = int(np.count_nonzero(mask)), int(rows[mask].sum()), int(cols[mask].sum())
        moments[k] = count, row_sum, col_sum
        # ndimage.center_of_mass of a boolean mask: this quotient of two exactly representable sums
        centres[k] = int(round(row_sum / float(count))), int(round(col_sum / float(count)))
        rays[k] = ray_distances_down(mask, centres[k], directions)
    return labels, moments, centres, rays


def object_shape_rays(img_objects, ray_step=5, on=None):
    """the stage of :func:`compute_object_shapes` in front of :func:`_finish_rays`, for one map: its objects in the reference's
    order with their labels, moments int64 [n, 3] (pixel count, row sum, column sum), rounded centres of mass int32 [n, 2] and raw
    'down' rays float32 [n, angles], -1 where a ray meets no edge.

    ``on='device'`` (the default when a device is present; ``IMSEGM_OBJECT_SHAPES_ON``): one ``imsegm_object_shapes`` call -- the
    map goes up, labelling, moments, centres and the rays of all objects are one chain of launches, the four tables come down.
    ``on='host'``: the numpy / scipy statement of the same definitions.  A map that is not integer-valued or leaves int32, label
    values that span ``_hip.OBJECT_SHAPES_MAX_SPAN`` or more, and more than ``OBJECT_SHAPES_CAPACITY`` objects take the host
    statement as well ("Object shapes").

    :param ndarray img_objects: annotated map: at most two values (objects are the 4-connected components of the non-zero pixels)
        or one value per object above the smallest one
    :param int ray_step: angular step of the rays in degrees
    :param str on: ``'device'``, ``'host'`` or None
    :return tuple(ndarray,ndarray,ndarray,ndarray): labels, moments, centres, raw_rays
    """
    place = _place(on, 'IMSEGM_OBJECT_SHAPES_ON')
    directions = _ray_directions(float(ray_step))
    segm = _int32_map(img_objects)
    if segm is not None and place == 'device':
        count, labels, moments, centres, rays = _hip.object_shapes(segm, directions, OBJECT_SHAPES_CAPACITY)
        if labels is not None:
            return labels, moments, centres, rays
    return _object_shape_rays_host(np.asarray(img_objects) if segm is None else segm, directions)


def compute_object_shapes(list_img_objects, ray_step=5, interp_order=3, smooth_coef=0, shift_method='phase', on=None):
    """ray distances and rotation of every object of every annotated map, objects of all maps one after the other (reference
    :289-331; its example is in tests/test_object_shapes_reference_host.py): :func:`object_shape_rays` per map -- one device call -- then the
    fill, smoothing and rotation of :func:`compute_segm_object_shape` per object on the host

    :param list(ndarray) list_img_objects: annotated maps
    :param int ray_step: angular step of the rays in degrees
    :param int interp_order: how rays that left the image are filled in; None: not at all
    :param float smooth_coef: sigma of the smoothing along the angle
    :param str shift_method: 'phase' or 'max'
    :param str on: ``'device'``, ``'host'`` or None (``IMSEGM_OBJECT_SHAPES_ON``)
    :return tuple(list(list(float)),list(float)): rays, rotations
    """
    list_rays, list_shifts = [], []
    for img_objects in list_img_objects:
        for raw in object_shape_rays(img_objects, ray_step, on)[3]:
            rays, shift = _finish_rays(raw, interp_order, smooth_coef, shift_method, _shift_rays_double)
            list_rays.append(rays)
            list_shifts.append(shift)
    return list_rays, list_shifts


def compute_cumulative_distrib(means, stds, weights, max_dist):
    """inverse cumulative distribution of the ray length per direction: the weighted normal cdfs of the components at the
    distances 0 .. int(max_dist), stretched to [0, 1] and turned over, plus 1e-9 (reference :334-361), all directions and samples at
    once; the components are added in their order

    :param ndarray means: [components, directions]
    :param ndarray stds: [components, directions]
    :param ndarray weights: [components]
    :param float max_dist: the largest distance of the table
    :return ndarray: [directions, int(max_dist) + 1]
    """
    means, stds = np.asarray(means), np.asarray(stds)
    samples = np.arange(int(max_dist) + 1)
    cdf = np.zeros((means.shape[1], int(max_dist + 1)))
    for j, weight in enumerate(weights):
        cdf += stats.norm.cdf(samples[None, :], means[j][:, None], stds[j][:, None]) * weight
    low, high = cdf.min(axis=1, keepdims=True), cdf.max(axis=1, keepdims=True)
    cdf = (cdf - low) / (high - low)
    return 1. - cdf + 1e-9


def _cdf_of_full_mixture(means, covariances, weights):
    """the table of :func:`transform_rays_model_cdf_mixture` from the fitted attributes (:393-400)"""
    means, covariances = np.asarray(means), np.asarray(covariances)
    max_dist = np.max([[m[i] + np.sqrt(c[i, i]) for i in range(len(m))] for m, c in zip(means, covariances)])
    stds = np.sqrt(abs(covariances))[:, np.eye(means.shape[1], dtype=bool)]
    return compute_cumulative_distrib(means, stds, weights, max_dist)


def _mean_cdfs_of_diag_mixture(means, covariances, slic_size):
    """(mean rays, table) per component of a mixture with diagonal covariances (:426-436)"""
    list_mean_cdf = []
    for mean, covar in zip(means, covariances):
        std = np.sqrt(covar + 1) * 2 + slic_size
        mean = ndimage.gaussian_filter1d(mean, 1)
        std = ndimage.gaussian_filter1d(std, 1)
        max_dist = np.max(mean + 2 * std)
        cdist = compute_cumulative_distrib(np.array([mean]), np.array([std]), np.array([1]), max_dist)
        list_mean_cdf.append((mean.tolist(), cdist))
    return list_mean_cdf


def _mean_cdfs_of_clusters(list_rays, centres, labels):
    """(mean rays, table) per cluster of a k-means fit (:459-468)"""
    list_mean_cdf = []
    for lb, mean in enumerate(centres):
        std = np.std(np.asarray(list_rays)[labels == lb], axis=0)
        mean = ndimage.gaussian_filter1d(mean, 1)
        std = ndimage.gaussian_filter1d(std, 1)
        std = (std + 1) * 5.
        max_dist = np.max(mean + 2 * std)
        cdist = compute_cumulative_distrib(np.array([mean]), np.array([std]), np.array([1]), max_dist)
        list_mean_cdf.append((mean.tolist(), cdist))
    return list_mean_cdf


def _cdf_of_clusters(list_rays, labels, centres=None):
    """one table from a clustering of the rays (:496-509, :542-553): per cluster the mean -- the smoothed mean of its members, or
    the given centre -- and the standard deviation of its members plus 1, weighted by the share of the cluster"""
    rays, labels = np.asarray(list_rays), np.asarray(labels)
    present = np.unique(labels)
    means = np.zeros((len(present), rays.shape[1])) if centres is None else np.asarray(centres)
    stds = np.zeros((len(means), rays.shape[1]))
    for i, lb in enumerate(present):
        if centres is None:
            means[i, :] = np.mean(rays[labels == lb], axis=0)
            means[i, :] = ndimage.gaussian_filter1d(means[i, :], 1)
        stds[i, :] = np.std(rays[labels == lb], axis=0)
    stds += 1
    weights = np.bincount(labels) / float(len(labels))
    max_dist = np.max([[m[i] + c[i] for i in range(len(m))] for m, c in zip(means, stds)])
    return compute_cumulative_distrib(means, stds, weights, max_dist)


def transform_rays_model_cdf_mixture(list_rays, coef_components=1):
    """a Bayesian Gaussian mixture of the ray vectors, with as many components as mean shift finds clusters times
    ``coef_components``, and its cumulative table (reference :364-401).  The fits are scikit-learn's on the host.

    :return tuple(BayesianGaussianMixture,list(list(float))): mixture, table [directions, distances]
    """
    rays = np.array(list_rays)
    ms = cluster.MeanShift()
    ms.fit(rays)
    nb_components = int(len(np.unique(ms.labels_)) * coef_components)
    mm = mixture.BayesianGaussianMixture(n_components=nb_components)
    mm.fit(rays, ms.labels_)
    covs = mm.covariances if hasattr(mm, 'covariances') else mm.covariances_
    return mm, _cdf_of_full_mixture(mm.means_, covs, mm.weights_).tolist()


def transform_rays_model_sets_mean_cdf_mixture(list_rays, nb_components=5, slic_size=15):
    """a Bayesian Gaussian mixture with diagonal covariances and, per component, its smoothed mean rays with a table of their own
    (reference :404-438)

    :return tuple(BayesianGaussianMixture,list(tuple(list(float),ndarray))): mixture, [(mean rays, table)]
    """
    rays = np.array(list_rays)
    mm = mixture.BayesianGaussianMixture(n_components=nb_components, covariance_type='diag')
    mm.fit(rays)
    return mm, _mean_cdfs_of_diag_mixture(mm.means_, mm.covariances_, slic_size)


def transform_rays_model_sets_mean_cdf_kmeans(list_rays, nb_components=5):
    """k-means of the ray vectors and, per cluster, its smoothed centre with a table of its own (reference :441-470)

    :return tuple(KMeans,list(tuple(list(float),ndarray))): k-means, [(mean rays, table)]
    """
    rays = np.array(list_rays)
    kmeans = cluster.KMeans(nb_components)
    kmeans.fit(rays)
    return kmeans, _mean_cdfs_of_clusters(list_rays, kmeans.cluster_centers_, kmeans.labels_)


def transform_rays_model_cdf_spectral(list_rays, nb_components=5):
    """spectral clustering of the ray vectors and one table of the clusters (reference :473-510)

    :return tuple(SpectralClustering,list(list(float))): clustering, table
    """
    rays = np.array(list_rays)
    sc = cluster.SpectralClustering(nb_components)
    sc.fit(rays)
    return sc, _cdf_of_clusters(list_rays, sc.labels_).tolist()


def transform_rays_model_cdf_kmeans(list_rays, nb_components=None):
    """k-means of the ray vectors -- with as many clusters as mean shift finds when ``nb_components`` is not given -- and one table
    of the clusters (reference :513-554)

    :return tuple(KMeans,list(list(float))): k-means, table
    """
    rays = np.array(list_rays)
    if not nb_components:
        ms = cluster.MeanShift()
        ms.fit(rays)
        nb_components = len(np.unique(ms.labels_))
        kmeans = cluster.KMeans(nb_components)
        kmeans.fit(rays, ms.labels_)
    else:
        kmeans = cluster.KMeans(nb_components)
        kmeans.fit(rays)
    return kmeans, _cdf_of_clusters(list_rays, kmeans.labels_, kmeans.cluster_centers_).tolist()


def transform_rays_model_cdf_histograms(list_rays, nb_bins=10):
    """one cumulative histogram per direction from all measured rays, read at integer bin centres (reference :557-588; its example
    is in tests/test_object_shapes_reference_host.py)

    :param list(list(int)) list_rays: integer ray lengths, one list per object
    :param int nb_bins: bins of the histogram of a direction
    :return list(list(float)): table [directions, max + 1]
    """
    rays = np.array(list_rays)
    max_dist = np.max(rays)
    list_chist = []
    for i in range(rays.shape[1]):
        cum = np.zeros(max_dist + 1)
        hist, bin_edges = np.histogram(rays[:, i], nb_bins)
        hist = hist.astype(float) / np.sum(hist)
        bin_edges = bin_edges.astype(int)
        bins = ((bin_edges[1:] + bin_edges[:-1]) / 2).astype(int)
        cum[:bins[0]] = 1
        for j, edge in enumerate(bins):
            cum[edge:] = cum[edge - 1] - hist[j]
        list_chist.append(cum.tolist())
    return list_chist


def compute_data_costs_points(slic, slic_prob_fg, centres, labels):
    """data cost of every (superpixel, label) pair -- ``-log`` of the background probability in column 0 and of the foreground
    probability in the column of every object -- and ``labels`` with the superpixel under every centre given to its object
    (reference :993-1011)

    :return tuple(ndarray,ndarray): costs [K, objects + 1], labels
    """
    foreground = np.asarray(slic_prob_fg, dtype=np.float64)
    proba = np.repeat(foreground[:, None], len(centres) + 1, axis=1)
    proba[:, 0] = 1. - foreground
    for number, position in enumerate(centres, start=1):
        labels[slic[position[0], position[1]]] = number
    return _replace_inf(-np.log(proba + 1e-9)), labels


def compute_pairwise_penalty(edges, labels, prob_bg_fg=0.05, prob_fg1_fg2=0.01):
    """cost of every edge for the labels at its two ends: nothing where they agree, ``-log(prob_bg_fg)`` where one of them is the
    background, ``-log(prob_fg1_fg2)`` between two objects (reference :1065-1085)

    :return ndarray: one cost per edge
    """
    first, second = np.asarray(labels)[np.asarray(edges)].T
    differ = first != second
    at_background = differ & ((first == 0) | (second == 0))
    return np.where(at_background, -np.log(prob_bg_fg), -np.log(prob_fg1_fg2) * differ)


def get_neighboring_candidates(slic_neighbours, labels, object_idx, use_other_obj=True):
    """the superpixels next to object ``object_idx`` that it could take, ascending: those of any other label, or of the background
    alone when ``use_other_obj`` is off (reference :1088-1111)

    :return list(int):
    """
    label_of = np.asarray(labels)
    around = set()
    for member in np.nonzero(label_of == object_idx)[0]:
        around.update(int(n) for n in slic_neighbours[member])
    if use_other_obj:
        return [n for n in sorted(around) if label_of[n] != object_idx]
    return [n for n in sorted(around) if label_of[n] == 0]


def compute_rg_crit(labels, lut_data_cost, lut_shape_cost, slic_weights, edges, coef_data, coef_shape, coef_pairwise,
                    prob_label_trans):
    """energy of a labelling: the weighted data and shape cost of every superpixel under its label, plus the penalty of every edge
    (reference :1114-1133)

    :return float:
    """
    rows = np.arange(len(labels))
    unary = coef_data * lut_data_cost[rows, labels] + coef_shape * lut_shape_cost[rows, labels]
    energy = np.sum(slic_weights * unary)
    if coef_pairwise > 0:
        penalty = compute_pairwise_penalty(edges, labels, prob_label_trans[0], prob_label_trans[1])
        energy += coef_pairwise * np.sum(_replace_inf(penalty))
    return energy


def enforce_center_labels(slic, labels, centres):
    """gives the superpixel under every centre to the object of that centre, so that no object can vanish (reference :1467-1479)"""
    for number, position in enumerate(centres, start=1):
        labels[slic[int(position[0]), int(position[1])]] = number
    return labels


def _csr_neighbours(slic_neighbours, nb_labels):
    degree = np.zeros(nb_labels, dtype=np.int64)
    degree[:len(slic_neighbours)] = [len(near) for near in slic_neighbours]
    nb_off = np.concatenate([[0], np.cumsum(degree)])
    nb_flat = np.array([n for near in slic_neighbours for n in near], dtype=np.int64)
    return nb_off, nb_flat


def prepare_graphcut_variables(candidates, slic_points, slic_neighbours, slic_weights, labels, nb_centres, lut_data_cost,
                               lut_shape_cost, coef_data, coef_shape, coef_pairwise, prob_label_trans):
    """the graph that is cut around the candidates, with its potentials (reference :1391-1464): a candidate may take the label of
    any of its neighbours at its weighted data and shape cost, a neighbour that is no candidate keeps its label at no cost, and
    everything else costs ``GC_REPLACE_INF``.  Vectorised, with the reference's vertex order: the candidates first (duplicates kept), then their
    neighbours in order of first appearance; one edge (i, j) per (candidate, neighbour) pair in that order, j the FIRST position of
    the neighbour among the vertexes

    :return: vertexes, edges, edge_weights, unary, pairwise
    """
    slic_points, labels = np.asarray(slic_points), np.asarray(labels)
    if np.max(candidates) >= len(slic_points):
        raise ValueError('max candidate idx: %d for %d centres' % (np.max(candidates), len(slic_points)))
    largest = max(max(near) for near in slic_neighbours if len(near))
    if largest >= len(slic_points):
        raise ValueError('max slic neighbours idx: %d for %d centres' % (largest, len(slic_points)))
    cand = np.asarray(candidates, dtype=np.int64)
    nb_off, nb_flat = _csr_neighbours(slic_neighbours, len(slic_points))
    degree = nb_off[cand + 1] - nb_off[cand]
    owner = np.repeat(np.arange(len(cand)), degree)
    near = nb_flat[np.repeat(nb_off[cand], degree) + (np.arange(degree.sum()) - np.repeat(np.cumsum(degree) - degree, degree))]
    position = np.full(len(slic_points), -1, dtype=np.int64)
    uniq, first = np.unique(cand, return_index=True)
    position[uniq] = first
    fresh = near[position[near] < 0]
    uniq, first = np.unique(fresh, return_index=True)
    added = uniq[np.argsort(first, kind='stable')]
    position[added] = len(cand) + np.arange(len(added))
    vertexes = np.concatenate([cand, added])
    edges = np.stack([owner, position[near]], axis=1)

    nb_labels = nb_centres + 1
    unary = np.full((len(vertexes), nb_labels), GC_REPLACE_INF, dtype=np.float64)
    cost = coef_data * lut_data_cost[cand] + coef_shape * lut_shape_cost[cand]
    seen = np.zeros((len(cand), nb_labels), dtype=bool)
    seen[owner, labels[near]] = True
    unary[:len(cand)] = np.where(seen, np.asarray(slic_weights)[cand][:, None] * cost, GC_REPLACE_INF)
    unary[len(cand) + np.arange(len(added)), labels[added]] = 0
    np.maximum(unary, -np.log(MAX_UNARY_PROB), out=unary)                  # no unary term claims more than MAX_UNARY_PROB
    # an edge weighs the inverse of its length, lengths relative to their mean
    edge_weights = 1. / compute_spatial_dist(slic_points[vertexes], edges, relative=True)
    pen_bg, pen_fg = -np.log(prob_label_trans[0]), -np.log(prob_label_trans[1])
    pairwise = np.full((nb_labels, nb_labels), pen_bg, dtype=np.float64)
    pairwise[1:, 1:] = pen_fg
    np.fill_diagonal(pairwise, 0)
    pairwise = np.minimum(pairwise * coef_pairwise, MAX_PAIRWISE_COST)
    return vertexes.tolist(), edges, edge_weights, unary, pairwise


# ------------------------------------------------------------------------------------------------
# cost updates: the threshold tests on the host, the columns by whoever holds the table
# ------------------------------------------------------------------------------------------------


def _update_decisions(points, labels, init_centres, centres, shifts, volumes, shape_model, shape_type, swap_shift, thresholds,
                      object_rays):
    """the per-object part of the two cost updates of the reference (:815-843, :938-982) without the columns: which objects get
    a new column, with which centre, shift and table.  ``centres`` / ``shifts`` / ``volumes`` are updated in place as the reference
    does.  ``object_rays()`` -> the raw 'down' rays [n_objects, A] and is asked for only when an object survives."""
    labels = np.asarray(labels)
    if shape_type not in ('cdf', 'set_cdfs'):
        raise NameError('Not supported type of shape model "%s"' % shape_type)
    mixture = shape_type == 'set_cdfs'
    if mixture:
        model = shape_model[0]
        tables = [np.asarray(table, dtype=np.float64) for _, table in shape_model[1]]
        widest = np.max([table.shape for table in tables], axis=0)
    else:
        single = np.asarray(shape_model[1], dtype=np.float64)
    limit_centre, limit_shift, limit_volume = thresholds['centre']**2, thresholds['shift'], thresholds['volume']
    reach = thresholds['centre_init']
    jobs, rays_all = [], None
    for i in range(len(centres)):
        member = labels == i + 1
        previous = np.array(centres[i])
        position, turn = compute_centre_moment_points(points[member])
        position = np.round(position).astype(int)
        if swap_shift:                                                     # the shake: a quarter turn, taken at once
            turn = (turn + 90) % 360
            shifts[i] = turn
        growth = 0
        if mixture:
            size = np.sum(member)
            growth = np.abs(size - volumes[i]) / float(volumes[i]) if volumes[i] != 0 else 0
        # a centre further than `reach` from where it began is pulled back onto that circle (and is no integer then)
        offset = np.asarray(position) - np.asarray(init_centres[i])
        from_start = np.sum(offset**2)
        if from_start > reach**2:
            position = init_centres[i] + (reach / np.sqrt(from_start)) * offset
        moved = np.sum((np.array(position) - previous)**2)
        settled = moved <= limit_centre and np.abs(turn - shifts[i]) <= limit_shift and growth <= limit_volume
        if settled and not swap_shift:
            continue                                                       # the column of this object stays
        if moved > limit_centre:
            centres[i] = position.tolist()
        if np.abs(turn - shifts[i]) > limit_shift:
            shifts[i] = turn
        if mixture:
            if growth > limit_volume:
                volumes[i] = size
            if rays_all is None:
                rays_all = object_rays()
            share = model.predict_proba([_finish_rays(rays_all[i])[0]]).ravel()
            table = np.zeros(widest)
            for weight, one in zip(share, tables):
                table[:, :one.shape[1]] += weight * one
        else:
            table = single
        jobs.append((i, [float(c) for c in centres[i]], float(shifts[i]), table))
    return jobs


def _mass_centres(sums, labels, n_objects):
    """rounded centre of mass of every object's mask ``labels[slic] == i + 1`` from the exact sums of its superpixels"""
    positions = np.zeros((n_objects, 2), dtype=np.int32)
    for i in range(n_objects):
        count, rows, cols = (int(v) for v in sums[np.asarray(labels) == i + 1].sum(axis=0))
        # (an object without pixels has no centre: the position outside the map gives rays of -1)
        positions[i] = [int(round(rows / float(count))), int(round(cols / float(count)))] if count else [-1, -1]
    return positions


def _public_update(lut_shape_cost, slic, points, labels, init_centres, centres, shifts, volumes, shape_model, shape_type,
                   selected_idx, swap_shift, thresholds):
    """the cost update on a table of the caller: the decisions of :func:`_update_decisions`, the columns in numpy"""
    points, labels = np.asarray(points), np.asarray(labels)
    if len(points) != len(labels):
        raise ValueError('number of points (%i) and labels (%i) should match' % (len(points), len(labels)))
    selected = np.arange(len(points)) if selected_idx is None else np.asarray(list(selected_idx), dtype=int)

    def object_rays():
        from pyimsegm_amd.descriptors import hip_ray_features_positions
        from scipy.ndimage import center_of_mass
        segm = labels.astype(int)[np.asarray(slic)]
        step = 360 / len(shape_model[1][0][1])
        rays = []
        for number in range(1, len(centres) + 1):
            start = [int(round(c)) for c in center_of_mass(segm == number)]
            rays.append(hip_ray_features_positions(segm == number, [start], step, 'down')[0])
        return rays

    jobs = _update_decisions(points, labels, init_centres, centres, shifts, volumes, shape_model, shape_type, swap_shift, thresholds,
                             object_rays)
    for i, centre, shift, table in jobs:
        prior = np.zeros(len(points))                                      # (a point that is not selected has prior 0)
        prior[selected] = shape_prior_points(points[selected], table, centre, shift)
        lut_shape_cost[:, i + 1] = _shape_cost(prior)
    _replace_inf(lut_shape_cost)
    return lut_shape_cost, np.array(centres), np.array(shifts, dtype=float), volumes


def compute_update_shape_costs_points_table_cdf(lut_shape_cost, points, labels, init_centres, centres, shifts, volumes, shape_chist,
                                                selected_idx=None, swap_shift=False, dict_thresholds=None):
    """shape cost columns for the objects whose centre or orientation moved past the thresholds, from one cumulative table
    ``shape_chist = (None, table)`` (reference :750-852; its example is in tests/doctests/region_growing.py)

    :return tuple: lut_shape_cost, centres, shifts, volumes
    """
    return _public_update(lut_shape_cost, None, points, labels, init_centres, centres, shifts, volumes, shape_chist, 'cdf',
                          selected_idx, swap_shift, dict_thresholds or RG2SP_THRESHOLDS)


def compute_update_shape_costs_points_close_mean_cdf(lut_shape_cost, slic, points, labels, init_centres, centres, shifts, volumes,
                                                     shape_model_cdfs, selected_idx=None, swap_shift=False, dict_thresholds=None):
    """as :func:`compute_update_shape_costs_points_table_cdf` for ``shape_model_cdfs = (mixture, [(mean rays, table), ...])``: the
    table of an object is the tables mixed by the mixture's responsibilities for the object's rays, and a change of its size also
    asks for a new column (reference :855-990; the rays of the objects' masks on the device)

    :return tuple: lut_shape_cost, centres, shifts, volumes
    """
    return _public_update(lut_shape_cost, slic, points, labels, init_centres, centres, shifts, volumes, shape_model_cdfs, 'set_cdfs',
                          selected_idx, swap_shift, dict_thresholds or RG2SP_THRESHOLDS)


def update_shape_costs_points(lut_shape_cost, slic, points, labels, init_centres, centres, shifts, volumes, shape_model, shape_type,
                              selected_idx=None, swap_shift=False, dict_thresholds=None):
    """the cost update for either kind of shape model, 'cdf' or 'set_cdfs' (reference :1014-1062)

    :return tuple: lut_shape_cost, centres, shifts, volumes
    """
    if shape_type not in ('cdf', 'set_cdfs'):
        raise NameError('Not supported type of shape model "%s"' % shape_type)
    return _public_update(lut_shape_cost, slic if shape_type == 'set_cdfs' else None, points, labels, init_centres, centres, shifts,
                          volumes, shape_model, shape_type, selected_idx, swap_shift, dict_thresholds or RG2SP_THRESHOLDS)


# ------------------------------------------------------------------------------------------------
# the two growth loops
# ------------------------------------------------------------------------------------------------


class _Growth(object):
    """what both growth functions set up (:1294-1330, :1619-1665) and the steps of an iteration"""

    def __init__(self, slic, slic_prob_fg, centres, shape_model, shape_type, coefs, prob_label_trans, dict_thresholds, on,
                 background_offset):
        slic = np.asarray(slic)
        slic_prob_fg = np.asarray(slic_prob_fg, dtype=np.float64)
        if len(slic_prob_fg) < np.max(slic):
            raise ValueError('dims of probs %s and slic %s not match' % (len(slic_prob_fg), np.max(slic)))
        if shape_type not in ('cdf', 'set_cdfs'):
            raise NameError('Not supported type of shape model "%s"' % shape_type)
        place = _place(on)
        slic_prob_fg = slic_prob_fg[:int(np.max(slic)) + 1]             # (the reference reads no entry past the last label)
        if slic.ndim != 2 or slic.min() < 0 or len(slic_prob_fg) != int(slic.max()) + 1:
            raise ValueError('a 2-D map of labels 0 .. %i is expected for %i probabilities' % (len(slic_prob_fg) - 1, len(slic_prob_fg)))
        self.slic, self.shape_model, self.shape_type = slic, shape_model, shape_type
        self.thresholds = dict_thresholds or RG2SP_THRESHOLDS
        self.init_centres = np.round(centres).astype(int).reshape(-1, 2)
        if len(self.init_centres) == 0:
            raise ValueError('at least one centre is required')
        for centre in self.init_centres:
            if not (0 <= centre[0] < slic.shape[0] and 0 <= centre[1] < slic.shape[1]):
                raise ValueError('centre %r lies outside the map %r' % (tuple(centre.tolist()), slic.shape))
        self.coef_data, self.coef_shape, self.coef_pairwise = coefs
        self.prob_label_trans = prob_label_trans
        self.terms = tuple(coefs) + _penalties(prob_label_trans)
        n_objects = len(self.init_centres)
        self.state = (_DeviceState if place == 'device' else _HostState)(slic, n_objects)
        try:
            sums = self.state.sums()
            self.sums, self.slic_weights = sums, sums[:, 0].copy()
            self.slic_points = self.state.points().astype(int)
            self.edges = np.asarray(self.state.edges).reshape(-1, 2)
            self.slic_neighbours = [[] for _ in range(len(self.slic_points))]
            for a, b in self.edges.tolist():
                self.slic_neighbours[a].append(b)
                self.slic_neighbours[b].append(a)
            self.state.attach(*_csr_neighbours(self.slic_neighbours, len(self.slic_points)))
            labels = np.zeros(len(self.slic_points), dtype=int)
            self.lut_data_cost, self.labels = compute_data_costs_points(slic, slic_prob_fg, self.init_centres, labels)
            lut_shape_cost = np.zeros((len(labels), n_objects + 1))
            with np.errstate(divide='ignore'):
                lut_shape_cost[:, 0] = -np.log(1 - slic_prob_fg + background_offset)
            self.state.set_costs(self.lut_data_cost, _replace_inf(lut_shape_cost))
            self.centres = np.ones(self.init_centres.shape) * np.inf
            self.shifts = np.zeros(n_objects)
            self.volumes = [1] * n_objects
            self.update(self.labels, False)
        except Exception:
            self.state.close()
            raise

    def _object_rays(self, labels):
        nb_angles = len(self.shape_model[1][0][1])
        positions = _mass_centres(self.sums, labels, len(self.init_centres))
        return self.state.object_rays(labels, positions, _ray_directions(float(360 / nb_angles)))

    def update(self, labels, swap_shift):
        """``update_shape_costs_points`` on the resident table"""
        centres = self.centres
        jobs = _update_decisions(self.slic_points, labels, self.init_centres, centres, self.shifts, self.volumes, self.shape_model,
                                 self.shape_type, swap_shift, self.thresholds, lambda: self._object_rays(labels))
        self.centres, self.shifts = np.array(centres), np.array(self.shifts, dtype=float)
        if jobs:
            self.state.update_shape_costs([j[0] for j in jobs], [j[1] for j in jobs], [j[2] for j in jobs], [j[3] for j in jobs])

    def start_history(self, debug_history):
        if debug_history is not None:
            debug_history.update({'criteria': [], 'labels': [], 'centres': [], 'shifts': [],
                                  'lut_data_cost': self.lut_data_cost.copy(), 'lut_shape_cost': []})

    def record(self, debug_history, labels):
        if debug_history is not None:
            debug_history['labels'].append(labels.copy())
            debug_history['criteria'].append(self.state.criterion(labels, *self.terms))
            debug_history['centres'].append(self.centres.copy())
            debug_history['shifts'].append(self.shifts.tolist())
            debug_history['lut_shape_cost'].append(self.state.shape_costs())


def region_growing_shape_slic_greedy(slic, slic_prob_fg, centres, shape_model, shape_type='cdf', coef_data=1., coef_shape=1,
                                     coef_pairwise=1, prob_label_trans=(.1, .01), allow_obj_swap=True, greedy_tol=1e-3,
                                     dict_thresholds=None, nb_iter=999, debug_history=None, on=None):
    """grows one object per centre over the superpixels, greedily: every iteration scores each superpixel next to an object by how
    much the energy falls if the object takes it, and applies the best changes together.  The energy weighs the foreground
    probability, a ray shape prior around the object's centre and orientation, and the labels of neighbours.  When nothing improves
    the orientations are turned by a quarter once (the shake); the growth ends when that does not help either
    (reference :1155-1388; its examples are in tests/doctests/region_growing.py).

    :param ndarray slic: superpixel map, labels 0 .. K - 1
    :param list(float) slic_prob_fg: foreground probability of every superpixel
    :param list(tuple(int,int)) centres: (row, col) where every object starts
    :param shape_model: ``(None, table)`` for 'cdf'; ``(mixture, [(mean rays, table), ...])`` for 'set_cdfs'
    :param str shape_type: 'cdf' or 'set_cdfs'
    :param float coef_data: weight of the data cost
    :param float coef_shape: weight of the shape cost
    :param float coef_pairwise: weight of the edge penalties
    :param prob_label_trans: probability of an edge between background and object, and between two objects
    :param bool allow_obj_swap: an object may take superpixels of another object, not only of the background
    :param float greedy_tol: changes within this relative distance of the best one are applied with it
    :param dict dict_thresholds: in place of ``RG2SP_THRESHOLDS``
    :param int nb_iter: at most this many iterations
    :param dict debug_history: filled with the criteria, labels, centres, shifts and cost tables of every iteration
    :param str on: 'device', 'host' or None (IMSEGM_RG_ON); the rules of the switch are ``_hip.resolve_place``
    :return ndarray: label of every superpixel
    """
    growth = _Growth(slic, slic_prob_fg, centres, shape_model, shape_type, (coef_data, coef_shape, coef_pairwise), prob_label_trans,
                     dict_thresholds, on, 0.)
    try:
        labels, state = growth.labels, growth.state
        shakes = [False]                                   # per iteration: is the next cost update a shake (the reference's list_swap_shift)
        growth.start_history(debug_history)
        for _ in range(nb_iter):
            labels = enforce_center_labels(growth.slic, labels, growth.centres)
            growth.record(debug_history, labels)
            growth.update(labels, shakes[-1])
            objects, superpixels, changes = state.greedy_step(labels, allow_obj_swap, *growth.terms)
            # falling change, equal changes in the order of the candidates (a stable sort, as the reference's sorted(reverse=True))
            order = np.argsort(-np.asarray(changes, dtype=np.float64), kind='stable')
            stuck = len(order) == 0 or changes[order[0]] < 0
            if stuck and any(shakes[-7:]):
                break                                          # a shake within the last seven iterations did not help
            shakes.append(stuck)
            if len(order) == 0:
                continue
            ranked = changes[order]
            with np.errstate(divide='ignore', invalid='ignore'):
                applied = ((ranked[0] - ranked) / ranked[0] < greedy_tol) & (ranked > 0)
            for i in order[applied]:                           # in rank order: the last change of a superpixel stays
                labels[superpixels[i]] = objects[i]
        return labels
    finally:
        growth.state.close()


def region_growing_shape_slic_graphcut(slic, slic_prob_fg, centres, shape_model, shape_type='cdf', coef_data=1., coef_shape=1,
                                       coef_pairwise=2, prob_label_trans=(0.1, 0.03), optim_global=True, allow_obj_swap=True,
                                       dict_thresholds=None, nb_iter=999, debug_history=None, on=None):
    """as :func:`region_growing_shape_slic_greedy`, with a graph cut in place of the greedy step: every iteration cuts the graph
    of the superpixels next to an object and their neighbours (:func:`prepare_graphcut_variables`), for all objects at once or
    object after object.  It ends when a cut changes nothing although the orientations were just shaken, or when the labelling has
    been seen before (reference :1482-1730; its examples are in tests/doctests/region_growing.py).

    :param bool optim_global: one cut for all objects; off: a cost update and a cut per object
    :return ndarray: label of every superpixel
    """
    growth = _Growth(slic, slic_prob_fg, centres, shape_model, shape_type, (coef_data, coef_shape, coef_pairwise), prob_label_trans,
                     dict_thresholds, on, 1e-9)
    try:
        labels, state = growth.labels, growth.state
        seen = [np.zeros(len(labels), dtype=int)]           # every labelling so far, the empty one first
        shakes = [False]
        growth.start_history(debug_history)
        nb_objects = len(growth.init_centres)

        def cut(candidates, result):
            if not len(candidates):
                raise ValueError('no candidate for the graph cut')
            vertexes, links, link_weights, unary, pairwise = prepare_graphcut_variables(
                candidates, growth.slic_points, growth.slic_neighbours, growth.slic_weights, labels, nb_objects, growth.lut_data_cost,
                state.shape_costs(), coef_data, coef_shape, coef_pairwise, prob_label_trans)
            if len(links):
                result[vertexes] = cut_general_graph(np.sort(links, axis=1), link_weights, unary, pairwise, n_iter=999)
                # (a superpixel that is a candidate twice takes the label of its last vertex)

        for _ in range(nb_iter):
            labels = enforce_center_labels(growth.slic, labels, growth.centres)
            growth.record(debug_history, labels)
            after = labels.copy()
            objects, superpixels, _ = state.greedy_step(labels, allow_obj_swap, *growth.terms, with_scores=False)
            if optim_global:
                growth.update(labels, shakes[-1])
                cut(superpixels, after)
            else:
                for number in range(1, nb_objects + 1):
                    growth.update(labels, shakes[-1])
                    cut(superpixels[objects == number], after)
            unchanged = np.array_equal(labels, after)
            if unchanged and (any(shakes[-2:]) or any(np.array_equal(after, old) for old in seen[:-1])):
                break                                          # shaken already, or back at an earlier labelling
            shakes.append(unchanged)
            labels = after
            seen.append(labels.copy())
        return labels
    finally:
        growth.state.close()


# ------------------------------------------------------------------------------------------------
# object segmentation by one graph cut, on pixels and on superpixels (reference :42-256)
# ------------------------------------------------------------------------------------------------


#: bytes of tables and centres ``imsegm_object_cut_pixels`` takes (OBJECT_UNARY_LDS_MAX of csrc/object_cut.h)
OBJECT_TABLES_DEVICE_MAX = 60 * 1024


def pygco_integers(unary, weights, pairwise, weight_max=None):
    """the integer energies pyGCO hands to GCO (gco/pygco.py ``cut_general_graph``): (unary, weights, pairwise, down-weight factor).
    ``weight_max``: enters the maximum of ``|weights|`` (weights of edges the caller has dropped)."""
    unary, weights, pairwise = (np.asarray(a, dtype=np.float64) for a in (unary, weights, pairwise))
    mu = np.max(np.abs(unary)) if unary.size else 0.
    have_edges = len(weights) > 0 or weight_max is not None
    mw = np.max(np.abs(weights)) if len(weights) else 0.
    if weight_max is not None and not weight_max <= mw:
        mw = weight_max
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        scaled = mw * np.max(pairwise)
        dwf = (scaled if have_edges and scaled > mu else mu) + 1e-10
        return (((unary / dwf) * 100000).astype(np.int32), ((weights / dwf) * 1000).astype(np.int32),
                (pairwise * 100).astype(np.int32), dwf)


def _isqrt(values):
    """floor(sqrt(v)) of non-negative integers, as integers"""
    root = np.floor(np.sqrt(values)).astype(np.int64)
    root -= root * root > values
    root += (root + 1) * (root + 1) <= values
    return root


def _object_tables(labels_fg_prob, coef_shape, shape_mean_std, max_dist):
    """the few values the unary costs of an object cut take: A_bg[l] = -log(1 - p[l]), A_fg[l] = -log(p[l]), S_bg[l] = log(1 - p[l])
    and B[d] = log(1 - norm.cdf(d) + 1e-9) for d = 0 .. int(max_dist) (one zero without a shape prior)"""
    prob_fg = np.array(labels_fg_prob, dtype=np.float64)
    prob_bg = 1. - prob_fg
    with np.errstate(divide='ignore', invalid='ignore'):
        a_bg, a_fg, s_bg = -np.log(prob_bg), -np.log(prob_fg), np.log(prob_bg)
    if coef_shape > 0:
        from scipy import stats
        shape_mean, shape_std = shape_mean_std
        cdf = stats.norm.cdf(range(int(max_dist + 1)), shape_mean, shape_std)
        with np.errstate(divide='ignore', invalid='ignore'):
            table = np.log(1. - cdf + 1e-9)
    else:
        table = np.zeros(1)
    return a_bg, a_fg, s_bg, table


def _max_centre_distance(shape, centres):
    """the largest distance between a centre and a pixel (a corner of the image)"""
    corners = np.array([(r, c) for r in (0, shape[0] - 1) for c in (0, shape[1] - 1)], dtype=np.int64)
    diff = corners[None, :, :] - np.array(centres, dtype=np.int64)[:, None, :]
    return float(np.sqrt(np.max(np.sum(diff * diff, axis=2))))


def _seed_window(pos, seed_size):
    """the square of side 2 * seed_size + 1 around a seed as (rows, columns); where it leaves the image the slices come out short
    or empty and numpy refuses to put the disc there"""
    row, col = int(pos[0]), int(pos[1])
    return slice(row - seed_size, row + seed_size + 1), slice(col - seed_size, col + seed_size + 1)


def _seed_disc(seed_size):
    span = np.arange(-seed_size, seed_size + 1)
    return (span[:, None]**2 + span[None, :]**2 <= seed_size**2).astype(np.uint8)


def _object_pixels_unary(segm, centres, tables, coef_shape, seed_size):
    """the float unary costs of :func:`object_segmentation_graphcut_pixels` (reference :214-242) from the tables: per pixel
    u = A - coef_shape * S, the reference's order of operations; the seeds are 0"""
    a_bg, a_fg, s_bg, table = tables
    height, width = segm.shape
    unary = np.empty((height, width, len(centres) + 1))
    use_shape = coef_shape > 0
    unary[:, :, 0] = a_bg[segm] - coef_shape * (s_bg[segm] if use_shape else 0.)
    # (centre[0] is a row and centre[1] a column: the reference names the row index grid_x and the column index grid_y)
    rows, cols = np.indices(segm.shape)
    for i, centre in enumerate(centres):
        if use_shape:
            dist = _isqrt((rows - int(centre[0]))**2 + (cols - int(centre[1]))**2)
            unary[:, :, i + 1] = a_fg[segm] - coef_shape * table[dist]
        else:
            unary[:, :, i + 1] = a_fg[segm] - coef_shape * 0.
    for i, pos in enumerate(centres):
        if seed_size > 0:
            disc = np.zeros(segm.shape, dtype=bool)
            disc[_seed_window(pos, seed_size)] = _seed_disc(seed_size)
            unary[disc & (segm > 0), i + 1] = 0
        else:
            unary[pos[0], pos[1], i + 1] = 0
    return unary


def _object_pixels_refusals(segm, centres, tables, coef_shape, seed_size):
    """what is refused before anything is launched; returns the seeds as rows and columns inside the image"""
    a_bg, a_fg, s_bg, table = tables
    probe = np.empty(segm.shape, dtype=bool)
    seeds = []
    for pos in centres:
        if seed_size > 0:                       # a disc that leaves the image: the reference's slice assignment raises ValueError
            probe[_seed_window(pos, seed_size)] = _seed_disc(seed_size)
        else:
            probe[pos[0], pos[1]] = False       # (IndexError as in the reference; a negative index counts from the end)
        seeds.append((int(pos[0]) % segm.shape[0], int(pos[1]) % segm.shape[1]))
    a_bg[[segm.min(), segm.max()]]              # (IndexError as in the reference)
    present = np.unique(segm)
    costs = [a_bg, a_fg] + ([s_bg] if coef_shape > 0 else [])
    for label in present:
        if not all(np.isfinite(cost[label]) for cost in costs):
            raise ValueError('label %d has a foreground probability of 0 or 1: its unary cost is not finite' % label)
    if not (np.isfinite(coef_shape) and np.all(np.isfinite(table))):
        raise ValueError('the shape prior gives a unary cost that is not finite')
    return seeds


def object_segmentation_graphcut_pixels(segm, centres, labels_fg_prob=(0.1, 0.9), gc_regul=1, seed_size=0, coef_shape=0.,
                                        shape_mean_std=(50., 10.), debug_visual=None, on=None):
    """Label every pixel with 0 (background) or i + 1 (the object grown from centre i) by one alpha-expansion on the 4-connected
    pixel grid (reference :159-256; the answers its docstring prints are in tests/object_cut_cases.py).  The data cost of a pixel
    follows from its class in ``segm`` and, with a shape prior, from its integer distance to the centre (DESIGN.md section 4,
    "Object cuts").

    ``on='device'`` (the default when a device is present; ``IMSEGM_OBJECT_CUT_ON``): the class map, the centres and four small
    tables go up; unary costs, pyGCO's integers, the grid and the cut are computed there (``imsegm_object_cut_pixels``).
    ``on='host'``: the same costs in numpy, cut by ``cut_grid_graph``.  Without an explicit ``on``, an image whose tables exceed
    what the device kernel keeps in LDS (a diagonal of several thousand pixels) takes the numpy costs as well.

    :param ndarray segm: class map, height x width, integer classes that index ``labels_fg_prob``
    :param list(tuple(int,int)) centres: (row, column) per object; rounded to integers
    :param list(float) labels_fg_prob: per class, the probability that a pixel of it is part of an object
    :param float gc_regul: cost of two neighbouring pixels with different labels
    :param int seed_size: radius of the disc around a centre that is bound to its object where the class is not 0; 0: the
        centre pixel alone
    :param float coef_shape: weight of the shape prior, a normal distribution of the distance to the centre; <= 0: none
    :param tuple(float,float) shape_mean_std: mean and standard deviation of that distribution
    :param dict debug_visual: when given, receives ``'unary_imgs'``, the float cost image of every label
    :param str on: ``'device'``, ``'host'`` or None
    :return ndarray: int32 labels, height x width
    """
    if np.min(labels_fg_prob) >= 1:
        raise ValueError('non label can ce strictly 1')
    segm = np.asarray(segm)
    if segm.max() > len(labels_fg_prob):
        raise ValueError('table of label proba is shorter then the nb of labels in segmentation')
    if not list(centres):
        raise ValueError('at least one center has to be given')
    centres = [np.round(c).astype(int) for c in centres]
    place = _place(on, 'IMSEGM_OBJECT_CUT_ON')
    tables = _object_tables(labels_fg_prob, coef_shape, shape_mean_std, _max_centre_distance(segm.shape, centres))
    seeds = _object_pixels_refusals(segm, centres, tables, coef_shape, seed_size)
    if on is None and place == 'device' and sum(t.nbytes for t in tables) + 16 * len(centres) > OBJECT_TABLES_DEVICE_MAX:
        place = 'host'                          # (asked for explicitly, the device entry refuses such tables)
    unary = None
    if place == 'host' or debug_visual is not None:
        unary = _object_pixels_unary(segm, centres, tables, coef_shape, seed_size)
    if place == 'host':
        height, width = segm.shape
        pairwise = (1 - np.eye(len(centres) + 1)) * gc_regul
        labels = cut_grid_graph(unary, pairwise, np.ones((height - 1, width)), np.ones((height, width - 1)), n_iter=999)
        segm_obj = np.asarray(labels).reshape(segm.shape)
    else:
        rows = np.array([[c[0], c[1], s[0], s[1]] for c, s in zip(centres, seeds)], dtype=np.int32)
        segm_obj, _ = _hip.object_cut_pixels(segm, rows, *tables, coef_shape=coef_shape, gc_regul=gc_regul, seed_size=max(seed_size, 0),
                                             n_iter=999)
    if debug_visual is not None:
        debug_visual['unary_imgs'] = [unary[:, :, i] for i in range(unary.shape[-1])]
    return segm_obj


def _object_slic_terms(slic, labels, slic_points, edges, centres, labels_fg_prob, gc_regul, edge_coef, edge_type, coef_shape,
                       shape_mean_std, add_neighbours):
    """The graph :func:`object_segmentation_graphcut_slic` cuts, from the class of every superpixel (``labels``), the superpixel
    centres and the adjacency: (edges, edge weights, unary, pairwise, weight maximum).

    The unary costs come from the tables of the pixel variant (:func:`_object_tables`), read at the class of a superpixel and at
    the truncated distance between its centre and the object's; the superpixel under a centre costs 0 for its object, and no
    cost is below ``-log(MAX_UNARY_PROB)``.  With ``add_neighbours`` the neighbours of that superpixel cost 0 as well, and the
    reference turns every edge at it into (0, 0), centre after centre: such self-edges still count where the 'model' weights take
    their standard deviation, then they are dropped, and the largest of their weights is returned for pyGCO's scaling (None where
    nothing was dropped)."""
    points = np.asarray(slic_points, dtype=np.float64)
    ends = np.array(edges)
    n_columns = len(centres) + 1
    use_shape = coef_shape > 0
    dists = [np.sqrt(np.sum((points - centre)**2, axis=1)) for centre in centres] if use_shape else []
    a_bg, a_fg, s_bg, table = _object_tables(labels_fg_prob, coef_shape, shape_mean_std, max([d.max() for d in dists] + [0.]))
    unary_cost = np.empty((len(labels), n_columns))
    unary_cost[:, 0] = a_bg[labels] - coef_shape * (s_bg[labels] if use_shape else 0.)
    for column in range(1, n_columns):
        unary_cost[:, column] = a_fg[labels] - coef_shape * (table[dists[column - 1].astype(int)] if use_shape else 0.)
    for column, centre in enumerate(centres, 1):
        seed = int(slic[centre[0], centre[1]])
        unary_cost[seed, column] = 0.
        if add_neighbours:
            touching = (ends == seed).any(axis=1)
            unary_cost[np.unique(ends[touching]), column] = 0.
            ends[touching] = 0
    np.maximum(unary_cost, -np.log(MAX_UNARY_PROB), out=unary_cost)
    if edge_type == 'model':
        class_fg = np.asarray(labels_fg_prob, dtype=np.float64)[labels]
        gap = np.abs(class_fg[ends[:, 0]] - class_fg[ends[:, 1]])
        with np.errstate(divide='ignore', invalid='ignore'):
            edge_weights = np.exp(-gap / (2 * np.std(gap)**2)) / compute_spatial_dist(points, ends, relative=True)
    else:
        edge_weights = np.ones(len(ends))
    edge_weights = edge_weights * edge_coef
    pairwise_cost = (1 - np.eye(n_columns)) * gc_regul
    keep = ends[:, 0] != ends[:, 1]
    weight_max = None
    if not keep.all():
        dropped = np.abs(edge_weights[~keep])
        weight_max = float('nan') if np.isnan(dropped).any() else float(dropped.max())
    return ends[keep], edge_weights[keep], unary_cost, pairwise_cost, weight_max


def object_segmentation_graphcut_slic(slic, segm, centres, labels_fg_prob=(0.1, 0.9), gc_regul=1, edge_coef=0.5, edge_type='model',
                                      coef_shape=0., shape_mean_std=(50., 10.), add_neighbours=False, debug_visual=None):
    """Label every superpixel with 0 (background) or i + 1 (the object of centre i) by one alpha-expansion on the superpixel
    adjacency graph (reference :42-156; the answers its docstring prints are in tests/object_cut_cases.py).  A composition of
    ``histogram_regions_labels_norm``, ``superpixel_centers``, ``get_vertexes_edges``, ``compute_spatial_dist`` and the general
    cut, all of which run on the device; the terms between them are numpy (:func:`_object_slic_terms`).

    :param ndarray slic: superpixel map, height x width
    :param ndarray segm: class map of the same shape; a superpixel takes the class most of its pixels have
    :param list(tuple(int,int)) centres: (row, column) per object; rounded to integers
    :param list(float) labels_fg_prob: per class, the probability that a superpixel of it is part of an object
    :param float gc_regul: cost of two neighbouring superpixels with different labels
    :param float edge_coef: factor on every edge weight
    :param str edge_type: ``'model'``: weights from the difference of the two class probabilities and the distance of the two
        centres; anything else: all edges weigh the same
    :param float coef_shape: weight of the shape prior, a normal distribution of the distance to the centre; <= 0: none
    :param tuple(float,float) shape_mean_std: mean and standard deviation of that distribution
    :param bool add_neighbours: bind the neighbours of the superpixel under a centre to its object too
    :param dict debug_visual: when given, receives ``'unary_imgs'``, the cost of every label as an image
    :return ndarray: int32 label per superpixel
    """
    from pyimsegm_amd.superpixels import superpixel_centers
    if np.min(labels_fg_prob) >= 1:
        raise ValueError('non label can ce strictly 1')
    slic, segm = np.asarray(slic), np.asarray(segm)
    labels = np.argmax(histogram_regions_labels_norm(slic, segm), axis=1)
    if segm.max() > len(labels_fg_prob):
        raise ValueError('table of label prob is shorter then the nb of labels in segmentation')
    if not list(centres):
        raise ValueError('at least one center has to be given')
    centres = [np.round(c).astype(int) for c in centres]
    edges, edge_weights, unary_cost, pairwise_cost, weight_max = _object_slic_terms(
        slic, labels, superpixel_centers(slic), get_vertexes_edges(slic)[1], centres, labels_fg_prob, gc_regul, edge_coef, edge_type,
        coef_shape, shape_mean_std, add_neighbours)
    graph_labels = _cut_scaled(edges, edge_weights, unary_cost, pairwise_cost, weight_max, n_iter=999)
    if debug_visual is not None:
        debug_visual['unary_imgs'] = [unary_cost[:, i][slic] for i in range(unary_cost.shape[-1])]
    return graph_labels


def _cut_scaled(edges, edge_weights, unary_cost, pairwise_cost, weight_max, n_iter):
    """the general cut; with dropped self-edges the entry that takes their weight maximum ("Object cuts")"""
    if weight_max is None:
        return cut_general_graph(edges, edge_weights, unary_cost, pairwise_cost, n_iter=n_iter)
    if np.isnan(weight_max):
        raise ValueError('an edge at a seed has a weight that is not a number')
    return _hip.cut_general_graph_scaled(edges, edge_weights, unary_cost, pairwise_cost, weight_max, n_iter=n_iter)
