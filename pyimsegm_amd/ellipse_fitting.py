"""Ellipse fitting for egg candidates: the RANSAC of the reference's ``imsegm/ellipse_fitting.py`` (``EllipseModelSegm``,
``ransac_segm``, ``get_slic_points_labels``) with the scoring of all trials on the device.

* ``EllipseModelSegm.estimate`` is the Halir-Flusser direct fit as scikit-image 0.18.3 states it (``skimage/measure/fit.py``
  ``EllipseModel.estimate``), in numpy on the host, for one sample set or a stack of them (:func:`estimate_stack`).  scikit-image is
  not imported.
* A RANSAC run draws the samples of every trial first (``np.random.choice`` once per trial in trial order: the global stream is
  consumed exactly as the reference's loop consumes it), estimates every trial on the host, and hands all trials of all egg
  candidates to ``imsegm_ellipse_ransac`` (csrc/ellipse.hip): the region criterion of every trial, the point-to-ellipse distance
  of every (trial, point) pair and the reference's update rule per egg.  ``on='host'`` computes the same three definitions in
  numpy (:func:`score_trials_host`) -- the CPU statement the kernels are tested against.
* The winner is re-estimated from the kept inliers on the host, as the reference does.
* The step in front of the RANSAC -- ``split_segm_background_foreground`` and ``prepare_boundary_points_ray_join`` / ``_edge`` /
  ``_mean`` / ``_dist`` -- smooths the class map and casts the rays of all centres on the device (``imsegm_boundary_rays``,
  csrc/morphology.hip); what follows the rays (at most 72 values per centre) is the reference's numpy in float64.  ``on='host'`` is
  the scipy / numpy statement of the same definitions (:func:`split_host`, :func:`ray_walk_host`).
* The step behind the fits -- ``add_overlap_ellipse`` / ``add_overlap_ellipses`` and ``ellipse_label_overlaps`` -- rasterises the
  ellipses (scikit-image's ``draw.ellipse``, restated as :func:`ellipse_pixels_host`) and applies the reference's overlap test on the
  device (``imsegm_ellipse_place`` / ``imsegm_ellipse_overlaps``, csrc/ellipse_place.hip); ``on='host'`` is the numpy statement
  (:func:`place_host`, :func:`overlaps_host`).  ``filter_boundary_points`` and ``prepare_boundary_points_close`` compose device calls
  of ``pyimsegm_amd.superpixels``.

Definitions ("Ellipse RANSAC"): the criterion keeps the reference's ``weights[labels_in]`` -- the weight is
looked up by the CLASS LABEL of a centre inside the ellipse, not by the centre; the residual is the distance to the closest
point of the ellipse in the basin of skimage's starting parameter (what its ``leastsq`` converges to, not its iteration).
"""
import numpy as np

from pyimsegm_amd import _hip
from pyimsegm_amd.descriptors import ray_walk_host  # noqa: F401  (the one host walk, also under this module's name)

#: what the reference's rays are clamped to from below (its spelling)
MIN_ELLIPSE_DAIM = 25.
#: radius of the disc the background / the foreground mask is opened with
STRUC_ELEM_BG = 15
STRUC_ELEM_FG = 5
#: cap of the closest-point iteration (``ER_ITERATIONS`` of csrc/ellipse.hip)
DISTANCE_ITERATIONS = 128
_CONSTRAINT_INV = np.linalg.inv(np.array([[0., 0., 2.], [0., -1., 0.], [2., 0., 0.]]))


def _positive(values):
    """``values > 0`` with numpy's ordering of complex numbers (real part first, then the imaginary part)"""
    values = np.asarray(values)
    if np.iscomplexobj(values):
        return (values.real > 0) | ((values.real == 0) & (values.imag > 0))
    return values > 0


def _conic_to_params(a, b, c, d, f, g):
    """centre, semi-axes and angle of a x^2 + b x y + c y^2 + d x + f y + g = 0 (arrays or scalars, real or complex); the steps
    and their order are those of scikit-image 0.18.3"""
    b = b / 2.
    d = d / 2.
    f = f / 2.
    x0 = (c * d - b * f) / (b * b - a * c)
    y0 = (a * f - b * d) / (b * b - a * c)
    numerator = a * (f * f) + c * (d * d) + g * (b * b) - 2 * b * d * f - a * c * g
    term = np.sqrt((a - c) * (a - c) + 4 * (b * b))
    denominator1 = (b * b - a * c) * (term - (a + c))
    denominator2 = (b * b - a * c) * (- term - (a + c))
    width = np.sqrt(2 * numerator / denominator1)
    height = np.sqrt(2 * numerator / denominator2)
    phi = 0.5 * np.arctan((2. * b) / (a - c))
    phi = np.where(_positive(a - c), phi + 0.5 * np.pi, phi)
    return np.real(np.nan_to_num(np.stack([x0, y0, width, height, phi], axis=-1)))


def estimate_stack(samples):
    """the direct ellipse fit of a stack of sample sets, ``samples`` [T, m, 2]: (params float64 [T, 5], success bool [T]).
    A trial fails on a singular scatter matrix or when other than one eigenvector meets 4ac - b^2 > 0; its params are zeros."""
    samples = np.asarray(samples, dtype=np.float64)
    if samples.ndim != 3 or samples.shape[2] != 2:
        raise ValueError('Input data must have shape (T, N, 2).')
    count = len(samples)
    params, success = np.zeros((count, 5)), np.zeros(count, dtype=bool)
    if count == 0:
        return params, success
    x, y = samples[..., 0], samples[..., 1]
    quad = np.ascontiguousarray(np.stack([x * x, x * y, y * y], axis=1))          # [T, 3, m]: the transposed design matrices
    lin = np.ascontiguousarray(np.stack([x, y, np.ones_like(x)], axis=1))
    s1 = quad @ quad.transpose(0, 2, 1)
    s2 = quad @ lin.transpose(0, 2, 1)
    s3 = lin @ lin.transpose(0, 2, 1)
    with np.errstate(all='ignore'):
        try:
            s3_inv = np.linalg.inv(s3)
        except np.linalg.LinAlgError:
            if count == 1:
                return params, success
            for i in range(count):                                               # find the singular ones one by one
                one, good = estimate_stack(samples[i:i + 1])
                params[i], success[i] = one[0], good[0]
            return params, success
        reduced = _CONSTRAINT_INV @ (s1 - s2 @ s3_inv @ s2.transpose(0, 2, 1))
        vectors = np.linalg.eig(reduced)[1]
        if np.iscomplexobj(vectors):
            # a stack comes back complex as soon as one matrix has complex eigenvalues: every matrix gets the type it has alone
            alone = [np.linalg.eig(m)[1] for m in reduced]
            real = np.array([not np.iscomplexobj(v) for v in alone])
        else:
            alone, real = None, np.ones(count, dtype=bool)
        back = -s3_inv @ s2.transpose(0, 2, 1)
        if real.any():
            rows = np.nonzero(real)[0]
            vec = vectors[rows].real if alone is not None else vectors
            cond = 4 * vec[:, 0, :] * vec[:, 2, :] - vec[:, 1, :] * vec[:, 1, :]
            chosen = cond > 0
            valid = chosen.sum(axis=1) == 1
            first = np.ascontiguousarray(np.take_along_axis(vec, np.argmax(chosen, axis=1)[:, None, None], axis=2))   # [R, 3, 1]
            second = back[rows] @ first
            fitted = _conic_to_params(first[:, 0, 0], first[:, 1, 0], first[:, 2, 0], second[:, 0, 0], second[:, 1, 0], second[:, 2, 0])
            params[rows[valid]] = fitted[valid]
            success[rows[valid]] = True
        for i in np.nonzero(~real)[0]:
            vec = alone[i]
            chosen = _positive(4 * vec[0, :] * vec[2, :] - vec[1, :] * vec[1, :])
            if chosen.sum() != 1:
                continue
            first = vec[:, chosen]
            second = (back[i] @ first).ravel()
            params[i] = _conic_to_params(*first.ravel(), *second)
            success[i] = True
    return params, success


def ellipse_distances(points, params):
    """distance of points [..., 2] to the ellipses params [..., 5] (broadcast against each other) at the closest point of the
    ellipse in the basin of ``t0 = arctan2(y - yc, x - xc) - theta``: the numpy statement of ``ellipse_distance`` in
    csrc/ellipse.hip, operation by operation.  In the ellipse's frame t0 is the polar angle of the point, so it lies in the
    point's quadrant, where the derivative of the squared distance changes sign once -- at the closest point of the whole ellipse.
    NaN parameters give NaN."""
    points, params = np.asarray(points, dtype=np.float64), np.asarray(params, dtype=np.float64)
    shape = np.broadcast_shapes(points.shape[:-1], params.shape[:-1])
    px, py = (np.broadcast_to(points[..., i], shape).ravel() for i in range(2))
    xc, yc, a, b, theta = (np.broadcast_to(params[..., i], shape).ravel() for i in range(5))
    with np.errstate(all='ignore'):
        ctheta, stheta = np.cos(theta), np.sin(theta)
        dx, dy = px - xc, py - yc
        u, v = np.abs(dx * ctheta + dy * stheta), np.abs(dy * ctheta - dx * stheta)
        a, b = np.abs(a), np.abs(b)
        big_a, big_b, big_c = a * u, b * v, b * b - a * a
        lo, hi, t = np.zeros_like(u), np.full_like(u, 1.5707963267948966), np.arctan2(v, u)
        before = hi.copy()
        active = np.arange(len(t))
        for _ in range(DISTANCE_ITERATIONS):
            if len(active) == 0:
                break
            ta = t[active]
            s, c = np.sin(ta), np.cos(ta)
            g = big_a[active] * s - big_b[active] * c + big_c[active] * s * c
            dg = big_a[active] * c + big_b[active] * s + big_c[active] * (c * c - s * s)
            sign = np.where((g == 0.0) & (dg < 0.0), np.where(ta < 0.7853981633974483, -1.0, 1.0), g)
            lo[active] = np.where(sign < 0.0, ta, lo[active])
            hi[active] = np.where(sign > 0.0, ta, hi[active])
            moving = (sign < 0.0) | (sign > 0.0)
            step = g / dg
            nxt = ta - step
            la, ha = lo[active], hi[active]
            newton = (dg > 0.0) & (nxt >= la) & (nxt <= ha) & (np.abs(step + step) <= np.abs(before[active]))
            nxt = np.where(newton, nxt, 0.5 * (la + ha))
            before[active] = np.where(newton, step, ha - la)
            moving &= nxt != ta
            t[active[moving]] = nxt[moving]
            active = active[moving]
        ex, ey = u - a * np.cos(t), v - b * np.sin(t)
        return np.sqrt(ex * ex + ey * ey).reshape(shape)


def _table_q(table_prob, labels):
    """-log of the 2 x C table of foreground / background probabilities ``criterion`` accepts (a vector or a one-row matrix of
    foreground probabilities gets its complement as second row)"""
    table_prob = np.array(table_prob)
    if 1 in (table_prob.ndim, table_prob.shape[0]):
        if table_prob.shape[0] == 1:
            table_prob = table_prob[0]
        table_prob = np.array([table_prob, 1. - table_prob])
    if table_prob.shape[0] != 2:
        raise ValueError('table shape %r' % (table_prob.shape, ))
    if np.max(labels) >= table_prob.shape[1]:
        raise ValueError('labels (%i) exceed the table %r' % (np.max(labels), table_prob.shape))
    with np.errstate(divide='ignore'):
        return -np.log(table_prob)


def point_values(points, weights, labels, table_prob):
    """what a centre adds to the criterion when it lies inside: ``weights[labels[n]] * (q[0, labels[n]] - q[1, labels[n]])`` --
    the weight of the centre's CLASS LABEL, as the reference indexes it"""
    if not len(points) == len(weights) == len(labels):
        raise ValueError('different sizes for points %i and weights %i and labels %i' % (len(points), len(weights), len(labels)))
    table_q = _table_q(table_prob, labels)
    classes = np.asarray(labels).astype(int)
    with np.errstate(invalid='ignore'):
        return np.asarray(weights)[classes] * (table_q[0, classes] - table_q[1, classes])


def inside_ellipses(points, params):
    """the reference's inside test of centres [N, 2] against ellipses [T, 5] (r_org, c_org, r_rad, c_rad, phi): bool [T, N]; a zero
    or NaN radius gives inf / NaN and a comparison that is false"""
    points, params = np.asarray(points, dtype=np.float64), np.asarray(params, dtype=np.float64).reshape(-1, 5)
    sin_phi, cos_phi = np.sin(params[:, 4])[:, None], np.cos(params[:, 4])[:, None]
    r, c = points[None, :, 0] - params[:, 0:1], points[None, :, 1] - params[:, 1:2]
    with np.errstate(all='ignore'):
        dist_1 = ((r * cos_phi + c * sin_phi) / params[:, 2:3]) ** 2
        dist_2 = ((r * sin_phi - c * cos_phi) / params[:, 3:4]) ** 2
        return (dist_1 + dist_2) <= 1


class EllipseModelSegm(object):
    """Total least squares estimator of 2-D ellipses with the region criterion of the egg segmentation; ``params`` is
    ``[xc, yc, a, b, theta]``.  Stand-alone: the estimator of scikit-image's ``EllipseModel`` restated in numpy."""

    def __init__(self):
        self.params = None

    def estimate(self, data):
        """direct least-squares fit to points [N, 2]; True on success (``params`` set), False otherwise (``params`` kept)"""
        data = np.asarray(data)
        if data.ndim != 2 or data.shape[1] != 2:
            raise ValueError('Input data must have shape (N, 2).')
        params, success = estimate_stack(data[None])
        if not success[0]:
            return False
        self.params = [float(v) for v in params[0]]
        return True

    def residuals(self, data):
        """shortest distance of every point [N, 2] to the ellipse (in the basin of scikit-image's starting parameter)"""
        data = np.asarray(data)
        if data.ndim != 2 or data.shape[1] != 2:
            raise ValueError('Input data must have shape (N, 2).')
        return ellipse_distances(data, np.asarray(self.params, dtype=np.float64))

    def predict_xy(self, t, params=None):
        """points of the ellipse at the angles ``t``: [..., 2]"""
        xc, yc, a, b, theta = self.params if params is None else params
        t = np.asarray(t)
        ct, st, ctheta, stheta = np.cos(t), np.sin(t), np.cos(theta), np.sin(theta)
        x = xc + a * ctheta * ct - b * stheta * st
        y = yc + a * stheta * ct + b * ctheta * st
        return np.concatenate((x[..., None], y[..., None]), axis=t.ndim)

    def criterion(self, points, weights, labels, table_prob=(0.1, 0.9)):
        """region criterion of the ellipse over superpixel centres ``points`` [N, 2] with class ``labels`` [N]: the sum over the
        centres inside of ``weights[label] * (q[0, label] - q[1, label])``, q = -log(table_prob).  ``table_prob`` is a vector (or
        one-row matrix) of foreground probabilities per class, or a 2 x C matrix of foreground and background probabilities."""
        value = point_values(points, weights, labels, table_prob)
        inside = inside_ellipses(np.asarray(points), self.params)[0]
        return np.sum(value[inside])


def score_trials_host(point_offsets, points, params, success, trial_egg, points_all, point_value, residual_threshold,
                      with_residuals=False):
    """the numpy statement of ``imsegm_ellipse_ransac`` (same arguments and results as ``_hip.ellipse_ransac``)"""
    point_offsets, trial_egg = np.asarray(point_offsets, dtype=np.int64), np.asarray(trial_egg, dtype=np.int64)
    points, params = np.asarray(points, dtype=np.float64).reshape(-1, 2), np.asarray(params, dtype=np.float64).reshape(-1, 5)
    success = np.asarray(success).astype(bool)
    n_eggs = len(point_offsets) - 1
    best, kept = np.full(n_eggs, -1, dtype=np.int32), np.full(n_eggs, -1, dtype=np.int32)
    mask = np.zeros(len(points), dtype=np.uint8)
    criterion = np.full(len(params), np.nan)
    if success.any():
        inside = inside_ellipses(points_all, params[success])
        # a fixed-length sum per trial (outside centres add 0.0): equal inside sets give equal bytes
        criterion[success] = np.where(inside, np.asarray(point_value, dtype=np.float64)[None, :], 0.0).sum(axis=1)
    residuals = []
    for egg in range(n_eggs):
        trials = np.nonzero(trial_egg == egg)[0]
        own = points[point_offsets[egg]:point_offsets[egg + 1]]
        dist = np.full((len(trials), len(own)), np.nan)
        good = success[trials]
        if good.any():
            dist[good] = ellipse_distances(own[None, :, :], params[trials[good]][:, None, :])
        residuals.append(dist.ravel())
        with np.errstate(invalid='ignore'):
            inliers = np.abs(dist) < residual_threshold
        best_fit, best_count = np.inf, 0
        for i, t in enumerate(trials):
            if not good[i] or not criterion[t] < best_fit:
                continue
            best[egg], best_fit = i, criterion[t]
            if inliers[i].sum() > best_count:
                kept[egg], best_count = i, inliers[i].sum()
        if kept[egg] >= 0:
            mask[point_offsets[egg]:point_offsets[egg + 1]] = inliers[kept[egg]]
    residuals = np.concatenate(residuals) if with_residuals and residuals else None
    return best, kept, mask, criterion, residuals


def _place(on):
    """'host' or 'device': ``_hip.resolve_place`` on IMSEGM_RANSAC_ON"""
    return _hip.resolve_place(on, 'IMSEGM_RANSAC_ON', False)[0]


def _nb_samples(min_samples, nb_points):
    if isinstance(min_samples, float):
        if not 0 < min_samples <= 1:
            raise ValueError("`min_samples` as ration must be in range (0, 1]")
        min_samples = int(min_samples * nb_points)
    if not 0 < min_samples <= nb_points:
        raise ValueError("`min_samples` must be in range (0, <nb-samples>]")
    return min_samples


def _ransac_generic(points, model_class, points_all, weights, labels, table_prob, min_samples, residual_threshold, max_trials):
    """the plain per-trial loop for any model class (estimate / residuals / criterion), on the host"""
    best_model, best_inliers, best_count, best_fit = None, None, 0, np.inf
    for _ in range(max_trials):
        model = model_class()
        success = model.estimate(points[np.random.choice(len(points), min_samples, replace=False)])
        if success is not None and not success:
            continue
        inliers = np.abs(model.residuals(points)) < residual_threshold
        fit = model.criterion(points_all, weights, labels, table_prob)
        if fit < best_fit:
            best_model, best_fit = model, fit
            if np.sum(inliers) > best_count:
                best_inliers, best_count = inliers, np.sum(inliers)
    if best_inliers is not None:
        best_model.estimate(points[best_inliers])
    return best_model, best_inliers


def ransac_segm_batch(list_points, points_all, weights, labels, table_prob, min_samples, residual_threshold=1, max_trials=100,
                      on=None, _details=None):
    """:func:`ransac_segm` with ``EllipseModelSegm`` for the boundary points of every centre of an image, all trials of all centres
    scored in one launch chain: the list of ``(model, inliers)`` that ``ransac_segm`` returns centre by centre, in order, on the
    same random stream."""
    place = _place(on)
    list_points = [np.array(points) for points in list_points]
    counts = [_nb_samples(min_samples, len(points)) for points in list_points]
    if max_trials < 0:
        raise ValueError("`max_trials` must be greater than zero")
    # every sample of every trial first: nothing else reads the random stream in between
    drawn = [np.array([np.random.choice(len(points), count, replace=False) for _ in range(max_trials)], dtype=np.int64).reshape(-1, count)
             for points, count in zip(list_points, counts)]
    if not list_points or max_trials == 0:
        return [(None, None)] * len(list_points)
    fits = [estimate_stack(points[idx]) for points, idx in zip(list_points, drawn)]
    params, success = np.concatenate([f[0] for f in fits]), np.concatenate([f[1] for f in fits])
    trial_egg = np.repeat(np.arange(len(list_points), dtype=np.int32), max_trials)
    offsets = np.concatenate([[0], np.cumsum([len(points) for points in list_points])]).astype(np.int32)
    all_points = np.concatenate([np.asarray(points, dtype=np.float64).reshape(-1, 2) for points in list_points])
    if not success.any():
        return [(None, None)] * len(list_points)
    value = point_values(points_all, weights, labels, table_prob)
    score = _hip.ellipse_ransac if place == 'device' else score_trials_host
    best, kept, mask, criterion, residuals = score(offsets, all_points, params, success, trial_egg,
                                                   np.asarray(points_all, dtype=np.float64), value, residual_threshold,
                                                   with_residuals=_details is not None)
    if _details is not None:
        _details.update(samples=drawn, params=params, success=success, best=best, kept=kept, criterion=criterion, residuals=residuals)
    results = []
    for egg, points in enumerate(list_points):
        if best[egg] < 0:
            results.append((None, None))
            continue
        model = EllipseModelSegm()
        model.params = [float(v) for v in params[egg * max_trials + best[egg]]]
        inliers = None
        if kept[egg] >= 0:
            inliers = mask[offsets[egg]:offsets[egg + 1]].astype(bool)
            model.estimate(points[inliers])
        results.append((model, inliers))
    return results


def ransac_segm(points, model_class, points_all, weights, labels, table_prob, min_samples, residual_threshold=1, max_trials=100,
                on=None):
    """Fit a model to ``points`` [N, 2] with the reference's RANSAC: per trial a random sample of ``min_samples`` points (an int, or
    a float ratio of N) is fitted; the trial with the lowest region criterion over the superpixel centres ``points_all`` (class
    ``labels``, ``weights`` and ``table_prob`` as in :meth:`EllipseModelSegm.criterion`) gives the model, and the inlier mask
    (``|residual| < residual_threshold``) follows it only when it has more inliers than the mask kept so far; the model is
    re-estimated from the kept inliers.  Returns ``(model, inliers)``, or ``(None, None)`` when no trial succeeded.

    With ``model_class=EllipseModelSegm`` all trials are scored at once, ``on='device'`` by ``imsegm_ellipse_ransac``, ``on='host'``
    by the numpy statement of the same definitions (``on=None``: the environment variable ``IMSEGM_RANSAC_ON``; the rules every
    ``on=`` keyword of this module follows are ``_hip.resolve_place``); any other model class runs the plain per-trial loop on the
    host."""
    if model_class is EllipseModelSegm:
        return ransac_segm_batch([points], points_all, weights, labels, table_prob, min_samples, residual_threshold, max_trials, on)[0]
    points = np.array(points)
    min_samples = _nb_samples(min_samples, len(points))
    if max_trials < 0:
        raise ValueError("`max_trials` must be greater than zero")
    return _ransac_generic(points, model_class, points_all, weights, labels, table_prob, min_samples, residual_threshold, max_trials)


def get_slic_points_labels(segm, img=None, slic_size=20, slic_regul=0.1):
    """SLIC superpixels of ``img`` (default: the segmentation scaled to [0, 1]) on the device, their centres as integers and the
    label of ``segm`` at every centre: ``(slic, centres [K, 2], labels [K])``"""
    from pyimsegm_amd.superpixels import segment_slic_img2d, superpixel_centers
    if img is None:
        img = segm / float(segm.max())
    slic = segment_slic_img2d(img, sp_size=slic_size, relative_compact=slic_regul)
    slic_centers = np.array(superpixel_centers(slic)).astype(int)
    labels = segm[slic_centers[:, 0], slic_centers[:, 1]]
    return slic, slic_centers, labels


# ------------------------------------------------------------------------------------------------
# from a class map with centre candidates to the boundary points of every centre (reference ellipse_fitting.py:352-597)
# ------------------------------------------------------------------------------------------------


def _points_place(on):
    """'host' or 'device': ``_hip.resolve_place`` on IMSEGM_BOUNDARY_POINTS_ON"""
    return _hip.resolve_place(on, 'IMSEGM_BOUNDARY_POINTS_ON', False)[0]


def _integer_radii(*radii):
    return all(float(r) == int(r) for r in radii)


def fill_holes_host(mask):
    """``scipy.ndimage.binary_fill_holes(mask)`` as the device states it: the mask plus every 4-connected component of its zero
    pixels that has no pixel on the image border"""
    from scipy import ndimage
    mask = np.asarray(mask, dtype=bool)
    zeros, _ = ndimage.label(~mask)                                # the default structure: 4-connected
    border = np.concatenate([zeros[0], zeros[-1], zeros[:, 0], zeros[:, -1]])
    return mask | ((zeros > 0) & ~np.isin(zeros, border[border > 0]))


def opening_host(mask, radius):
    """``skimage.morphology.opening(mask, disk(radius))`` for an integer radius (scikit-image 0.18.3: scipy's grey erosion and
    dilation with boundary mode 'reflect') as two thresholds of exact distances inside the image: a pixel survives the erosion
    when its squared distance to the nearest 0 is > radius^2 (a mask without a 0 stays as it is), and is set by the dilation when
    its squared distance to the nearest survivor is <= radius^2.  A mirrored pixel is never nearer than its original, so the
    reflected border adds nothing.  (``distance_transform_edt`` returns the correctly rounded root of an integer, and
    sqrt(n) > radius exactly when n > radius^2.)"""
    from scipy import ndimage
    mask = np.asarray(mask, dtype=bool)
    radius = int(radius)
    if not mask.all():
        mask = ndimage.distance_transform_edt(mask) > radius
    if not mask.any():
        return mask
    return ndimage.distance_transform_edt(~mask) <= radius


def split_host(seg, sel_bg=STRUC_ELEM_BG, sel_fg=STRUC_ELEM_FG, with_fg=True):
    """the scipy / numpy statement of ``imsegm_split_background_foreground`` for integer radii: (seg_bg, seg_fg) bool"""
    seg = np.asarray(seg)
    seg_bg = ~fill_holes_host(seg > 0)
    if sel_bg > 0:
        seg_bg = opening_host(seg_bg, sel_bg)
    seg_fg = None
    if with_fg:
        seg_fg = seg == 1
        if sel_fg > 0:
            seg_fg = opening_host(seg_fg, sel_fg)
    return seg_bg, seg_fg


def boundary_rays_host(seg, sel_bg, sel_fg, positions, directions, with_fg=True):
    """the scipy / numpy statement of ``imsegm_boundary_rays`` (same arguments and results as ``_hip.boundary_rays``)"""
    seg_bg, seg_fg = split_host(seg, sel_bg, sel_fg, with_fg)
    return ray_walk_host(seg_bg, positions, directions, 1), (ray_walk_host(seg_fg, positions, directions, -1) if with_fg else None)


def _on_device(place, *radii):
    """the device takes the call: asked for (or present) and every radius within ``IMSEGM_MORPH_MAX_RADIUS``"""
    return place == 'device' and max(radii) <= _hip.MORPH_MAX_RADIUS


def _split_skimage(seg, sel_bg, sel_fg):
    """the reference's statement itself, for radii that are no integers (``disk(1.5)`` is an even-sided footprint that
    scikit-image shifts by its own rules)"""
    from scipy import ndimage
    from skimage import morphology
    seg_bg = 1 - ndimage.binary_fill_holes(seg > 0)
    if sel_bg > 0:
        seg_bg = morphology.opening(seg_bg, morphology.disk(sel_bg))
    seg_fg = seg == 1
    if sel_fg > 0:
        seg_fg = morphology.opening(seg_fg, morphology.disk(sel_fg))
    return seg_bg, seg_fg


def split_segm_background_foreground(seg, sel_bg=STRUC_ELEM_BG, sel_fg=STRUC_ELEM_FG, on=None):
    """ smooth a class map into the mask of the background around the filled objects and the mask of class 1 (reference
    ``ellipse_fitting.py:400-443``): ``seg_bg = 1 - binary_fill_holes(seg > 0)`` and ``seg_fg = (seg == 1)``, each opened with
    ``disk(sel)`` when ``sel > 0``.

    Integer radii up to ``IMSEGM_MORPH_MAX_RADIUS`` run on the device (``imsegm_split_background_foreground``: one union-find
    labelling of the zero pixels, tiled disc erosion and dilation in integers); ``on='host'`` (or the environment variable
    ``IMSEGM_BOUNDARY_POINTS_ON=host``, no device, a larger radius) runs the scipy / numpy statement of the same definitions,
    :func:`split_host`.  A radius that is no integer (the reference's docstring uses ``sel_bg=1.5``) goes to scikit-image, which is
    imported in that branch only.

    :param ndarray seg: class map H x W
    :param int|float sel_bg: radius of the disc the background is opened with
    :param int|float sel_fg: radius of the disc class 1 is opened with
    :return tuple(ndarray,ndarray): seg_bg (int), seg_fg (bool)
    """
    seg = np.asarray(seg)
    if seg.ndim != 2:
        raise ValueError('the class map has to be 2-D, not %r' % (seg.shape, ))
    if not _integer_radii(sel_bg, sel_fg):
        return _split_skimage(seg, sel_bg, sel_fg)
    if seg.size and _on_device(_points_place(on), sel_bg, sel_fg):
        seg_bg, seg_fg = _hip.split_background_foreground(_class_map_i32(seg), int(sel_bg), int(sel_fg))
    else:
        seg_bg, seg_fg = split_host(seg, int(sel_bg), int(sel_fg))
    return seg_bg.astype(int), seg_fg.astype(bool)


def _class_map_i32(seg):
    """the class map as the device reads it: what matters is ``seg > 0`` and ``seg == 1``, which a map that int32 does not hold
    (or a float map) keeps as 0 / 1 / 2"""
    info = np.iinfo(np.int32)
    if seg.dtype.kind in 'iub' and (seg.dtype.itemsize <= 2 or seg.dtype == np.int32 or (info.min <= seg.min() and seg.max() <= info.max)):
        return seg
    return np.where(seg == 1, 1, np.where(seg > 0, 2, 0)).astype(np.int32)


def reconstruct_ray_features_2d(position, ray_features, shift=0):
    """ the end points of the rays of ``position`` (reference ``descriptors.py:1965-2002``): ray a of A points at the angle
    ``pi / 2 - 2 pi a / A - deg2rad(shift)``; rays that are negative or infinite are left out.  numpy on the host, float64.  It
    lives here, where the reference's ``ellipse_fitting`` imports it to, and not in ``pyimsegm_amd.descriptors``: that name of
    ``imsegm.descriptors`` is the overlay's pinned example of a name only an installed reference answers (imsegm/__init__.py).

    >>> reconstruct_ray_features_2d((10., 10), np.array([1] * 4)).round(12).tolist()
    [[10.0, 11.0], [11.0, 10.0], [10.0, 9.0], [9.0, 10.0]]
    >>> reconstruct_ray_features_2d((10., 10), np.array([-1, 0, 1, np.inf])).round(12).tolist()
    [[10.0, 10.0], [10.0, 9.0]]

    :param tuple(float,float) position: (row, col)
    :param ndarray ray_features: one distance per angle, more than 2
    :param float shift: rotation in degrees
    :return ndarray: points N x 2
    """
    if len(position) != 2:
        raise ValueError('positions has to have 2 coordinates')
    if len(ray_features) <= 2:
        raise ValueError('required at least 2 features')
    ray_features = np.asarray(ray_features)
    angles = np.linspace(0, 2 * np.pi, len(ray_features), endpoint=False)
    angles = (np.pi / 2.) - angles - np.deg2rad(shift)
    mask = np.logical_and(ray_features >= 0, ~np.isinf(ray_features))
    angles, ray_features = angles[mask], ray_features[mask]
    dx = np.cos(angles) * ray_features
    dy = np.sin(angles) * ray_features
    return np.tile(position, (len(ray_features), 1)) + np.array([dx, dy]).T


def _centre_rays(seg, centers, sel_bg, sel_fg, with_fg, on, angle_step=5.):
    """float32 rays [P, A] of all centres on seg_bg (edge 'up') and, ``with_fg``, on seg_fg (edge 'down')"""
    from pyimsegm_amd.descriptors import _ray_directions
    seg = np.asarray(seg)
    if seg.ndim != 2:
        raise ValueError('the class map has to be 2-D, not %r' % (seg.shape, ))
    for center in centers:
        if len(center) != 2:
            raise ValueError('Segmentation dim of %r and position (%i) does not match' % (seg.ndim, len(center)))
    positions = np.array([[int(v) for v in center] for center in centers], dtype=np.int64).reshape(-1, 2)
    directions = _ray_directions(angle_step)
    place = _points_place(on)
    if not _integer_radii(sel_bg, sel_fg):
        seg_bg, seg_fg = _split_skimage(seg, sel_bg, sel_fg)
        if place == 'device':
            return (_hip.ray_features_binary2d(seg_bg != 0, positions, directions, 1),
                    _hip.ray_features_binary2d(seg_fg != 0, positions, directions, -1) if with_fg else None)
        return ray_walk_host(seg_bg, positions, directions, 1), (ray_walk_host(seg_fg, positions, directions, -1) if with_fg else None)
    info = np.iinfo(np.int32)
    if seg.size and len(positions) and _on_device(place, sel_bg, sel_fg):
        return _hip.boundary_rays(_class_map_i32(seg), int(sel_bg), int(sel_fg), np.clip(positions, info.min, info.max), directions,
                                  with_fg)
    return boundary_rays_host(seg, int(sel_bg), int(sel_fg), positions, directions, with_fg)


def prepare_boundary_points_ray_join(seg, centers, close_points=5, min_diam=MIN_ELLIPSE_DAIM, sel_bg=STRUC_ELEM_BG,
                                     sel_fg=STRUC_ELEM_FG, on=None):
    """ per centre the ends of its rays to the smoothed background and of its rays to the end of class 1, one list after the other
    (reference ``ellipse_fitting.py:352-397``): rays below ``min_diam`` (those that met no edge too) are set to it, each list is
    thinned with ``reduce_close_points``.  Masks and rays of all centres: :func:`split_segm_background_foreground` and one launch on
    the device (``imsegm_boundary_rays``), or the host statement with ``on='host'``; radii that are no integers import scikit-image.

    :param ndarray seg: class map H x W
    :param list(tuple(int,int)) centers: (row, col)
    :param float close_points: smallest distance between two points kept
    :param float min_diam: smallest ray
    :param int sel_bg: radius of the disc the background is opened with
    :param int sel_fg: radius of the disc class 1 is opened with
    :return list(ndarray): points per centre
    """
    from pyimsegm_amd.descriptors import reduce_close_points
    rays_bg, rays_fg = _centre_rays(seg, centers, sel_bg, sel_fg, True, on)
    points_centers = []
    for center, ray_bg, ray_fc in zip(centers, rays_bg, rays_fg):
        both = []
        for ray in (ray_bg, ray_fc):
            ray = np.array(ray)
            ray[ray < min_diam] = min_diam
            both.append(reduce_close_points(reconstruct_ray_features_2d(center, ray), close_points))
        points_centers.append(np.vstack(both))
    return points_centers


def _closest_rays(ray_bg, ray_fc, min_diam):
    """both rays in float64 with those that met no edge at infinity and the others clamped from below (:485-487)"""
    rays = np.array([ray_bg, ray_fc], dtype=float)
    rays[rays < 0] = np.inf
    rays[rays < min_diam] = min_diam
    return rays


def prepare_boundary_points_ray_edge(seg, centers, close_points=5, min_diam=MIN_ELLIPSE_DAIM, sel_bg=STRUC_ELEM_BG,
                                     sel_fg=STRUC_ELEM_FG, on=None):
    """ per centre the ends of the shorter of its two rays per angle -- to the smoothed background, to the end of class 1 --
    (reference ``ellipse_fitting.py:446-494``); arguments, places and the scikit-image branch as
    :func:`prepare_boundary_points_ray_join`

    :return list(ndarray): points per centre
    """
    from pyimsegm_amd.descriptors import reduce_close_points
    rays_bg, rays_fg = _centre_rays(seg, centers, sel_bg, sel_fg, True, on)
    points_centers = []
    for center, ray_bg, ray_fc in zip(centers, rays_bg, rays_fg):
        ray_close = np.min(_closest_rays(ray_bg, ray_fc, min_diam), axis=0)
        points_centers.append(reduce_close_points(reconstruct_ray_features_2d(center, ray_close), close_points))
    return points_centers


def prepare_boundary_points_ray_mean(seg, centers, close_points=5, min_diam=MIN_ELLIPSE_DAIM, sel_bg=STRUC_ELEM_BG,
                                     sel_fg=STRUC_ELEM_FG, on=None):
    """ per centre the ends of the mean of its two rays per angle, of the one that met an edge where only one did (reference
    ``ellipse_fitting.py:497-549``); arguments, places and the scikit-image branch as :func:`prepare_boundary_points_ray_join`

    :return list(ndarray): points per centre
    """
    from pyimsegm_amd.descriptors import reduce_close_points
    rays_bg, rays_fg = _centre_rays(seg, centers, sel_bg, sel_fg, True, on)
    points_centers = []
    for center, ray_bg, ray_fc in zip(centers, rays_bg, rays_fg):
        rays = _closest_rays(ray_bg, ray_fc, min_diam)
        ray_min, ray_mean = np.min(rays, axis=0), np.mean(rays, axis=0)
        ray_mean[np.isinf(ray_mean)] = ray_min[np.isinf(ray_mean)]
        points_centers.append(reduce_close_points(reconstruct_ray_features_2d(center, ray_mean), close_points))
    return points_centers


def prepare_boundary_points_ray_dist(seg, centers, close_points=1, sel_bg=STRUC_ELEM_BG, sel_fg=STRUC_ELEM_FG, on=None):
    """ the ends of the rays of all centres to the smoothed background, each given to the centre nearest to it (reference
    ``ellipse_fitting.py:552-597``, with its quirks: coordinates in (-1e-3, 0) become 0, and the list ends at the last centre that
    got a point).  The foreground mask is never opened (``imsegm_boundary_rays`` with a NULL foreground output); places and the
    scikit-image branch as :func:`prepare_boundary_points_ray_join`.  These lists are what :func:`ransac_segm_batch` takes.

    :param ndarray seg: class map H x W
    :param list(tuple(int,int)) centers: (row, col)
    :param float close_points: smallest distance between two points kept
    :param int sel_bg: radius of the disc the background is opened with
    :param int sel_fg: unused, as in the reference
    :return list(ndarray): points per centre
    """
    from scipy.spatial.distance import cdist

    from pyimsegm_amd.descriptors import reduce_close_points
    rays_bg, _ = _centre_rays(seg, centers, sel_bg, 0, False, on)
    points = []
    for center, ray in zip(centers, rays_bg):
        points += reduce_close_points(reconstruct_ray_features_2d(center, np.array(ray), 0), close_points).tolist()
    points = np.array(points)
    points[(points < 0) & (points > -1e-3)] = 0.
    close_center = np.argmin(cdist(points, centers, metric='euclidean'), axis=1)
    return [points[close_center == i] for i in range(close_center.max() + 1)]


# ------------------------------------------------------------------------------------------------
# fitted ellipses into a label map with the overlap test (reference ellipse_fitting.py:282-349), and what stands around it
# ------------------------------------------------------------------------------------------------

#: a single ``add_overlap_ellipse`` goes to the device by default only from this ``max(segm)`` on: below it the host statement's
#: ``max(segm)`` passes over the map cost less than carrying the map to the device and back (tools/time_ellipse_place.py)
SINGLE_CALL_DEVICE_FROM_LABELS = 2


def _place_place(on):
    """'host', 'device' or None (the default: the device when one is present, the host for a single ellipse on a map with few
    labels): ``_hip.resolve_place`` on IMSEGM_ELLIPSE_PLACE_ON ('device' without a device raises)"""
    place, explicit = _hip.resolve_place(on, 'IMSEGM_ELLIPSE_PLACE_ON', True)
    return place if explicit or place == 'host' else None


def _ellipse_box(r, c, r_radius, c_radius, orientation, shape):
    """sine and cosine of the angle modulo pi and the bounding box of the rotated ellipse, clipped to ``shape`` when given:
    (sin, cos, upper_left int [2], lower_right int [2]), the operations of scikit-image 0.18.3's ``draw.ellipse`` in its order"""
    center = np.array([r, c])
    orientation = orientation % np.pi
    sin_alpha, cos_alpha = np.sin(orientation), np.cos(orientation)
    r_radius_rot = abs(r_radius * cos_alpha) + c_radius * abs(sin_alpha)
    c_radius_rot = r_radius * abs(sin_alpha) + abs(c_radius * cos_alpha)
    radii_rot = np.array([r_radius_rot, c_radius_rot])
    upper_left = np.ceil(center - radii_rot).astype(int)
    lower_right = np.floor(center + radii_rot).astype(int)
    if shape is not None:
        upper_left = np.maximum(upper_left, np.array([0, 0]))
        lower_right = np.minimum(lower_right, np.array(shape[:2]) - 1)
    return sin_alpha, cos_alpha, upper_left, lower_right


def ellipse_pixels_host(r, c, r_radius, c_radius, orientation=0., shape=None):
    """ the pixels of an ellipse: scikit-image 0.18.3's ``draw.ellipse(r, c, r_radius, c_radius, shape, rotation=orientation)``, which
    the reference's ``utilities.drawing.ellipse`` hands its arguments to, restated in numpy.  The angle is taken modulo pi; the
    bounding box runs from ``ceil(centre - radii_rot)`` to ``floor(centre + radii_rot)`` with the rotated radii
    ``|r_radius cos| + c_radius |sin|`` and ``r_radius |sin| + |c_radius cos|`` and is clipped to ``shape``; a pixel with the offsets
    (a, b) from the centre is inside when ``((a cos + b sin) / r_radius)**2 + ((a sin - b cos) / c_radius)**2 < 1`` in float64,
    every operation rounded on its own.  Row-major order.

    >>> rr, cc = ellipse_pixels_host(7, 10, 5, 8, np.deg2rad(30), (15, 20))
    >>> len(rr), int(rr.min()), int(rr.max()), int(cc.min()), int(cc.max())
    (127, 2, 12, 3, 17)

    :param int r: centre row
    :param int c: centre column
    :param int r_radius: radius along the rows
    :param int c_radius: radius along the columns
    :param float orientation: angle in radians
    :param tuple(int,int) shape: size of the image the pixels are clipped to
    :return tuple(ndarray,ndarray): rows, columns
    """
    sin_alpha, cos_alpha, upper_left, lower_right = _ellipse_box(r, c, r_radius, c_radius, orientation, shape)
    r_org, c_org = np.array([r, c]) - upper_left
    bounding_shape = lower_right - upper_left + 1
    r_lim, c_lim = np.ogrid[0:float(bounding_shape[0]), 0:float(bounding_shape[1])]
    rows, cols = (r_lim - r_org), (c_lim - c_org)
    with np.errstate(all='ignore'):
        distances = ((rows * cos_alpha + cols * sin_alpha) / r_radius) ** 2 + ((rows * sin_alpha - cols * cos_alpha) / c_radius) ** 2
    rr, cc = np.nonzero(distances < 1)
    return rr + upper_left[0], cc + upper_left[1]


def _int_params(ellipse_params):
    """the reference's reading of (c1, c2, h, w, phi): the first four truncated with ``int()``"""
    c1, c2, h, w, phi = ellipse_params
    return int(c1), int(c2), int(h), int(w), phi


def place_host(segm, list_params, labels, thr_overlap):
    """the numpy statement of ``imsegm_ellipse_place``: the reference's ``add_overlap_ellipse`` ellipse by ellipse, ``segm`` changed
    in place; placed bool [E] -- painted, with at least one pixel"""
    placed = np.zeros(len(list_params), dtype=bool)
    for e, (params, label) in enumerate(zip(list_params, labels)):
        if not params:
            continue
        c1, c2, h, w, phi = _int_params(params)
        rr, cc = ellipse_pixels_host(c1, c2, h, w, orientation=phi, shape=segm.shape)
        under, area, accepted = segm[rr, cc], len(rr), True
        for lb in range(1, int(np.max(segm) + 1)):
            overlap = np.sum(under == lb)
            sizes = [s for s in [np.sum(segm == lb), area] if s > 0]
            if not sizes or float(overlap) / float(min(sizes)) > thr_overlap:
                accepted = False
                break
        if accepted:
            segm[rr, cc] = label
            placed[e] = area > 0
    return placed


def overlaps_host(segm, list_params, nb_labels):
    """the numpy statement of ``imsegm_ellipse_overlaps``: (counts int64 [E, nb_labels], areas int64 [E])"""
    nb_labels = max(int(nb_labels), 0)
    counts, areas = np.zeros((len(list_params), nb_labels), dtype=np.int64), np.zeros(len(list_params), dtype=np.int64)
    for e, params in enumerate(list_params):
        if not params:
            continue
        c1, c2, h, w, phi = _int_params(params)
        rr, cc = ellipse_pixels_host(c1, c2, h, w, orientation=phi, shape=segm.shape)
        under = segm[rr, cc]
        areas[e] = len(rr)
        under = under[(under >= 0) & (under < nb_labels)]
        whole = under.astype(np.int64)
        counts[e] = np.bincount(whole[whole == under], minlength=nb_labels)[:nb_labels]
    return counts, areas


def ellipse_geometry(list_params, shape):
    """what the device takes of ellipses that were read with :func:`_int_params`: (geom int32 [E, 8] -- centre, radii, clipped
    bounding box --, sincos float64 [E, 2]), or None when one of them is not the device's: a radius below 1, a centre or radius beyond
    2^30, an angle that is not finite"""
    geom, sincos = np.zeros((len(list_params), 8), dtype=np.int32), np.zeros((len(list_params), 2), dtype=np.float64)
    for e, (c1, c2, h, w, phi) in enumerate(list_params):
        try:
            phi = float(phi)
        except (TypeError, ValueError):
            return None
        if not (np.isfinite(phi) and 1 <= h <= _hip.ELLIPSE_PLACE_MAX_COORD and 1 <= w <= _hip.ELLIPSE_PLACE_MAX_COORD
                and abs(c1) <= _hip.ELLIPSE_PLACE_MAX_COORD and abs(c2) <= _hip.ELLIPSE_PLACE_MAX_COORD):
            return None
        sin_alpha, cos_alpha, upper_left, lower_right = _ellipse_box(c1, c2, h, w, phi, shape)
        if np.any(lower_right < upper_left):
            upper_left, lower_right = np.array([0, 0]), np.array([-1, -1])
        geom[e] = (c1, c2, h, w, upper_left[0], upper_left[1], lower_right[0], lower_right[1])
        sincos[e] = (sin_alpha, cos_alpha)
    return geom, sincos


def _device_map(segm, upper):
    """``segm`` as the C-contiguous int32 map the device reads (``segm`` itself when it is one), or None when the device does not take
    it: not a non-empty 2-D array below 2^31 pixels, values that are no integers, below int32 or above ``upper``"""
    if not isinstance(segm, np.ndarray) or segm.ndim != 2 or segm.size == 0 or segm.size >= 2 ** 31 or segm.dtype.kind not in 'biuf':
        return None
    low, high = segm.min(), segm.max()
    if not (low >= np.iinfo(np.int32).min and high <= upper):                  # (NaN fails both)
        return None
    if segm.dtype.kind == 'f' and not np.array_equal(segm, np.trunc(segm)):
        return None
    if segm.dtype == np.int32 and segm.flags.c_contiguous:
        return segm
    return np.ascontiguousarray(segm, dtype=np.int32)


def _device_labels(labels, dtype):
    """the labels as int32, or None when one is no integer below the label table, or is not itself once stored in a map of
    ``dtype`` (the fold then reads back another value than it painted)"""
    try:
        values = np.asarray(labels, dtype=np.float64).ravel()
    except (TypeError, ValueError):
        return None
    if len(values) and not (np.all(values == np.trunc(values)) and values.min() >= np.iinfo(np.int32).min
                            and values.max() < _hip.ELLIPSE_PLACE_LABELS):
        return None
    whole = values.astype(np.int64)
    with np.errstate(all='ignore'):
        if not np.array_equal(whole.astype(dtype).astype(np.float64), values):
            return None
    return whole.astype(np.int32)


def add_overlap_ellipses(segm, list_params, labels=None, thr_overlap=1., on=None):
    """ the fold of :func:`add_overlap_ellipse` over a list of ellipses -- what the loops of ``segment_fit_ellipse``,
    ``segment_fit_ellipse_ransac`` and ``segment_fit_ellipse_ransac_segm`` do with their fits: ellipse e is painted into ``segm`` with
    ``labels[e]`` unless it overlaps a label of the map as it stands by more than ``thr_overlap``.  One upload of the map, one
    histogram launch, one launch that walks the ellipses, one download (``imsegm_ellipse_place``, csrc/ellipse_place.hip);
    ``on='host'`` (or the environment variable ``IMSEGM_ELLIPSE_PLACE_ON=host``, or no device) runs the numpy statement
    :func:`place_host`, and so does every call the device does not take: a radius below 1 after truncation, ``thr_overlap`` negative
    or NaN, a map that is not 2-D, not integer-valued or beyond int32, a value or label beyond ``IMSEGM_ELLIPSE_PLACE_LABELS``.

    :param ndarray segm: label map, changed in place
    :param list(tuple) list_params: (row, column, row radius, column radius, angle) per ellipse; a falsy entry is skipped
    :param list(int) labels: label per ellipse, default 1 .. E
    :param float thr_overlap: largest accepted overlap relative to the smaller of the two objects
    :return tuple(ndarray,ndarray): ``segm`` itself and placed bool [E]: the ellipse was painted (with at least one pixel)
    """
    list_params = list(list_params)
    labels = list(range(1, len(list_params) + 1)) if labels is None else list(labels)
    if len(labels) != len(list_params):
        raise ValueError('%i labels for %i ellipses' % (len(labels), len(list_params)))
    place = _place_place(on)
    kept = [e for e, params in enumerate(list_params) if params]
    ints = [_int_params(list_params[e]) for e in kept]
    placed = np.zeros(len(list_params), dtype=bool)
    if not kept:
        return segm, placed
    work = geometry = device_labels = None
    if place != 'host':
        try:
            threshold_ok = float(thr_overlap) >= 0
        except (TypeError, ValueError):
            threshold_ok = False
        if threshold_ok:
            work = _device_map(segm, _hip.ELLIPSE_PLACE_LABELS - 1)
        if work is not None:
            geometry = ellipse_geometry(ints, segm.shape)
            device_labels = _device_labels([labels[e] for e in kept], segm.dtype)
        if place is None and work is not None and len(kept) == 1 and segm.max() < SINGLE_CALL_DEVICE_FROM_LABELS:
            work = None
    if work is None or geometry is None or device_labels is None:
        placed[kept] = place_host(segm, [list_params[e] for e in kept], [labels[e] for e in kept], thr_overlap)
        return segm, placed
    placed[kept] = _hip.ellipse_place(work, geometry[0], geometry[1], device_labels, float(thr_overlap)).astype(bool)
    if work is not segm:
        segm[...] = work
    return segm, placed


def add_overlap_ellipse(segm, ellipse_params, label, thr_overlap=1., on=None):
    """ add to existing image ellipse with specific label
    if the new ellipse does not ouvelap with already existing object / ellipse (reference ``ellipse_fitting.py:282-349``): for every
    label ``1 .. max(segm)`` the overlap with the ellipse relative to the smaller of the two must not exceed ``thr_overlap``.  The
    ellipse is that of :func:`ellipse_pixels_host` after ``int()`` of centre and radii; ``segm`` is changed in place and returned.
    Places and the calls the device does not take as :func:`add_overlap_ellipses`, of which this is the list of one; by default a
    single ellipse goes to the device only when ``max(segm) >= SINGLE_CALL_DEVICE_FROM_LABELS``.

    >>> seg = np.zeros((15, 20), dtype=int)
    >>> ell = add_overlap_ellipse(seg, (7, 10, 5, 8, np.deg2rad(30)), 1, on='host')
    >>> ell is seg, int(ell.sum())
    (True, 127)
    >>> int((add_overlap_ellipse(ell, (4, 5, 2, 3, np.deg2rad(-30)), 2, on='host') == 2).sum())
    19

    :param ndarray segm: segmentation
    :param tuple ellipse_params: parameters
    :param int label: selected label
    :param float thr_overlap: relative overlap with existing objects
    :return ndarray:
    """
    if not ellipse_params:
        return segm
    return add_overlap_ellipses(segm, [ellipse_params], [label], thr_overlap, on)[0]


def ellipse_label_overlaps(segm, list_params, nb_labels=None, on=None):
    """ for every ellipse on its own the number of its pixels inside ``segm`` and the histogram of the labels
    ``0 .. nb_labels - 1`` under it: with ``np.bincount(segm.ravel())`` the Jaccard index of every candidate ellipse against every
    annotated egg, which ``select_optimal_ellipse`` of ``run_ellipse_annot_match.py`` gets from one rasterised mask per pair.  One
    launch over ellipses and bands of their boxes (``imsegm_ellipse_overlaps``); ``on='host'`` and every call the device does not
    take (see :func:`add_overlap_ellipses`; ``nb_labels`` beyond ``IMSEGM_ELLIPSE_PLACE_LABELS`` too) run :func:`overlaps_host`.

    :param ndarray segm: label map
    :param list(tuple) list_params: (row, column, row radius, column radius, angle) per ellipse; a falsy entry counts nothing
    :param int nb_labels: default ``max(segm) + 1``
    :return tuple(ndarray,ndarray): counts int64 [E, nb_labels], areas int64 [E]
    """
    segm = np.asarray(segm)
    list_params = list(list_params)
    nb_labels = int(np.max(segm) + 1) if nb_labels is None else int(nb_labels)
    place = _place_place(on)
    kept = [e for e, params in enumerate(list_params) if params]
    ints = [_int_params(list_params[e]) for e in kept]
    work = geometry = None
    if place != 'host' and kept and 1 <= nb_labels <= _hip.ELLIPSE_PLACE_LABELS:
        work = _device_map(segm, np.iinfo(np.int32).max)
        if work is not None:
            geometry = ellipse_geometry(ints, segm.shape)
    if work is None or geometry is None:
        return overlaps_host(segm, list_params, nb_labels)
    counts, areas = np.zeros((len(list_params), nb_labels), dtype=np.int64), np.zeros(len(list_params), dtype=np.int64)
    counts[kept], areas[kept] = _hip.ellipse_overlaps(work, geometry[0], geometry[1], nb_labels)
    return counts, areas


def filter_boundary_points(segm, slic):
    """ the centres of the superpixels on the border between background and objects (reference ``ellipse_fitting.py:600-622``):
    background superpixels (class 0 at their centre) with a neighbour of another class, and superpixels of class 1 with a background
    neighbour.  Centres and the edge list come from the device (``superpixel_centers``, ``make_graph_segm_connect_grid2d_conn4``);
    the share of every class among a superpixel's neighbours is two scatter-adds over the edge list.

    :param ndarray segm: class map H x W
    :param ndarray slic: superpixels H x W
    :return ndarray: points N x 2 (int)
    """
    from pyimsegm_amd.superpixels import make_graph_segm_connect_grid2d_conn4, superpixel_centers
    slic_centers = np.array(superpixel_centers(slic)).astype(int)
    labels = segm[slic_centers[:, 0], slic_centers[:, 1]]
    vertices, edges = make_graph_segm_connect_grid2d_conn4(slic)
    edges = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    neighbour_labels = np.zeros((int(np.max(vertices)) + 1, int(labels.max()) + 1))
    np.add.at(neighbour_labels, (edges[:, 0], labels[edges[:, 1]]), 1)
    np.add.at(neighbour_labels, (edges[:, 1], labels[edges[:, 0]]), 1)
    with np.errstate(invalid='ignore', divide='ignore'):
        neighbour_labels = neighbour_labels / neighbour_labels.sum(axis=1)[:, None]
        filter_bg = np.logical_and(labels == 0, neighbour_labels[:, 0] < 1)
        filter_fc = np.logical_and(labels == 1, neighbour_labels[:, 0] > 0)
    return slic_centers[np.logical_or(filter_bg, filter_fc)]


def prepare_boundary_points_close(seg, centers, sp_size=25, relative_compact=0.3):
    """ extract some point around foreground boundaries (reference ``ellipse_fitting.py:625-653``): SLIC superpixels of the class map
    scaled to [0, 1] on the device, :func:`filter_boundary_points`, every point given to the centre nearest to it; the list ends at
    the last centre that got a point

    :param ndarray seg: input segmentation
    :param list(tuple(int,int)) centers: list of centers
    :param int sp_size: superpixel size
    :param float relative_compact: SLIC regularisation
    :return list(ndarray):
    """
    from pyimsegm_amd.superpixels import segment_slic_img2d
    slic = segment_slic_img2d(seg / float(seg.max()), sp_size=sp_size, relative_compact=relative_compact)
    points_all = filter_boundary_points(seg, slic)
    centers = np.asarray(centers, dtype=np.float64).reshape(-1, 2)
    diff = points_all[:, None, :].astype(np.float64) - centers[None, :, :]
    close_center = np.argmin(np.sqrt((diff * diff).sum(axis=2)), axis=1)
    return [points_all[close_center == i] for i in range(int(close_center.max() + 1))]
