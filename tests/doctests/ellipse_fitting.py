"""The doctest vectors of the reference module pyimsegm_amd/ellipse_fitting.py mirrors (/root/reference/imsegm/ellipse_fitting.py:51-73,
:91-105, :196-208), run against the module by tests/test_ellipse_reference_host.py.  What the reference's examples get from
scikit-image and its drawing helpers (``ellipse_perimeter``, ``add_overlap_ellipse``, ``prepare_boundary_points_ray_dist``, the SLIC
behind ``get_slic_points_labels``) is read from tests/golden/ellipse.npz, which the runner puts into the namespace as ``golden``;
the RANSAC example runs the numpy statement (``on='host'``) so that it needs no GPU."""

EXAMPLES = {
    'EllipseModelSegm': r"""
>>> xy = golden['doctest_perimeter']
>>> ellipse = EllipseModelSegm()
>>> ellipse.estimate(xy)
True
>>> np.round(ellipse.params, 2).tolist()
[19.5, 29.5, 12.45, 16.52, 0.53]
>>> params = 20, 30, 12, 16, np.deg2rad(30)
>>> xy = EllipseModelSegm().predict_xy(np.linspace(0, 2 * np.pi, 25), params)
>>> ellipse = EllipseModelSegm()
>>> ellipse.estimate(xy)
True
>>> np.round(ellipse.params, 2).tolist()
[20.0, 30.0, 12.0, 16.0, 0.52]
>>> np.round(abs(ellipse.residuals(xy)), 5).tolist() == [0.] * 25
True
>>> ellipse.params[2] += 2
>>> ellipse.params[3] += 2
>>> np.round(abs(ellipse.residuals(xy))).tolist() == [2.] * 25
True
""",
    'EllipseModelSegm.criterion': r"""
>>> seg = np.zeros((10, 15), dtype=int)
>>> r, c = np.meshgrid(range(seg.shape[1]), range(seg.shape[0]))
>>> el = EllipseModelSegm()
>>> el.params = [4, 7, 3, 6, np.deg2rad(10)]
>>> weights = np.ones(seg.ravel().shape)
>>> seg[4:5, 6:8] = 1
>>> table_prob = [[0.1, 0.9]]
>>> float(el.criterion(np.array([r.ravel(), c.ravel()]).T, weights, seg.ravel(), table_prob))  # doctest: +ELLIPSIS
87.888...
>>> seg[2:7, 4:11] = 1
>>> float(el.criterion(np.array([r.ravel(), c.ravel()]).T, weights, seg.ravel(), table_prob))  # doctest: +ELLIPSIS
17.577...
>>> seg[1:9, 1:14] = 1
>>> float(el.criterion(np.array([r.ravel(), c.ravel()]).T, weights, seg.ravel(), table_prob))   # doctest: +ELLIPSIS
-70.311...
""",
    'ransac_segm': r"""
>>> table_prob = [[0.01, 0.75, 0.95, 0.9], [0.99, 0.25, 0.05, 0.1]]
>>> ransac_model, _ = ransac_segm(golden['doctest_points'], EllipseModelSegm, golden['doctest_points_all'],
...     golden['doctest_weights'], golden['doctest_labels'], table_prob, 0.6, 3, max_trials=15, on='host')
>>> np.round(ransac_model.params[:4]).astype(int).tolist()
[60, 75, 41, 65]
>>> float(np.round(ransac_model.params[4], 1))
0.5
""",
}
