"""The doctest vectors of the reference module pyimsegm_amd/region_growing.py mirrors (imsegm/region_growing.py:601-620, :710-721,
:782-799, :1074-1077, :1098-1101, :1144-1147 is left to the GPU suite, :1217-1291), run against the module by
tests/test_region_growing_reference_host.py.  The growth examples run the numpy statement (``on='host'``) so that they need no
GPU; ``cases`` is tests/region_growing_cases.py, whose ``prob_fg`` stands in for ``compute_segm_prob_fg`` (the device histogram)."""

EXAMPLES = {
    'compute_shape_prior_table_cdf': r"""
>>> chist = [[1.0, 1.0, 0.8, 0.7, 0.6, 0.5, 0.3, 0.0, 0.0],
...          [1.0, 1.0, 0.9, 0.8, 0.7, 0.3, 0.2, 0.2, 0.0],
...          [1.0, 1.0, 1.0, 0.7, 0.6, 0.5, 0.3, 0.1, 0.1],
...          [1.0, 1.0, 0.6, 0.5, 0.4, 0.3, 0.2, 0.0, 0.0]]
>>> centre = (1, 1)
>>> compute_cdf = lambda *args, **kwargs: float(compute_shape_prior_table_cdf(*args, **kwargs))
>>> compute_cdf([1, 1], chist, centre)
1.0
>>> compute_cdf([10, 10], chist, centre)
0.0
>>> compute_cdf([10, -10], chist, centre)   # (the table's own 0.1: the far branch)
0.1
>>> compute_cdf([2, 3], chist, centre) # doctest: +ELLIPSIS
0.805...
>>> compute_cdf([-3, -2], chist, centre) # doctest: +ELLIPSIS
0.381...
>>> compute_cdf([3, -2], chist, centre) # doctest: +ELLIPSIS
0.676...
>>> compute_cdf([2, 3], chist, centre, angle_shift=270) # doctest: +ELLIPSIS
0.891...
""",
    'compute_centre_moment_points': r"""
>>> show = lambda result: (result[0].tolist(), result[1])
>>> points = list(zip([0] * 10, np.arange(10))) + [(0, 0)] * 5
>>> show(compute_centre_moment_points(points))
([0.0, 3.0], 0.0)
>>> points = list(zip(np.arange(10), [0] * 10)) + [(10, 0)]
>>> show(compute_centre_moment_points(points))
([5.0, 0.0], 90.0)
>>> points = list(zip(-np.arange(10), -np.arange(10))) + [(0, 0)] * 5
>>> show(compute_centre_moment_points(points))
([-3.0, -3.0], 45.0)
>>> points = list(zip(-np.arange(10), np.arange(10))) + [(-10, 10)]
>>> show(compute_centre_moment_points(points))
([-5.0, 5.0], 135.0)
""",
    'compute_update_shape_costs_points_table_cdf': r"""
>>> cdf = np.zeros((8, 20))
>>> cdf[:10] = 0.5
>>> cdf[:4] = 1.0
>>> points = np.array([[13, 16], [1, 5], [10, 15], [15, 25], [10, 5]])
>>> labels = np.ones(len(points))
>>> s_costs = np.zeros((len(points), 2))
>>> s_costs, centres, shifts, _ = compute_update_shape_costs_points_table_cdf(
...     s_costs, points, labels, [(0, 0)], [(np.inf, np.inf)], [0], [0], (None, cdf))
>>> centres.tolist()
[[10, 13]]
>>> shifts.tolist()
[209.0]
>>> np.round(s_costs, 3).tolist()
[[0.0, 0.673], [0.0, -0.01], [0.0, 0.184], [0.0, 0.543], [0.0, 0.374]]
>>> dict_thrs = dict(RG2SP_THRESHOLDS)
>>> dict_thrs['centre_init'] = 1
>>> _, centres, _, _ = compute_update_shape_costs_points_table_cdf(
...     s_costs, points, labels, [(7, 18)], [(np.inf, np.inf)], [0], [0], (None, cdf),
...     dict_thresholds=dict_thrs)
>>> np.round(centres, 1).tolist()
[[7.5, 17.1]]
""",
    'compute_pairwise_penalty': r"""
>>> edges = np.array([[0, 1], [1, 2], [0, 3], [2, 3], [2, 4]])
>>> labels = np.array([0, 0, 1, 2, 1])
>>> np.round(compute_pairwise_penalty(edges, labels, 0.05, 0.01), 8).tolist()
[0.0, 2.99573227, 2.99573227, 4.60517019, 0.0]
""",
    'get_neighboring_candidates': r"""
>>> neighbours = [[1], [0, 2, 3], [1, 3], [1, 2]]
>>> labels = np.array([0, 0, 1, 1])
>>> get_neighboring_candidates(neighbours, labels, 1)
[1]
""",
    'region_growing_shape_slic_greedy': r"""
>>> slic, segm = cases.grid_slic(), cases.doctest_block()
>>> centres = [(7.5, 10)]
>>> dict_debug = {}
>>> slic_prob_fg = cases.prob_fg(slic, segm, [0.1, 0.9])
>>> labels = region_growing_shape_slic_greedy(slic, slic_prob_fg, centres, (None, cases.DOCTEST_CHIST), coef_pairwise=0,
...                                           debug_history=dict_debug, on='host')
>>> np.round(dict_debug['criteria']).astype(int).tolist()[:9]
[397, 325, 307, 289, 272, 238, 204, 188, 173]
>>> np.round(dict_debug['criteria']).astype(int).tolist()[-2:]
[81, 81]
>>> np.array_equal(labels[slic], cases.doctest_expected_block())
True
>>> labels = region_growing_shape_slic_greedy(slic, slic_prob_fg, centres, (None, cases.DOCTEST_CHIST), coef_pairwise=1,
...                                           debug_history=dict_debug, on='host')
>>> np.round(dict_debug['criteria']).astype(int).tolist()[:11]
[406, 352, 334, 316, 300, 283, 270, 254, 238, 226, 210]
>>> np.round(dict_debug['criteria']).astype(int).tolist()[-2:]
[123, 123]
>>> np.array_equal(labels[slic], cases.doctest_expected_block())
True
>>> slic_prob_fg = cases.prob_fg(slic, np.ones((15, 20), dtype=int), [0.1, 0.9])
>>> labels = region_growing_shape_slic_greedy(slic, slic_prob_fg, [(6.5, 9)], (None, cases.disc_chist()), coef_shape=10,
...                                           coef_pairwise=1, debug_history=dict_debug, on='host')
>>> np.round(dict_debug['criteria']).astype(int).tolist()
[7506, 7120, 6715, 6328, 5719, 5719]
>>> np.array_equal(labels[slic], cases.doctest_expected_disc())
True
""",
}
