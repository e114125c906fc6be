"""Examples of pyimsegm_amd/center_annotation.py, run by tests/test_center_annotation_reference_host.py.  The reference's
`run_create_annotation.py` has no doctests of its own; the expected arrays are what its functions write for these inputs under
scikit-image 0.18.3 / scipy 1.7.1 (the 9 x 9 square is the case 'tie' of tests/center_annotation_cases.py: its one pixel above 0.8 gives a disc of radius 0, so no level 3).  Every call asks for the host statement."""

EXAMPLES = {
    'correct_segm': r"""
>>> img = np.zeros((8, 12), dtype=np.uint8)
>>> img[1:7, 1:6] = 255
>>> img[2:5, 8:11] = 7
>>> img[6, 11] = 1
>>> seg, seg_lb = correct_segm(img, sel_radius=1, min_size=6, on='host')
>>> seg_lb
array([[0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0],
       [0, 0, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0],
       [0, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0],
       [0, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0],
       [0, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0],
       [0, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0],
       [0, 0, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0],
       [0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]], dtype=int32)
>>> bool((seg == (seg_lb > 0)).all())
True
""",
    'compute_eggs_center': r"""
>>> seg = np.zeros((6, 9), dtype=int)
>>> seg[1:3, 1:4] = 1
>>> seg[2:6, 5:9] = 3
>>> compute_eggs_center(seg, on='host').tolist()
[[2.0, 1.5], [6.5, 3.5]]
""",
    'segm_center_levels': r"""
>>> seg = np.zeros((11, 13), dtype=int)
>>> seg[1:10, 2:11] = 1
>>> segm_center_levels(seg, [0., 0.4, 0.8], on='host')
array([[0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0],
       [0, 0, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0],
       [0, 0, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0],
       [0, 0, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0],
       [0, 0, 1, 1, 1, 2, 2, 2, 1, 1, 1, 0, 0],
       [0, 0, 1, 1, 1, 2, 2, 2, 1, 1, 1, 0, 0],
       [0, 0, 1, 1, 1, 2, 2, 2, 1, 1, 1, 0, 0],
       [0, 0, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0],
       [0, 0, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0],
       [0, 0, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0],
       [0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]])
""",
    'create_annot_centers': r"""
>>> img = np.zeros((11, 13), dtype=np.uint8)
>>> img[1:10, 2:11] = 200
>>> level_map, centres = create_annot_centers(img, on='host', sel_radius=0, min_size=4)
>>> level_map.dtype, int(level_map.max()), centres.tolist()
(dtype('uint8'), 2, [[6.0, 5.0]])
""",
}
