"""The doctest vectors of the reference's `add_padding` and `cut_object` (imsegm/utilities/data_io.py:1039-1128), run against
pyimsegm_amd/utilities/data_io.py by tests/test_cut_objects_reference_host.py.  The image and the mask are integer arrays, as in the
reference: such a call is evaluated by the host statement wherever it runs."""

EXAMPLES = {
    'add_padding': r"""
>>> add_padding((50, 50), 5, 15, 25, 35, 55)
(10, 20, 40, 50)
""",
    'cut_object': r"""
>>> img = np.ones((10, 20), dtype=int)
>>> img[3:7, 4:16] = 2
>>> mask = np.zeros((10, 20), dtype=int)
>>> mask[4:6, 5:15] = 1
>>> cut_object(img, mask, 2)
array([[1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1],
       [1, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 1],
       [1, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 1],
       [1, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 1],
       [1, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 1],
       [1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1]])
>>> cut_object(img, mask, 2, use_mask=True, allow_rotate=False)
array([[1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1],
       [1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1],
       [1, 1, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 1, 1],
       [1, 1, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 1, 1],
       [1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1],
       [1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1]])
""",
    'cut_objects': r"""
>>> img = np.ones((10, 20), dtype=np.uint8)
>>> img[3:7, 4:16] = 2
>>> segm = np.zeros((10, 20), dtype=int)
>>> segm[4:6, 5:15] = 7
>>> [crop.tolist() for crop in cut_objects(img, segm, padding=1, use_mask=True, allow_rotate=False, on='host')]
[[[1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1], [1, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 1], [1, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 1], [1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1]]]
""",
}
