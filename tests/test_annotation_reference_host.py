"""The host statements of pyimsegm_amd/annotation.py against the recorded results of the reference's imsegm/annotation.py
(tests/golden/annotation.npz, made by tests/golden/make_golden_annotation.py on the inputs of tests/annotation_cases.py): byte for
byte with dtypes and errors; the nearest-pixel functions at every pixel outside the ambiguous mask, inside it one of the tied labels.
No GPU."""
import json
import os
import re

import numpy as np
import pytest

import annotation_cases as cases

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.fixture(scope='module')
def golden():
    return dict(np.load(os.path.join(HERE, 'golden', 'annotation.npz')))


@pytest.fixture(scope='module')
def ann():
    from pyimsegm_amd import annotation
    return annotation


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)


def as_dict(keys, counts):
    return {tuple(int(v) for v in k): int(c) for k, c in zip(keys, counts)}


@pytest.mark.parametrize('name', sorted(cases.PAINTED))
def test_nearest_colour_functions(golden, ann, name):
    image, colors, _, _ = cases.painted(name)
    assert same(ann.image_color_2_labels(image, colors, on='host'), golden[name + '_color_2_labels'])
    assert same(ann.quantize_image_nearest_color(image, colors, on='host'), golden[name + '_nearest_color'])
    # without colours the frequent colours are numbered in key order here and in PIL's order there: the same colour per pixel,
    # except where two colours are equally near -- there each takes the first of its own order, at the same distance
    mine = ann.image_color_2_labels(image, on='host')
    my_colors = np.array(list(ann.image_frequent_colors(image, on='host').keys()), dtype=np.int64)
    assert list(map(tuple, my_colors)) == sorted(map(tuple, golden[name + '_default_colors']))
    assert mine.dtype == golden[name + '_color_2_labels_default'].dtype
    theirs = golden[name + '_default_colors'][golden[name + '_color_2_labels_default']]
    dist = np.abs(image.astype(np.int64)[:, :, None, :] - my_colors[None, None]).sum(axis=3)
    my_dist = np.take_along_axis(dist, mine[:, :, None], axis=2)[:, :, 0]
    assert np.array_equal(my_dist, dist.min(axis=2))
    assert np.array_equal(my_dist, np.abs(image.astype(np.int64) - theirs).sum(axis=2))
    unique_nearest = (dist == dist.min(axis=2, keepdims=True)).sum(axis=2) == 1
    assert unique_nearest.mean() > 0.9 and np.array_equal(my_colors[mine][unique_nearest], theirs[unique_nearest])
    assert np.array_equal(mine, np.argmin(dist, axis=2))


@pytest.mark.parametrize('name', sorted(cases.PAINTED))
def test_colour_counts(golden, ann, name):
    image = cases.painted(name)[0]
    assert ann.unique_image_colors(image, on='host') == [tuple(int(v) for v in c) for c in golden[name + '_unique_sorted']]
    found = ann.image_frequent_colors(image, on='host')
    assert found == as_dict(golden[name + '_frequent_keys'], golden[name + '_frequent_counts'])
    assert all(type(v) is int for k in found for v in k + (found[k], ))
    at = float(golden[name + '_frequent_at'])
    expected = as_dict(golden[name + '_frequent_at_keys'], golden[name + '_frequent_at_counts'])
    assert ann.image_frequent_colors(image, at, on='host') == expected
    assert round(at * image.shape[0] * image.shape[1]) in expected.values()        # (the threshold sits at a count that is kept)


@pytest.mark.parametrize('name', sorted(cases.PAINTED))
def test_colours_and_labels(golden, ann, name):
    image, colors, _, _ = cases.painted(name)
    clean, lut, segm = cases.clean(name)
    assert same(ann.convert_img_colors_to_labels(clean, lut, on='host'), golden[name + '_to_labels'])
    assert np.array_equal(golden[name + '_to_labels'], segm)
    reverted = {c: i + 5 for i, c in enumerate(colors)}
    assert same(ann.convert_img_colors_to_labels_reverted(clean, reverted, on='host'), golden[name + '_to_labels_reverted'])
    assert same(ann.convert_img_labels_to_colors(segm, lut, on='host'), golden[name + '_to_colors'])
    shifted, shifted_lut = cases.shifted_labels(name)
    assert same(ann.convert_img_labels_to_colors(shifted, shifted_lut, on='host'), golden[name + '_to_colors_shifted'])
    assert str(golden[name + '_reverted_error']) == str(golden[name + '_to_colors_error']) == 'ValueError'
    with pytest.raises(ValueError):
        ann.convert_img_colors_to_labels_reverted(image, {c: i for i, c in enumerate(colors)}, on='host')
    with pytest.raises(ValueError):
        ann.convert_img_labels_to_colors(segm, {k: v for k, v in lut.items() if k != 1}, on='host')


@pytest.mark.parametrize('name', sorted(cases.PAINTED))
def test_nearest_pixel(golden, ann, name):
    image, colors, segm, kept = cases.painted(name)
    ambiguous = cases.ambiguous_mask(segm, kept)
    share = float(ambiguous.mean())
    print(name, 'ambiguous share', share)
    assert share <= cases.AMBIGUOUS_CAP
    labels = np.where(kept, segm, np.nan)
    recorded = golden[name + '_inpaint']
    assert cases.tied_labels_ok(recorded, segm, kept).all()
    for result in (ann.image_inpaint_pixels(labels, kept, on='host'), ann.nearest_valid_host(labels, kept)):
        assert result.dtype == recorded.dtype and result.shape == recorded.shape
        assert np.array_equal(result[~ambiguous], recorded[~ambiguous])
        assert cases.tied_labels_ok(result, segm, kept).all()
    quantized = ann.quantize_image_nearest_pixel(image, colors, on='host')
    recorded = golden[name + '_nearest_pixel']
    assert quantized.dtype == recorded.dtype and quantized.shape == recorded.shape
    assert np.array_equal(quantized[~ambiguous], recorded[~ambiguous])
    table = np.array(colors)
    index = (quantized[:, :, None, :] == table[None, None]).all(axis=3).argmax(axis=2)
    assert np.array_equal(table[index], quantized) and cases.tied_labels_ok(index, segm, kept).all()


def test_nearest_valid_host_rule(ann):
    """the smallest row-major index among the pixels at the smallest distance, on maps small enough to see"""
    labels = np.array([[5, -1, 6], [-1, -1, -1], [7, -1, 8]])
    assert ann.nearest_valid_host(labels, labels >= 0).tolist() == [[5, 5, 6], [5, 5, 6], [7, 7, 8]]
    column = np.array([[1], [-1], [2]])
    assert ann.nearest_valid_host(column, column >= 0).tolist() == [[1], [1], [2]]
    with pytest.raises(ValueError):
        ann.nearest_valid_host(np.zeros((3, 3)), np.zeros((3, 3), dtype=bool))
    big = np.full((8, 700), -1)
    big[0, 0] = 4
    assert (ann.nearest_valid_host(big, big >= 0, rows_per_chunk=3) == 4).all()


def test_errors_and_an_image_without_the_colours(golden, ann):
    from pyimsegm_amd.utilities import ImageDimensionError
    assert str(golden['inpaint_shape_error']) == 'ImageDimensionError'
    with pytest.raises(ImageDimensionError):
        ann.image_inpaint_pixels(np.zeros((3, 4)), np.ones((4, 3), dtype=bool), on='host')
    # scipy answers NaN for an empty point set, the cast to int makes an index no colour table has (README_annotation.md)
    assert str(golden['all_invalid_error']) == 'IndexError'
    with pytest.raises(IndexError), np.errstate(invalid='ignore'):
        ann.quantize_image_nearest_pixel(np.full((4, 5, 3), 7, dtype=np.uint8), [(0, 0, 0), (1, 1, 1)], on='host')
    with pytest.raises(ValueError):
        ann.image_color_2_labels(np.zeros((2, 2, 3), dtype=np.uint8), [(0, 0, 0)], on='elsewhere')


def test_doctest_values(golden, ann):
    np.random.seed(0)
    img = np.random.randint(0, 2, (50, 50, 3))
    assert ann.unique_image_colors(img, on='host') == [tuple(int(v) for v in c) for c in golden['doctest_unique_sorted']]
    np.random.seed(0)
    seg = np.random.randint(0, 2, (5, 7))
    img = np.array([(0.2, 0.2, 0.2), (0.9, 0.9, 0.9)])[seg]
    assert same(ann.convert_img_colors_to_labels(img, {0: (0.2, 0.2, 0.2), 1: (0.9, 0.9, 0.9)}), golden['doctest_to_labels'])
    assert same(ann.convert_img_colors_to_labels_reverted(img, {(0.2, 0.2, 0.2): 0, (0.9, 0.9, 0.9): 1}), golden['doctest_to_labels_reverted'])
    assert same(ann.convert_img_labels_to_colors(seg, {0: (0.2, 0.2, 0.2), 1: (0.9, 0.9, 0.9)}), golden['doctest_to_colors'])
    np.random.seed(0)
    img = np.random.randint(0, 2, (50, 50, 3)).astype(np.uint8)
    assert ann.image_frequent_colors(img, on='host') == as_dict(golden['doctest_frequent_keys'], golden['doctest_frequent_counts'])
    np.random.seed(0)
    rand = np.random.randint(0, 2, (5, 7)).astype(np.uint8)
    gray = np.rollaxis(np.array([rand] * 3), 0, 3)
    mine = ann.image_color_2_labels(gray, on='host')
    my_colors = np.array(list(ann.image_frequent_colors(gray, on='host').keys()))
    assert np.array_equal(my_colors[mine], golden['doctest_color_2_labels_colors'][golden['doctest_color_2_labels']])
    np.random.seed(0)
    img = np.random.randint(0, 2, (5, 7, 3)).astype(np.uint8)
    assert same(ann.quantize_image_nearest_color(img, [(0, 0, 0), (1, 1, 1)], on='host'), golden['doctest_nearest_color'])
    # (5 x 7 with two colours: every second pixel has ties, so only the definition is checked: one of the nearest exact pixels)
    exact = (img == img[:, :, :1]).all(axis=2)
    result = ann.quantize_image_nearest_pixel(img, [(0, 0, 0), (1, 1, 1)], on='host')
    assert result.dtype == golden['doctest_nearest_pixel'].dtype
    for answer in (result, golden['doctest_nearest_pixel']):
        assert cases.tied_labels_ok(answer[:, :, 0], img[:, :, 0], exact).all()


def test_host_by_default_holds_for_every_pixel_function(ann, monkeypatch):
    """with a device present (here: pretended) a function named in HOST_BY_DEFAULT makes no device call unless ``on`` or the
    environment asks for one"""
    from pyimsegm_amd import _hip

    def device_call(*args, **kwargs):
        raise AssertionError('a device call')

    monkeypatch.delenv('IMSEGM_ANNOTATION_ON', raising=False)
    monkeypatch.setattr(_hip, 'device_count', lambda: 1)
    for entry in ('annot_match', 'annot_paint', 'annot_color_hist', 'annot_nearest_valid', 'annot_quantize_nearest_pixel'):
        monkeypatch.setattr(_hip, entry, device_call)
    image, colors, segm, kept = cases.painted(sorted(cases.PAINTED)[0])
    clean, lut, _ = cases.clean(sorted(cases.PAINTED)[0])
    calls = {
        'unique_image_colors': lambda on: ann.unique_image_colors(image, on=on),
        'image_frequent_colors': lambda on: ann.image_frequent_colors(image, on=on),
        'convert_img_colors_to_labels': lambda on: ann.convert_img_colors_to_labels(clean, lut, on=on),
        'convert_img_colors_to_labels_reverted': lambda on: ann.convert_img_colors_to_labels_reverted(clean, {c: i for i, c in lut.items()}, on=on),
        'convert_img_labels_to_colors': lambda on: ann.convert_img_labels_to_colors(segm, lut, on=on),
        'image_color_2_labels': lambda on: ann.image_color_2_labels(image, colors, on=on),
        'quantize_image_nearest_color': lambda on: ann.quantize_image_nearest_color(image, colors, on=on),
        'image_inpaint_pixels': lambda on: ann.image_inpaint_pixels(np.where(kept, segm, 0), kept, on=on),
        'quantize_image_nearest_pixel': lambda on: ann.quantize_image_nearest_pixel(image, colors, on=on),
    }
    with open(os.path.join(HERE, 'golden', 'annotation_names.json')) as fp:
        assert set(calls) == set(json.load(fp)['functions']) - {'group_images_frequent_colors', 'load_info_group_by_slices'}
    for name, call in calls.items():
        monkeypatch.setattr(ann, 'HOST_BY_DEFAULT', frozenset())
        with pytest.raises(AssertionError, match='a device call'):
            call(None)
        monkeypatch.setattr(ann, 'HOST_BY_DEFAULT', frozenset([name]))
        on_host = call('host')
        assert same(call(None), on_host) if isinstance(on_host, np.ndarray) else call(None) == on_host
        with pytest.raises(AssertionError, match='a device call'):
            call('device')


def test_public_names(ann):
    import inspect
    with open(os.path.join(HERE, 'golden', 'annotation_names.json')) as fp:
        names = json.load(fp)
    functions = sorted(n for n, f in inspect.getmembers(ann, inspect.isfunction) if f.__module__ == ann.__name__ and not n.startswith('_'))
    assert set(names['functions']) <= set(functions)
    assert set(functions) - set(names['functions']) == {'color_counts_host', 'colors_to_labels_host', 'labels_to_colors_host',
                                                        'nearest_color_index_host', 'nearest_valid_host', 'inpaint_host',
                                                        'exact_color_index_host'}
    assert sorted(n for n in vars(ann) if n.isupper() and not n.startswith('_') and n != 'HOST_BY_DEFAULT') == names['constants']
    reference = inspect.signature
    assert list(reference(ann.image_frequent_colors).parameters) == ['img', 'ratio_threshold', 'on']
    assert reference(ann.image_frequent_colors).parameters['ratio_threshold'].default == 1e-3
    assert list(reference(ann.load_info_group_by_slices).parameters) == ['path_txt', 'stages', 'pos_columns', 'dict_slice_tol']
    assert ann.DICT_COLOURS[3] == (255, 229, 0) and ann.ANNOT_SLICE_DIST_TOL[4] == 3 and ann.SLICE_NAME_GROUPING == 'stack_path'
    assert ann.COLUMNS_POSITION == ('ant_x', 'ant_y', 'post_x', 'post_y', 'lat_x', 'lat_y')


def test_load_info_group_by_slices(ann, tmp_path):
    path = tmp_path / 'info.txt'
    rows = ['\tstage\tstack_path\tslice_index\timage_path\tant_x\tant_y\tpost_x\tpost_y\tlat_x\tlat_y',
            '0\t4\tstack_a\t3\ta_3.png\t1\t2\t3\t4\t5\t6', '1\t4\tstack_a\t5\ta_5.png\t11\t12\t13\t14\t15\t16',
            '2\t4\tstack_a\t9\ta_9.png\t21\t22\t23\t24\t25\t26', '3\t2\tstack_b\t1\tb_1.png\t31\t32\t33\t34\t35\t36']
    path.write_text('\n'.join(rows) + '\n')
    df = ann.load_info_group_by_slices(str(path), [4])
    assert sorted(df.index) == ['a_3', 'a_5', 'a_9']
    assert df.loc['a_3', 'ant_x'].tolist() == [1, 11] and df.loc['a_9', 'lat_y'].tolist() == [26]
    assert ann.load_info_group_by_slices(str(path), [6]).empty


def test_library_exports_the_annotation_calls():
    from pyimsegm_amd import _hip, build
    build.build(verbose=False)
    header = open(os.path.join(ROOT, 'include', 'imsegm_hip.h')).read()
    declared = set(re.findall(r'IMSEGM_API\s+[\w\s\*]*?\b(imsegm_annot_\w+)\s*\(', header))
    assert declared == {'imsegm_annot_match', 'imsegm_annot_paint', 'imsegm_annot_color_hist', 'imsegm_annot_nearest_valid',
                        'imsegm_annot_quantize_nearest_pixel'}
    lib = _hip.load_library()
    for name in declared:
        assert hasattr(lib, name) and name in _hip.EXPORTED_SYMBOLS
    assert int(re.search(r'#define IMSEGM_ANNOT_MAX_COLORS (\d+)', header).group(1)) == _hip.ANNOT_MAX_COLORS == 256
    assert 'annotation.hip' in build.SOURCES and 'api_annotation.hip' in build.SOURCES
