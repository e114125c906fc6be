"""The ``on=None | 'host' | 'device'`` switch of the egg pipeline, cell by cell, through the private function that reads each of the
seven environment variables -- the keyword crossed with the variable crossed with what ``_hip.device_count`` says -- and the two
names of the one host ray walk.  No GPU."""
import numpy as np
import pytest

from pyimsegm_amd import _hip
from pyimsegm_amd import annotation as ann
from pyimsegm_amd import ellipse_fitting as ell
from pyimsegm_amd import region_growing as rg
from pyimsegm_amd.descriptors import _ray_directions

VALUES = (None, 'host', 'device', 'elsewhere')                     # of the keyword; of the variable, None: unset
ANSWERS = {'H': 'host', 'D': 'device', 'N': None, 'V': ValueError, 'U': _hip.HipUnavailableError}


def _unavailable():
    raise _hip.HipUnavailableError('the library is not built')


DEVICES = (lambda: 0, lambda: 1, _unavailable)

# one row per (keyword, variable) in the order of VALUES x VALUES, one letter per entry of DEVICES
#: 'device' without a device is handed back: the call fails later, where it needs the device
HANDS_BACK = ('HDH', 'HHH', 'DDD', 'VVV') + ('HHH', ) * 4 + ('DDD', ) * 4 + ('VVV', ) * 4
#: 'device' without a device raises at once
RAISES = ('HDH', 'HHH', 'UDU', 'VVV') + ('HHH', ) * 4 + ('UDU', ) * 4 + ('VVV', ) * 4
#: the same, and the default with a device present stays open (None): the caller decides by the size of the call
STAYS_OPEN = ('HNH', ) + RAISES[1:]

SWITCHES = {
    'IMSEGM_ANNOTATION_ON': (lambda on: ann._place(on, 'convert_img_colors_to_labels'), RAISES),
    'IMSEGM_RANSAC_ON': (lambda on: ell._place(on), HANDS_BACK),
    'IMSEGM_BOUNDARY_POINTS_ON': (lambda on: ell._points_place(on), HANDS_BACK),
    'IMSEGM_ELLIPSE_PLACE_ON': (lambda on: ell._place_place(on), STAYS_OPEN),
    'IMSEGM_RG_ON': (lambda on: rg._place(on), HANDS_BACK),
    'IMSEGM_OBJECT_SHAPES_ON': (lambda on: rg._place(on, 'IMSEGM_OBJECT_SHAPES_ON'), HANDS_BACK),
    'IMSEGM_OBJECT_CUT_ON': (lambda on: rg._place(on, 'IMSEGM_OBJECT_CUT_ON'), HANDS_BACK),
}


@pytest.mark.parametrize('variable', sorted(SWITCHES))
def test_every_cell_of_the_switch(monkeypatch, variable):
    call, table = SWITCHES[variable]
    for other in SWITCHES:
        monkeypatch.delenv(other, raising=False)
    cells = 0
    for k, keyword in enumerate(VALUES):
        for e, value in enumerate(VALUES):
            if value is None:
                monkeypatch.delenv(variable, raising=False)
            else:
                monkeypatch.setenv(variable, value)
            for d, count in enumerate(DEVICES):
                monkeypatch.setattr(_hip, 'device_count', count)
                want = ANSWERS[table[4 * k + e][d]]
                where = '%s: on=%r, variable %r, devices %d' % (variable, keyword, value, d)
                if isinstance(want, type):
                    with pytest.raises(want):
                        call(keyword)
                        pytest.fail(where + ': no ' + want.__name__)
                else:
                    assert call(keyword) == want, where
                cells += 1
    assert cells == 48


def test_the_text_of_a_rejected_value(monkeypatch):
    monkeypatch.setattr(_hip, 'device_count', lambda: 1)
    for variable, (call, _) in SWITCHES.items():
        with pytest.raises(ValueError) as caught:
            call('elsewhere')
        assert str(caught.value) == "on is 'host' or 'device', not 'elsewhere'", variable


def test_host_by_default_decides_only_the_default(monkeypatch):
    monkeypatch.delenv('IMSEGM_ANNOTATION_ON', raising=False)
    monkeypatch.setattr(_hip, 'device_count', lambda: 1)
    monkeypatch.setattr(ann, 'HOST_BY_DEFAULT', frozenset(['image_inpaint_pixels']))
    assert ann._place(None, 'image_inpaint_pixels') == 'host' and ann._place(None, 'unique_image_colors') == 'device'
    assert ann._place('device', 'image_inpaint_pixels') == 'device'
    monkeypatch.setenv('IMSEGM_ANNOTATION_ON', 'device')
    assert ann._place(None, 'image_inpaint_pixels') == 'device'


def test_the_two_names_of_the_host_walk():
    """``region_growing.ray_distances_down`` is the one-position 'down' call of ``ray_walk_host``, byte for byte: on the square of
    test_region_growing_reference_host.py::test_ray_walk_of_a_square and from a position outside the image"""
    img = np.zeros((100, 100), dtype=bool)
    img[20:70, 30:80] = True
    directions = _ray_directions(45.)
    for position in ((45, 55), (-1, 5)):
        one = rg.ray_distances_down(img, position, directions)
        many = ell.ray_walk_host(img, [position], directions, -1)
        assert one.dtype == many.dtype == np.float32 and one.shape == many[0].shape == (8, )
        assert one.tobytes() == many[0].tobytes()
    assert (ell.ray_walk_host(img, [(45, 55)], directions, -1) > 0).all()
