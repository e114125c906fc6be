"""The one-workgroup exclusive prefix sum that the labelling, graph and compaction stages share (csrc/scan.hip, through
``imsegm_debug_exclusive_scan``) against ``numpy.cumsum``, exactly: lengths at the edge of a wave (64), at the edge of one turn of
the workgroup (1 024 lanes x 4 entries) and in a third turn with a ragged tail.  The entry runs the int32 instantiation; the uint32
one (the point compaction of csrc/boundary.hip) is the same template -- wrap-around addition, the same machine code -- and is held
to its results by tests/test_gpu_boundary.py."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LENGTHS = (0, 1, 63, 64, 65, 4095, 4096, 4097, 12289)


@pytest.fixture(scope='module')
def hip():
    from pyimsegm_amd import _hip
    _hip.default_context()
    return _hip


def check(hip, values):
    values = np.asarray(values, dtype=np.int32)
    out, total = hip.exclusive_scan(values)
    incl = np.cumsum(values, dtype=np.int64)
    assert out.dtype == np.int32 and out.shape == values.shape
    assert np.array_equal(out, np.concatenate([[0], incl[:-1]])[:values.size])
    assert total == (int(incl[-1]) if values.size else 0)


@pytest.mark.parametrize('n', LENGTHS)
def test_seeded_values(hip, n):
    check(hip, np.random.default_rng(n).integers(0, 1000, size=n))


@pytest.mark.parametrize('fill', (0, 1))
def test_constant_values(hip, fill):
    check(hip, np.full(4097, fill))
