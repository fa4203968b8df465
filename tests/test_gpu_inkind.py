"""
GPU: ``Index.gather`` and ``Index.emit`` (xugrid_amd/inkind.py) across sides -- data on the host or in HBM, the index made with
``host=`` or with ``dev=`` -- at the sizes where they can go wrong: one entry, no ids, one id, an id of -1.  Comparisons are
exact: a gather copies.  The torch variants run with each module's ``test_torch_in_torch_out``; torch is not initialised here.
"""
import numpy as np
import pytest

from xugrid_amd import engine
from xugrid_amd.inkind import Index

pytestmark = pytest.mark.gpu


def ids_of(n, length):
    """``length`` ids into ``n`` entries; the longest carries one -1."""
    ids = np.random.default_rng(10 * n + length).permutation(max(n, length))[:length] % n
    if length == 7:
        ids[3] = -1
    return ids.astype(np.int64)


def make_index(ids, side):
    return Index(host=ids.copy()) if side == "host" else Index(dev=engine.DeviceArray.from_host(ids))


@pytest.mark.parametrize("index_side", ["host", "dev"])
@pytest.mark.parametrize("data_side", ["host", "dev"])
@pytest.mark.parametrize("length", [0, 1, 7])
@pytest.mark.parametrize("n", [1, 7])
def test_gather_across_sides(hip, n, length, data_side, index_side):
    values = np.random.default_rng(n).normal(size=(2, n))
    ids = ids_of(n, length)
    want = np.where(ids == -1, np.nan, values[..., ids])
    data = values if data_side == "host" else engine.DeviceArray.from_host(values)
    index = make_index(ids, index_side)
    for _ in range(2):  # (the second time from the cached side)
        got = index.gather(data, n)
        assert isinstance(got, np.ndarray if data_side == "host" else engine.DeviceArray)
        got = got if data_side == "host" else got.download()
        assert got.shape == (2, length) and got.dtype == np.float64 and np.array_equal(got, want, equal_nan=True)
        if data_side == "host":
            assert index.host is not None and index.host.dtype == np.int64 and np.array_equal(index.host, ids)
        else:
            assert isinstance(index.dev, engine.DeviceArray) and np.array_equal(index.dev.download(), ids)
    if data_side != index_side:  # the index had to move: both sides are kept, neither is made again
        host, dev = index.host, index.dev
        index.gather(data, n)
        assert index.host is host and index.dev is dev
    else:  # the index was where it was needed: it did not move
        assert (index.dev is None) if index_side == "host" else (index.host is None)


def test_gather_fill_value(hip):
    values = np.arange(6.0).reshape(2, 3)
    ids = np.array([2, -1, 0], dtype=np.int64)
    for data in (values, engine.DeviceArray.from_host(values)):
        got = make_index(ids, "dev").gather(data, 3, fill_value=-9.0)
        got = got if isinstance(got, np.ndarray) else got.download()
        assert np.array_equal(got, [[2.0, -9.0, 0.0], [5.0, -9.0, 3.0]])


@pytest.mark.parametrize("length", [0, 1, 7])
def test_emit_across_sides(hip, length):
    ids = ids_of(7, length)
    host_index = make_index(ids, "host")
    emitted = host_index.emit(like=None, to_numpy=False)
    assert isinstance(emitted, engine.DeviceArray) and emitted.dtype == np.int64 and np.array_equal(emitted.download(), ids)
    assert host_index.emit(like=None, to_numpy=False) is emitted  # (uploaded once)
    assert host_index.emit(like=None, to_numpy=True) is host_index.host
    dev_index = make_index(ids, "dev")
    assert dev_index.emit(like=None, to_numpy=False) is dev_index.dev  # already a ``DeviceArray``: passed through
    got = dev_index.emit(like=None, to_numpy=True)
    assert isinstance(got, np.ndarray) and got.dtype == np.int64 and np.array_equal(got, ids)
    assert dev_index.emit(like=None, to_numpy=True) is got  # (downloaded once)
