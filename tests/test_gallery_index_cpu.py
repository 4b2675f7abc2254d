"""GalleryIndex without a device: construction, argument errors, and the limits of trid_index_search_p16, which are checked
before any launch."""

import pytest
import torch

from textreid_amd import GalleryIndex
from textreid_amd import lib as L


def test_exported_from_the_package_and_constructs_without_a_device():
    import textreid_amd
    from textreid_amd.index import GalleryIndex as G2

    assert textreid_amd.GalleryIndex is G2
    idx = GalleryIndex()
    assert len(idx) == 0 and idx.pids is None and idx.dim == 256
    assert len(GalleryIndex(dim=256, capacity=100)) == 0
    sd = idx.state_dict()
    assert sd["rows"] is None and sd["pids"] is None


def test_value_errors():
    with pytest.raises(ValueError):
        GalleryIndex(dim=128)
    idx = GalleryIndex()
    with pytest.raises(ValueError, match="empty"):
        idx.search(torch.zeros(1, 256), k=1)
    with pytest.raises(ValueError):
        idx.add(torch.zeros(3, 128))
    with pytest.raises(ValueError):
        idx.add(torch.zeros(3, 256), pids=torch.zeros(2, dtype=torch.int64))
    with pytest.raises(ValueError, match="2\\*\\*21 - 1"):
        idx.add(torch.zeros(1, 256).expand(1 << 21, 256))


def test_k_beyond_16_is_a_value_error():
    idx = GalleryIndex()
    idx._n = 100  # (rows held: the k rule is checked before anything touches the storage)
    with pytest.raises(ValueError, match="k must be"):
        idx.search(torch.zeros(1, 256), k=17)
    with pytest.raises(ValueError, match="k must be"):
        idx.search(torch.zeros(1, 256), k=0)
    idx._n = 5
    with pytest.raises(ValueError, match="k must be"):
        idx.search(torch.zeros(1, 256), k=6)


def test_pids_on_every_add_or_on_none():
    """the rule is an argument check: it comes before the device check, so it shows without a device"""
    idx = GalleryIndex()
    idx._has_pids = True  # (as an earlier add with pids leaves it)
    with pytest.raises(ValueError, match="every add or on none"):
        idx.add(torch.zeros(2, 256))
    idx._has_pids = False
    with pytest.raises(ValueError, match="every add or on none"):
        idx.add(torch.zeros(2, 256), pids=torch.zeros(2, dtype=torch.int64))


def test_cpu_tensors_are_refused():
    idx = GalleryIndex()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        idx.add(torch.zeros(2, 256))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        idx.add(torch.zeros(2, 256), pids=torch.zeros(2, dtype=torch.int64))
    assert len(idx) == 0 and idx.pids is None
    idx._n = 4
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        idx.search(torch.zeros(1, 256), k=1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        GalleryIndex().load_state_dict({"rows": torch.zeros(2, 256), "pids": None})


def test_ws_bytes_positive_and_grows_with_workgroups():
    lib = L.load()
    sizes = [lib.trid_index_search_ws_bytes(20037, 32, 16, w) for w in (1, 2, 3, 64, 256)]
    assert sizes[0] > 0 and all(a < b for a, b in zip(sizes, sizes[1:]))
    assert lib.trid_index_search_ws_bytes(20037, 5, 10, 3) == 3 * 5 * 10 * 8
    auto = lib.trid_index_search_ws_bytes(1000000, 32, 16, 0)
    assert 0 < auto <= lib.trid_index_search_ws_bytes(1000000, 32, 16, 4096)
    assert lib.trid_index_search_ws_bytes(1, 1, 1, 0) > 0
    # one worker per step tile at most when the library chooses
    assert lib.trid_index_search_ws_bytes(65, 1, 1, 0) == 2 * 8


FAKE = 0x10000  # a 16-byte aligned non-null address: every limit is checked before anything is dereferenced or launched


def _search(q16=FAKE, g16=FAKE, unit=FAKE, Q=4, G=100, k=10, off=0, val=FAKE, idx=FAKE, ws=FAKE, wg=0):
    L.call("trid_index_search_p16", q16, g16, unit, Q, G, k, off, val, idx, ws, wg, None)


@pytest.mark.parametrize("kw,word", [
    (dict(q16=None, g16=None, unit=None, val=None, idx=None, ws=None), "null"),
    (dict(g16=None), "null"),
    (dict(Q=33), "Q"),
    (dict(Q=0), "Q"),
    (dict(k=17), "k must be"),
    (dict(k=0), "k must be"),
    (dict(k=11, G=10), "k must be"),
    (dict(G=1 << 21), "2\\^31"),
    (dict(G=0), "G"),
    (dict(q16=FAKE + 4), "aligned"),
    (dict(wg=-1), "workgroups"),
    (dict(wg=1 << 20), "workgroups"),
])
def test_entry_point_limits_are_errors_that_name_the_function(kw, word):
    with pytest.raises(RuntimeError, match="trid_index_search_p16") as e:
        _search(**kw)
    assert __import__("re").search(word, str(e.value)), str(e.value)
    # the process survives and the library still answers
    assert L.load().trid_index_search_ws_bytes(100, 4, 10, 0) > 0
