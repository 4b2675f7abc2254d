"""Row removal and filtered search of GalleryIndex without a device: the two new entry points exist and reject bad arguments by
name before any launch, the host rules of remove / search(mask=...) that need no storage, and the CPU comparator of the GPU tests
(gallery_mask_ref) against brute force."""

import re

import pytest
import torch

import gallery_mask_ref as MR
from textreid_amd import GalleryIndex
from textreid_amd import lib as L

NEW = ("trid_index_search_masked_p16", "trid_index_pack_mask_u32")


def test_new_symbols_are_declared_and_exported():
    lib = L.load()
    for name in NEW:
        assert name in L.DECLS, name
        assert hasattr(lib, name), name
    assert L.DECLS["trid_index_search_masked_p16"] == ("int", "pppp" + "iii" + "l" + "ppp" + "i" + "p")
    assert L.DECLS["trid_index_pack_mask_u32"] == ("int", "ppipip")
    # the unmasked entry point keeps its signature
    assert L.DECLS["trid_index_search_p16"] == ("int", "ppp" + "iii" + "l" + "ppp" + "i" + "p")


FAKE = 0x10000  # a 16-byte aligned non-null address: every limit is checked before anything is dereferenced or launched


def _masked(q16=FAKE, g16=FAKE, unit=FAKE, words=FAKE, Q=4, G=100, k=10, off=0, val=FAKE, idx=FAKE, ws=FAKE, wg=0):
    L.call("trid_index_search_masked_p16", q16, g16, unit, words, Q, G, k, off, val, idx, ws, wg, None)


@pytest.mark.parametrize("kw,word", [
    (dict(words=None), "null mask_words"),
    (dict(g16=None), "null"),
    (dict(words=FAKE + 2), "4-byte aligned"),
    (dict(Q=33), "Q"),
    (dict(Q=0), "Q"),
    (dict(k=17), "k must be"),
    (dict(k=11, G=10), "k must be"),
    (dict(G=1 << 21), "2\\^31"),
    (dict(q16=FAKE + 4), "aligned"),
    (dict(wg=-1), "workgroups"),
])
def test_masked_search_limits_are_errors_that_name_the_function(kw, word):
    with pytest.raises(RuntimeError, match="trid_index_search_masked_p16") as e:
        _masked(**kw)
    assert re.search(word, str(e.value)), str(e.value)
    assert L.load().trid_index_search_ws_bytes(100, 4, 10, 0) > 0  # the process survives and the library still answers


def _pack(live=FAKE, allow=FAKE, n=100, words=FAKE, n_words=4):
    L.call("trid_index_pack_mask_u32", live, allow, n, words, n_words, None)


@pytest.mark.parametrize("kw,word", [
    (dict(live=None, allow=None), "both NULL"),
    (dict(n_words=3), "n_words"),
    (dict(n=129, n_words=4), "n_words"),
    (dict(words=None), "null words"),
    (dict(words=FAKE + 1), "4-byte aligned"),
    (dict(n=0), "n >= 1"),
])
def test_pack_mask_limits_are_errors_that_name_the_function(kw, word):
    with pytest.raises(RuntimeError, match="trid_index_pack_mask_u32") as e:
        _pack(**kw)
    assert re.search(word, str(e.value)), str(e.value)


def test_remove_takes_exactly_one_of_rows_and_pids():
    idx = GalleryIndex()
    with pytest.raises(ValueError, match="exactly one"):
        idx.remove()
    with pytest.raises(ValueError, match="exactly one"):
        idx.remove(rows=[0], pids=[1])
    idx._n = 10  # (rows held: the rule is an argument check that comes before anything touches the storage)
    with pytest.raises(ValueError, match="exactly one"):
        idx.remove(rows=torch.tensor([1]), pids=torch.tensor([1]))


def test_remove_by_pid_needs_pids():
    with pytest.raises(ValueError, match="no pids"):
        GalleryIndex().remove(pids=[3])  # an empty index
    idx = GalleryIndex()
    idx._n, idx._has_pids = 10, False  # (as adds without pids leave it)
    with pytest.raises(ValueError, match="no pids"):
        idx.remove(pids=torch.tensor([3]))


def test_remove_rows_argument_rules_without_storage():
    idx = GalleryIndex()
    assert idx.remove(rows=[]) == 0
    with pytest.raises(ValueError, match="rows must be in"):
        idx.remove(rows=[0])  # an empty index has no row 0
    idx._n = 10
    with pytest.raises(ValueError, match="rows must be in"):
        idx.remove(rows=[3, 10])
    with pytest.raises(ValueError, match="rows must be in"):
        idx.remove(rows=torch.tensor([-1, 2]))
    with pytest.raises(ValueError, match="int64"):
        idx.remove(rows=torch.tensor([1.0]))


def test_live_properties_of_an_empty_index_and_state_dict_key():
    idx = GalleryIndex()
    assert idx.live is None and idx.live_count == 0
    sd = idx.state_dict()
    assert "live" in sd and sd["live"] is None
    assert idx.compact().numel() == 0


def test_mask_type_and_shape_checks():
    idx = GalleryIndex()
    idx._n = 100  # (the mask rules are argument checks: they come before the device check)
    q = torch.zeros(1, 256)
    with pytest.raises(ValueError, match="bool or uint8"):
        idx.search(q, k=1, mask=torch.ones(100))
    with pytest.raises(ValueError, match="bool or uint8"):
        idx.search(q, k=1, mask=torch.ones(100, dtype=torch.int64))
    with pytest.raises(ValueError, match="bool or uint8"):
        idx.search(q, k=1, mask=[True] * 100)
    with pytest.raises(ValueError, match="shape"):
        idx.search(q, k=1, mask=torch.ones(99, dtype=torch.bool))
    with pytest.raises(ValueError, match="shape"):
        idx.search(q, k=1, mask=torch.ones(101, dtype=torch.uint8))
    with pytest.raises(ValueError, match="shape"):
        idx.search(q, k=1, mask=torch.ones(1, 100, dtype=torch.bool))
    with pytest.raises(ValueError, match="k must be"):  # the k <= len rule holds with a mask too
        idx.search(q, k=17, mask=torch.ones(100, dtype=torch.bool))
    with pytest.raises(RuntimeError, match="no CPU fallback"):  # a well-formed mask gets as far as the device check
        idx.search(q, k=1, mask=torch.ones(100, dtype=torch.bool))


def test_k_beyond_live_count_is_a_value_error():
    idx = GalleryIndex()
    idx._n, idx._dead = 20, 15  # (as removals leave the host counts)
    assert idx.live_count == 5
    with pytest.raises(ValueError, match="live_count = 5"):
        idx.search(torch.zeros(1, 256), k=6)
    with pytest.raises(RuntimeError, match="no CPU fallback"):  # k = 5 passes the rule
        idx.search(torch.zeros(1, 256), k=5)


# ------------------------------------------------------------------------------------------------ the comparator itself
@pytest.mark.parametrize("n", [1, 31, 32, 33, 64, 65, 100])
def test_pack_words_against_bit_loops(n):
    g = torch.Generator().manual_seed(n)
    allow = torch.rand(n, generator=g) < 0.5
    allow[n - 1] = True
    words = MR.pack_words(allow)
    assert words.dtype == torch.int64 and words.numel() == (n + 31) // 32
    want = [0] * ((n + 31) // 32)
    for r in range(n):
        if bool(allow[r]):
            want[r >> 5] |= 1 << (r & 31)
    assert words.tolist() == want
    assert MR.pack_words(torch.ones(n, dtype=torch.uint8)).tolist()[-1] == (1 << (((n - 1) & 31) + 1)) - 1
    assert MR.words_as_int64(torch.tensor([-1, 5], dtype=torch.int32)).tolist() == [0xFFFFFFFF, 5]


def _brute(sim, allow, k):
    vals, rows = [], []
    for q in range(sim.shape[0]):
        pairs = sorted(((-float(sim[q, r]), r) for r in range(sim.shape[1]) if bool(allow[r])))[:k]
        vals.append([-v for v, _ in pairs] + [float("-inf")] * (k - len(pairs)))
        rows.append([r for _, r in pairs] + [-1] * (k - len(pairs)))
    return torch.tensor(vals, dtype=sim.dtype), torch.tensor(rows, dtype=torch.int64)


@pytest.mark.parametrize("Q,G,k,keep", [(1, 1, 1, 1.0), (3, 7, 5, 0.5), (4, 40, 10, 0.5), (2, 40, 10, 0.1), (2, 9, 4, 0.0), (5, 70, 16, 1.0)])
def test_masked_topk_against_brute_force(Q, G, k, keep):
    g = torch.Generator().manual_seed(100 * G + k)
    sim = torch.randn(Q, G, generator=g)
    sim = (sim * 2).round() / 2  # (a coarse grid: exact ties, which the row rule must order)
    allow = torch.rand(G, generator=g) < keep
    vals, rows = MR.masked_topk(sim, allow, k)
    bv, br = _brute(sim, allow, k)
    assert torch.equal(rows, br) and torch.equal(vals, bv)
    if int(allow.sum()) < k:
        assert bool((rows[:, int(allow.sum()):] == -1).all()) and bool(torch.isinf(vals[:, int(allow.sum()):]).all())
