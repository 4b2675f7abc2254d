"""GalleryIndex.search_pids without a device: the CPU comparator of the GPU tests (gallery_distinct_ref.distinct_topk) against a
dict-based brute force, index.group_ids, the new entry point's declaration and argument errors, the host rules of search_pids."""

import re

import pytest
import torch

import gallery_distinct_ref as DR
from textreid_amd import GalleryIndex
from textreid_amd import lib as L

NAME = "trid_index_search_distinct_p16"


# ------------------------------------------------------------------------------------------------ the comparator itself
def _brute(sim, gid, allow, k):
    vals, rows = [], []
    for q in range(sim.shape[0]):
        best = {}  # group -> (-value, row) of its first allowed row in the order rule
        for r in range(sim.shape[1]):
            if bool(allow[r]) and float(sim[q, r]) != float("-inf"):
                key = (-float(sim[q, r]), r)
                g = int(gid[r])
                if g not in best or key < best[g]:
                    best[g] = key
        pairs = sorted(best.values())[:k]
        vals.append([-v for v, _ in pairs] + [float("-inf")] * (k - len(pairs)))
        rows.append([r for _, r in pairs] + [-1] * (k - len(pairs)))
    return torch.tensor(vals, dtype=sim.dtype), torch.tensor(rows, dtype=torch.int64)


@pytest.mark.parametrize("levels", [2, 4, 50])
@pytest.mark.parametrize("G,k", [(1, 1), (7, 5), (40, 10), (70, 16)])
def test_distinct_topk_against_brute_force(G, k, levels):
    g = torch.Generator().manual_seed(1000 * G + 10 * k + levels)
    Q = 3
    for groups in sorted({1, max(k - 1, 1), k, k + 1, G}):
        sim = torch.randint(0, levels, (Q, G), generator=g).float() / levels - 0.5  # few distinct values: exact ties
        gid = torch.randint(0, groups, (G,), generator=g) * 977 - 5
        gid[: min(groups, G)] = torch.arange(min(groups, G)) * 977 - 5  # (every group occurs when there is room)
        for keep in (1.0, 0.5, 0.0):
            allow = torch.rand(G, generator=g) < keep
            vals, rows = DR.distinct_topk(sim, gid, allow, k)
            bv, br = _brute(sim, gid, allow, k)
            assert torch.equal(rows, br) and torch.equal(vals, bv), (groups, keep)
            n = len(set(gid[allow].tolist()))
            assert bool((rows[:, :min(n, k)] >= 0).all()) and bool((rows[:, n:] == -1).all()) and bool(torch.isinf(vals[:, n:]).all())
            for q in range(Q):  # at most one row per group
                real = rows[q][rows[q] >= 0]
                assert len(set(gid[real].tolist())) == real.numel()


def test_distinct_topk_with_all_groups_different_is_the_masked_topk():
    import gallery_mask_ref as MR

    g = torch.Generator().manual_seed(3)
    sim = (torch.randn(4, 50, generator=g) * 2).round() / 2
    allow = torch.rand(50, generator=g) < 0.6
    a, b = DR.distinct_topk(sim, torch.arange(50), allow, 10), MR.masked_topk(sim, allow, 10)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ----------------------------------------------------------------------------------------------------------- group ids
def test_group_ids_equal_pids_equal_ids():
    from textreid_amd.index import group_ids

    g = torch.Generator().manual_seed(5)
    pool = torch.tensor([-(1 << 40), -7, -1, 0, 1, 5, (1 << 31) - 1, 1 << 31, (1 << 31) + 1, (1 << 40) + 5, (1 << 62)], dtype=torch.int64)
    pids = pool[torch.randint(0, pool.numel(), (200,), generator=g)]
    ids = group_ids(pids)
    assert ids.dtype == torch.int32 and ids.shape == (200,) and ids.device == pids.device
    assert torch.equal(ids.view(-1, 1) == ids.view(1, -1), pids.view(-1, 1) == pids.view(1, -1))
    assert int(ids.min()) >= 0 and int(ids.max()) < 200
    # 2^31 and 2^31 + 2^32 differ in their upper halves only
    assert group_ids(torch.tensor([1 << 31, (1 << 31) + (1 << 32), 1 << 31])).tolist() == [0, 1, 0]
    assert group_ids(torch.tensor([], dtype=torch.int64)).shape == (0,) and group_ids([3]).tolist() == [0]
    assert group_ids([9, 9, 9]).tolist() == [0, 0, 0] and group_ids(torch.tensor([[4, 2], [4, 7]])).tolist() == [1, 0, 1, 2]


def test_group_ids_are_stable_under_appending():
    """rows appended later never change which earlier rows belong together, and a later row of an earlier pid joins its group"""
    from textreid_amd.index import group_ids

    g = torch.Generator().manual_seed(6)
    old = torch.randint(-20, 20, (100,), generator=g) * (1 << 33)
    new = torch.randint(-30, 30, (60,), generator=g) * (1 << 33)
    a, b = group_ids(old), group_ids(torch.cat([old, new]))
    assert torch.equal(a.view(-1, 1) == a.view(1, -1), b[:100].view(-1, 1) == b[:100].view(1, -1))
    both = torch.cat([old, new])
    assert torch.equal(b.view(-1, 1) == b.view(1, -1), both.view(-1, 1) == both.view(1, -1))
    assert torch.equal(group_ids(old), a)  # a function of its argument


# --------------------------------------------------------------------------------------------------------- the C entry
def test_new_symbol_is_declared_and_exported():
    lib = L.load()
    assert NAME in L.DECLS and NAME in L.EXPORTS and hasattr(lib, NAME)
    assert L.DECLS[NAME] == ("int", "ppppp" + "iii" + "l" + "ppp" + "i" + "p")
    # the existing entry points keep their signatures
    assert L.DECLS["trid_index_search_masked_p16"] == ("int", "pppp" + "iii" + "l" + "ppp" + "i" + "p")
    assert L.DECLS["trid_index_search_p16"] == ("int", "ppp" + "iii" + "l" + "ppp" + "i" + "p")


FAKE = 0x10000  # a 16-byte aligned non-null address: every limit is checked before anything is dereferenced or launched


def _distinct(q16=FAKE, g16=FAKE, unit=FAKE, gids=FAKE, words=FAKE, Q=4, G=100, k=10, off=0, val=FAKE, idx=FAKE, ws=FAKE, wg=0):
    L.call(NAME, q16, g16, unit, gids, words, Q, G, k, off, val, idx, ws, wg, None)


@pytest.mark.parametrize("kw,word", [
    (dict(gids=None), "null group_ids"),
    (dict(g16=None), "null operand"),
    (dict(q16=None), "null operand"),
    (dict(ws=None), "null operand"),
    (dict(gids=FAKE + 2), "group_ids must be 4-byte aligned"),
    (dict(words=FAKE + 2), "mask_words must be 4-byte aligned"),
    (dict(Q=33), "Q"),
    (dict(Q=0), "Q"),
    (dict(k=17), "k must be"),
    (dict(k=11, G=10), "k must be"),
    (dict(G=1 << 21), "2\\^31"),
    (dict(q16=FAKE + 4), "aligned"),
    (dict(wg=-1), "workgroups"),
    (dict(wg=4097), "workgroups"),
])
def test_distinct_search_limits_are_errors_that_name_the_function(kw, word):
    with pytest.raises(RuntimeError, match=NAME) as e:
        _distinct(**kw)
    assert re.search(word, str(e.value)), str(e.value)
    assert L.load().trid_index_search_ws_bytes(100, 4, 10, 0) > 0  # the process survives and the library still answers


# ---------------------------------------------------------------------------------------------------- the host rules
def test_search_pids_needs_pids():
    q = torch.zeros(1, 256)
    with pytest.raises(ValueError, match="no pids"):
        GalleryIndex().search_pids(q, k=1)  # an empty index
    idx = GalleryIndex()
    idx._n, idx._has_pids = 10, False  # (as adds without pids leave it)
    with pytest.raises(ValueError, match="search_pids: the index holds no pids"):
        idx.search_pids(q, k=1)


def _with_pids(n, dead=0):
    idx = GalleryIndex()
    idx._n, idx._has_pids, idx._dead = n, True, dead  # (the host state adds with pids and removals leave: the rules need no storage)
    return idx


def test_search_pids_follows_the_k_rules():
    q = torch.zeros(1, 256)
    idx = _with_pids(100)
    for k in (0, 17, -1):
        with pytest.raises(ValueError, match="search_pids: k must be"):
            idx.search_pids(q, k=k)
    with pytest.raises(ValueError, match="k must be"):
        _with_pids(5).search_pids(q, k=6)
    with pytest.raises(ValueError, match="k must be"):  # the k <= len rule holds with a mask too
        idx.search_pids(q, k=17, mask=torch.ones(100, dtype=torch.bool))
    with pytest.raises(ValueError, match="live_count = 5"):
        _with_pids(20, dead=15).search_pids(q, k=6)
    with pytest.raises(ValueError, match="expected a \\[Q, 256\\]"):
        idx.search_pids(torch.zeros(1, 128), k=1)
    with pytest.raises(ValueError, match="no queries"):
        idx.search_pids(torch.zeros(0, 256), k=1)
    with pytest.raises(ValueError, match="bool or uint8"):
        idx.search_pids(q, k=1, mask=torch.ones(100))
    with pytest.raises(ValueError, match="shape"):
        idx.search_pids(q, k=1, mask=torch.ones(99, dtype=torch.bool))
    with pytest.raises(ValueError, match="the index is empty"):
        _with_pids(0).search_pids(q, k=1)


def test_search_pids_refuses_cpu_tensors():
    q = torch.zeros(1, 256)
    with pytest.raises(RuntimeError, match="search_pids runs on the HIP kernel library only.*no CPU fallback"):
        _with_pids(100).search_pids(q, k=16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):  # k = live_count passes the rule
        _with_pids(20, dead=15).search_pids(q, k=5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):  # a well-formed mask gets as far as the device check
        _with_pids(100).search_pids(q, k=1, mask=torch.ones(100, dtype=torch.bool))
