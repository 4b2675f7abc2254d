"""The neighbour graph over gallery shards without a device: the numpy merge reference (gallery_shard_graph_ref.merge) against a
from-scratch top-n under heavy ties with candidate ids below and above the stored ids, the refresh argument on the reference (add,
remove, both), the C ABI of trid_index_nn_merge_sharded_f32 (declared, exported, every argument error reported before anything is
dereferenced or launched) and the host rules of GalleryShards.build_neighbours / refresh_neighbours / search_reranked / state_dict."""

import re

import numpy as np
import pytest
import torch

import gallery_shard_graph_ref as SG
import topk_deep_ref as TR
from textreid_amd import GalleryIndex, GalleryShards
from textreid_amd import lib as L

NAME = "trid_index_nn_merge_sharded_f32"


# ------------------------------------------------------------------ the reference
def tie_matrix(rng, G):
    """[G, G] float32, every value a multiple of 1/8 in [-1, 1] (heavy exact ties), not symmetric, both zeros present"""
    sim = (rng.randint(-8, 9, size=(G, G)) / 8).astype(np.float32)
    sim[rng.randint(0, 4, size=(G, G)) == 0] *= np.float32(-1.0)  # (some +0 become -0)
    assert (sim != sim.T).any() and np.signbit(sim[sim == 0]).any() and not np.signbit(sim[sim == 0]).all()
    return sim


def grown(old_sizes, sizes):
    """-> the rows of the concatenated NEW gallery that the old graph covered"""
    off = SG.offsets(sizes)
    old = list(old_sizes) + [0] * (len(sizes) - len(old_sizes))
    return np.concatenate([np.arange(off[s], off[s] + old[s]) for s in range(len(sizes))]).astype(np.int64)


# candidates below the ids of shard 2 and above those of shard 0 (shard 1 grows); above every stored id (a new shard); both
CASES = [([30, 20, 25], [30, 29, 25]), ([30, 20, 25], [30, 20, 25, 7]), ([30, 20, 25], [30, 32, 25, 40]), ([5, 0, 9], [5, 3, 9])]


@pytest.mark.parametrize("n", [1, 5, 8])
@pytest.mark.parametrize("old_sizes,sizes", CASES)
def test_merge_equals_a_from_scratch_top_n_under_heavy_ties(old_sizes, sizes, n):
    rng = np.random.RandomState(17 * n + sum(sizes))
    G = sum(sizes)
    sim = tie_matrix(rng, G)
    keep = grown(old_sizes, sizes)
    live = np.ones(G, dtype=bool)
    live[keep[rng.permutation(keep.size)[: keep.size // 7]]] = False  # removed before the build: no list holds them
    nn_old, val_old = SG.graph(sim[np.ix_(keep, keep)], n, old_sizes, live[keep])
    new = np.setdiff1d(np.arange(G), keep)
    live[new[rng.permutation(new.size)[: new.size // 4]]] = False  # dead candidates
    lives = SG.split(live, sizes)
    want_nn, want_val = SG.graph(sim, n, sizes, live)
    off, off_old = SG.offsets(sizes), SG.offsets(old_sizes)
    checked = 0
    for s, n0 in enumerate(old_sizes):
        if n0 == 0:
            continue
        a, b = nn_old[off_old[s] : off_old[s + 1]], val_old[off_old[s] : off_old[s + 1]]
        for t in range(len(sizes)):
            first = old_sizes[t] if t < len(old_sizes) else 0
            m = sizes[t] - first
            if m == 0:
                continue
            cand = np.ascontiguousarray(sim[off[s] : off[s] + n0, off[t] + first : off[t + 1]].T)
            a, b, redo = SG.merge(cand, m, t * SG.SHARD_STRIDE + first, n0, lives, s, a, b)
            assert redo.sum() == 0  # (nothing a list holds was removed)
        assert np.array_equal(a, want_nn[off[s] : off[s] + n0]), (s, n)
        assert np.array_equal(TR.bits(b), TR.bits(want_val[off[s] : off[s] + n0])), (s, n)
        checked += n0
    assert checked == sum(old_sizes)
    # the candidates were numbered below and above stored rows somewhere
    ids = want_nn[keep][want_nn[keep][:, 0] >= 0]
    if sizes == [30, 29, 25] and n >= 5:
        assert (ids >> SG.SHARD_BITS == 2).any() and (ids >> SG.SHARD_BITS == 0).any() and ((ids >> SG.SHARD_BITS == 1) & ((ids & SG.LOCAL_MASK) >= old_sizes[1])).any()


def test_merge_rules_row_by_row():
    """own row removed; a live row no graph covered; entries that point at a removed row, at a shard >= n_shards and at a local row >=
    live_len; an equal value with a LOWER id goes in front, with a higher id behind; +0 == -0 and the bits are kept; m == 0"""
    S = SG.SHARD_STRIDE
    lives = [np.array([1, 0, 1, 1, 1, 1, 1, 1], dtype=np.uint8), np.zeros(0, dtype=np.uint8), np.array([1, 1, 0, 1], dtype=np.uint8)]
    n = 3
    nn = np.array([[0, 5, 2 * S + 3],           # row 0: fine
                   [0, 2, 3],                   # row 1: removed itself
                   [-1, -1, -1],                # row 2: live, uncovered
                   [0, 2 * S + 2, 3],           # row 3: holds a removed row
                   [0, 3 * S, 3],               # row 4: shard 3 of 3
                   [0, 2 * S + 4, 3],           # row 5: local row 4 of 4
                   [0, S, 3],                   # row 6: the empty shard
                   [2, 2 * S + 3, -1]],         # row 7: a short list: the absent slot is behind every candidate
                  dtype=np.int32)
    val = np.array([[1.0, 0.5, 0.0]] * 8, dtype=np.float32)
    val[7] = [1.0, 0.5, -np.inf]
    # the candidates are the rows 0 (live), 1 (live) and 2 (removed) of shard 2: ids 2 S, 2 S + 1, 2 S + 2
    cand = np.zeros((3, 8), dtype=np.float32)
    cand[:, 0] = [-0.0, 0.0, 9.0]
    cand[:, 7] = [-1.0, -2.0, 9.0]
    a, b, redo = SG.merge(cand, 3, 2 * S, 8, lives, 0, nn, val)
    assert redo.tolist() == [0, 0, 1, 1, 1, 1, 1, 0]
    assert (a[1] == -1).all() and np.isneginf(b[1]).all()
    for i in (2, 3, 4, 5, 6):
        assert np.array_equal(a[i], nn[i]) and np.array_equal(TR.bits(b[i]), TR.bits(val[i]))
    # row 0: -0.0 of id 2 S equals the +0.0 of id 2 S + 3 and has the LOWER id: in front, with its sign bit; +0.0 of id 2 S + 1 equals
    # that -0.0 and has the higher id: behind, so it does not get in; the removed candidate's 9.0 is never looked at
    assert a[0].tolist() == [0, 5, 2 * S] and TR.bits(b[0]).tolist() == TR.bits(np.float32([1.0, 0.5, -0.0])).tolist()
    # row 7: -1.0 fills the absent slot, -2.0 does not displace it
    assert a[7].tolist() == [2, 2 * S + 3, 2 * S] and TR.bits(b[7]).tolist() == TR.bits(np.float32([1.0, 0.5, -1.0])).tolist()
    # the pure-removal pass flags the same rows and moves nothing else
    a0, b0, r0 = SG.merge(None, 0, 0, 8, lives, 0, nn, val)
    assert r0.tolist() == redo.tolist() and np.array_equal(a0[[0, 7]], nn[[0, 7]])


@pytest.mark.parametrize("n", [1, 5, 8])
@pytest.mark.parametrize("old_sizes,sizes", CASES)
def test_reference_refresh_equals_the_graph_of_the_final_gallery(old_sizes, sizes, n):
    """the refresh argument: a stored top-n list that holds no removed row, merged with the new live rows under (value, global id),
    is the top n of the union - add alone, remove alone, both"""
    rng = np.random.RandomState(29 * n + sum(sizes))
    G = sum(sizes)
    sim = tie_matrix(rng, G)
    keep = grown(old_sizes, sizes)
    live0 = np.ones(G, dtype=bool)
    nn_old, val_old = SG.graph(sim[np.ix_(keep, keep)], n, old_sizes, live0[keep])
    nn_parts, val_parts = SG.split(nn_old, old_sizes), SG.split(val_old, old_sizes)

    def check(live, old, now, nn, val, sub=None):
        m = sim if sub is None else sim[np.ix_(sub, sub)]
        got = SG.refresh(m, live, old, now, nn, val, group=4)
        want = SG.graph(m, n, now, live)
        assert np.array_equal(got[0], want[0]) and np.array_equal(TR.bits(got[1]), TR.bits(want[1]))
        return got[2], got[3]

    # add alone
    assert check(live0, old_sizes, sizes, nn_parts, val_parts) == (G - keep.size, 0)
    # remove alone (on the old gallery): rows that lists hold
    live = np.ones(keep.size, dtype=bool)
    held = SG.to_concat(nn_old[:, 0], old_sizes)
    live[np.unique(held)[:3]] = False
    if live.sum() >= n:
        new_rows, redone = check(live, old_sizes, old_sizes, nn_parts, val_parts, sub=keep)
        assert new_rows == 0 and (redone > 0 or n == 1)
    # both: old and just-added rows removed
    live = np.ones(G, dtype=bool)
    live[keep[rng.permutation(keep.size)[: keep.size // 6]]] = False
    new = np.setdiff1d(np.arange(G), keep)
    live[new[: max(1, new.size // 3)]] = False
    new_rows, redone = check(live, old_sizes, sizes, nn_parts, val_parts)
    assert new_rows == int(live[new].sum())


# ------------------------------------------------------------------ the C ABI
def test_the_symbol_is_declared_and_exported():
    lib = L.load()
    assert NAME in L.EXPORTS and hasattr(lib, NAME)
    assert L.DECLS[NAME] == ("int", "pliiipppliippipp")
    assert NAME + "(" in open(L.HEADER_PATH).read()


FAKE = 0x10000  # a 16-byte aligned non-null address: every limit is checked before anything is dereferenced or launched


def _merge(cand=FAKE, ld_cand=100, m=4, cand_first=(2 << 21) + 7, rows=100, live_all=FAKE, live_off=FAKE, live_len=FAKE, live_bytes=500, n_shards=3,
           self_shard=1, nn=FAKE, nn_val=FAKE, n=5, redo=FAKE):
    L.call(NAME, cand, ld_cand, m, cand_first, rows, live_all, live_off, live_len, live_bytes, n_shards, self_shard, nn, nn_val, n, redo, None)


@pytest.mark.parametrize("kw,word", [
    (dict(live_all=None), "null"),
    (dict(live_off=None), "null"),
    (dict(live_len=None), "null"),
    (dict(nn=None), "null"),
    (dict(nn_val=None), "null"),
    (dict(redo=None), "null"),
    (dict(cand=None), "null"),
    (dict(n=0), "n must be"),
    (dict(n=9), "n must be"),
    (dict(m=-1), "m must be"),
    (dict(n_shards=0), "n_shards must be"),
    (dict(n_shards=1024, self_shard=0), "n_shards must be"),
    (dict(self_shard=-1), "self_shard must be"),
    (dict(self_shard=3), "self_shard must be"),
    (dict(rows=0), "rows must be"),
    (dict(rows=-3), "rows must be"),
    (dict(rows=1 << 21, ld_cand=1 << 21), "rows must be"),
    (dict(live_bytes=0), "live_bytes"),
    (dict(cand_first=-1), "cand_first"),
    (dict(cand_first=(1 << 21) - 3, m=4), "ONE shard"),
    (dict(ld_cand=99), "ld_cand"),
    (dict(ld_cand=0), "ld_cand"),
    (dict(cand=FAKE + 2), "aligned"),
    (dict(nn=FAKE + 1), "aligned"),
    (dict(nn_val=FAKE + 2), "aligned"),
    (dict(live_len=FAKE + 2), "aligned"),
    (dict(live_off=FAKE + 4), "aligned"),
])
def test_bad_arguments_are_errors_that_name_the_function(kw, word):
    with pytest.raises(RuntimeError, match=NAME) as e:
        _merge(**kw)
    assert re.search(word, str(e.value)), str(e.value)
    assert L.last_error().startswith(NAME + ":")
    # the process survives and the library still answers
    assert L.load().trid_topk_rows_deep_ws_bytes(4, 100, 10, 0) > 0


# ------------------------------------------------------------------ host rules of the shards
def _fake_graph(sh, n=5):
    """lists and values as a build would leave them, on the host (the rules are checked before anything touches a device)"""
    sh._g_nn = [torch.full((max(len(p), 8), n), -1, dtype=torch.int32) for p in sh.parts]
    sh._g_val = [torch.full((max(len(p), 8), n), float("-inf")) for p in sh.parts]
    sh._g_sig = sh._sig()


def test_no_graph_is_a_runtime_error_that_names_build_neighbours():
    sh = GalleryShards(shard_rows=32)
    assert sh.neighbours is None and sh.neighbour_values is None and not sh.neighbours_current and not sh.neighbours_refreshable
    with pytest.raises(RuntimeError, match="refresh_neighbours: .*build_neighbours"):
        sh.refresh_neighbours()
    q = torch.zeros(3, 256)
    for name in ("search_reranked", "search_reranked_pids"):
        with pytest.raises(RuntimeError, match=name + ": the neighbour graph is absent.*build_neighbours"):
            getattr(sh, name)(q, k=5)
    # the argument rules come first, the device's rule last
    with pytest.raises(ValueError, match="search_reranked: k must be"):
        sh.search_reranked(q, k=0)
    with pytest.raises(ValueError, match="search_reranked: expected"):
        sh.search_reranked(torch.zeros(3, 8), k=5)
    _fake_graph(sh)
    assert sh.neighbours_current and sh.neighbours_refreshable
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        sh.search_reranked(q, k=5)
    # lists without values: current, not refreshable
    sh._g_val = None
    assert sh.neighbours_current and not sh.neighbours_refreshable and sh.neighbour_values is None
    with pytest.raises(RuntimeError, match="refresh_neighbours: .*without its values.*build_neighbours"):
        sh.refresh_neighbours()


def test_build_rules():
    sh = GalleryShards()
    for n in (0, 9, 2.0):
        with pytest.raises(ValueError, match="build_neighbours: n must be in \\[1, 8\\]"):
            sh.build_neighbours(n)
    with pytest.raises(ValueError, match="build_neighbours: the shards are empty"):
        sh.build_neighbours(5)
    sh._parts[0]._n = 10
    sh._parts[0]._dead = 7
    with pytest.raises(ValueError, match="build_neighbours: n must be <= live_count = 3"):
        sh.build_neighbours(5)


def test_more_than_1023_shards_are_refused():
    sh = GalleryShards(shard_rows=1)
    sh._parts = [GalleryIndex() for _ in range(1024)]
    assert sh.n_shards == 1024
    with pytest.raises(ValueError, match="build_neighbours: .*1023 shards"):
        sh.build_neighbours(5)
    sh._parts = sh._parts[:1023]
    with pytest.raises(ValueError, match="build_neighbours: the shards are empty"):  # (the next rule)
        sh.build_neighbours(5)


def test_the_graph_goes_stale_after_add_and_remove():
    sh = GalleryShards(shard_rows=32)
    sh._parts[0]._n = 20
    _fake_graph(sh)
    assert sh.neighbours_current and tuple(sh.neighbours[0].shape) == (20, 5) and tuple(sh.neighbour_values[0].shape) == (20, 5)
    assert sh.refresh_neighbours() == (0, 0)  # (current: no launch)
    sh._parts[0]._n = 21  # what add leaves behind
    assert not sh.neighbours_current and sh.neighbours_refreshable
    with pytest.raises(RuntimeError, match="search_reranked: the neighbour graph is stale.*build_neighbours"):
        sh.search_reranked(torch.zeros(1, 256), k=5)
    assert sh.state_dict()["neighbours"] is None and sh.state_dict()["neighbour_values"] is None
    sh._parts[0]._n = 20
    assert sh.neighbours_current
    sh._parts[0]._dead = 1  # what remove leaves behind
    assert not sh.neighbours_current
    sh._parts[0]._dead = 0
    sh._parts.append(GalleryIndex())  # a part opened since
    assert not sh.neighbours_current
    # n beyond live_count is build_neighbours' error, raised before anything is modified
    sh._parts[0]._dead = 17
    with pytest.raises(ValueError, match="build_neighbours: n must be <= live_count = 3"):
        sh.refresh_neighbours()


def test_a_state_dict_written_before_the_graph_existed_loads_without_one():
    sh = GalleryShards(shard_rows=32)
    _fake_graph(sh)
    old = {"shard_rows": 96, "collective": False, "parts": [GalleryIndex().state_dict(), GalleryIndex().state_dict()]}
    sh.load_state_dict(old)
    assert sh.shard_rows == 96 and sh.n_shards == 2 and sh.neighbours is None and not sh.neighbours_current and not sh.neighbours_refreshable
    sd = sh.state_dict()
    assert sd["neighbours"] is None and sd["neighbour_values"] is None and len(sd["parts"]) == 2
    # malformed lists are refused by name
    for bad in ([torch.zeros(0, 5, dtype=torch.int32)], [torch.zeros(0, 5), torch.zeros(0, 5)], [torch.zeros(0, 9, dtype=torch.int32)] * 2,
                [torch.zeros(1, 5, dtype=torch.int32)] * 2):
        with pytest.raises(ValueError, match="load_state_dict: neighbours must be"):
            sh.load_state_dict(dict(old, neighbours=bad))
    with pytest.raises(ValueError, match="load_state_dict: neighbour_values must be"):
        sh.load_state_dict(dict(old, neighbours=[torch.zeros(0, 5, dtype=torch.int32)] * 2, neighbour_values=[torch.zeros(0, 4)] * 2))
    sh.load_state_dict(dict(old, neighbours=[torch.zeros(0, 5, dtype=torch.int32)] * 2, neighbour_values=[torch.zeros(0, 5)] * 2))
    assert sh.neighbours_current and sh.neighbours_refreshable and len(sh.neighbours) == 2


def test_by_rank_refresh_is_refused():
    sh = GalleryShards(collective=True)
    with pytest.raises(RuntimeError, match="refresh_neighbours: the by-rank form.*build_neighbours"):
        sh.refresh_neighbours()
    _fake_graph(sh)
    with pytest.raises(RuntimeError, match="refresh_neighbours: the by-rank form.*build_neighbours"):
        sh.refresh_neighbours()
