"""The deep distinct select without a device: the numpy reference (gallery_deep_distinct_ref) against a dict-based brute force and
against the older gallery_distinct_ref, group_table against group_ids, the C ABI of trid_index_group_best_f32 and
trid_topk_rows_deep_pairs_f32 (declared, exported, every argument error before anything is dereferenced) and the host rules of
GalleryIndex.shortlist_pids / search_reranked_pids."""

import re

import numpy as np
import pytest
import torch

import gallery_deep_distinct_ref as DR
import gallery_distinct_ref as OLD
import topk_deep_ref as TR
from textreid_amd import GalleryIndex
from textreid_amd import index as IX
from textreid_amd import lib as L


# ------------------------------------------------------------------ the reference
def brute(sim, groups, k, allowed):
    """a dict per query: group -> its best (value, row) by a strict > over ascending rows (the first allowed row starts it whatever
    its value, a real -inf included); then repeated selection of the best remaining representative, ties to the lower row"""
    Q, G = sim.shape
    vals = np.full((Q, k), -np.inf, dtype=np.float32)
    rows = np.full((Q, k), -1, dtype=np.int64)
    for q in range(Q):
        best = {}
        for g in range(G):
            if allowed is not None and not allowed[g]:
                continue
            key = int(groups[g])
            if key not in best or sim[q, g] > sim[q, best[key]]:
                best[key] = g
        left = sorted(best.values())
        for t in range(k):
            if not left:
                break
            top = left[0]
            for g in left[1:]:
                if sim[q, g] > sim[q, top]:
                    top = g
            left.remove(top)
            vals[q, t] = sim[q, top]
            rows[q, t] = top
    return vals, rows


def level_matrix(Q, G, levels, seed, specials=True):
    """values drawn from `levels` levels - heavy ties - with +0 / -0 and real -inf among them"""
    rng = np.random.RandomState(seed)
    pool = np.linspace(-1.0, 1.0, levels).astype(np.float32)
    if specials:
        pool = np.concatenate([pool, np.array([0.0, -0.0, -np.inf], dtype=np.float32)])
    return pool[rng.randint(0, pool.size, size=(Q, G))]


def group_patterns(G, seed):
    rng = np.random.RandomState(seed)
    return {"distinct": np.arange(G), "one": np.zeros(G, dtype=np.int64), "quads": np.arange(G) // 4, "mod7": np.arange(G) % 7,
            "random": rng.randint(0, max(G // 3, 1), size=G), "big values": rng.randint(0, 5, size=G).astype(np.int64) * (1 << 40) - (1 << 41)}


@pytest.mark.parametrize("levels", [2, 4, 50])
@pytest.mark.parametrize("G,k", [(1, 1), (9, 4), (40, 8), (40, 40), (67, 17)])
def test_reference_equals_brute_force_with_heavy_ties_zeros_and_inf(levels, G, k):
    sim = level_matrix(4, G, levels, 5 + G + levels)
    for name, groups in group_patterns(G, G).items():
        assert TR.same(DR.distinct_topk(sim, groups, k), brute(sim, groups, k, None)), name


@pytest.mark.parametrize("left", ["0", "k-1", "k", "k+1"])
def test_reference_masks_that_leave_few_groups(left):
    G, k = 60, 6
    n = {"0": 0, "k-1": k - 1, "k": k, "k+1": k + 1}[left]
    sim = level_matrix(3, G, 4, 11)
    groups = np.arange(G) % 12
    keep = np.random.RandomState(n).permutation(12)[:n]
    allowed = np.isin(groups, keep) & (np.random.RandomState(3).rand(G) < 0.7)
    for g in keep:  # (every kept group keeps at least one row)
        allowed[np.nonzero(groups == g)[0][0]] = True
    got = DR.distinct_topk(sim, groups, k, allowed)
    assert TR.same(got, brute(sim, groups, k, allowed))
    m = min(n, k)
    assert (got[1][:, m:] == -1).all() and np.isneginf(got[0][:, m:]).all() and (got[1][:, :m] >= 0).all()


def test_a_group_whose_only_allowed_score_is_minus_inf_is_a_result():
    sim = np.array([[-np.inf, 1.0, -np.inf, 0.5]], dtype=np.float32)
    groups = np.array([0, 1, 0, 2])
    vals, rows = DR.distinct_topk(sim, groups, 4)
    assert rows.tolist() == [[1, 3, 0, -1]] and np.isneginf(vals[0, 2:]).all()
    bv, br = DR.group_best(sim, *DR.table(groups), 5)
    assert br.tolist() == [[0, 1, 3, DR.ABSENT, DR.ABSENT]]
    allowed = np.array([False, True, True, True])
    assert DR.distinct_topk(sim, groups, 4, allowed)[1].tolist() == [[1, 3, 2, -1]]
    assert TR.same(DR.distinct_topk(sim, groups, 4, allowed), brute(sim, groups, 4, allowed))


def test_ties_between_groups_go_to_the_lower_representative_row():
    # A = {0, 5} with its best at row 5, B = {3}, equal values: B must win (numbering groups by their first row would say A)
    sim = np.array([[0.0, 9.0, 9.0, 1.0, 9.0, 1.0]], dtype=np.float32)
    groups = np.array([7, 1, 2, 8, 3, 7])
    vals, rows = DR.distinct_topk(sim, groups, 5)
    assert rows.tolist() == [[1, 2, 4, 3, 5]]
    assert TR.same((vals, rows), brute(sim, groups, 5, None))


def test_zero_signs_tie_by_row_and_keep_their_bits():
    sim = np.array([[-0.0, 0.0, -0.0, 0.0, -1.0]], dtype=np.float32)
    vals, rows = DR.distinct_topk(sim, np.array([0, 0, 1, 2, 2]), 3)
    assert rows.tolist() == [[0, 2, 3]] and np.signbit(vals).tolist() == [[True, True, False]]


def test_pairs_topk_sentinel_columns_are_absent_whatever_their_value():
    val = np.array([[5.0, 1.0, 7.0, 1.0]], dtype=np.float32)
    col = np.array([[DR.ABSENT, 9, DR.ABSENT, 2]], dtype=np.int32)
    vals, idx = DR.pairs_topk(val, col, 3, offset=100)
    assert idx.tolist() == [[102, 109, -1]] and vals[0, :2].tolist() == [1.0, 1.0] and np.isneginf(vals[0, 2])


def test_pairs_topk_with_numbered_columns_is_the_deep_reference():
    sim = level_matrix(3, 50, 4, 21)
    col = np.broadcast_to(np.arange(50, dtype=np.int32), sim.shape)
    for k in (1, 7, 50):
        assert TR.same(DR.pairs_topk(sim, col, k, 5), TR.topk(sim, k, None, 5))


def test_reference_equals_the_older_distinct_reference_without_inf():
    for levels, seed in ((3, 1), (50, 2)):
        sim = level_matrix(4, 45, levels, seed, specials=False)
        groups = np.random.RandomState(seed).randint(0, 11, size=45)
        allowed = np.random.RandomState(seed + 7).rand(45) < 0.6
        for k in (3, 11, 16):
            want = OLD.distinct_topk(torch.from_numpy(sim), groups, allowed, k)
            assert TR.same(DR.distinct_topk(sim, groups, k, allowed), (want[0].numpy(), want[1].numpy())), (levels, k)


def test_group_best_skips_bad_order_entries_and_clamps_starts():
    sim = level_matrix(2, 10, 50, 8, specials=False)
    order, starts, n = DR.table(np.arange(10) // 3)
    want = DR.group_best(sim, order, starts, n, n)
    bad = order.copy()
    bad[4] = -1  # row 4 (group 1) is skipped: as if it were masked
    allowed = np.ones(10, dtype=bool)
    allowed[4] = False
    assert TR.same(DR.group_best(sim, bad, starts, n, n), DR.group_best(sim, order, starts, n, n, allowed))
    bad[4] = 10
    assert TR.same(DR.group_best(sim, bad, starts, n, n), DR.group_best(sim, order, starts, n, n, allowed))
    wild = starts.copy()
    wild[0], wild[-1] = -5, 1000
    assert TR.same(DR.group_best(sim, order, wild, n, n), want)


# ------------------------------------------------------------------ group_table
@pytest.mark.parametrize("n", [1, 2, 33, 500])
def test_group_table_agrees_with_group_ids(n):
    rng = np.random.RandomState(n)
    for pids in (torch.arange(n), torch.zeros(n, dtype=torch.int64), torch.from_numpy(rng.randint(-5, max(n // 3, 1), size=n)) * (1 << 40),
                 torch.from_numpy(rng.randint(0, 7, size=n)).int()):
        gid = IX.group_ids(pids)
        order, starts, n_groups = IX.group_table(pids)
        assert order.dtype == torch.int32 and starts.dtype == torch.int32 and isinstance(n_groups, int)
        assert n_groups == int(gid.max()) + 1 and tuple(starts.shape) == (n_groups + 1,) and tuple(order.shape) == (n,)
        assert int(starts[0]) == 0 and int(starts[-1]) == n and bool((starts[1:] > starts[:-1]).all())
        assert sorted(order.tolist()) == list(range(n))
        for s in range(n_groups):
            rows = order[int(starts[s]) : int(starts[s + 1])].long()
            assert bool((gid[rows] == s).all()) and bool((rows[1:] > rows[:-1]).all())
        ref = DR.table(pids.numpy())
        assert np.array_equal(order.numpy(), ref[0]) and np.array_equal(starts.numpy(), ref[1]) and n_groups == ref[2]


def test_group_table_of_nothing():
    order, starts, n_groups = IX.group_table(torch.zeros(0, dtype=torch.int64))
    assert order.numel() == 0 and starts.tolist() == [0] and n_groups == 0


# ------------------------------------------------------------------ the C ABI
def test_the_symbols_are_declared_and_exported_and_the_old_signatures_stand():
    lib = L.load()
    for name in ("trid_index_group_best_f32", "trid_topk_rows_deep_pairs_f32"):
        assert name in L.EXPORTS and hasattr(lib, name)
    assert L.DECLS["trid_index_group_best_f32"] == ("int", "plliippiipppllp")
    assert L.DECLS["trid_topk_rows_deep_pairs_f32"] == ("int", "pplliiilppplip")
    assert L.DECLS["trid_topk_rows_deep_f32"] == ("int", "plliiiplppplip")
    assert L.DECLS["trid_topk_rows_deep_ws_bytes"] == ("long long", "iiii") and L.DECLS["trid_topk_rows_deep_chunk"] == ("int", "i")
    assert L.DECLS["trid_index_rerank_add_f32"] == ("int", "plliippifpp")
    assert L.DECLS["trid_index_search_distinct_p16"] == ("int", "pppppiiilpppip")


FAKE = 0x10000  # a 16-byte aligned non-null address: every limit is checked before anything is dereferenced or launched


def _best(scores=FAKE, ld_q=100, ld_g=1, Q=4, G=100, order=FAKE, starts=FAKE, n_groups=30, n_slots=40, mask=None, val=FAKE, row=FAKE,
          out_ld_q=40, out_ld_g=1):
    L.call("trid_index_group_best_f32", scores, ld_q, ld_g, Q, G, order, starts, n_groups, n_slots, mask, val, row, out_ld_q, out_ld_g, None)


@pytest.mark.parametrize("kw,word", [
    (dict(scores=None, order=None, starts=None, val=None, row=None), "null"),
    (dict(scores=None), "null"),
    (dict(order=None), "null"),
    (dict(starts=None), "null"),
    (dict(val=None), "null"),
    (dict(row=None), "null"),
    (dict(Q=0), "Q and G"),
    (dict(G=0), "Q and G"),
    (dict(n_slots=0, n_groups=0), "n_slots"),
    (dict(n_groups=41), "n_groups <= n_slots"),
    (dict(n_groups=-1), "n_groups"),
    (dict(ld_q=99), "alias"),
    (dict(ld_q=1, ld_g=3), "alias"),
    (dict(ld_q=0), "alias"),
    (dict(ld_g=0), "alias"),
    (dict(out_ld_q=39), "output alias"),
    (dict(out_ld_q=1, out_ld_g=3), "output alias"),
    (dict(out_ld_q=0), "output alias"),
    (dict(out_ld_g=0), "output alias"),
    (dict(scores=FAKE + 2), "aligned"),
    (dict(order=FAKE + 2), "aligned"),
    (dict(starts=FAKE + 1), "aligned"),
    (dict(mask=FAKE + 1), "aligned"),
    (dict(val=FAKE + 2), "aligned"),
    (dict(row=FAKE + 3), "aligned"),
    (dict(Q=32 * 65535 + 1, ld_q=1, ld_g=1 << 22, out_ld_q=1, out_ld_g=1 << 22), "groups of queries"),
])
def test_group_best_bad_arguments_are_errors_that_name_the_function(kw, word):
    with pytest.raises(RuntimeError, match="trid_index_group_best_f32") as e:
        _best(**kw)
    assert re.search(word, str(e.value)), str(e.value)
    assert L.last_error().startswith("trid_index_group_best_f32:")
    # the process survives and the library still answers
    assert L.load().trid_topk_rows_deep_ws_bytes(4, 100, 10, 0) > 0


def _pairs(val=FAKE, col=FAKE, ld_q=100, ld_g=1, Q=4, S=100, k=10, off=0, out_val=FAKE, idx=FAKE, ws=FAKE, ws_bytes=None, chunk=0):
    if ws_bytes is None:
        ws_bytes = 1 << 40
    L.call("trid_topk_rows_deep_pairs_f32", val, col, ld_q, ld_g, Q, S, k, off, out_val, idx, ws, ws_bytes, chunk, None)


@pytest.mark.parametrize("kw,word", [
    (dict(val=None, col=None, out_val=None, idx=None, ws=None), "null"),
    (dict(val=None), "null"),
    (dict(col=None), "null"),
    (dict(out_val=None), "null"),
    (dict(idx=None), "null"),
    (dict(ws=None), "null"),
    (dict(k=0), "k must be"),
    (dict(k=1025, S=2000, ld_q=2000), "k must be in \\[1,1024\\]"),
    (dict(k=11, S=10), "<= n_slots = 10"),
    (dict(Q=0), "Q and n_slots"),
    (dict(S=0), "Q and n_slots"),
    (dict(chunk=48), "chunk"),
    (dict(k=100, chunk=128), "chunk"),
    (dict(k=1024, S=4000, ld_q=4000, chunk=1024), "chunk"),
    (dict(chunk=16384), "chunk"),
    (dict(Q=1 << 24, ld_q=1, ld_g=1 << 24), "grid"),
    (dict(Q=1 << 16, S=1 << 16, ld_q=1 << 16, chunk=64), "ceil\\(n_slots / chunk\\)"),
    (dict(ld_q=99), "alias"),
    (dict(ld_q=1, ld_g=3), "alias"),
    (dict(ld_q=0), "alias"),
    (dict(val=FAKE + 2), "aligned"),
    (dict(col=FAKE + 2), "aligned"),
    (dict(idx=FAKE + 4), "aligned"),
    (dict(ws=FAKE + 4), "aligned"),
    (dict(S=20000, ld_q=20000, k=100, ws_bytes=L.load().trid_topk_rows_deep_ws_bytes(4, 20000, 100, 0) - 1), "ws_bytes"),
    (dict(S=3000, ld_q=3000, k=100, chunk=256, ws_bytes=L.load().trid_topk_rows_deep_ws_bytes(4, 3000, 100, 256) - 1), "ws_bytes"),
])
def test_pairs_select_bad_arguments_are_errors_that_name_the_function(kw, word):
    with pytest.raises(RuntimeError, match="trid_topk_rows_deep_pairs_f32") as e:
        _pairs(**kw)
    assert re.search(word, str(e.value)), str(e.value)
    assert L.last_error().startswith("trid_topk_rows_deep_pairs_f32:")
    assert L.load().trid_topk_rows_deep_ws_bytes(4, 100, 10, 0) > 0


def test_the_row_select_keeps_its_messages():
    with pytest.raises(RuntimeError, match="trid_topk_rows_deep_f32: k must be in \\[1,1024\\] and <= G = 10; got 11"):
        L.call("trid_topk_rows_deep_f32", FAKE, 100, 1, 4, 10, 11, None, 0, FAKE, FAKE, FAKE, 1 << 40, 0, None)
    with pytest.raises(RuntimeError, match="trid_topk_rows_deep_f32: sim / mask_words must be 4-byte, out_idx / ws 8-byte aligned"):
        L.call("trid_topk_rows_deep_f32", FAKE + 2, 100, 1, 4, 100, 10, None, 0, FAKE, FAKE, FAKE, 1 << 40, 0, None)
    with pytest.raises(RuntimeError, match="trid_topk_rows_deep_f32: Q and G must be >= 1; got Q = 0, G = 100"):
        L.call("trid_topk_rows_deep_f32", FAKE, 100, 1, 0, 100, 10, None, 0, FAKE, FAKE, FAKE, 1 << 40, 0, None)


# ------------------------------------------------------------------ host rules of the index
@pytest.mark.parametrize("name", ["shortlist_pids", "search_reranked_pids"])
def test_host_rules_hold_without_a_device(name):
    assert IX.MAX_SHORTLIST_K == 1024
    q = torch.zeros(1, 256)
    idx = GalleryIndex()
    fn = getattr(idx, name)
    idx._n = 5000  # (rows held: the rules are checked before anything touches the storage)
    with pytest.raises(ValueError, match="%s: the index holds no pids" % name):
        fn(q, k=10)
    idx._has_pids = True
    for k in (0, -1, 1025):
        with pytest.raises(ValueError, match="%s: k must be in \\[1, 1024\\]" % name):
            fn(q, k=k)
    with pytest.raises(ValueError, match="%s: expected" % name):
        fn(torch.zeros(1, 128), k=1)
    with pytest.raises(ValueError, match="%s: no queries" % name):
        fn(torch.zeros(0, 256), k=1)
    with pytest.raises(ValueError, match="%s: mask must have shape" % name):
        fn(q, k=1, mask=torch.ones(7, dtype=torch.bool))
    with pytest.raises(ValueError, match="%s: mask must be a bool or uint8" % name):
        fn(q, k=1, mask=torch.ones(5000))
    idx._n = 50
    with pytest.raises(ValueError, match="%s: k must be" % name):
        fn(q, k=51)
    idx._dead = 10
    with pytest.raises(ValueError, match="%s: k must be <= live_count = 40" % name):
        fn(q, k=41)
    idx._dead = 0
    if name == "search_reranked_pids":
        with pytest.raises(RuntimeError, match="search_reranked_pids: the neighbour graph is absent.*build_neighbours"):
            fn(q, k=10)
        idx._nn, idx._nn_ok = torch.zeros(50, 5, dtype=torch.int32), False
        with pytest.raises(RuntimeError, match="search_reranked_pids: the neighbour graph is stale.*build_neighbours"):
            fn(q, k=10)
        idx._nn_ok = True
    for k in (1, 17, 50):
        with pytest.raises(RuntimeError, match="%s runs on the HIP kernel library only.*no CPU fallback" % name):
            fn(torch.zeros(2, 256), k=k)
    idx._n = 0
    with pytest.raises(ValueError, match="%s: the index is empty" % name):
        fn(q, k=1)


def test_topk_distinct_rows_refuses_cpu_tensors_and_bad_arguments():
    from textreid_amd import evaluation as E

    with pytest.raises(RuntimeError, match="topk_distinct_rows runs on the HIP kernel library only.*no CPU fallback"):
        E.topk_distinct_rows(torch.zeros(2, 50), torch.zeros(50, dtype=torch.int64), 20)
    with pytest.raises(ValueError, match="topk_distinct_rows: expected"):
        E.topk_distinct_rows(torch.zeros(50), torch.zeros(50, dtype=torch.int64), 20)
