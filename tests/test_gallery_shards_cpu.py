"""GalleryShards without a device: the numpy reference of the list merge (gallery_shards_ref) against a per-candidate insertion
loop, the C ABI of trid_index_merge_lists_f32 (declared, exported, every argument error before anything is dereferenced or
launched), the host rules of GalleryShards and locate."""

import re

import numpy as np
import pytest
import torch

import gallery_shards_ref as SR
from textreid_amd import lib as L


# ------------------------------------------------------------------ the reference
def before(v, r, bv, br):
    return v > bv or (v == bv and r < br)


def brute(val, row, k, list_base=None, pid=None):
    """one candidate at a time into a list kept in the order (value descending by float comparison, global row ascending); with
    pids a candidate replaces a worse entry of its pid and is dropped behind a better one; the first k of the list are the result"""
    Q, S, kin = val.shape
    out_v = np.full((Q, k), -np.inf, dtype=np.float32)
    out_r = np.full((Q, k), -1, dtype=np.int64)
    out_p = np.full((Q, k), -1, dtype=np.int64)
    for q in range(Q):
        held = []  # (value, global row, pid)
        for s in range(S):
            for t in range(kin):
                if row[q, s, t] < 0:
                    continue
                v, r = val[q, s, t], int(row[q, s, t]) + (0 if list_base is None else int(list_base[s]))
                p = None if pid is None else int(pid[q, s, t])
                if p is not None:
                    old = [e for e in held if e[2] == p]
                    if old and not before(v, r, old[0][0], old[0][1]):
                        continue
                    held = [e for e in held if e[2] != p]
                at = 0
                while at < len(held) and before(held[at][0], held[at][1], v, r):
                    at += 1
                held.insert(at, (v, r, p))
        for t, (v, r, p) in enumerate(held[:k]):
            out_v[q, t], out_r[q, t] = v, r
            if p is not None:
                out_p[q, t] = p
    return (out_v, out_r) if pid is None else (out_v, out_r, out_p)


@pytest.mark.parametrize("levels", [2, 4, 50])
@pytest.mark.parametrize("S,kin,k", [(1, 1, 1), (2, 16, 16), (3, 17, 17), (5, 20, 7), (6, 9, 54), (4, 8, 3)])
def test_reference_equals_insertion_loop_with_ties_zeros_inf_and_absent_slots(levels, S, kin, k):
    for sort_lists in (False, True):
        val, row, base, pid = SR.special_inputs(3, S, kin, 7 * S + kin + levels, levels=levels, sort_lists=sort_lists)
        assert SR.same(SR.merge(val, row, k, base), brute(val, row, k, base))
        assert SR.same(SR.merge(val, row, k, None), brute(val, row, k, None))
        assert SR.same(SR.merge(val, row, k, base, pid), brute(val, row, k, base, pid))


def test_reference_all_lists_absent():
    val = np.full((2, 3, 4), np.inf, dtype=np.float32)
    row = np.full((2, 3, 4), -1, dtype=np.int64)
    pid = np.zeros((2, 3, 4), dtype=np.int64)
    for got in (SR.merge(val, row, 5), SR.merge(val, row, 5, None, pid)):
        assert np.isneginf(got[0]).all() and all((g == -1).all() for g in got[1:])
    assert SR.same(SR.merge(val, row, 5, None, pid), brute(val, row, 5, None, pid))


def test_reference_a_pid_in_every_list_with_equal_values_goes_to_the_lowest_global_row():
    val = np.full((1, 3, 2), 0.5, dtype=np.float32)
    val[0, :, 1] = [0.25, 0.75, 0.25]
    row = np.array([[[4, 1], [0, 2], [3, 5]]], dtype=np.int64)
    base = np.array([200, 100, 0], dtype=np.int64)  # (the bases need not ascend: list 2 holds the lowest global rows)
    pid = np.array([[[7, 1], [7, 2], [7, 3]]], dtype=np.int64)
    v, r, p = SR.merge(val, row, 4, base, pid)
    assert r.tolist() == [[102, 3, 5, 201]] and p.tolist() == [[2, 7, 3, 1]] and v.tolist() == [[0.75, 0.5, 0.25, 0.25]]
    assert SR.same((v, r, p), brute(val, row, 4, base, pid))


def test_reference_fewer_distinct_pids_than_k_and_real_minus_inf():
    val = np.array([[[1.0, -np.inf], [-np.inf, 0.0]]], dtype=np.float32)
    row = np.array([[[0, 1], [0, -1]]], dtype=np.int64)
    pid = np.array([[[5, 6], [6, 9]]], dtype=np.int64)
    base = np.array([0, 10], dtype=np.int64)
    v, r, p = SR.merge(val, row, 4, base, pid)
    assert r.tolist() == [[0, 1, -1, -1]] and p.tolist() == [[5, 6, -1, -1]] and np.isneginf(v[0, 1:]).all()
    assert SR.merge(val, row, 4, base)[1].tolist() == [[0, 1, 10, -1]]  # (the real -inf rows are results, the absent slot is not)
    assert SR.same((v, r, p), brute(val, row, 4, base, pid))


def test_reference_zero_signs_tie_by_row_and_keep_their_bits():
    val = np.array([[[-0.0, 0.0], [0.0, -0.0]]], dtype=np.float32)
    row = np.array([[[1, 0], [1, 0]]], dtype=np.int64)
    v, r = SR.merge(val, row, 4, np.array([10, 0], dtype=np.int64))
    assert r.tolist() == [[0, 1, 10, 11]] and np.signbit(v).tolist() == [[True, False, False, True]]


def test_merging_groups_of_lists_and_then_the_results_is_exact():
    val, row, base, pid = SR.special_inputs(3, 6, 12, 3)
    for k in (1, 5, 12, 30):
        for p in (None, pid):
            whole = SR.merge(val, row, k, base, p)
            halves = [SR.merge(val[:, a : a + 2], row[:, a : a + 2], min(k, 24), base[a : a + 2], None if p is None else p[:, a : a + 2]) for a in (0, 2, 4)]
            again = SR.merge(np.stack([h[0] for h in halves], 1), np.stack([h[1] for h in halves], 1), k, None,
                             None if p is None else np.stack([h[2] for h in halves], 1))
            assert SR.same(again, whole), (k, p is None)


# ------------------------------------------------------------------ the C ABI
def test_the_symbols_are_declared_and_exported():
    lib = L.load()
    for name in ("trid_index_merge_lists_f32", "trid_index_merge_max_candidates"):
        assert name in L.EXPORTS and hasattr(lib, name)
    assert L.DECLS["trid_index_merge_lists_f32"] == ("int", "ppppiiiipppp")
    assert L.DECLS["trid_index_merge_max_candidates"] == ("int", "")
    assert lib.trid_index_merge_max_candidates() == 8192
    assert "trid_index_merge_lists_f32(" in open(L.HEADER_PATH).read()


FAKE = 0x10000  # a 16-byte aligned non-null address: every limit is checked before anything is dereferenced or launched


def _merge(val=FAKE, row=FAKE, base=FAKE, pid=FAKE, Q=4, S=4, kin=16, k=10, out_val=FAKE, out_row=FAKE, out_pid=FAKE):
    L.call("trid_index_merge_lists_f32", val, row, base, pid, Q, S, kin, k, out_val, out_row, out_pid, None)


@pytest.mark.parametrize("kw,word", [
    (dict(val=None), "null"),
    (dict(row=None), "null"),
    (dict(out_val=None), "null"),
    (dict(out_row=None), "null"),
    (dict(out_pid=None), "null"),
    (dict(k=0), "k must be in \\[1,1024\\]"),
    (dict(k=1025, S=8, kin=1024), "k must be in \\[1,1024\\]"),
    (dict(S=8193, kin=1), "8192 candidates"),
    (dict(S=1, kin=8193), "8192 candidates"),
    (dict(S=8, kin=1025), "8192 candidates"),
    (dict(S=1 << 20, kin=1 << 20), "8192 candidates"),
    (dict(S=0), "n_lists and k_in must be >= 1"),
    (dict(kin=0), "n_lists and k_in must be >= 1"),
    (dict(S=2, kin=4, k=9), "k must be <= n_lists \\* k_in = 8"),
    (dict(Q=0), "Q must be in"),
    (dict(Q=-1), "Q must be in"),
    (dict(Q=1 << 22), "Q must be in"),
    (dict(val=FAKE + 2), "aligned"),
    (dict(row=FAKE + 4), "aligned"),
    (dict(base=FAKE + 4), "aligned"),
    (dict(pid=FAKE + 4), "aligned"),
    (dict(out_val=FAKE + 2), "aligned"),
    (dict(out_row=FAKE + 4), "aligned"),
    (dict(out_pid=FAKE + 4), "aligned"),
])
def test_merge_bad_arguments_are_errors_that_name_the_function(kw, word):
    with pytest.raises(RuntimeError, match="trid_index_merge_lists_f32") as e:
        _merge(**kw)
    assert re.search(word, str(e.value)), str(e.value)
    assert L.last_error().startswith("trid_index_merge_lists_f32:")
    # the process survives and the library still answers
    assert L.load().trid_index_merge_max_candidates() == 8192


# ------------------------------------------------------------------ host rules of GalleryShards
def test_shard_rows_out_of_range():
    from textreid_amd import GalleryShards
    from textreid_amd import index_shards as IS
    from textreid_amd.index import MAX_ROWS

    assert IS.SHARD_STRIDE == 1 << 21 and MAX_ROWS < IS.SHARD_STRIDE
    for bad in (0, -1, MAX_ROWS + 1, 2.5):
        with pytest.raises(ValueError, match="GalleryShards: shard_rows must be in \\[1, %d\\]" % MAX_ROWS):
            GalleryShards(shard_rows=bad)
    g = GalleryShards(shard_rows=96)
    assert g.shard_rows == 96 and g.n_shards == 1 and len(g) == 0 and g.live_count == 0 and len(g.parts) == 1
    assert GalleryShards().shard_rows == MAX_ROWS
    assert GalleryShards(collective=True).n_shards == 1  # (no process group: the one-shard case)


@pytest.mark.parametrize("name,max_k", [("search", 16), ("search_pids", 16), ("shortlist", 1024), ("shortlist_pids", 1024)])
def test_search_rules_hold_without_a_device(name, max_k):
    from textreid_amd import GalleryShards

    q = torch.zeros(1, 256)
    for g in (GalleryShards(shard_rows=96), GalleryShards(collective=True)):
        fn = getattr(g, name)
        for k in (0, -1, max_k + 1):
            with pytest.raises(ValueError, match="GalleryShards.%s: k must be in \\[1, %d\\]" % (name, max_k)):
                fn(q, k=k)
        with pytest.raises(ValueError, match="GalleryShards.%s: expected a \\[Q, 256\\]" % name):
            fn(torch.zeros(1, 128), k=1)
        with pytest.raises(ValueError, match="GalleryShards.%s: no queries" % name):
            fn(torch.zeros(0, 256), k=1)
        with pytest.raises(ValueError, match="GalleryShards.%s: the mask of shard 0 must be a bool or uint8" % name):
            fn(q, k=1, mask=torch.zeros(0) if g.collective else [torch.zeros(0)])
        with pytest.raises(ValueError, match="GalleryShards.%s: the mask of shard 0 must have shape \\[0\\]" % name):
            fn(q, k=1, mask=torch.ones(3, dtype=torch.bool) if g.collective else [torch.ones(3, dtype=torch.bool)])
        for k in (1, max_k):
            with pytest.raises(RuntimeError, match="GalleryShards.%s runs on the HIP kernel library only.*no CPU fallback" % name):
                fn(torch.zeros(2, 256), k=k)
    g = GalleryShards(shard_rows=96)
    for bad in ([], [None, None], (None, None, None), torch.ones(0, dtype=torch.bool)):
        with pytest.raises(ValueError, match="GalleryShards.%s: mask must be a sequence of n_shards = 1" % name):
            getattr(g, name)(q, k=1, mask=bad)
    if name.endswith("pids"):
        g._has_pids = False
        with pytest.raises(ValueError, match="GalleryShards.%s: the shards hold no pids" % name):
            getattr(g, name)(q, k=1)


def test_add_and_remove_rules_hold_without_a_device():
    from textreid_amd import GalleryShards

    g = GalleryShards(shard_rows=96)
    with pytest.raises(ValueError, match="GalleryShards.add: expected a \\[n, 256\\]"):
        g.add(torch.zeros(3, 128))
    with pytest.raises(ValueError, match="GalleryShards.add: 2 pids for 3 rows"):
        g.add(torch.zeros(3, 256), pids=[1, 2])
    with pytest.raises(RuntimeError, match="GalleryShards.add runs on the HIP kernel library only.*no CPU fallback"):
        g.add(torch.zeros(3, 256))
    with pytest.raises(ValueError, match="GalleryShards.remove: give exactly one of rows and pids"):
        g.remove()
    with pytest.raises(ValueError, match="GalleryShards.remove: give exactly one of rows and pids"):
        g.remove(rows=[1], pids=[1])
    with pytest.raises(ValueError, match="GalleryShards.remove\\(rows=...\\): a list or an int64 tensor"):
        g.remove(rows=torch.zeros(2, dtype=torch.int32))
    with pytest.raises(ValueError, match="GalleryShards.remove\\(rows=...\\): rows must be >= 0"):
        g.remove(rows=[-1])
    with pytest.raises(ValueError, match="GalleryShards.remove\\(rows=...\\): row %d lies in shard 1 of 1" % (1 << 21)):
        g.remove(rows=[1 << 21])
    with pytest.raises(ValueError, match="GalleryShards.remove\\(rows=...\\): shard 0 holds 0 rows"):
        g.remove(rows=[5])
    with pytest.raises(ValueError, match="GalleryShards.remove\\(pids=...\\): the shards hold no pids"):
        g.remove(pids=[5])
    assert g.remove(rows=[]) == 0


def test_locate_round_trips():
    from textreid_amd import GalleryShards
    from textreid_amd.index_shards import SHARD_STRIDE

    shard = torch.tensor([0, 0, 1, 5, 1000, 3])
    local = torch.tensor([0, SHARD_STRIDE - 2, 0, 17, SHARD_STRIDE - 2, 95])
    rows = shard * SHARD_STRIDE + local
    assert rows.dtype == torch.int64
    s, r = GalleryShards.locate(rows)
    assert s.dtype == torch.int64 and r.dtype == torch.int64 and torch.equal(s, shard) and torch.equal(r, local)
    s, r = GalleryShards.locate(torch.tensor([[-1, 5], [SHARD_STRIDE + 1, -1]]))
    assert s.tolist() == [[-1, 0], [1, -1]] and r.tolist() == [[-1, 5], [1, -1]]
    s, r = GalleryShards.locate([3 * SHARD_STRIDE + 4, -1])
    assert s.tolist() == [3, -1] and r.tolist() == [4, -1]


def test_state_dict_of_an_empty_object_round_trips():
    from textreid_amd import GalleryShards

    g = GalleryShards(shard_rows=96)
    sd = g.state_dict()
    assert sd["shard_rows"] == 96 and sd["collective"] is False and len(sd["parts"]) == 1
    h = GalleryShards()
    h.load_state_dict(sd)
    assert h.shard_rows == 96 and len(h) == 0 and h.n_shards == 1
    with pytest.raises(ValueError, match="GalleryShards.load_state_dict: the by-rank form holds one part per rank"):
        GalleryShards(collective=True).load_state_dict({"shard_rows": 96, "parts": [sd["parts"][0], sd["parts"][0]]})
