"""Deep top-k without a device: the numpy reference against brute force, the C ABI of trid_topk_rows_deep_f32 (exports, workspace
sizes, argument errors - every limit is checked before anything is dereferenced or launched) and the argument rules of
GalleryIndex.shortlist."""

import re

import numpy as np
import pytest
import torch

import topk_deep_ref as TR
from textreid_amd import GalleryIndex
from textreid_amd import index as IX
from textreid_amd import lib as L


# ------------------------------------------------------------------ the reference
def brute(sim, k, allowed, offset):
    """selection by repeated scan: the best remaining (value, column) by float comparison, ties to the lower column"""
    Q, G = sim.shape
    vals = np.full((Q, k), -np.inf, dtype=np.float32)
    idx = np.full((Q, k), -1, dtype=np.int64)
    for q in range(Q):
        left = [g for g in range(G) if allowed is None or allowed[g]]
        for t in range(k):
            if not left:
                break
            best = left[0]
            for g in left[1:]:
                if sim[q, g] > sim[q, best]:  # (strict: an equal value at a higher column never replaces; +0 == -0)
                    best = g
            left.remove(best)
            vals[q, t] = sim[q, best]
            idx[q, t] = best + offset
    return vals, idx


def tie_matrix(Q, G, seed):
    rng = np.random.RandomState(seed)
    pool = np.array([0.0, -0.0, 1.0, -1.0, 0.5, -np.inf, 2.0], dtype=np.float32)
    return pool[rng.randint(0, pool.size, size=(Q, G))]


@pytest.mark.parametrize("G,k", [(1, 1), (7, 3), (40, 8), (40, 40), (33, 17)])
def test_reference_equals_brute_force_with_ties_zeros_and_inf(G, k):
    sim = tie_matrix(4, G, 3 + G)
    assert (np.signbit(sim) & (sim == 0)).any() or G < 7
    for offset in (0, 1000):
        assert TR.same(TR.topk(sim, k, None, offset), brute(sim, k, None, offset))


@pytest.mark.parametrize("left", ["0", "k-1", "k", "k+1"])
def test_reference_masks_that_leave_few_columns(left):
    G, k = 37, 6
    n = {"0": 0, "k-1": k - 1, "k": k, "k+1": k + 1}[left]
    sim = tie_matrix(3, G, 11)
    allowed = np.zeros(G, dtype=bool)
    allowed[np.random.RandomState(n).permutation(G)[:n]] = True
    got = TR.topk(sim, k, allowed, 5)
    assert TR.same(got, brute(sim, k, allowed, 5))
    assert (got[1][:, n:] == -1).all() and np.isneginf(got[0][:, n:]).all()
    if n:
        assert (got[1][:, : min(n, k)] >= 5).all()


def test_reference_returns_the_original_zero_bits():
    sim = np.array([[-0.0, 0.0, -0.0, -1.0]], dtype=np.float32)
    vals, idx = TR.topk(sim, 3)
    assert idx.tolist() == [[0, 1, 2]]
    assert np.signbit(vals).tolist() == [[True, False, True]]


# ------------------------------------------------------------------ the C ABI
def test_symbols_are_exported_and_the_default_chunk_is_a_power_of_two():
    lib = L.load()
    for name in ("trid_topk_rows_deep_chunk", "trid_topk_rows_deep_ws_bytes", "trid_topk_rows_deep_f32"):
        assert name in L.EXPORTS and hasattr(lib, name)
    for k in (1, 512, 1024):
        c = lib.trid_topk_rows_deep_chunk(k)
        assert c >= 64 and c & (c - 1) == 0 and c >= 2 * k
    assert lib.trid_topk_rows_deep_chunk(512) == 8192 and lib.trid_topk_rows_deep_chunk(1024) == 2048
    assert lib.trid_topk_rows_deep_chunk(0) == 0 and lib.trid_topk_rows_deep_chunk(1025) == 0


def test_ws_bytes():
    ws = L.load().trid_topk_rows_deep_ws_bytes
    for args in ((1, 1, 1, 0), (33, 17, 17, 0), (5, 1000000, 100, 0), (1, 1024, 1024, 0), (3, 3000, 100, 256), (3, 5000, 17, 64)):
        assert ws(*args) > 0, args
    for args in ((0, 10, 1, 0), (1, 0, 1, 0), (1, 10, 0, 0), (1, 2000, 1025, 0), (1, 10, 11, 0), (1, 100, 10, 48), (1, 100, 10, 16384),
                 (1, 5000, 100, 128), (1, 100, 10, -64)):
        assert ws(*args) == 0, args
    for chunk, k in ((0, 100), (256, 100), (64, 17), (0, 1024)):
        by_q = [ws(q, 20000, k, chunk) for q in (1, 2, 5, 32, 33, 1000)]
        assert all(a <= b for a, b in zip(by_q, by_q[1:])), by_q
        by_g = [ws(5, g, k, chunk) for g in (1024, 2047, 2048, 2049, 8192, 8193, 20000, 100000, 1000000)]
        assert all(a <= b for a, b in zip(by_g, by_g[1:])), by_g
    # the staged lists: ceil(G / chunk) lists of k pairs per query after level 1, ceil(that / (chunk / k)) after the first merge
    assert ws(3, 3000, 100, 256) == 3 * (12 + 6) * 100 * 8
    assert ws(1 << 20, 1 << 30, 1, 64) == 0  # (more workgroups than the grid holds)
    # one launch of Q * ceil(G / chunk) workgroups of 256 threads, fewer than 2^32 threads in all
    assert ws((1 << 24) - 1, 10, 1, 0) > 0 and ws(1 << 24, 10, 1, 0) == 0 and ws(1 << 23, 8193, 1, 0) == 0


FAKE = 0x10000  # a 16-byte aligned non-null address: every limit is checked before anything is dereferenced or launched


def _deep(sim=FAKE, ld_q=100, ld_g=1, Q=4, G=100, k=10, mask=None, off=0, val=FAKE, idx=FAKE, ws=FAKE, ws_bytes=None, chunk=0):
    if ws_bytes is None:
        ws_bytes = 1 << 40
    L.call("trid_topk_rows_deep_f32", sim, ld_q, ld_g, Q, G, k, mask, off, val, idx, ws, ws_bytes, chunk, None)


@pytest.mark.parametrize("kw,word", [
    (dict(sim=None, val=None, idx=None, ws=None), "null"),
    (dict(sim=None), "null"),
    (dict(val=None), "null"),
    (dict(idx=None), "null"),
    (dict(ws=None), "null"),
    (dict(k=0), "k must be"),
    (dict(k=1025, G=2000, ld_q=2000), "k must be"),
    (dict(k=11, G=10), "k must be"),
    (dict(Q=0), "Q"),
    (dict(chunk=48), "chunk"),
    (dict(k=100, chunk=128), "chunk"),   # (a power of two below max(64, 2 * next_pow2(k)) = 256)
    (dict(k=1024, G=4000, ld_q=4000, chunk=1024), "chunk"),
    (dict(chunk=16384), "chunk"),
    (dict(Q=1 << 24, ld_q=1, ld_g=1 << 24), "grid"),
    (dict(ld_q=99), "alias"),
    (dict(ld_q=1, ld_g=3), "alias"),
    (dict(ld_q=0), "alias"),
    (dict(G=20000, ld_q=20000, k=100, ws_bytes=L.load().trid_topk_rows_deep_ws_bytes(4, 20000, 100, 0) - 1), "ws_bytes"),
    (dict(G=3000, ld_q=3000, k=100, chunk=256, ws_bytes=L.load().trid_topk_rows_deep_ws_bytes(4, 3000, 100, 256) - 1), "ws_bytes"),
])
def test_bad_arguments_are_errors_that_name_the_function(kw, word):
    with pytest.raises(RuntimeError, match="trid_topk_rows_deep_f32") as e:
        _deep(**kw)
    assert re.search(word, str(e.value)), str(e.value)
    # the process survives and the library still answers
    assert L.load().trid_topk_rows_deep_ws_bytes(4, 100, 10, 0) > 0


# ------------------------------------------------------------------ GalleryIndex.shortlist without a device
def test_shortlist_limit_is_1024_and_search_stays_at_16():
    assert IX.MAX_SHORTLIST_K == 1024 and IX.MAX_K == 16


def test_shortlist_k_range():
    idx = GalleryIndex()
    idx._n = 5000  # (rows held: the k rule is checked before anything touches the storage)
    for k in (0, -1, 1025):
        with pytest.raises(ValueError, match="shortlist: k must be"):
            idx.shortlist(torch.zeros(1, 256), k=k)
    idx._n = 50
    with pytest.raises(ValueError, match="shortlist: k must be"):
        idx.shortlist(torch.zeros(1, 256), k=51)
    with pytest.raises(ValueError, match="shortlist: k must be"):
        idx.shortlist(torch.zeros(1, 256))  # (the default k = 100 > len)
    idx._dead = 10
    with pytest.raises(ValueError, match="shortlist: k must be <= live_count"):
        idx.shortlist(torch.zeros(1, 256), k=41)


def test_shortlist_on_an_empty_index_and_bad_queries():
    idx = GalleryIndex()
    with pytest.raises(ValueError, match="shortlist: the index is empty"):
        idx.shortlist(torch.zeros(1, 256), k=1)
    idx._n = 40
    with pytest.raises(ValueError, match="shortlist: expected"):
        idx.shortlist(torch.zeros(1, 128), k=1)
    with pytest.raises(ValueError, match="shortlist: no queries"):
        idx.shortlist(torch.zeros(0, 256), k=1)


def test_shortlist_refuses_cpu_tensors():
    idx = GalleryIndex()
    idx._n = 40
    for k in (1, 17, 40):
        with pytest.raises(RuntimeError, match="shortlist runs on the HIP kernel library only.*no CPU fallback"):
            idx.shortlist(torch.zeros(2, 256), k=k)


def test_shortlist_mask_rules():
    idx = GalleryIndex()
    idx._n = 40
    with pytest.raises(ValueError, match="shortlist: mask must have shape"):
        idx.shortlist(torch.zeros(1, 256), k=20, mask=torch.ones(39, dtype=torch.bool))
    with pytest.raises(ValueError, match="shortlist: mask must have shape"):
        idx.shortlist(torch.zeros(1, 256), k=20, mask=torch.ones(40, 1, dtype=torch.bool))
    with pytest.raises(ValueError, match="shortlist: mask must be a bool or uint8"):
        idx.shortlist(torch.zeros(1, 256), k=20, mask=torch.ones(40, dtype=torch.float32))
    with pytest.raises(ValueError, match="shortlist: mask must be a bool or uint8"):
        idx.shortlist(torch.zeros(1, 256), k=20, mask=[True] * 40)


def test_topk_rows_and_rank_refuse_cpu_tensors():
    from textreid_amd import evaluation as E

    with pytest.raises(RuntimeError, match="no CPU fallback"):
        E.topk_rows(torch.zeros(2, 50), 20)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        E.rank(torch.zeros(2, 50), torch.zeros(2), torch.zeros(50), topk=(1, 20), get_mAP=False)
