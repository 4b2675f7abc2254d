"""Neighbour graph and re-ranked search without a device: the numpy reference against a brute-force loop over Python sets and against
the pinned oracle (oracle.evaluation.k_reciprocal), the C ABI of trid_index_rerank_add_f32 (declared, exported, every argument
error reported before anything is dereferenced or launched) and the host rules of GalleryIndex.build_neighbours /
search_reranked / state_dict."""

import re

import numpy as np
import pytest
import torch

import gallery_rerank_ref as RR
import oracle.evaluation as OE
import oracle.fill as OF
import topk_deep_ref as TR
from textreid_amd import GalleryIndex
from textreid_amd import index as IX
from textreid_amd import lib as L

SEED = 13


# ------------------------------------------------------------------ the reference
def test_counts_equal_a_loop_over_sets_with_absent_slots():
    rng = np.random.RandomState(4)
    G, Q, n = 60, 7, 5
    gnn = np.stack([rng.permutation(G)[:n] for _ in range(G)]).astype(np.int32)
    gnn[3] = -1                      # a removed row
    gnn[9, 2:] = -1
    qnn = np.stack([rng.permutation(G)[:n] for _ in range(Q)]).astype(np.int64)
    qnn[0] = gnn[5]                  # c == n
    qnn[1, :3] = gnn[6, 2:][::-1]    # c >= 3, other positions
    qnn[2, 3:] = -1                  # nq == 3
    qnn[3] = -1                      # nq == 0
    got = RR.counts(qnn, gnn)
    want = np.zeros((Q, G), dtype=np.int64)
    for q in range(Q):
        a = {int(v) for v in qnn[q] if v >= 0}
        for g in range(G):
            want[q, g] = len(a & {int(v) for v in gnn[g] if v >= 0})
    assert np.array_equal(got, want)
    assert got[0, 5] == n and got[1, 6] >= 3 and (got[3] == 0).all() and (got[:, 3] == 0).all()


def test_bonus_is_float32_step_by_step_and_the_jaccard_term_at_full_lists():
    n, alpha = 5, 0.05
    for nq in range(1, n + 1):
        for c in range(1, nq + 1):
            want = np.float32(np.float32(alpha) * np.float32(c)) / np.float32(nq + n - c)
            got = RR.bonus(nq, c, n, alpha)
            assert got.dtype == np.float32 and TR.bits(got) == TR.bits(np.float32(want))
    # nq == n: alpha * c / (2 n - c), the expression of trid_jaccard_add_f32
    c = np.arange(1, n + 1)
    assert np.array_equal(TR.bits(RR.bonus(np.full(n, n), c, n, alpha)), TR.bits((np.float32(alpha) * c.astype(np.float32)) / (2 * n - c).astype(np.float32)))


def test_counts_equal_the_pinned_oracle():
    Q, G, n, alpha = 9, 200, 5, 0.05
    q = torch.nn.functional.normalize(OF.randn("grr:oq", (Q, 256), SEED), dim=1)
    g = torch.nn.functional.normalize(OF.randn("grr:og", (G, 256), SEED), dim=1)
    qg, gg = (q @ g.t()).numpy(), (g @ g.t()).numpy()
    for s in (qg, gg):  # tie-free: the order does not hang on a tie rule
        top = np.sort(s, axis=1)[:, ::-1][:, : n + 1]
        assert (np.diff(top, axis=1) < 0).all()
    J = OE.k_reciprocal(q, g, neighbor_num=n, alpha=alpha).numpy() / alpha
    c_oracle = np.rint(2 * n * J / (1 + J)).astype(np.int64)
    qnn = TR.topk(qg, n)[1]
    gnn = RR.graph(gg, n)
    c = RR.counts(qnn, gnn)
    assert np.array_equal(c, c_oracle)
    assert c.max() >= 1
    # ... and the bonus is the oracle's term to float32 rounding
    b = RR.rerank_scores(np.zeros((Q, G), dtype=np.float32), qnn, gnn, n, alpha)
    assert np.abs(b - alpha * J).max() < 1e-8


def test_reranked_topk_moves_a_boosted_row_and_respects_the_allow_set():
    # four rows; row 3 shares the query's whole list, row 0 is the plain winner by less than the bonus
    sim = np.array([[0.50, 0.30, 0.20, 0.49]], dtype=np.float32)
    gnn = np.array([[0, 2], [1, 2], [2, 1], [0, 3]], dtype=np.int32)  # n = 2; the query's list is [0, 3]
    vals, rows = RR.reranked_topk(sim, gnn, 2, 0.05, 4)
    assert rows.tolist() == [[3, 0, 1, 2]]
    assert TR.bits(vals[0, 0]) == TR.bits(np.float32(0.49) + np.float32(np.float32(0.05) * np.float32(2)) / np.float32(2))
    # row 0 disallowed: the query's list becomes [3, 1]
    allow = np.array([False, True, True, True])
    vals, rows = RR.reranked_topk(sim, gnn, 2, 0.05, 4, allow)
    assert rows.tolist() == [[3, 1, 2, -1]] and np.isneginf(vals[0, 3])


# ------------------------------------------------------------------ the C ABI
def test_the_symbol_is_declared_and_exported():
    lib = L.load()
    assert "trid_index_rerank_add_f32" in L.EXPORTS and hasattr(lib, "trid_index_rerank_add_f32")
    assert L.DECLS["trid_index_rerank_add_f32"] == ("int", "plliippifpp")


FAKE = 0x10000  # a 16-byte aligned non-null address: every limit is checked before anything is dereferenced or launched


def _rerank(scores=FAKE, ld_q=100, ld_g=1, Q=4, G=100, qnn=FAKE, gnn=FAKE, n=5, alpha=0.05, mask=None):
    L.call("trid_index_rerank_add_f32", scores, ld_q, ld_g, Q, G, qnn, gnn, n, alpha, mask, None)


@pytest.mark.parametrize("kw,word", [
    (dict(scores=None, qnn=None, gnn=None), "null"),
    (dict(scores=None), "null"),
    (dict(qnn=None), "null"),
    (dict(gnn=None), "null"),
    (dict(Q=0), "Q and G"),
    (dict(G=0), "Q and G"),
    (dict(n=0), "n must be"),
    (dict(n=9), "n must be"),
    (dict(n=5, G=3, ld_q=3), "n must be"),
    (dict(ld_q=99), "alias"),
    (dict(ld_q=1, ld_g=3), "alias"),
    (dict(ld_q=0), "alias"),
    (dict(ld_g=0), "alias"),
    (dict(scores=FAKE + 2), "aligned"),
    (dict(gnn=FAKE + 2), "aligned"),
    (dict(qnn=FAKE + 4), "aligned"),
    (dict(mask=FAKE + 1), "aligned"),
    (dict(Q=32 * 65535 + 1, ld_q=1, ld_g=1 << 22), "groups"),
])
def test_bad_arguments_are_errors_that_name_the_function(kw, word):
    with pytest.raises(RuntimeError, match="trid_index_rerank_add_f32") as e:
        _rerank(**kw)
    assert re.search(word, str(e.value)), str(e.value)
    assert L.last_error().startswith("trid_index_rerank_add_f32:")
    # the process survives and the library still answers
    assert L.load().trid_topk_rows_deep_ws_bytes(4, 100, 10, 0) > 0


# ------------------------------------------------------------------ host rules of the index
def test_build_neighbours_argument_rules():
    assert IX.MAX_NEIGHBOURS == 8
    idx = GalleryIndex()
    idx._n = 40  # (rows held: the rules are checked before anything touches the storage)
    for n in (0, -1, 9):
        with pytest.raises(ValueError, match="build_neighbours: n must be in"):
            idx.build_neighbours(n)
    idx._dead = 37
    with pytest.raises(ValueError, match="build_neighbours: n must be <= live_count"):
        idx.build_neighbours(5)
    with pytest.raises(ValueError, match="build_neighbours: the index is empty"):
        GalleryIndex().build_neighbours()


def test_search_reranked_needs_a_graph_after_the_argument_rules_and_before_the_device():
    idx = GalleryIndex()
    with pytest.raises(ValueError, match="search_reranked: the index is empty"):
        idx.search_reranked(torch.zeros(1, 256), k=1)
    idx._n = 5000
    assert idx.neighbours is None and not idx.neighbours_current
    with pytest.raises(RuntimeError, match="search_reranked: .*build_neighbours"):
        idx.search_reranked(torch.zeros(1, 256), k=10)
    for k in (0, 1025):
        with pytest.raises(ValueError, match="search_reranked: k must be"):
            idx.search_reranked(torch.zeros(1, 256), k=k)
    with pytest.raises(ValueError, match="search_reranked: expected"):
        idx.search_reranked(torch.zeros(1, 128), k=1)
    with pytest.raises(ValueError, match="search_reranked: no queries"):
        idx.search_reranked(torch.zeros(0, 256), k=1)
    with pytest.raises(ValueError, match="search_reranked: mask must have shape"):
        idx.search_reranked(torch.zeros(1, 256), k=1, mask=torch.ones(7, dtype=torch.bool))
    idx._dead = 4995
    with pytest.raises(ValueError, match="search_reranked: k must be <= live_count"):
        idx.search_reranked(torch.zeros(1, 256), k=6)
    # a stale graph is named as such; a current one lets the call reach the device rule
    idx._dead = 0
    idx._nn, idx._nn_ok = torch.zeros(5000, 5, dtype=torch.int32), False
    with pytest.raises(RuntimeError, match="stale.*build_neighbours"):
        idx.search_reranked(torch.zeros(1, 256), k=10)
    idx._nn_ok = True
    assert idx.neighbours_current and tuple(idx.neighbours.shape) == (5000, 5)
    with pytest.raises(RuntimeError, match="search_reranked runs on the HIP kernel library only.*no CPU fallback"):
        idx.search_reranked(torch.zeros(1, 256), k=10)
    # the other entry points do not ask for a graph
    idx._nn = None
    with pytest.raises(RuntimeError, match="shortlist runs on the HIP kernel library only"):
        idx.shortlist(torch.zeros(1, 256), k=10)


def test_state_dict_key_of_an_empty_index():
    sd = GalleryIndex().state_dict()
    assert "neighbours" in sd and sd["neighbours"] is None


@pytest.mark.parametrize("nn,word", [
    (torch.zeros(6, 5, dtype=torch.int32), "int32 \\[7, n\\]"),            # one list per row
    (torch.zeros(7, 9, dtype=torch.int32), "1 <= n <= 8"),
    (torch.zeros(7, 0, dtype=torch.int32), "1 <= n <= 8"),
    (torch.zeros(35, dtype=torch.int32), "int32 \\[7, n\\]"),
    (torch.zeros(7, 5, dtype=torch.int64), "int32"),
    ([[0] * 5] * 7, "int32"),
    (torch.full((7, 5), 7, dtype=torch.int32), "rows in \\[-1, 7\\); got 7"),
    (torch.full((7, 5), -2, dtype=torch.int32), "rows in \\[-1, 7\\); got -2"),
])
def test_load_state_dict_refuses_bad_lists(nn, word):
    idx = GalleryIndex()
    with pytest.raises(ValueError, match="load_state_dict: neighbours must") as e:
        idx.load_state_dict({"rows": torch.zeros(7, 256), "pids": None, "neighbours": nn})
    assert re.search(word, str(e.value)), str(e.value)
    assert len(idx) == 0 and idx.neighbours is None
    # well-formed lists pass the list rules: the next rule is the device's
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        idx.load_state_dict({"rows": torch.zeros(7, 256), "pids": None, "neighbours": torch.full((7, 5), -1, dtype=torch.int32)})
