"""The deep distinct select on the GPU: trid_index_group_best_f32 and trid_topk_rows_deep_pairs_f32 through the raw entries and
evaluation.topk_distinct_rows (matrices with heavy ties, every layout, masks with garbage tail bits, whole output buffers compared
bitwise so that nothing outside the extents moves), GalleryIndex.shortlist_pids against the dense trid_gemm_p16 product of the
index's OWN operands followed by gallery_deep_distinct_ref, and search_reranked_pids against gallery_rerank_ref.rerank_scores plus the
same reference.  Nothing here needs a tolerance: values are compared as bit patterns, rows and pids exactly."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import gallery_deep_distinct_ref as DR  # noqa: E402
import gallery_rerank_ref as RR  # noqa: E402
import oracle.fill as OF  # noqa: E402
import topk_deep_ref as TR  # noqa: E402
from gallery_support import dense_product, fresh_index, gpu, Inputs, same_bits as same, unit_rows, words_tensor  # noqa: E402,F401

SEED = 14
ABSENT = DR.ABSENT
IN = Inputs("gdd:", SEED)
coin, gallery, queries = IN.coin_one_in, IN.gallery, IN.queries


def same3(got, want, pids, what=""):
    """(values, rows, pids) of the index against the reference's (values, rows): pids follow from the rows"""
    same(got[:2], want, what)
    rows = np.asarray(want[1])
    want_pids = np.where(rows >= 0, np.asarray(pids)[np.maximum(rows, 0)], -1)
    assert got[2].dtype == torch.int64 and np.array_equal(got[2].cpu().numpy(), want_pids), what


def level_matrix(Q, G, levels, seed, specials=True):
    rng = np.random.RandomState(seed)
    pool = np.linspace(-1.0, 1.0, levels).astype(np.float32)
    if specials:
        pool = np.concatenate([pool, np.array([0.0, -0.0, -np.inf], dtype=np.float32)])
    return pool[rng.randint(0, pool.size, size=(Q, G))]


def pattern_buffer(size):
    return (0x5A5A0000 + (np.arange(size) & 0xFFFF)).astype(np.uint32).view(np.float32).copy()


def place(sim, layout, wide=0):
    """sim [Q, G] -> (flat host buffer holding it, ld_q, ld_g): 'rows' = row-major with ld_q = G + 3 > G, 'cols' = the [G, wide]
    product layout (ld_q = 1, ld_g = wide >= Q); a recognisable pattern everywhere else"""
    Q, G = sim.shape
    if layout == "cols":
        assert wide >= Q
        ld_q, ld_g, size = 1, wide, (G + 2) * wide
    else:
        ld_q, ld_g, size = G + 3, 1, Q * (G + 3) + 5
    at = np.arange(Q)[:, None] * ld_q + np.arange(G)[None, :] * ld_g
    buf = pattern_buffer(size)
    buf[at] = sim
    return buf, ld_q, ld_g


def run_group_best(gpu, sim, order, starts, n_groups, n_slots, layout, allowed=None, out_layout="slots"):
    """the raw entry -> (values [Q, n_slots], rows [Q, n_slots]) read from output buffers whose every other word is checked to be
    untouched"""
    from textreid_amd import ops
    from textreid_amd.ops import _p

    Q, G = sim.shape
    wide = 32 if Q <= 32 else 64
    buf, ld_q, ld_g = place(sim, layout, wide)
    if out_layout == "slots":  # the index's [n_slots, 32] form
        o_q, o_g, size = 1, wide, (n_slots + 1) * wide
    else:
        o_q, o_g, size = n_slots + 2, 1, Q * (n_slots + 2) + 3
    at = np.arange(Q)[:, None] * o_q + np.arange(n_slots)[None, :] * o_g
    ov, orow = pattern_buffer(size), pattern_buffer(size).view(np.int32).copy()
    dv, dr = torch.from_numpy(ov).to(gpu), torch.from_numpy(orow).to(gpu)
    dev = torch.from_numpy(buf).to(gpu)
    d_order, d_starts = torch.from_numpy(np.asarray(order, dtype=np.int32)).to(gpu), torch.from_numpy(np.asarray(starts, dtype=np.int32)).to(gpu)
    words = None if allowed is None else words_tensor(allowed, gpu, garbage=True, seed=G)
    ops.call("trid_index_group_best_f32", _p(dev), ld_q, ld_g, Q, G, _p(d_order), _p(d_starts), n_groups, n_slots, _p(words), _p(dv), _p(dr),
             o_q, o_g, ops.stream())
    gv, gr = dv.cpu().numpy(), dr.cpu().numpy()
    assert np.array_equal(dev.cpu().numpy().view(np.uint32), buf.view(np.uint32))  # (the scores are read only)
    keep = np.ones(size, dtype=bool)
    keep[at] = False
    assert np.array_equal(gv.view(np.uint32)[keep], ov.view(np.uint32)[keep]) and np.array_equal(gr[keep], orow[keep]), "a word outside the extent moved"
    return gv[at], gr[at]


def run_pairs(gpu, val, col, k, layout="rows", offset=0, chunk=0):
    from textreid_amd import lib as L
    from textreid_amd.ops import _p, stream

    Q, S = val.shape
    wide = 32 if Q <= 32 else 64
    bv, ld_q, ld_g = place(val, layout, wide)
    bc = place(np.asarray(col, dtype=np.int32).view(np.float32), layout, wide)[0].view(np.int32)
    dv, dc = torch.from_numpy(bv).to(gpu), torch.from_numpy(bc.copy()).to(gpu)
    nws = L.load().trid_topk_rows_deep_ws_bytes(Q, S, k, chunk)
    assert nws > 0, (Q, S, k, chunk)
    ws = torch.empty(nws, dtype=torch.uint8, device=gpu)
    vals = torch.empty(Q, k, dtype=torch.float32, device=gpu)
    idx = torch.empty(Q, k, dtype=torch.int64, device=gpu)
    L.call("trid_topk_rows_deep_pairs_f32", _p(dv), _p(dc), ld_q, ld_g, Q, S, k, offset, _p(vals), _p(idx), _p(ws), nws, chunk, stream())
    return vals, idx


def group_patterns(G, k, seed):
    rng = np.random.RandomState(seed)
    sizes = np.repeat(np.arange(6), [1, 2, 3, 64, 65, 130])  # groups of 1 / 2 / 3 / 64 / 65 / 130 rows ...
    sized = np.concatenate([sizes, 6 + np.arange(max(G - sizes.size, 0)) // 5])[:G]
    straddle = np.arange(G) // 2 + 100
    straddle[max(G - 1, 0) if G < 33 else 29 : 35] = 7  # (... and one group that straddles rows 31 | 32)
    pats = {"distinct": np.arange(G), "one": np.zeros(G, dtype=np.int64), "quads": np.arange(G) // 4, "random": rng.randint(0, max(G // 3, 1), size=G),
            "sizes": sized[rng.permutation(G)] if G > 300 else sized, "straddle": straddle}
    for P in (k - 1, k, k + 1):
        pats["mod%d" % P] = np.arange(G) % P
    return pats


# ------------------------------------------------------------------------------------------------------------------ the two kernels
@pytest.mark.parametrize("G", [1, 31, 33, 65, 300, 2000])
def test_group_best_and_the_composition_on_tied_matrices(gpu, G):
    from textreid_amd import evaluation as E

    k = 17
    Qs = (1, 5, 32, 33, 40)
    case = 0
    for name, groups in group_patterns(G, k, G).items():
        order, starts, n_groups = DR.table(groups)
        for levels in (2, 50):
            Q = Qs[case % 5]
            layout, out_layout = ("cols", "rows")[case % 2], ("slots", "rows")[(case // 2) % 2]
            case += 1
            sim = level_matrix(Q, G, levels, 100 * G + case)
            if levels == 2 and name in ("one", "quads", "random"):
                sim[:] = np.float32(0.25)  # all-equal rows: the lowest allowed row of every group, groups by that row
            allowed = None if case % 3 == 0 else np.random.RandomState(case).rand(G) < (0.5 if case % 3 == 1 else 0.1)
            n_slots = max(n_groups, k) + (case % 2)
            want = DR.group_best(sim, order, starts, n_groups, n_slots, allowed)
            got = run_group_best(gpu, sim, order, starts, n_groups, n_slots, layout, allowed, out_layout)
            what = "G=%d %s levels=%d Q=%d %s/%s" % (G, name, levels, Q, layout, out_layout)
            assert TR.same(got, want), what
            assert (got[1][:, n_groups:] == ABSENT).all() and np.isneginf(got[0][:, n_groups:]).all(), what  # the padding slots
            dev = torch.from_numpy(sim).to(gpu)
            mask = None if allowed is None else torch.from_numpy(allowed).to(gpu)
            for kk in (1, k, min(100, G)):
                same(E.topk_distinct_rows(dev, torch.from_numpy(groups).to(gpu), kk, mask=mask), DR.pairs_topk(want[0], want[1], kk), what + " k=%d" % kk)
            if case % 4 == 0:  # a transposed view is read in place
                same(E.topk_distinct_rows(dev.t().contiguous().t(), torch.from_numpy(groups), k, mask=mask), DR.pairs_topk(want[0], want[1], k), what + " view")


def test_all_queries_on_one_random_grouping(gpu):
    G = 300
    groups = np.random.RandomState(3).randint(0, 70, size=G)
    order, starts, n_groups = DR.table(groups)
    for Q in (1, 5, 32, 33, 40):
        for layout in ("rows", "cols"):
            sim = level_matrix(Q, G, 4, Q)
            allowed = np.random.RandomState(Q).rand(G) < 0.6
            for out_layout in ("slots", "rows"):
                assert TR.same(run_group_best(gpu, sim, order, starts, n_groups, 100, layout, allowed, out_layout),
                               DR.group_best(sim, order, starts, n_groups, 100, allowed)), (Q, layout, out_layout)


def test_ties_between_groups_go_to_the_lower_representative_row(gpu):
    from textreid_amd import evaluation as E

    # A = {0, 5} with its best at row 5, B = {3}, equal values: B must win
    sim = np.array([[0.0, 9.0, 9.0, 1.0, 9.0, 1.0]], dtype=np.float32)
    groups = np.array([7, 1, 2, 8, 3, 7])
    vals, rows = E.topk_distinct_rows(torch.from_numpy(sim).to(gpu), torch.from_numpy(groups).to(gpu), 6)
    assert rows.cpu().tolist() == [[1, 2, 4, 3, 5, -1]]
    same((vals, rows), DR.distinct_topk(sim, groups, 6))


def test_zero_signs_and_a_group_of_only_minus_inf(gpu):
    from textreid_amd import evaluation as E

    sim = np.array([[-0.0, 0.0, -0.0, 0.0, -1.0, -np.inf, -np.inf]], dtype=np.float32)
    groups = np.array([0, 0, 1, 2, 2, 3, 3])
    vals, rows = E.topk_distinct_rows(torch.from_numpy(sim).to(gpu), torch.from_numpy(groups).to(gpu), 5)
    assert rows.cpu().tolist() == [[0, 2, 3, 5, -1]]
    assert np.signbit(vals.cpu().numpy()[0, :3]).tolist() == [True, True, False]
    same((vals, rows), DR.distinct_topk(sim, groups, 5))
    mask = torch.tensor([1, 1, 1, 1, 1, 0, 1], dtype=torch.uint8, device=gpu)
    assert E.topk_distinct_rows(torch.from_numpy(sim).to(gpu), torch.from_numpy(groups).to(gpu), 5, mask=mask)[1].cpu().tolist() == [[0, 2, 3, 6, -1]]


@pytest.mark.parametrize("G", [33, 300])
def test_every_mask_pattern_with_garbage_tail_bits(gpu, G):
    groups = np.arange(G) // 3
    order, starts, n_groups = DR.table(groups)
    sim = level_matrix(5, G, 4, G)
    rng = np.random.RandomState(G)
    whole = np.ones(G, dtype=bool)
    whole[groups == 4] = False  # a whole group masked out
    single = np.zeros(G, dtype=bool)
    single[G - 1] = True
    for name, allowed in (("all", np.ones(G, dtype=bool)), ("none", np.zeros(G, dtype=bool)), ("random", rng.rand(G) < 0.5), ("single", single),
                          ("whole group", whole), ("first word", np.arange(G) < 32), ("not first word", np.arange(G) >= 32)):
        got = run_group_best(gpu, sim, order, starts, n_groups, n_groups, "cols", allowed)
        assert TR.same(got, DR.group_best(sim, order, starts, n_groups, n_groups, allowed)), name
        if name == "none":
            assert (got[1] == ABSENT).all() and np.isneginf(got[0]).all()
        if name == "whole group":
            assert (got[1][:, 4] == ABSENT).all() and (got[1][:, 3] != ABSENT).all()
    assert TR.same(run_group_best(gpu, sim, order, starts, n_groups, n_groups, "cols", np.ones(G, dtype=bool)),
                   run_group_best(gpu, sim, order, starts, n_groups, n_groups, "cols", None))


def test_bad_order_entries_are_skipped_and_starts_are_clamped(gpu):
    G = 65
    sim = level_matrix(5, G, 50, 9, specials=False)
    order, starts, n = DR.table(np.arange(G) // 3)
    allowed = np.ones(G, dtype=bool)
    allowed[[4, 64]] = False
    want = DR.group_best(sim, order, starts, n, n, allowed)
    for bad_value in (-1, G, -(1 << 31), (1 << 31) - 1):
        bad = order.astype(np.int64)
        bad[[4, 64]] = bad_value  # (rows 4 and 64 sit at their own positions: the table of row // 3 is the identity)
        assert TR.same(run_group_best(gpu, sim, bad.astype(np.int32), starts, n, n, "cols"), want), bad_value
    wild = starts.copy()
    wild[0], wild[-1] = -5, 1 << 30
    assert TR.same(run_group_best(gpu, sim, order, wild, n, n, "rows"), DR.group_best(sim, order, starts, n, n))


# ------------------------------------------------------------------------------------------------------------------ the pairs select
def pair_case(Q, S, seed, present=0.8):
    rng = np.random.RandomState(seed)
    val = level_matrix(Q, S, 4, seed)
    col = np.stack([rng.permutation(3 * S + 7)[:S] for _ in range(Q)]).astype(np.int32)
    gone = rng.rand(Q, S) >= present
    col[gone] = ABSENT  # sentinel columns keep a finite value: they are absent whatever it is
    val[gone & (rng.rand(Q, S) < 0.5)] = np.float32(7.5)
    return val, col


@pytest.mark.parametrize("S", [1, 63, 65, 300, 8193])
def test_pairs_select(gpu, S):
    for Q, layout in ((5, "rows"), (33, "cols")):
        val, col = pair_case(Q, S, S + Q)
        for k in (1, 16, 17, 100, 1024, S):
            if k > S or k > 1024:
                continue
            want = DR.pairs_topk(val, col, k, 0)
            same(run_pairs(gpu, val, col, k, layout), want, "S=%d Q=%d k=%d" % (S, Q, k))
            for chunk in (64, 256):  # forced small chunks: several merge levels
                if chunk >= 2 * (1 << (k - 1).bit_length()):
                    same(run_pairs(gpu, val, col, k, layout, chunk=chunk), want, "S=%d Q=%d k=%d chunk=%d" % (S, Q, k, chunk))
    val, col = pair_case(5, S, S, present=1.0)
    k = min(S, 100)
    same(run_pairs(gpu, val, col, k, offset=123456789012), DR.pairs_topk(val, col, k, 123456789012), "offset")
    few = col.copy()
    few[:, k // 2 :] = ABSENT
    got = run_pairs(gpu, val, few, k, offset=1 << 40)
    same(got, DR.pairs_topk(val, few, k, 1 << 40), "fewer than k present")
    assert bool((got[1][:, k // 2 :] == -1).all()) and bool(torch.isneginf(got[0][:, k // 2 :]).all())


@pytest.mark.parametrize("G,k,chunk", [(65, 17, 0), (300, 100, 256), (8193, 100, 0), (8193, 1024, 0), (3000, 16, 64)])
def test_pairs_select_with_numbered_columns_is_the_row_select(gpu, G, k, chunk):
    from textreid_amd import lib as L
    from textreid_amd.ops import _p, stream

    Q = 5
    sim = level_matrix(Q, G, 4, G + k)
    col = np.broadcast_to(np.arange(G, dtype=np.int32), sim.shape).copy()
    got = run_pairs(gpu, sim, col, k, chunk=chunk)
    dev = torch.from_numpy(sim).to(gpu)
    nws = L.load().trid_topk_rows_deep_ws_bytes(Q, G, k, chunk)
    ws = torch.empty(nws, dtype=torch.uint8, device=gpu)
    vals = torch.empty(Q, k, dtype=torch.float32, device=gpu)
    idx = torch.empty(Q, k, dtype=torch.int64, device=gpu)
    L.call("trid_topk_rows_deep_f32", _p(dev), G, 1, Q, G, k, None, 0, _p(vals), _p(idx), _p(ws), nws, chunk, stream())
    assert torch.equal(got[0].view(torch.int32), vals.view(torch.int32)) and torch.equal(got[1], idx)
    same(got, TR.topk(sim, k))


# ------------------------------------------------------------------------------------------------------------------ the index
def some_pids(G, per=4, tag="p"):
    """about `per` rows per pid, scattered; pid values far apart (the group numbering must not depend on them)"""
    return OF.randint("gdd:%s%d" % (tag, G), 0, max(G // per, 1), (G,), SEED).long() * 1000003 - 77


class Ref:
    """the reference on one product: the group-best pairs are formed once per allow set (padding slots change nothing), every k
    selects from them"""

    def __init__(self, sim, pids, allow=None):
        sim = sim.numpy() if torch.is_tensor(sim) else sim
        order, starts, n_groups = DR.table(np.asarray(pids))
        self.best = DR.group_best(sim, order, starts, n_groups, max(n_groups, 1024), None if allow is None else np.asarray(allow))

    def __call__(self, k):
        return DR.pairs_topk(self.best[0], self.best[1], k)


@pytest.mark.parametrize("G", [20, 65, 2000, 20037])
def test_shortlist_pids_equals_the_dense_product(gpu, G):
    pids = some_pids(G)
    idx = fresh_index(gpu, gallery(G), pids)
    n_pids = int(torch.unique(pids).numel())
    for Q in (1, 5, 32, 40):
        qu = queries(gpu, Q)
        ref = Ref(dense_product(idx, qu), pids)
        for k in (17, 64, 100, 1024):
            if k > G:
                with pytest.raises(ValueError, match="shortlist_pids: k must be"):
                    idx.shortlist_pids(qu, k=k, normalize=False)
                continue
            got = idx.shortlist_pids(qu, k=k, normalize=False)
            assert got[0].shape == (Q, k) and got[1].dtype == torch.int64
            same3(got, ref(k), pids, "G=%d Q=%d k=%d" % (G, Q, k))
            m = min(k, n_pids)  # k beyond the number of pids: slots at the end
            assert bool((got[1][:, :m] >= 0).all()) and bool((got[1][:, m:] == -1).all()) and bool((got[2][:, m:] == -1).all())
            p = got[2][:, :m].cpu()
            assert all(torch.unique(p[q]).numel() == m for q in range(Q))
    raw = OF.randn("gdd:raw", (5, 256), SEED).to(gpu)
    k = min(G, 100)
    same3(idx.shortlist_pids(raw, k=k), Ref(dense_product(idx, unit_rows(raw)), pids)(k), pids, "normalize=True")


def test_the_crowd(gpu):
    """one person holds the 300 best rows of the query: shortlist's page is that person 300 times over, shortlist_pids' page is 100
    people"""
    G, k = 2000, 100
    q = OF.randn("gdd:crowd_q", (1, 256), SEED)
    rows = gallery(G).clone()
    rows[100:400] = 3.0 * q + 0.3 * OF.randn("gdd:crowd_n", (300, 256), SEED)
    pids = some_pids(G).clone()
    pids[100:400] = 424242
    idx = fresh_index(gpu, rows, pids)
    qu = unit_rows(q.to(gpu))
    top = idx.shortlist(qu, k=300, normalize=False)[1].cpu()
    assert bool(((top >= 100) & (top < 400)).all())
    got = idx.shortlist_pids(qu, k=k, normalize=False)
    same3(got, Ref(dense_product(idx, qu), pids)(k), pids)
    assert int(got[2][0, 0]) == 424242 and int(got[1][0, 0]) == int(top[0, 0]) and torch.unique(got[2]).numel() == k


def test_up_to_16_equals_search_pids_and_distinct_pids_equal_shortlist(gpu):
    G = 20037
    pids = some_pids(G)
    idx = fresh_index(gpu, gallery(G), pids)
    raw = OF.randn("gdd:raw_s", (40, 256), SEED).to(gpu)

    def agree(mask=None):
        for Q in (5, 32, 40):
            for k in (1, 10, 16):
                a = idx.search_pids(raw[:Q], k=k, mask=mask)
                b = idx.shortlist_pids(raw[:Q], k=k, mask=mask)
                assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]), (Q, k)

    agree()
    agree(coin("s_mask", G).to(gpu))
    best = idx.search_pids(raw[:32], k=16)[1].reshape(-1)
    assert idx.remove(rows=torch.unique(best)) > 0
    agree()
    agree(coin("s_mask2", G).to(gpu))
    # every pid different: the representatives are the rows
    alone = fresh_index(gpu, gallery(2000), torch.arange(2000) * 7 - 5000)
    m = coin("alone_mask", 2000).to(gpu)
    for k in (17, 100, 1024):
        for mask in (None, m):
            a = alone.shortlist(raw[:33], k=k, mask=mask)
            b = alone.shortlist_pids(raw[:33], k=k, mask=mask)
            assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1], b[1]), k
            assert torch.equal(b[2], torch.where(b[1] >= 0, b[1] * 7 - 5000, torch.full_like(b[1], -1)))


def test_exact_duplicate_rows_with_equal_and_with_different_pids(gpu):
    base = gallery(2000)[:500]
    rows = torch.cat([base, base, base], dim=0)  # row r, r + 500, r + 1000 are one image
    qu = queries(gpu, 5)
    # equal pids: one person, the lowest copy represents it
    pids = (torch.arange(1500) % 500) // 2
    idx = fresh_index(gpu, rows, pids)
    sim = dense_product(idx, qu)
    assert torch.equal(sim[:, :500], sim[:, 500:1000]) and torch.equal(sim[:, :500], sim[:, 1000:])
    got = idx.shortlist_pids(qu, k=99, normalize=False)
    same3(got, Ref(sim, pids)(99), pids, "equal pids")
    assert bool((got[1] < 500).all())
    # different pids: three people with equal scores, in insertion order
    pids = torch.arange(1500)
    idx = fresh_index(gpu, rows, pids)
    got = idx.shortlist_pids(qu, k=99, normalize=False)
    same3(got, Ref(sim, pids)(99), pids, "different pids")
    r = got[1].cpu().view(5, 33, 3)
    assert bool((r[:, :, 1] == r[:, :, 0] + 500).all()) and bool((r[:, :, 2] == r[:, :, 0] + 1000).all())


def test_tombstones_and_masks(gpu):
    G, Q, k = 2000, 5, 100
    pids = some_pids(G)
    idx = fresh_index(gpu, gallery(G), pids)
    qu = queries(gpu, Q)
    sim = dense_product(idx, qu)
    allow = torch.ones(G, dtype=torch.bool)
    first = idx.shortlist_pids(qu, k=k, normalize=False)
    # the representative of every query's best person goes: another row of that person (or nobody) takes its place
    best = first[1][:, 0].cpu()
    assert idx.remove(rows=best) == int(torch.unique(best).numel())
    allow[best] = False
    got = idx.shortlist_pids(qu, k=k, normalize=False)
    same3(got, Ref(sim, pids, allow)(k), pids, "representatives removed")
    assert not bool(torch.isin(got[1].cpu(), best).any())
    # whole persons go: the group table stays as it is, the pids yield the sentinel
    table_before = idx._ws["gtable"]
    some = torch.unique(first[2][:, 1].cpu())
    idx.remove(pids=some)
    allow &= ~torch.isin(pids, some)
    got = idx.shortlist_pids(qu, k=k, normalize=False)
    same3(got, Ref(sim, pids, allow)(k), pids, "pids removed")
    assert not bool(torch.isin(got[2].cpu(), some).any()) and idx._ws["gtable"] is table_before
    # masks: all, none, few - they compose with the tombstones (live & mask)
    ones = torch.ones(G, dtype=torch.bool)
    same3(idx.shortlist_pids(qu, k=k, normalize=False, mask=ones.to(gpu)), Ref(sim, pids, allow)(k), pids, "mask all")
    none = idx.shortlist_pids(qu, k=k, normalize=False, mask=torch.zeros(G, dtype=torch.uint8, device=gpu))
    assert bool((none[1] == -1).all()) and bool(torch.isneginf(none[0]).all()) and bool((none[2] == -1).all())
    few = torch.zeros(G, dtype=torch.bool)
    few[OF.randint("gdd:few", 0, G, (k - 10,), SEED)] = True
    n_ok = int(torch.unique(pids[few & allow]).numel())
    assert 0 < n_ok < k
    got = idx.shortlist_pids(qu, k=k, normalize=False, mask=few.to(gpu))
    same3(got, Ref(sim, pids, few & allow)(k), pids, "fewer than k allowed pids")
    assert bool((got[1][:, n_ok:] == -1).all()) and bool((got[1][:, :n_ok] >= 0).all())
    m = coin("tm_mask", G)
    same3(idx.shortlist_pids(qu, k=k, normalize=False, mask=m.to(gpu)), Ref(sim, pids, m & allow)(k), pids, "tombstones & mask")
    # k beyond the live rows without a mask is refused on the host
    idx.remove(rows=torch.nonzero(~few).reshape(-1))
    with pytest.raises(ValueError, match="shortlist_pids: k must be <= live_count"):
        idx.shortlist_pids(qu, k=k, normalize=False)
    live = int((few & allow).sum())
    same3(idx.shortlist_pids(qu, k=live, normalize=False), Ref(sim, pids, few & allow)(live), pids, "k == live_count > allowed pids")


def test_add_growth_compact_and_state_dict(gpu):
    from textreid_amd import GalleryIndex

    rows, pids = gallery(2000), some_pids(2000)
    idx = fresh_index(gpu, rows[:300], pids[:300])
    qu = queries(gpu, 5)
    k = 64
    same3(idx.shortlist_pids(qu, k=k, normalize=False), Ref(dense_product(idx, qu), pids[:300])(k), pids[:300], "first")
    assert idx._ws["gtable"][0].numel() == 300
    idx.add(rows[300:].to(gpu), pids=pids[300:])  # growth: new rows join old persons
    assert len(idx) == 2000
    sim = dense_product(idx, qu)
    same3(idx.shortlist_pids(qu, k=k, normalize=False), Ref(sim, pids)(k), pids, "after add")
    assert idx._ws["gtable"][0].numel() == 2000
    gone = coin("sc_gone", 2000, 3)
    idx.remove(rows=torch.nonzero(gone).reshape(-1))
    same3(idx.shortlist_pids(qu, k=k, normalize=False), Ref(sim, pids, ~gone)(k), pids, "after remove")
    sd = idx.state_dict()
    idx.compact()
    kept = pids[~gone]
    assert len(idx) == int((~gone).sum())
    same3(idx.shortlist_pids(qu, k=k, normalize=False), Ref(dense_product(idx, qu), kept)(k), kept, "after compact")
    back = GalleryIndex()
    back.load_state_dict(sd)
    same3(back.shortlist_pids(qu, k=k, normalize=False), Ref(dense_product(back, qu), pids, ~gone)(k), pids, "state_dict round trip")


def test_a_shortlist_after_a_shortlist_pids_is_unchanged(gpu):
    G = 2000
    idx = fresh_index(gpu, gallery(G), some_pids(G))
    qu = queries(gpu, 33)
    m = coin("after_mask", G).to(gpu)
    before = [idx.shortlist(qu, k=k, normalize=False, mask=mask) for k in (16, 100, 1024) for mask in (None, m)]
    idx.shortlist_pids(qu, k=1024, normalize=False, mask=m)
    idx.shortlist_pids(qu, k=17, normalize=False)
    after = [idx.shortlist(qu, k=k, normalize=False, mask=mask) for k in (16, 100, 1024) for mask in (None, m)]
    for a, b in zip(before, after):
        assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1], b[1])


def test_shortlist_pids_records_and_replays(gpu):
    G, Q, k = 20037, 4, 100
    pids = some_pids(G)
    idx = fresh_index(gpu, gallery(G), pids)
    idx.remove(rows=torch.nonzero(coin("cap_dead", G, 10)).reshape(-1))
    qa = OF.randn("gdd:cap_a", (Q, 256), SEED).to(gpu)
    qb = OF.randn("gdd:cap_b", (Q, 256), SEED).to(gpu)
    ma, mb = coin("cap_ma", G).to(gpu), coin("cap_mb", G).to(gpu)
    buf, m = qa.clone(), ma.clone()
    idx.shortlist_pids(buf, k=k, mask=m)  # (builds the group table, the score and pair buffers, the workspaces and the word buffer)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        vals, rows, got_pids = idx.shortlist_pids(buf, k=k, mask=m)
    g.replay()
    torch.cuda.synchronize()
    va, ra, pa = idx.shortlist_pids(qa, k=k, mask=ma)
    assert torch.equal(vals, va) and torch.equal(rows, ra) and torch.equal(got_pids, pa)
    buf.copy_(qb)
    m.copy_(mb)
    g.replay()
    torch.cuda.synchronize()
    got = (vals.clone(), rows.clone(), got_pids.clone())
    vb, rb, pb = idx.shortlist_pids(qb, k=k, mask=mb)
    assert torch.equal(got[0], vb) and torch.equal(got[1], rb) and torch.equal(got[2], pb)
    assert not torch.equal(rb, ra)
    ref = Ref(dense_product(idx, unit_rows(qb)), pids, mb.cpu() & idx.live.cpu())
    same3(got, ref(k), pids, "replay against the host reference")
    # a recording with another k than any eager call used: still nothing but launches
    g17 = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g17):
        out17 = idx.shortlist_pids(buf, k=17, mask=m)
    g17.replay()
    torch.cuda.synchronize()
    same3(out17, ref(17), pids, "k = 17 recorded after an eager k = 100")


# ------------------------------------------------------------------------------------------------------------------ search_reranked_pids
def reranked_ref(idx, sim, pids, alpha, allow=None):
    nn = idx.neighbours.cpu().numpy()
    n = nn.shape[1]
    a = None if allow is None else allow.numpy()
    qnn = TR.topk(sim.numpy(), n, a)[1]
    return Ref(RR.rerank_scores(sim.numpy(), qnn, nn, n, alpha, a), pids, allow)


@pytest.mark.parametrize("G,n", [(65, 5), (2000, 5), (2000, 8)])
def test_search_reranked_pids(gpu, G, n):
    pids = some_pids(G)
    # a clustered gallery, so that neighbour lists overlap and the bonus moves rows
    centres = OF.randn("gdd:centres", ((G + 7) // 8, 256), SEED)
    rows = centres.repeat_interleave(8, dim=0)[:G] + 2.0 * OF.randn("gdd:cnoise%d" % G, (G, 256), SEED)
    idx = fresh_index(gpu, rows, pids)
    idx.build_neighbours(n)
    alpha = 0.05
    for Q in (5, 40):
        qu = unit_rows((centres[torch.arange(Q) % centres.shape[0]] + 2.0 * OF.randn("gdd:cq%d" % Q, (Q, 256), SEED)).to(gpu))
        sim = dense_product(idx, qu)
        ref = reranked_ref(idx, sim, pids, alpha)
        plain = Ref(sim, pids)
        for k in (10, 17, 64):
            if k > G:
                continue
            same3(idx.search_reranked_pids(qu, k=k, alpha=alpha, normalize=False), ref(k), pids, "G=%d n=%d Q=%d k=%d" % (G, n, Q, k))
            a = idx.search_reranked_pids(qu, k=k, alpha=0.0, normalize=False)
            b = idx.shortlist_pids(qu, k=k, normalize=False)
            assert all(torch.equal(x, y) for x, y in zip(a, b)) and torch.equal(a[0].view(torch.int32), b[0].view(torch.int32))
        if G == 2000:
            assert not TR.same(ref(10), plain(10))  # (the bonus changes the page: a pass that did nothing cannot pass)
        m = coin("rr_mask%d" % G, G)
        k = min(G, 17)
        same3(idx.search_reranked_pids(qu, k=k, alpha=alpha, normalize=False, mask=m.to(gpu)), reranked_ref(idx, sim, pids, alpha, m)(k), pids, "mask")


def test_search_reranked_pids_with_tombstones_and_capture(gpu):
    G, n, k, alpha = 2000, 5, 50, 0.05
    pids = some_pids(G)
    idx = fresh_index(gpu, gallery(G), pids)
    gone = coin("rr_gone", G, 5)
    idx.remove(rows=torch.nonzero(gone).reshape(-1))
    idx.build_neighbours(n)
    qa, qb = queries(gpu, 4, "rra"), queries(gpu, 4, "rrb")
    ma, mb = coin("rr_ma", G), coin("rr_mb", G)
    same3(idx.search_reranked_pids(qa, k=k, alpha=alpha, normalize=False), reranked_ref(idx, dense_product(idx, qa), pids, alpha, ~gone)(k), pids, "tombstones")
    buf, m = qa.clone(), ma.to(gpu)
    idx.search_reranked_pids(buf, k=k, alpha=alpha, normalize=False, mask=m)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = idx.search_reranked_pids(buf, k=k, alpha=alpha, normalize=False, mask=m)
    g.replay()
    torch.cuda.synchronize()
    same3(out, reranked_ref(idx, dense_product(idx, qa), pids, alpha, ma & ~gone)(k), pids, "first replay")
    buf.copy_(qb)
    m.copy_(mb.to(gpu))
    g.replay()
    torch.cuda.synchronize()
    same3(out, reranked_ref(idx, dense_product(idx, qb), pids, alpha, mb & ~gone)(k), pids, "replay with other queries and another mask")
