"""The neighbour graph and the exact re-ranked search of GalleryIndex on the GPU: trid_index_rerank_add_f32 alone (every layout, masks
with garbage tail bits, the whole buffer compared bitwise so that nothing outside the touched elements moves), build_neighbours
against the dense trid_gemm_p16 product of the index's OWN operands, search_reranked against gallery_rerank_ref.reranked_topk on
that product.  Nothing here needs a tolerance: values are compared as bit patterns, rows exactly."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import gallery_rerank_ref as RR  # noqa: E402
import oracle.fill as OF  # noqa: E402
import topk_deep_ref as TR  # noqa: E402
from gallery_support import dense_product, fresh_index, gpu, Inputs, same_bits as same, unit_rows  # noqa: E402,F401

SEED = 13
# the clustered gallery's generator seed: with 13 the CPU trial of the recipe (fp32 matmul) left ONE pair with c = 5, which a last-bit
# difference of the P16 product could remove; 15 leaves 7 (c = 1 .. 5: 392 / 84 / 84 / 48 / 7, 29 of 40 orders and 10 of 40 sets
# changed at k = 10).  The noise factor stays at 2.0 and the two conditions are asserted as they stand.
CLUSTER_SEED = 15
IN = Inputs("grr:", SEED, graph_n=5)  # (test_gallery_refresh_gpu.py and test_gallery_expand_gpu.py name the same inputs and share the caches)
coin, gallery, queries = IN.coin_one_in, IN.gallery, IN.queries
shared_index, self_product = IN.shared_index, IN.self_product  # (one index with a built graph per (length, n), never modified by a test)


def reference(idx, sim, k, alpha=0.05, allow=None):
    """reranked_topk on the dense product with the index's own lists (checked against the graph reference by the graph tests)"""
    nn = idx.neighbours.cpu().numpy()
    return RR.reranked_topk(sim.numpy(), nn, nn.shape[1], alpha, k, None if allow is None else allow.numpy())


# ------------------------------------------------------------------------------------------------------------------ the kernel alone
def _lists(rng, rows, n, G):
    """[rows, n] lists of distinct rows of [0, G)"""
    if G <= 512:
        return np.stack([rng.permutation(G)[:n] for _ in range(rows)]).astype(np.int64)
    start, step = rng.randint(0, G, size=(rows, 1)), rng.randint(1, G // n, size=(rows, 1))  # (step * (n - 1) < G: no wrap onto itself)
    return ((start + step * np.arange(n)[None, :]) % G).astype(np.int64)


def _kernel_case(gpu, G, n, layout, Q, wide, alpha, use_mask, seed):
    from textreid_amd import ops
    from textreid_amd.ops import _p

    rng = np.random.RandomState(seed)
    gnn = _lists(rng, G, n, G)
    qnn = _lists(rng, Q, n, G)
    nqs = [n, 0, 1, n - 1]
    for q in range(Q):
        qnn[q, nqs[q % 4]:] = -1
    # planted overlaps: for every query and every c up to its nq TWO rows whose lists share exactly c rows with the query's, at rows
    # q * 2 (n + 1) + 2 c and + 1 (mod G; query 0 is planted last, rows 2 .. 2 n + 1, so nothing overwrites its rows)
    for q in reversed(range(Q)):
        nq = int((qnn[q] >= 0).sum())
        others = np.setdiff1d(np.arange(G), qnn[q][:nq])
        for c in range(1, nq + 1):
            for j in (0, 1):
                if others.size >= n - c:
                    g = (q * 2 * (n + 1) + 2 * c + j) % G
                    gnn[g] = np.concatenate([qnn[q, :c], rng.permutation(others)[: n - c]])[rng.permutation(n)]
    if G >= 63:
        gnn[G - 1] = -1  # (a removed row's list)
    gnn = gnn.astype(np.int32)
    allow = None
    words = None
    if use_mask:
        allow = rng.randint(0, 4, size=G) != 0
        if G >= 63:  # (of query 0's two rows per c one is allowed, one is not)
            allow[2 : 2 * n + 2 : 2], allow[3 : 2 * n + 3 : 2] = True, False
        nw = (G + 31) // 32
        bits = np.zeros(nw * 32, dtype=np.uint64)
        bits[:G] = allow
        bits[G:] = rng.randint(0, 2, size=nw * 32 - G)  # garbage tail bits
        if nw * 32 > G:
            bits[G] = 1
        w = (bits.reshape(nw, 32) << np.arange(32, dtype=np.uint64)[None, :]).sum(axis=1).astype(np.uint32)
        words = torch.from_numpy(w.view(np.int32).copy()).to(gpu)
    c = RR.counts(qnn, gnn)
    if G >= 63:
        assert set(np.unique(c).tolist()) >= set(range(n + 1)), (G, n, Q)
    # the buffer: larger than the extent, a recognisable pattern outside it
    if layout == "cols":
        ld_q, ld_g, size = 1, wide, (G + 2) * wide
        at = np.arange(G)[None, :] * wide + np.arange(Q)[:, None]
    else:
        ld_q, ld_g, size = G + 3, 1, Q * (G + 3) + 5
        at = np.arange(Q)[:, None] * (G + 3) + np.arange(G)[None, :]
    buf = (0x5A5A0000 + (np.arange(size) & 0xFFFF)).astype(np.uint32).view(np.float32).copy()
    sim = rng.standard_normal((Q, G)).astype(np.float32)
    ok = np.ones((Q, G), dtype=bool) if allow is None else np.broadcast_to(allow[None, :], (Q, G))
    zero, hit = np.argwhere(c == 0), np.argwhere((c > 0) & ok)
    if len(zero) >= 2:
        sim[tuple(zero[0])], sim[tuple(zero[-1])] = -np.inf, -0.0
    if len(hit):
        sim[tuple(hit[0])] = -np.inf
    if G >= 63 and use_mask:
        assert len(hit) and ((c > 0) & ~ok).any()
    buf[at] = sim
    want = buf.copy()
    want[at] = RR.rerank_scores(sim, qnn, gnn, n, alpha, allow)
    dev = torch.from_numpy(buf).to(gpu)
    dq, dg = torch.from_numpy(qnn).to(gpu), torch.from_numpy(gnn).to(gpu)
    ops.call("trid_index_rerank_add_f32", _p(dev), ld_q, ld_g, Q, G, _p(dq), _p(dg), n, alpha, _p(words), ops.stream())
    got = dev.cpu().numpy()
    bad = np.nonzero(got.view(np.uint32) != want.view(np.uint32))[0]
    assert bad.size == 0, "G=%d n=%d %s Q=%d: %d words differ, first at %d (got %r, want %r)" % (G, n, layout, Q, bad.size, bad[0], got[bad[0]], want[bad[0]])


@pytest.mark.parametrize("G,n", [(G, n) for G in (1, 63, 64, 65, 255, 257, 5000) for n in (1, 5, 8) if n <= G])
def test_kernel_adds_the_bonus_and_touches_nothing_else(gpu, G, n):
    cases = [("cols", 1, 32, 0.05, True), ("cols", 5, 32, 0.3, False), ("cols", 32, 32, 0.05, True), ("cols", 32, 64, 0.05, True),
             ("rows", 1, 0, 0.05, True), ("rows", 33, 0, 0.05, True), ("rows", 70, 0, 0.3, False)]
    for i, (layout, Q, wide, alpha, use_mask) in enumerate(cases):
        _kernel_case(gpu, G, n, layout, Q, wide, alpha, use_mask, 1000 * G + 10 * n + i)


# ------------------------------------------------------------------------------------------------------------------ the graph
@pytest.mark.parametrize("G", [20, 65, 2000])
def test_whole_graph_equals_the_dense_product(gpu, G):
    sim = self_product(gpu, G)
    for n in (1, 5, 8):
        idx = shared_index(gpu, G, n)
        assert idx.neighbours_current
        nn = idx.neighbours
        assert nn.dtype == torch.int32 and tuple(nn.shape) == (G, n)
        assert np.array_equal(nn.cpu().numpy(), RR.graph(sim, n)), (G, n)
    assert bool((shared_index(gpu, G, 5).neighbours[:, 0].cpu() == torch.arange(G)).all())  # (no duplicates: every row leads its own list)


def test_sampled_graph_at_20037_rows(gpu):
    G, n = 20037, 5
    idx = shared_index(gpu, G, n)
    fixed = [0, 31, 32, 20032, 20033, 20034, 20035, 20036]
    rest = [int(r) for r in OF.randint("grr:sample", 0, G, (200,), SEED).tolist() if r not in fixed]
    sample = torch.tensor(fixed + list(dict.fromkeys(rest))[: 64 - len(fixed)])
    assert sample.numel() == 64
    sim = dense_product(idx, idx.rows[sample.to(gpu)].contiguous()).numpy()
    assert np.array_equal(idx.neighbours.cpu()[sample].numpy(), TR.topk(sim, n)[1].astype(np.int32))


def test_duplicates_start_with_the_lowest_numbered_copy(gpu):
    base = gallery(2000)[:300]
    idx = fresh_index(gpu, torch.cat([base, base, base], dim=0), n=5)  # row r, r + 300, r + 600 are one image
    nn = idx.neighbours.cpu()
    r = torch.arange(900) % 300
    assert torch.equal(nn[:, 0].long(), r) and torch.equal(nn[:, 1].long(), r + 300) and torch.equal(nn[:, 2].long(), r + 600)
    assert np.array_equal(nn.numpy(), RR.graph(dense_product(idx, idx.rows).numpy(), 5))


def test_graph_built_after_remove(gpu):
    G, n = 2000, 5
    idx = fresh_index(gpu, gallery(G))
    gone = coin("dead", G, 3)
    assert idx.remove(rows=torch.nonzero(gone).reshape(-1)) == int(gone.sum())
    idx.build_neighbours(n)
    nn = idx.neighbours.cpu()
    assert bool((nn[gone] == -1).all()) and bool((nn[~gone] >= 0).all())
    assert not bool(gone[nn[~gone].long()].any())  # no live list holds a dead row
    assert np.array_equal(nn.numpy(), RR.graph(self_product(gpu, G), n, (~gone).numpy()))


def test_what_makes_the_graph_stale(gpu):
    from textreid_amd import GalleryIndex

    rows = gallery(2000)
    idx = fresh_index(gpu, rows[:65])
    q = queries(gpu, 3)
    assert idx.neighbours is None and not idx.neighbours_current
    with pytest.raises(RuntimeError, match="build_neighbours"):
        idx.search_reranked(q, k=5, normalize=False)
    for bad in (0, 9):
        with pytest.raises(ValueError, match="build_neighbours: n must be in"):
            idx.build_neighbours(bad)
    idx.build_neighbours(5)
    assert idx.neighbours_current
    # a mask is a property of one question: searches with one leave the graph current
    m = coin("stale_mask", 65).to(gpu)
    idx.search(q, k=5, normalize=False, mask=m)
    idx.shortlist(q, k=20, normalize=False, mask=m)
    idx.search_reranked(q, k=5, normalize=False, mask=m)
    assert idx.neighbours_current
    # add
    idx.add(rows[65:100].to(gpu))
    assert not idx.neighbours_current and tuple(idx.neighbours.shape) == (100, 5) and bool((idx.neighbours[65:] == -1).all())
    with pytest.raises(RuntimeError, match="stale.*build_neighbours"):
        idx.search_reranked(q, k=5, normalize=False)
    idx.build_neighbours(5)
    assert idx.neighbours_current and bool((idx.neighbours >= 0).all())
    # remove: only when it removed something
    assert idx.remove(rows=[3, 4]) == 2 and not idx.neighbours_current
    idx.build_neighbours(5)
    assert idx.remove(rows=[3]) == 0 and idx.neighbours_current
    sd = idx.state_dict()
    assert sd["neighbours"] is not None and torch.equal(sd["neighbours"], idx.neighbours)
    # compact: only when it dropped something
    idx.compact()
    assert len(idx) == 98 and not idx.neighbours_current and idx.state_dict()["neighbours"] is None
    with pytest.raises(RuntimeError, match="build_neighbours"):
        idx.search_reranked(q, k=5, normalize=False)
    idx.build_neighbours(8)
    assert tuple(idx.neighbours.shape) == (98, 8)
    idx.compact()
    assert idx.neighbours_current
    # n beyond the live rows
    idx.remove(rows=list(range(5, 98)))
    with pytest.raises(ValueError, match="build_neighbours: n must be <= live_count"):
        idx.build_neighbours(6)
    idx.build_neighbours(5)
    # a state dict written before the graph existed loads with no graph
    old = {k: v for k, v in sd.items() if k != "neighbours"}
    back = GalleryIndex()
    back.load_state_dict(sd)
    assert back.neighbours_current and torch.equal(back.neighbours, sd["neighbours"])
    back.load_state_dict(old)
    assert not back.neighbours_current and back.neighbours is None and back.state_dict()["neighbours"] is None
    with pytest.raises(RuntimeError, match="build_neighbours"):
        back.search_reranked(q, k=5, normalize=False)
    for bad in (sd["neighbours"][:-1], sd["neighbours"].long(), sd["neighbours"] + 100):
        with pytest.raises(ValueError, match="load_state_dict: neighbours must"):
            back.load_state_dict(dict(sd, neighbours=bad))


# ------------------------------------------------------------------------------------------------------------------ search_reranked
def test_clustered_gallery_where_the_term_bites(gpu):
    n, alpha, noise = 5, 0.05, 2.0
    centres = OF.randn("grr:centres", (250, 256), CLUSTER_SEED)
    rows = centres.repeat_interleave(8, dim=0) + noise * OF.randn("grr:cnoise", (2000, 256), CLUSTER_SEED)
    rows = rows[torch.from_numpy(np.argsort(OF.randn("grr:cperm", (2000,), CLUSTER_SEED).numpy(), kind="stable"))]
    qu = unit_rows((centres[:40] + noise * OF.randn("grr:cq", (40, 256), CLUSTER_SEED)).to(gpu))
    idx = fresh_index(gpu, rows, n=n)
    sim = dense_product(idx, qu).numpy()
    gnn = RR.graph(dense_product(idx, idx.rows).numpy(), n)
    assert np.array_equal(idx.neighbours.cpu().numpy(), gnn)
    # the two conditions, on the REFERENCE's output: a bonus that does nothing cannot pass
    c = RR.counts(TR.topk(sim, n)[1], gnn)
    print("pairs with c = 1 .. 5:", [int((c == i).sum()) for i in range(1, n + 1)])
    assert set(np.unique(c).tolist()) >= set(range(1, n + 1))
    want = RR.reranked_topk(sim, gnn, n, alpha, 10)
    plain = TR.topk(sim, 10)
    moved = sum(set(want[1][q].tolist()) != set(plain[1][q].tolist()) for q in range(40))
    print("queries whose top-10 row set changes:", moved, "whose order changes:", sum(not np.array_equal(want[1][q], plain[1][q]) for q in range(40)))
    assert moved >= 1
    same(idx.search_reranked(qu, k=10, alpha=alpha, normalize=False), want, "k = 10")
    same(idx.shortlist(qu, k=10, normalize=False), plain, "shortlist next to it")
    for k in (1, 100, 1024):
        same(idx.search_reranked(qu, k=k, alpha=alpha, normalize=False), RR.reranked_topk(sim, gnn, n, alpha, k), "k = %d" % k)
    same(idx.search_reranked(qu, k=10, alpha=0.3, normalize=False), RR.reranked_topk(sim, gnn, n, 0.3, 10), "alpha = 0.3")
    # a mask: the query's own list is its n best ALLOWED rows
    m = coin("cl_mask", 2000)
    same(idx.search_reranked(qu, k=10, alpha=alpha, normalize=False, mask=m.to(gpu)), RR.reranked_topk(sim, gnn, n, alpha, 10, m.numpy()), "masked")


@pytest.mark.parametrize("G,n", [(20, 5), (65, 5), (2000, 5), (2000, 1), (2000, 8), (20037, 5)])
def test_search_reranked_equals_the_reference(gpu, G, n):
    idx = shared_index(gpu, G, n)
    for Q in (1, 5, 32, 40):
        qu = queries(gpu, Q)
        sim = dense_product(idx, qu)
        for k in (1, 10, 17, 100, 1024):
            if k > G:
                with pytest.raises(ValueError, match="search_reranked: k must be"):
                    idx.search_reranked(qu, k=k, normalize=False)
                continue
            got = idx.search_reranked(qu, k=k, normalize=False)
            assert got[0].shape == (Q, k) and got[1].dtype == torch.int64 and got[0].dtype == torch.float32
            same(got, reference(idx, sim, k), "G=%d n=%d Q=%d k=%d" % (G, n, Q, k))
    # raw queries: normalised by the same kernel search uses
    raw = OF.randn("grr:raw", (5, 256), SEED).to(gpu)
    k = min(G, 10)
    same(idx.search_reranked(raw, k=k), reference(idx, dense_product(idx, unit_rows(raw)), k), "normalize=True")
    assert idx.neighbours_current and idx.live_count == G


def test_alpha_zero_equals_shortlist_and_search(gpu):
    idx = shared_index(gpu, 20037)
    raw = OF.randn("grr:raw_s", (40, 256), SEED).to(gpu)
    m = coin("a0_mask", 20037).to(gpu)
    for mask in (None, m):
        for Q in (5, 32, 40):
            for k in (10, 16, 100):
                a = idx.search_reranked(raw[:Q], k=k, alpha=0.0, mask=mask)
                b = idx.shortlist(raw[:Q], k=k, mask=mask)
                assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1], b[1]), (Q, k)
                if k <= 16 and Q <= 32:
                    s = idx.search(raw[:Q], k=k, mask=mask)
                    assert torch.equal(a[0].view(torch.int32), s[0].view(torch.int32)) and torch.equal(a[1], s[1]), (Q, k)


def test_masks_and_tombstones(gpu):
    G, Q, k, n = 2000, 5, 100, 5
    idx = fresh_index(gpu, gallery(G))
    qu = queries(gpu, Q)
    sim = dense_product(idx, qu)
    gone = coin("mt_gone", G, 4)
    idx.remove(rows=torch.nonzero(gone).reshape(-1))
    live = ~gone
    idx.build_neighbours(n)
    same(idx.search_reranked(qu, k=k, normalize=False), reference(idx, sim, k, allow=live), "tombstones")
    ones = torch.ones(G, dtype=torch.bool)
    same(idx.search_reranked(qu, k=k, normalize=False, mask=ones.to(gpu)), reference(idx, sim, k, allow=live), "mask all")
    none = idx.search_reranked(qu, k=k, normalize=False, mask=torch.zeros(G, dtype=torch.uint8, device=gpu))
    assert bool((none[1] == -1).all()) and bool(torch.isneginf(none[0]).all())
    # fewer than k allowed: real results first, then (-inf, -1)
    few = torch.zeros(G, dtype=torch.bool)
    few[OF.randint("grr:few", 0, G, (k - 10,), SEED)] = True
    n_ok = int((few & live).sum())
    assert n < n_ok < k
    got = idx.search_reranked(qu, k=k, normalize=False, mask=few.to(gpu))
    same(got, reference(idx, sim, k, allow=few & live), "fewer than k allowed")
    assert bool((got[1][:, n_ok:] == -1).all()) and bool((got[1][:, :n_ok] >= 0).all()) and bool(torch.isneginf(got[0][:, n_ok:]).all())
    # fewer than n allowed: the query's own list has -1 slots, nq < n
    live_rows = torch.nonzero(live).reshape(-1)
    for left in (3, 1):
        m = torch.zeros(G, dtype=torch.bool)
        m[live_rows[torch.unique(OF.randint("grr:left%d" % left, 0, live_rows.numel(), (40,), SEED))[:left]]] = True
        m |= gone  # (removed rows the mask allows stay removed: live & mask)
        assert int((m & live).sum()) == left
        got = idx.search_reranked(qu, k=10, normalize=False, mask=m.to(gpu))
        same(got, reference(idx, sim, 10, allow=m & live), "%d allowed" % left)
        assert bool((got[1][:, :left] >= 0).all()) and bool((got[1][:, left:] == -1).all())
        # every allowed row leads its own list and is in the query's (all allowed rows are): c >= 1, so every value moved up
        plain = idx.shortlist(qu, k=10, normalize=False, mask=m.to(gpu))
        gr, gi = torch.sort(got[1][:, :left], dim=1)
        pr, pi = torch.sort(plain[1][:, :left], dim=1)
        assert torch.equal(gr, pr) and bool((got[0][:, :left].gather(1, gi) > plain[0][:, :left].gather(1, pi)).all())
    m = coin("mt_mask", G)
    same(idx.search_reranked(qu, k=k, normalize=False, mask=m.to(gpu)), reference(idx, sim, k, allow=m & live), "tombstones & mask")
    # k beyond the live rows without a mask is refused on the host
    idx.remove(rows=torch.nonzero(~few).reshape(-1))
    assert idx.live_count == n_ok and not idx.neighbours_current
    idx.build_neighbours(n)
    with pytest.raises(ValueError, match="search_reranked: k must be <= live_count"):
        idx.search_reranked(qu, k=k, normalize=False)
    same(idx.search_reranked(qu, k=n_ok, normalize=False), reference(idx, sim, n_ok, allow=few & live), "k == live_count")
    same(idx.search_reranked(qu, k=k, normalize=False, mask=ones.to(gpu)), reference(idx, sim, k, allow=few & live), "k > live_count under a mask")


def test_a_shortlist_after_a_reranked_search_is_unchanged(gpu):
    idx = shared_index(gpu, 2000)
    qu = queries(gpu, 40)
    sim = dense_product(idx, qu)
    want = TR.topk(sim.numpy(), 100)
    before = idx.shortlist(qu, k=100, normalize=False)
    idx.search_reranked(qu, k=100, alpha=0.5, normalize=False)  # (the score buffer is shared and was modified in place)
    same(idx.shortlist(qu, k=100, normalize=False), want, "after")
    same(before, want, "before")
    same(idx.search_reranked(qu[:7], k=100, normalize=False), reference(idx, sim[:7], 100), "a smaller panel next")
    same(idx.search(qu[:7], k=10, normalize=False), TR.topk(sim[:7].numpy(), 10), "search next")


def test_state_dict_round_trip_and_growth(gpu):
    from textreid_amd import GalleryIndex

    rows = gallery(2000)
    idx = fresh_index(gpu, rows[:300], n=5)
    qu = queries(gpu, 5)
    k = 64
    same(idx.search_reranked(qu, k=k, normalize=False), reference(idx, dense_product(idx, qu), k), "first")
    held = idx._ws["scores"].shape[0]
    idx.add(rows[300:].to(gpu))  # growth past the cached score buffer and the lists' storage
    assert len(idx) == 2000 and len(idx) > held and not idx.neighbours_current
    idx.build_neighbours(5)
    assert torch.equal(idx.neighbours, shared_index(gpu, 2000).neighbours)  # (the same rows: the same graph)
    sim = dense_product(idx, qu)
    want = reference(idx, sim, k)
    same(idx.search_reranked(qu, k=k, normalize=False), want, "after growth")
    assert idx._ws["scores"].shape[0] >= 2000
    gone = coin("sd_gone", 2000, 3)
    idx.remove(rows=torch.nonzero(gone).reshape(-1))
    assert idx.state_dict()["neighbours"] is None  # (stale lists are not saved)
    idx.build_neighbours(5)
    sd = idx.state_dict()
    assert sd["neighbours"].dtype == torch.int32 and tuple(sd["neighbours"].shape) == (2000, 5)
    sd["neighbours"][0, 0] = -1  # (a clone: the index does not see this)
    assert int(idx.neighbours[0, 0]) != -1 or bool(gone[0])
    sd = idx.state_dict()
    back = GalleryIndex()
    back.load_state_dict(sd)
    assert back.neighbours_current and torch.equal(back.neighbours, idx.neighbours) and back.live_count == idx.live_count
    want = reference(idx, sim, k, allow=~gone)
    same(idx.search_reranked(qu, k=k, normalize=False), want, "tombstones")
    same(back.search_reranked(qu, k=k, normalize=False), want, "state_dict round trip")


# ------------------------------------------------------------------------------------------------------------------ capture
def test_search_reranked_records_and_replays(gpu):
    G, Q, k = 20037, 4, 100
    idx = fresh_index(gpu, gallery(G))
    idx.remove(rows=torch.nonzero(coin("cap_dead", G, 10)).reshape(-1))
    idx.build_neighbours(5)
    qa = OF.randn("grr:cap_a", (Q, 256), SEED).to(gpu)
    qb = OF.randn("grr:cap_b", (Q, 256), SEED).to(gpu)
    ma, mb = coin("cap_ma", G).to(gpu), coin("cap_mb", G).to(gpu)
    buf, m = qa.clone(), ma.clone()
    idx.search_reranked(buf, k=k, mask=m)  # (allocates the score buffer, the workspaces and the word buffer)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        vals, rows = idx.search_reranked(buf, k=k, mask=m)
    g.replay()
    torch.cuda.synchronize()
    va, ra = idx.search_reranked(qa, k=k, mask=ma)
    assert torch.equal(vals, va) and torch.equal(rows, ra)
    buf.copy_(qb)
    m.copy_(mb)
    g.replay()
    torch.cuda.synchronize()
    got_v, got_r = vals.clone(), rows.clone()
    vb, rb = idx.search_reranked(qb, k=k, mask=mb)
    assert torch.equal(got_v, vb) and torch.equal(got_r, rb)
    assert not torch.equal(rb, ra)
    live = idx.live.cpu()
    same((got_v, got_r), reference(idx, dense_product(idx, unit_rows(qb)), k, allow=mb.cpu() & live), "replay against the host reference")
