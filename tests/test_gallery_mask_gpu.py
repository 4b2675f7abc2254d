"""Row removal and filtered search of GalleryIndex on the GPU.  The comparator is exact: the dense trid_gemm_p16 product of the index's
own P16 operands (gallery_support.dense_product), disallowed rows at -inf, stable descending sort, rows of -inf values reported as -1
(gallery_mask_ref.masked_topk).  Values and rows are compared bit for bit everywhere but in the one oracle test."""

import pytest
import torch

pytestmark = pytest.mark.gpu

import gallery_mask_ref as MR  # noqa: E402
import oracle.evaluation as OE  # noqa: E402
import oracle.fill as OF  # noqa: E402
from gallery_support import c_search, dense_product, fresh_index, gpu, Inputs, same_values as same, unit_rows  # noqa: E402,F401

SEED = 8
SHAPES = [(1, 1, 1), (2, 33, 10), (5, 63, 5), (32, 64, 16), (7, 65, 10), (5, 4099, 16), (17, 20037, 10)]
ADV_G = 20037
NEG = float("-inf")
IN = Inputs("gmk:", SEED)
raw, coin, built = IN.raw, IN.coin_keep, IN.built  # (built: the index is shared and never modified by a test)


# ----------------------------------------------------------------------------------------------------------- 1. pack kernel
@pytest.mark.parametrize("n", [1, 31, 32, 33, 63, 64, 65, 4099])
def test_pack_kernel_equals_pack_words(gpu, n):
    from textreid_amd import lib as L
    from textreid_amd.ops import _p, stream

    live = coin("pack_live%d" % n, n, 3) == False  # noqa: E712  (about two thirds live)
    allow = coin("pack_allow%d" % n, n)
    live[n - 1] = allow[n - 1] = True  # the last row's bit is the highest that may be set
    extra = 3
    nw = (n + 31) // 32 + extra
    lg, ag = live.to(gpu), allow.to(torch.uint8).to(gpu) * 3  # (uint8 and any non-zero value = allowed)
    for what, lp, ap, want in (("live", lg, None, live), ("allow", None, ag, allow), ("both", lg, ag, live & allow)):
        words = torch.full((nw,), -1, dtype=torch.int32, device=gpu)  # pre-filled with ones: tail bits and tail words must come out 0
        L.call("trid_index_pack_mask_u32", _p(lp), _p(ap), n, _p(words), nw, stream())
        got = MR.words_as_int64(words)
        ref = torch.cat([MR.pack_words(want), torch.zeros(extra, dtype=torch.int64)])
        assert torch.equal(got, ref), (what, n, got, ref)
        assert int(got[(n - 1) >> 5]) >> ((n - 1) & 31) == 1  # the last row's bit is set and nothing above it


# ------------------------------------------------------------------------------------- 2. masked search, exact
def mask_patterns(Q, G, k):
    """{name: allow bool [G]} - the patterns that apply to the shape"""
    tiles, nwords = (G + 63) // 64, (G + 31) // 32
    ar = torch.arange(G)
    pats = {"ones": torch.ones(G, dtype=torch.bool), "random half": coin("half%d" % G, G), "none": torch.zeros(G, dtype=torch.bool)}
    if nwords >= 2:
        w = nwords // 2 if nwords > 2 else 0
        pats["one word zero"] = (ar >> 5) != w
    if tiles >= 2:
        t = tiles // 2 if tiles > 2 else 0
        pats["one step tile zero"] = (ar >> 6) != t
        # worker 1 of 3 owns the step tiles [T / 3, 2 T / 3)
        lo, hi = tiles // 3, 2 * tiles // 3
        pats["worker 1 of 3 zero"] = ((ar >> 6) < lo) | ((ar >> 6) >= hi)
        pats["only the ragged last tile"] = (ar >> 6) == tiles - 1
    if k >= 2:
        few = torch.zeros(G, dtype=torch.bool)
        few[torch.linspace(0, G - 1, k - 1).long()] = True  # k - 1 rows at most, the first and the last row among them
        pats["fewer than k"] = few
    return pats


@pytest.mark.parametrize("Q,G,k", SHAPES)
def test_masked_search_equals_dense_p16_product(gpu, Q, G, k):
    idx, te, ie, qu, sim = built(gpu, Q, G)
    plain = idx.search(te.to(gpu), k=k)
    same(plain, MR.masked_topk(sim, torch.ones(G, dtype=torch.bool), k), "unmasked")
    pats = mask_patterns(Q, G, k)
    assert len(pats) >= (3 if G == 1 else 4)
    for name, allow in pats.items():
        ref = MR.masked_topk(sim, allow, k)
        n_ok = int(allow.sum())
        if n_ok < k:  # short rows: the real results first, then (-inf, -1)
            assert bool((ref[1][:, n_ok:] == -1).all()) and bool((ref[0][:, n_ok:] == NEG).all()) and bool((ref[1][:, :n_ok] >= 0).all())
        got = idx.search(te.to(gpu), k=k, mask=allow.to(gpu))
        same(got, ref, "search(mask) %s" % name)
        same(idx.search(qu, k=k, normalize=False, mask=allow.to(torch.uint8).to(gpu)), ref, "search(uint8 mask), unit queries, %s" % name)
        if name == "ones":  # bit for bit the unmasked search
            assert torch.equal(got[0], plain[0]) and torch.equal(got[1], plain[1])
        for wg in (0, 1, 3):
            same(c_search(idx, qu, k, wg, allow), ref, "%s workgroups=%d" % (name, wg))
    assert idx.live_count == G  # a mask leaves no trace on the index
    same(idx.search(te.to(gpu), k=k), (plain[0].cpu(), plain[1].cpu()), "unmasked again")


# --------------------------------------------------------------------------------- 3. the winners are the removed rows
def test_removing_the_winners(gpu):
    Q, G, k = 5, 4099, 10
    _, te, ie, qu, sim = built(gpu, Q, G)
    idx = fresh_index(gpu, ie)
    v0, r0 = idx.search(qu, k=k, normalize=False)
    gone = r0[0].clone()
    assert idx.remove(rows=gone) == k and idx.live_count == G - k
    allow = torch.ones(G, dtype=torch.bool)
    allow[gone.cpu()] = False
    ref = MR.masked_topk(sim, allow, k)
    got = idx.search(qu, k=k, normalize=False)
    same(got, ref, "top-k of query 0 removed")
    assert not bool(torch.isin(got[1].cpu(), gone.cpu()).any())
    assert float(got[0][0, 0]) < float(v0[0, k - 1])  # query 0 now starts below its old k-th value
    for wg in (1, 3):
        same(c_search(idx, qu, k, wg, allow), ref, "workgroups=%d" % wg)


def _adversarial(kind):
    G = ADV_G
    q = OF.randn("gix:advq", (5, 256), SEED)
    g = OF.randn("gix:advg:" + kind, (G, 256), SEED)
    if kind == "rising":
        # query 0 = e_0, gallery row i = c_i e_0 + (noise in the other coordinates): similarity to query 0 is c_i exactly
        q[0] = 0.0
        q[0, 0] = 1.0
        g[:, 0] = 0.0
        g = 0.5 * g / g.norm(dim=1, keepdim=True)
        c = (torch.arange(G, dtype=torch.float32) + 1.0) / G
        g[:, 0] = 0.75 * c
    elif kind == "ties":
        g[10000:20000] = g[:10000]
    q = q / q.norm(dim=1, keepdim=True)
    if kind == "ties":
        g = g / g.norm(dim=1, keepdim=True)
    return q, g


def test_ties_the_higher_copy_takes_the_place_of_the_removed_lower_copy(gpu):
    q, g = _adversarial("ties")
    qg = q.to(gpu)
    idx = fresh_index(gpu, g, normalize=False)
    k = 10
    sim = dense_product(idx, qg)
    before = MR.masked_topk(sim, torch.ones(ADV_G, dtype=torch.bool), k)
    same(idx.search(qg, k=k, normalize=False), before, "ties, nothing removed")
    r = before[1]
    pairs = (r[:, :-1] < 10000) & (r[:, 1:] == r[:, :-1] + 10000)
    assert int(pairs.sum()) >= 5
    qi, pos = [int(x) for x in torch.nonzero(pairs)[0]]
    low = int(r[qi, pos])
    assert idx.remove(rows=[low]) == 1
    allow = torch.ones(ADV_G, dtype=torch.bool)
    allow[low] = False
    after = MR.masked_topk(sim, allow, k)
    got = idx.search(qg, k=k, normalize=False)
    same(got, after, "ties, lower copy removed")
    assert int(got[1][qi, pos]) == low + 10000 and float(got[0][qi, pos]) == float(before[0][qi, pos])
    same(c_search(idx, qg, k, 3, allow), after, "ties workgroups=3")


def test_rising_every_other_row_removed(gpu):
    q, g = _adversarial("rising")
    qg = q.to(gpu)
    idx = fresh_index(gpu, g, normalize=False)
    k = 10
    sim = dense_product(idx, qg)
    gone = torch.arange(0, ADV_G, 2)
    assert idx.remove(rows=gone.to(gpu)) == gone.numel()
    allow = torch.ones(ADV_G, dtype=torch.bool)
    allow[gone] = False
    ref = MR.masked_topk(sim, allow, k)
    assert ref[1][0].tolist() == list(range(ADV_G - 2, ADV_G - 2 - 2 * k, -2))  # every admitted row of query 0 beats the last
    same(idx.search(qg, k=k, normalize=False), ref, "rising")
    for wg in (1, 0):
        same(c_search(idx, qg, k, wg, allow), ref, "rising workgroups=%d" % wg)


# ------------------------------------------------------------------------------------------------------------ 4. lifecycle
def test_lifecycle_remove_add_pids_compact_state_dict(gpu):
    from textreid_amd import GalleryIndex

    Q, G, k = 5, 4099, 16
    _, te, ie, qu, sim = built(gpu, Q, G)
    pid = OF.randint("gmk:pid", 0, 300, (G,), SEED)
    idx = fresh_index(gpu, ie, pids=pid)
    assert idx.live_count == G and bool(idx.live.all()) and idx.live.dtype == torch.bool and idx.live.shape == (G,)

    # remove: counts, duplicates, idempotence, range
    assert idx.remove(rows=[5, 5, 70, 4098]) == 3
    assert idx.remove(rows=torch.tensor([5, 70, 71])) == 1 and idx.remove(rows=torch.tensor([5, 70, 71], device=gpu)) == 0
    assert idx.live_count == G - 4 and len(idx) == G and idx.rows.shape[0] == G
    with pytest.raises(ValueError, match="rows must be in"):
        idx.remove(rows=[G])
    allow = torch.ones(G, dtype=torch.bool)
    allow[[5, 70, 71, 4098]] = False
    assert torch.equal(idx.live.cpu(), allow)

    # remove(pids=...) = removing the rows of those pids
    some = [int(pid[0]), int(pid[100]), 100000]
    of_pids = torch.isin(pid, torch.tensor(some))
    assert idx.remove(pids=some) == int((of_pids & allow).sum())
    allow &= ~of_pids
    assert idx.remove(pids=torch.tensor(some)) == 0 and torch.equal(idx.live.cpu(), allow)
    same(idx.search(qu, k=k, normalize=False), MR.masked_topk(sim, allow, k), "after removals")

    # add after remove: new rows are live and numbered from len
    more = OF.randn("gmk:more", (40, 256), SEED)
    assert idx.add(more.to(gpu), pids=torch.arange(40) + 5000) == G
    n = G + 40
    allow = torch.cat([allow, torch.ones(40, dtype=torch.bool)])
    assert len(idx) == n and idx.live_count == int(allow.sum()) and torch.equal(idx.live.cpu(), allow)
    sim2 = dense_product(idx, qu)
    assert torch.equal(sim2[:, :G], sim)
    ref2 = MR.masked_topk(sim2, allow, k)
    same(idx.search(qu, k=k, normalize=False), ref2, "add after remove")
    # tombstones and a mask together
    m = coin("life_mask", n)
    same(idx.search(qu, k=k, normalize=False, mask=m.to(gpu)), MR.masked_topk(sim2, allow & m, k), "tombstones & mask")

    # state_dict keeps the tombstones; one without "live" loads as all-live
    sd = idx.state_dict()
    assert sd["live"].dtype == torch.bool and torch.equal(sd["live"].cpu(), allow)
    other = GalleryIndex()
    other.load_state_dict(sd)
    assert len(other) == n and other.live_count == idx.live_count and torch.equal(other.live, idx.live)
    same(other.search(qu, k=k, normalize=False), ref2, "state_dict round trip")
    old = {key: v for key, v in sd.items() if key != "live"}
    alive = GalleryIndex()
    alive.load_state_dict(old)
    assert alive.live_count == n and bool(alive.live.all()) and alive.state_dict()["live"] is None
    same(alive.search(qu, k=k, normalize=False), MR.masked_topk(sim2, torch.ones(n, dtype=torch.bool), k), "no live key")

    # k beyond live_count
    tiny = fresh_index(gpu, ie[:12])
    assert tiny.remove(rows=list(range(8))) == 8
    with pytest.raises(ValueError, match="live_count = 4"):
        tiny.search(qu, k=5, normalize=False)
    v, r = tiny.search(qu, k=4, normalize=False)
    assert sorted(r[0].tolist()) == [8, 9, 10, 11]
    v, r = tiny.search(qu, k=5, normalize=False, mask=torch.ones(12, dtype=torch.bool, device=gpu))  # with a mask: short rows
    assert r[:, 4].tolist() == [-1] * Q and bool((v[:, 4] == NEG).all()) and bool((r[:, :4] >= 8).all())

    # compact
    keep = torch.nonzero(allow).reshape(-1)
    new_of = idx.compact()
    want = torch.full((n,), -1, dtype=torch.int64)
    want[keep] = torch.arange(keep.numel())
    assert new_of.is_cuda and new_of.dtype == torch.int64 and torch.equal(new_of.cpu(), want)
    assert len(idx) == keep.numel() and idx.live_count == len(idx) and bool(idx.live.all())
    all_rows = torch.cat([ie, more])
    all_pids = torch.cat([pid, torch.arange(40) + 5000])
    again = fresh_index(gpu, all_rows[keep], pids=all_pids[keep])
    assert torch.equal(idx.rows.view(torch.int32), again.rows.view(torch.int32))
    assert torch.equal(idx.rows_p16.view(torch.int32), again.rows_p16.view(torch.int32))
    assert torch.equal(idx.pids, again.pids)
    a, b = idx.search(qu, k=k, normalize=False), again.search(qu, k=k, normalize=False)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    same((a[0], new_of.new_tensor(keep.tolist())[a[1]]), ref2, "compacted rows map back to the old result")
    assert idx.state_dict()["live"] is None
    assert torch.equal(idx.compact().cpu(), torch.arange(len(idx)))  # nothing to drop: the identity map
    assert idx.add(more[:3].to(gpu), pids=torch.tensor([1, 2, 3])) == keep.numel() and idx.live_count == keep.numel() + 3


def test_unmasked_path_is_kept_for_an_index_without_tombstones(gpu, monkeypatch):
    """never removed and no mask: trid_index_search_p16, no pack launch; after compact() again"""
    import textreid_amd.index as IX

    _, te, ie, qu, sim = built(gpu, 5, 4099)
    idx = fresh_index(gpu, ie)
    names = []
    real = IX.call

    def logging(name, *args):
        names.append(name)
        return real(name, *args)

    monkeypatch.setattr(IX, "call", logging)
    idx.search(qu, k=5, normalize=False)
    assert "trid_index_search_p16" in names and not any("mask" in n for n in names), names
    idx.remove(rows=[1])
    del names[:]
    idx.search(qu, k=5, normalize=False)
    idx.search(qu, k=5, normalize=False)
    assert names.count("trid_index_search_masked_p16") == 2 and names.count("trid_index_pack_mask_u32") == 1, names  # the words are cached
    idx.compact()
    del names[:]
    idx.search(qu, k=5, normalize=False)
    assert "trid_index_search_p16" in names and not any("mask" in n for n in names), names


# -------------------------------------------------------------------------------------------------------------- 5. Q > 32
def test_more_than_32_queries_run_in_masked_panels(gpu):
    Q, G, k = 70, 8192 + 69, 10
    te, ie = raw(Q, G)
    idx = fresh_index(gpu, ie)
    qu = unit_rows(te.to(gpu))
    sim = dense_product(idx, qu)
    dead = coin("big_dead", G, 10)
    assert idx.remove(rows=torch.nonzero(dead).reshape(-1)) == int(dead.sum())
    m = coin("big_mask", G)
    same(idx.search(te.to(gpu), k=k, mask=m.to(gpu)), MR.masked_topk(sim, m & ~dead, k), "Q = 70, tombstones & mask")
    same(idx.search(te.to(gpu), k=k), MR.masked_topk(sim, ~dead, k), "Q = 70, tombstones")


# ---------------------------------------------------------------------------------------------------------------- 6. capture
def test_masked_search_records_and_replays(gpu):
    Q, G, k = 4, 4099, 10
    _, te5, ie, qu5, sim5 = built(gpu, 5, G)
    idx = fresh_index(gpu, ie)
    idx.remove(rows=torch.nonzero(coin("cap_dead", G, 10)).reshape(-1))
    qa = OF.randn("gmk:cap_a", (Q, 256), SEED).to(gpu)
    qb = OF.randn("gmk:cap_b", (Q, 256), SEED).to(gpu)
    ma = coin("cap_ma", G).to(gpu)
    mb = coin("cap_mb", G).to(gpu)
    buf, m = qa.clone(), ma.clone()
    idx.search(buf, k=k, mask=m)  # (allocates the cached workspace and the word buffer)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        vals, rows = idx.search(buf, k=k, mask=m)
    g.replay()
    torch.cuda.synchronize()
    va, ra = idx.search(qa, k=k, mask=ma)
    assert torch.equal(vals, va) and torch.equal(rows, ra)
    buf.copy_(qb)
    m.copy_(mb)
    g.replay()
    torch.cuda.synchronize()
    got_v, got_r = vals.clone(), rows.clone()
    vb, rb = idx.search(qb, k=k, mask=mb)
    assert torch.equal(got_v, vb) and torch.equal(got_r, rb)
    assert not torch.equal(rb, ra)
    # the mask alone changes the answer too: queries a with mask b
    buf.copy_(qa)
    g.replay()
    torch.cuda.synchronize()
    vc, rc = idx.search(qa, k=k, mask=mb)
    assert torch.equal(vals, vc) and torch.equal(rows, rc) and not torch.equal(rc, ra)
    allowed = (mb & idx.live).cpu()
    assert bool(allowed[rc.cpu()].all())


# ------------------------------------------------------------------------------------------------------ 7. against the oracle
def test_masked_search_matches_oracle(gpu):
    # seed 9: every gap among the top k + 1 ALLOWED oracle values of every query is >= 2.1e-5 for this shape, mask and set of
    # removed rows (checked on the CPU when the test was written: the smallest gap is 2.8e-4)
    Q, G, k, seed = 5, 4099, 10, 9
    te = OF.randn("gmk:oq%d" % Q, (Q, 256), seed)
    ie = OF.randn("gmk:og%d" % G, (G, 256), seed)
    allow = OF.randint("gmk:omask", 0, 2, (G,), seed).bool()
    dead = OF.randint("gmk:odead", 0, 10, (G,), seed) == 0
    ok = allow & ~dead
    sim = OE.similarity(te, ie).clone()
    sim[:, ~ok] = NEG
    top = torch.topk(sim, k + 1, dim=1).values
    assert float((top[:, :-1] - top[:, 1:]).min()) >= 2.1e-5
    rv, ri = torch.topk(sim, k, dim=1)
    idx = fresh_index(gpu, ie)
    assert idx.remove(rows=torch.nonzero(dead).reshape(-1)) == int(dead.sum())
    got = idx.search(te.to(gpu), k=k, mask=allow.to(gpu))
    assert torch.equal(got[1].cpu(), ri)
    assert torch.allclose(got[0].cpu(), rv, atol=2e-6, rtol=0), float((got[0].cpu() - rv).abs().max())
