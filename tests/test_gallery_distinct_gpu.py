"""GalleryIndex.search_pids on the GPU: the exact top-k over distinct pids in the one-pass kernel.  The comparator is exact, as in
test_gallery_mask_gpu.py: the dense trid_gemm_p16 product of the index's own P16 operands (gallery_support.dense_product), then
gallery_distinct_ref.distinct_topk (stable descending sort, the first allowed row of every group, -inf rows reported as -1).  Values
and rows are compared bit for bit."""

import pytest
import torch

pytestmark = pytest.mark.gpu

import gallery_distinct_ref as DR  # noqa: E402
import gallery_mask_ref as MR  # noqa: E402
import oracle.fill as OF  # noqa: E402
from gallery_support import c_search, dense_product, fresh_index, gpu, Inputs, same_values as same, unit_rows  # noqa: E402,F401

SEED = 8
SHAPES = [(1, 1, 1), (2, 33, 10), (5, 63, 5), (32, 64, 16), (7, 65, 10), (5, 4099, 16), (17, 20037, 10)]
ADV_G = 20037
NEG = float("-inf")
IN = Inputs("gds:", SEED, raw_tag="gmk:")  # (the raw queries and galleries carry the names of test_gallery_mask_gpu.py; no cache entry is shared)
coin = IN.coin_keep


def relabel(pids):
    """other int32 labels with the same equalities (negative ones among them): only equality may matter to the C entry"""
    from textreid_amd.index import group_ids

    return group_ids(pids) * -7 + 3


def built(gpu, Q, G):
    """the seed-8 queries and gallery of the shape (on the device too), an index over the gallery WITHOUT pids that no test modifies,
    the dense similarities: computed once, shared, left unchanged"""
    idx, te, ie, qu, sim = IN.built(gpu, Q, G)
    return idx, te.to(gpu), ie.to(gpu), qu, sim


def ones(G):
    return torch.ones(G, dtype=torch.bool)


# ------------------------------------------------------------------------------------------ 1. pid patterns, both entries
def pid_patterns(G, k):
    ar = torch.arange(G)
    pats = {"all distinct": ar * 3 - 7, "one pid": torch.full((G,), 1 << 33), "row // 4": ar // 4 + (1 << 31),
            "random G/3": OF.randint("gds:pid%d" % G, 0, max(G // 3, 1), (G,), SEED).long() - 5}
    for P in (k - 1, k, k + 1):
        if P >= 1:
            pats["row %% %d" % P] = ar % P
    return pats


@pytest.mark.parametrize("Q,G,k", SHAPES)
def test_search_pids_equals_distinct_topk_of_the_dense_product(gpu, Q, G, k):
    plain_idx, te, ieg, qu, sim = built(gpu, Q, G)
    plain = plain_idx.search(te, k=k)
    same(plain, MR.masked_topk(sim, ones(G), k), "search")
    pats = pid_patterns(G, k)
    assert len(pats) == (7 if k > 1 else 6)
    for name, pid in pats.items():
        idx = fresh_index(gpu, ieg, pids=pid)
        ref = DR.distinct_topk(sim, pid, ones(G), k)
        n_pid = len(set(pid.tolist()))
        if n_pid < k:  # short rows: the real results first, then (-inf, -1)
            assert bool((ref[1][:, n_pid:] == -1).all()) and bool((ref[0][:, n_pid:] == NEG).all()) and bool((ref[1][:, :n_pid] >= 0).all())
        got = idx.search_pids(te, k=k)
        same(got, ref, "search_pids %s" % name, pid)
        same(idx.search_pids(qu, k=k, normalize=False), ref, "search_pids, unit queries, %s" % name, pid)
        if name == "all distinct":  # bit for bit the search over rows
            assert torch.equal(got[0], plain[0]) and torch.equal(got[1], plain[1])
        gid = relabel(pid)
        for wg in (0, 1, 3):
            same(c_search(idx, qu, k, wg, gid=gid), ref, "%s workgroups=%d" % (name, wg))
        same(c_search(idx, qu, k, 3, ones(G), gid=gid), ref, "%s workgroups=3, all-ones words" % name)
        same(idx.search(te, k=k), (plain[0].cpu(), plain[1].cpu()), "search on the index that answered search_pids")
    same(plain_idx.search(te, k=k), (plain[0].cpu(), plain[1].cpu()), "search again")


# ---------------------------------------------------------------------------------------------------------- 2. the crowd
def test_a_crowd_of_one_person_leaves_room_for_fifteen_others(gpu):
    Q, G, k = 5, 4099, 16
    _, te, ieg, qu, sim = built(gpu, Q, G)
    crowd = torch.sort(sim[0], descending=True, stable=True).indices[:40]
    pid = torch.arange(G) + 10
    pid[crowd] = 5
    ref = DR.distinct_topk(sim, pid, ones(G), k)
    # what a caller had before: the best 16 rows, de-duplicated afterwards - ONE result for query 0
    rv, rr = MR.masked_topk(sim, ones(G), k)
    keep0 = [int(r) for i, r in enumerate(rr[0]) if int(pid[r]) not in [int(pid[x]) for x in rr[0][:i]]]
    assert keep0 == [int(crowd[0])] and keep0 != ref[1][0].tolist()
    assert int(ref[1][0, 0]) == int(crowd[0]) and not bool(torch.isin(ref[1][0, 1:], crowd).any()) and bool((ref[1][0] >= 0).all())
    idx = fresh_index(gpu, ieg, pids=pid)
    same(idx.search_pids(te, k=k), ref, "crowd", pid)
    for wg in (0, 1, 3):
        same(c_search(idx, qu, k, wg, gid=relabel(pid)), ref, "crowd workgroups=%d" % wg)


# ------------------------------------------------------------------------------------------------------------- 3. ties
def _tied_gallery():
    """rows 10000 .. 19999 are exact copies of rows 0 .. 9999 (bit-equal similarities): a copy lies 156 step tiles behind its
    original and, with 3 workers over the 314 tiles (cuts at rows 6656 and 13376), always in another worker"""
    q = OF.randn("gix:advq", (5, 256), SEED)
    g = OF.randn("gix:advg:ties", (ADV_G, 256), SEED)
    g[10000:20000] = g[:10000]
    return q / q.norm(dim=1, keepdim=True), g / g.norm(dim=1, keepdim=True)


def test_ties_go_to_the_lower_row_inside_a_pid_and_between_pids(gpu):
    q, g = _tied_gallery()
    qg, k = q.to(gpu), 10
    ar = torch.arange(ADV_G)
    together = torch.where(ar < 20000, ar % 10000, ar)  # a copy has the pid of its original
    apart = ar.clone()                                  # every row its own pid
    sim = None
    for name, pid in (("together", together), ("apart", apart)):
        idx = fresh_index(gpu, g.to(gpu), pids=pid, normalize=False)
        if sim is None:
            sim = dense_product(idx, qg)
            assert torch.equal(sim[:, :10000], sim[:, 10000:20000])
        ref = DR.distinct_topk(sim, pid, ones(ADV_G), k)
        if name == "together":  # the original represents the pair: no copy is returned, and the values are those of the row search
            assert bool(((ref[1] < 10000) | (ref[1] >= 20000)).all())
            assert int((ref[1] < 10000).sum()) >= 5
        else:  # both are returned, the original first
            pairs = (ref[1][:, :-1] < 10000) & (ref[1][:, 1:] == ref[1][:, :-1] + 10000)
            assert int(pairs.sum()) >= 5
        same(idx.search_pids(qg, k=k, normalize=False), ref, "ties %s" % name, pid)
        for wg in (0, 1, 3):
            same(c_search(idx, qg, k, wg, gid=relabel(pid)), ref, "ties %s workgroups=%d" % (name, wg))


# ------------------------------------------------------------------------------------------------------ 4. composition
def mask_patterns(Q, G, k):
    """{name: allow bool [G]}: the patterns of test_gallery_mask_gpu.py, restated"""
    tiles, nwords = (G + 63) // 64, (G + 31) // 32
    ar = torch.arange(G)
    pats = {"ones": ones(G), "random half": coin("half%d" % G, G), "none": torch.zeros(G, dtype=torch.bool)}
    if nwords >= 2:
        w = nwords // 2 if nwords > 2 else 0
        pats["one word zero"] = (ar >> 5) != w
    if tiles >= 2:
        t = tiles // 2 if tiles > 2 else 0
        pats["one step tile zero"] = (ar >> 6) != t
        lo, hi = tiles // 3, 2 * tiles // 3  # worker 1 of 3 owns the step tiles [T / 3, 2 T / 3)
        pats["worker 1 of 3 zero"] = ((ar >> 6) < lo) | ((ar >> 6) >= hi)
        pats["only the ragged last tile"] = (ar >> 6) == tiles - 1
    if k >= 2:
        few = torch.zeros(G, dtype=torch.bool)
        few[torch.linspace(0, G - 1, k - 1).long()] = True
        pats["fewer than k"] = few
    return pats


@pytest.mark.parametrize("Q,G,k", [(2, 33, 10), (7, 65, 10), (5, 4099, 16)])
def test_search_pids_with_a_mask(gpu, Q, G, k):
    _, te, ieg, qu, sim = built(gpu, Q, G)
    pid = torch.arange(G) // 4 * 11 - 40
    idx = fresh_index(gpu, ieg, pids=pid)
    before = idx.search(te, k=k)
    for name, allow in mask_patterns(Q, G, k).items():
        ref = DR.distinct_topk(sim, pid, allow, k)
        same(idx.search_pids(te, k=k, mask=allow.to(gpu)), ref, "search_pids(mask) %s" % name, pid)
        same(idx.search_pids(qu, k=k, normalize=False, mask=allow.to(torch.uint8).to(gpu)), ref, "uint8 mask, unit queries, %s" % name, pid)
        for wg in (1, 3):
            same(c_search(idx, qu, k, wg, allow, gid=relabel(pid)), ref, "%s workgroups=%d" % (name, wg))
    assert idx.live_count == G
    after = idx.search(te, k=k)
    assert torch.equal(before[0], after[0]) and torch.equal(before[1], after[1])


def test_removing_a_representative_and_removing_a_pid(gpu):
    Q, G, k = 5, 4099, 10
    _, te, ieg, qu, sim = built(gpu, Q, G)
    a, b, c, d = [int(x) for x in torch.sort(sim[0], descending=True, stable=True).indices[:4]]
    pid = torch.arange(G) + 100
    pid[[a, b, c]] = 7  # the three best rows of query 0 are one person
    idx = fresh_index(gpu, ieg, pids=pid)
    allow = ones(G)
    got = idx.search_pids(qu, k=k, normalize=False)
    same(got, DR.distinct_topk(sim, pid, allow, k), "nothing removed", pid)
    assert got[1][0, :2].tolist() == [a, d] and got[2][0, :2].tolist() == [7, d + 100]
    # the representative goes: the person's next row takes its place
    assert idx.remove(rows=[a]) == 1
    allow[a] = False
    got = idx.search_pids(qu, k=k, normalize=False)
    same(got, DR.distinct_topk(sim, pid, allow, k), "representative removed", pid)
    assert got[1][0, :2].tolist() == [b, d] and got[2][0, 0].item() == 7
    # tombstones and a mask together: the mask takes b away too
    m = coin("rep_mask", G)
    m[b], m[c], m[d] = False, True, True
    got = idx.search_pids(qu, k=k, normalize=False, mask=m.to(gpu))
    same(got, DR.distinct_topk(sim, pid, allow & m, k), "tombstones & mask", pid)
    assert got[1][0, :2].tolist() == [c, d]
    for wg in (1, 3):
        same(c_search(idx, qu, k, wg, allow & m, gid=relabel(pid)), DR.distinct_topk(sim, pid, allow & m, k), "tombstones & mask workgroups=%d" % wg)
    # every row of the person goes: the person is absent
    assert idx.remove(pids=[7]) == 2
    allow[[b, c]] = False
    got = idx.search_pids(qu, k=k, normalize=False)
    same(got, DR.distinct_topk(sim, pid, allow, k), "pid removed", pid)
    assert int(got[1][0, 0]) == d and not bool((got[2] == 7).any())


# -------------------------------------------------------------------------------------------------------------- 5. state
def test_group_ids_follow_add_compact_and_state_dict(gpu):
    from textreid_amd import GalleryIndex

    Q, G, k = 5, 4099, 16
    _, te, ieg, qu, sim = built(gpu, Q, G)
    pid = OF.randint("gds:state_pid", 0, 1000, (G,), SEED).long() * (1 << 32) - 3
    first = 3000
    idx = GalleryIndex()
    idx.add(ieg[:first], pids=pid[:first])
    idx.search_pids(qu, k=k, normalize=False)  # (the group ids of the first 3000 rows are cached now)
    assert idx.add(ieg[first:], pids=pid[first:]) == first  # pids that overlap the earlier ones
    assert len(set(pid[first:].tolist()) & set(pid[:first].tolist())) > 100
    ref = DR.distinct_topk(sim, pid, ones(G), k)
    same(idx.search_pids(qu, k=k, normalize=False), ref, "after add", pid)
    # remove leaves the ids valid
    dead = coin("state_dead", G, 5)
    assert idx.remove(rows=torch.nonzero(dead).reshape(-1)) == int(dead.sum())
    ref_live = DR.distinct_topk(sim, pid, ~dead, k)
    same(idx.search_pids(qu, k=k, normalize=False), ref_live, "after remove", pid)
    # state_dict round trip (tombstones included)
    other = GalleryIndex()
    other.load_state_dict(idx.state_dict())
    same(other.search_pids(qu, k=k, normalize=False), ref_live, "state_dict round trip", pid)
    other.load_state_dict(fresh_index(gpu, ieg[:100], pids=torch.arange(100) // 2).state_dict())  # other contents in the same object
    same(other.search_pids(qu, k=k, normalize=False), DR.distinct_topk(sim[:, :100], torch.arange(100) // 2, ones(100), k), "second load")
    # compact: new row numbers, new ids
    new_of = idx.compact().cpu()
    keep = torch.nonzero(~dead).reshape(-1)
    assert len(idx) == keep.numel() and torch.equal(idx.pids.cpu(), pid[keep])
    got = idx.search_pids(qu, k=k, normalize=False)
    same((got[0], torch.where(got[1] >= 0, keep.to(gpu)[got[1].clamp(min=0)], got[1])), ref_live, "compacted rows map back")
    assert torch.equal(got[2].cpu(), torch.where(ref_live[1] >= 0, pid[ref_live[1].clamp(min=0)], ref_live[1]))
    assert torch.equal(new_of[keep], torch.arange(keep.numel()))
    # growth: an index that started small
    small = GalleryIndex(capacity=64)
    small.add(ieg[:64], pids=pid[:64])
    small.search_pids(qu, k=k, normalize=False)
    small.add(ieg[64:], pids=pid[64:])
    same(small.search_pids(qu, k=k, normalize=False), ref, "after growth", pid)


# -------------------------------------------------------------------------------------------------------------- 6. Q > 32
def test_forty_queries_run_in_panels(gpu):
    Q, G, k = 40, 4099, 10
    _, te, ieg, qu, sim = built(gpu, Q, G)
    pid = torch.arange(G) // 4
    idx = fresh_index(gpu, ieg, pids=pid)
    same(idx.search_pids(te, k=k), DR.distinct_topk(sim, pid, ones(G), k), "Q = 40", pid)
    m = coin("q40_mask", G)
    same(idx.search_pids(te, k=k, mask=m.to(gpu)), DR.distinct_topk(sim, pid, m, k), "Q = 40, mask", pid)


# ------------------------------------------------------------------------------------------------------------ 7. capture
def test_search_pids_records_and_replays(gpu):
    Q, G, k = 4, 4099, 10
    _, te5, ieg, qu5, sim5 = built(gpu, 5, G)
    pid = torch.arange(G) // 4
    idx = fresh_index(gpu, ieg, pids=pid)
    idx.remove(rows=torch.nonzero(coin("cap_dead", G, 10)).reshape(-1))
    qa = OF.randn("gds:cap_a", (Q, 256), SEED).to(gpu)
    qb = OF.randn("gds:cap_b", (Q, 256), SEED).to(gpu)
    ma, mb = coin("cap_ma", G).to(gpu), coin("cap_mb", G).to(gpu)
    buf, m = qa.clone(), ma.clone()
    idx.search_pids(buf, k=k, mask=m)  # (builds the group ids, the workspace and the word buffer)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):  # (a host read inside would end the capture with an error)
        vals, rows, pids = idx.search_pids(buf, k=k, mask=m)
    g.replay()
    torch.cuda.synchronize()
    va, ra, pa = idx.search_pids(qa, k=k, mask=ma)
    assert torch.equal(vals, va) and torch.equal(rows, ra) and torch.equal(pids, pa)
    buf.copy_(qb)
    m.copy_(mb)
    g.replay()
    torch.cuda.synchronize()
    got = (vals.clone(), rows.clone(), pids.clone())
    vb, rb, pb = idx.search_pids(qb, k=k, mask=mb)
    assert torch.equal(got[0], vb) and torch.equal(got[1], rb) and torch.equal(got[2], pb) and not torch.equal(rb, ra)
    allow = (mb & idx.live).cpu()
    same(got, DR.distinct_topk(dense_product(idx, unit_rows(qb)), pid, allow, k), "replay against the reference", pid)
    # the mask alone changes the answer too: queries a with mask b
    buf.copy_(qa)
    g.replay()
    torch.cuda.synchronize()
    vc, rc, pc = idx.search_pids(qa, k=k, mask=mb)
    assert torch.equal(vals, vc) and torch.equal(rows, rc) and torch.equal(pids, pc) and not torch.equal(rc, ra)
    assert bool(allow[rc.cpu()].all())
