"""GalleryIndex.shortlist on the GPU.  The comparator is the dense trid_gemm_p16 product of the index's OWN operands (P16 gallery as A,
the zero-padded query panel as B, unit scale: gallery_support.dense_product) read back to the host, then topk_deep_ref over the allowed rows (gallery_mask_ref's
masked_topk turns a real -inf into an absent row, so it only serves where no score is -inf: it is used as a cross-check).  Nothing
here needs a tolerance: values are compared as bit patterns, rows exactly."""

import pytest
import torch

pytestmark = pytest.mark.gpu

import gallery_mask_ref as MR  # noqa: E402
import oracle.fill as OF  # noqa: E402
import topk_deep_ref as TR  # noqa: E402
from gallery_support import dense_product, fresh_index, gpu, Inputs, same_bits as same, unit_rows  # noqa: E402,F401

SEED = 12
IN = Inputs("gsl:", SEED)
coin, gallery, queries, shared_index = IN.coin_one_in, IN.gallery, IN.queries, IN.shared_index  # (a shared index is never modified by a test)


def reference(sim, k, allow=None):
    vals, rows = TR.topk(sim.numpy(), k, None if allow is None else allow.numpy())
    if not bool(torch.isinf(sim).any()):  # (the older host comparator says the same wherever no score is -inf)
        mv, mr = MR.masked_topk(sim, torch.ones(sim.shape[1], dtype=torch.bool) if allow is None else allow, k)
        assert TR.same((mv.numpy(), mr.numpy()), (vals, rows))
    return vals, rows


# ------------------------------------------------------------------------------------------------------------------ shapes
@pytest.mark.parametrize("G", [20, 65, 2000, 20037])
def test_shortlist_equals_the_dense_product(gpu, G):
    idx = shared_index(gpu, G)
    for Q in (1, 5, 32, 40):
        qu = queries(gpu, Q)
        sim = dense_product(idx, qu)
        for k in (17, 64, 100, 1024):
            if k > G:
                with pytest.raises(ValueError, match="shortlist: k must be"):
                    idx.shortlist(qu, k=k, normalize=False)
                continue
            got = idx.shortlist(qu, k=k, normalize=False)
            assert got[0].shape == (Q, k) and got[1].dtype == torch.int64
            same(got, reference(sim, k), "G=%d Q=%d k=%d" % (G, Q, k))
    # raw queries: normalised by the same kernel search uses
    raw = OF.randn("gsl:raw", (5, 256), SEED).to(gpu)
    k = min(G, 100)
    same(idx.shortlist(raw, k=k), reference(dense_product(idx, unit_rows(raw)), k), "normalize=True")
    assert idx.live_count == G


def test_exact_duplicate_rows_come_back_in_insertion_order(gpu):
    base = gallery(2000)[:500]
    idx = fresh_index(gpu, torch.cat([base, base, base], dim=0))  # row r, r + 500, r + 1000 are one image
    qu = queries(gpu, 5)
    sim = dense_product(idx, qu)
    assert torch.equal(sim[:, :500], sim[:, 500:1000]) and torch.equal(sim[:, :500], sim[:, 1000:])
    vals, rows = idx.shortlist(qu, k=99, normalize=False)
    same((vals, rows), reference(sim, 99))
    r = rows.cpu().view(5, 33, 3)
    assert bool((r[:, :, 1] == r[:, :, 0] + 500).all()) and bool((r[:, :, 2] == r[:, :, 0] + 1000).all())


# ------------------------------------------------------------------------------------------------------------------ search
def test_shortlist_up_to_16_equals_search_bit_for_bit(gpu):
    G = 20037
    idx = fresh_index(gpu, gallery(G))
    raw = OF.randn("gsl:raw_s", (40, 256), SEED).to(gpu)

    def agree(mask=None):
        for Q in (5, 32, 40) if (mask is not None or idx._dead) else (5, 32):  # (Q > 32 unmasked: search takes the large-batch route)
            for k in (10, 16):
                a = idx.search(raw[:Q], k=k, mask=mask)
                b = idx.shortlist(raw[:Q], k=k, mask=mask)
                assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1], b[1]), (Q, k)

    agree()
    agree(coin("s_mask", G).to(gpu))
    best = idx.search(raw[:32], k=16)[1].reshape(-1)
    assert idx.remove(rows=torch.unique(best)) > 0
    agree()
    agree(coin("s_mask2", G).to(gpu))


# ------------------------------------------------------------------------------------------------------------------ tombstones and masks
def test_tombstones_and_masks(gpu):
    G, Q, k = 2000, 5, 100
    pids = OF.randint("gsl:pids", 0, 300, (G,), SEED)
    idx = fresh_index(gpu, gallery(G), pids=pids)
    qu = queries(gpu, Q)
    sim = dense_product(idx, qu)
    allow = torch.ones(G, dtype=torch.bool)
    # the current best row of every query
    best = idx.shortlist(qu, k=k, normalize=False)[1][:, 0].cpu()
    assert idx.remove(rows=best) == int(torch.unique(best).numel())
    allow[best] = False
    got = idx.shortlist(qu, k=k, normalize=False)
    same(got, reference(sim, k, allow), "best rows removed")
    assert not bool(torch.isin(got[1].cpu(), best).any())
    # by pid
    some = [3, 17, 250]
    of_pids = torch.isin(pids, torch.tensor(some))
    idx.remove(pids=some)
    allow &= ~of_pids
    same(idx.shortlist(qu, k=k, normalize=False), reference(sim, k, allow), "pids removed")
    # masks: all, none, fewer than k - alone they compose with the tombstones (live & mask)
    ones = torch.ones(G, dtype=torch.bool)
    same(idx.shortlist(qu, k=k, normalize=False, mask=ones.to(gpu)), reference(sim, k, allow), "mask all")
    none = idx.shortlist(qu, k=k, normalize=False, mask=torch.zeros(G, dtype=torch.uint8, device=gpu))
    assert bool((none[1] == -1).all()) and bool(torch.isneginf(none[0]).all())
    few = torch.zeros(G, dtype=torch.bool)
    few[OF.randint("gsl:few", 0, G, (k - 10,), SEED)] = True
    n_ok = int((few & allow).sum())
    assert 0 < n_ok < k
    got = idx.shortlist(qu, k=k, normalize=False, mask=few.to(gpu))
    same(got, reference(sim, k, few & allow), "fewer than k allowed")
    assert bool((got[1][:, n_ok:] == -1).all()) and bool((got[1][:, :n_ok] >= 0).all())
    m = coin("tm_mask", G)
    same(idx.shortlist(qu, k=k, normalize=False, mask=m.to(gpu)), reference(sim, k, m & allow), "tombstones & mask")
    # k beyond the live rows without a mask is refused on the host; with a mask it ends in (-inf, -1)
    idx.remove(rows=torch.nonzero(~few).reshape(-1))
    assert idx.live_count == n_ok
    with pytest.raises(ValueError, match="shortlist: k must be <= live_count"):
        idx.shortlist(qu, k=k, normalize=False)
    same(idx.shortlist(qu, k=n_ok, normalize=False), reference(sim, n_ok, few & allow), "k == live_count")
    same(idx.shortlist(qu, k=k, normalize=False, mask=ones.to(gpu)), reference(sim, k, few & allow), "k > live_count under a mask")
    # an index without tombstones on the same storage pattern: a mask alone
    clean = shared_index(gpu, G)
    same(clean.shortlist(qu, k=k, normalize=False, mask=m.to(gpu)), reference(dense_product(clean, qu), k, m), "mask alone")


# ------------------------------------------------------------------------------------------------------------------ storage changes
def test_add_compact_and_state_dict(gpu):
    from textreid_amd import GalleryIndex

    rows = gallery(2000)
    idx = fresh_index(gpu, rows[:300])
    qu = queries(gpu, 5)
    k = 64
    same(idx.shortlist(qu, k=k, normalize=False), reference(dense_product(idx, qu), k), "first")
    held = idx._ws["scores"].shape[0]
    idx.add(rows[300:].to(gpu))  # growth past the cached score buffer
    assert len(idx) == 2000 and len(idx) > held
    sim = dense_product(idx, qu)
    same(idx.shortlist(qu, k=k, normalize=False), reference(sim, k), "after add")
    assert idx._ws["scores"].shape[0] >= 2000
    gone = coin("sc_gone", 2000, 3)
    idx.remove(rows=torch.nonzero(gone).reshape(-1))
    same(idx.shortlist(qu, k=k, normalize=False), reference(sim, k, ~gone), "after remove")
    sd = idx.state_dict()
    new_of = idx.compact().cpu()
    old_of = torch.nonzero(~gone).reshape(-1)
    assert len(idx) == int((~gone).sum()) and torch.equal(new_of[old_of], torch.arange(old_of.numel()))
    got = idx.shortlist(qu, k=k, normalize=False)
    same(got, reference(dense_product(idx, qu), k), "after compact")
    assert torch.equal(old_of[got[1].cpu()], torch.from_numpy(reference(sim, k, ~gone)[1]))  # the same rows under their old numbers
    back = GalleryIndex()
    back.load_state_dict(sd)
    assert len(back) == 2000 and back.live_count == len(idx)
    same(back.shortlist(qu, k=k, normalize=False), reference(dense_product(back, qu), k, ~gone), "state_dict round trip")


# ------------------------------------------------------------------------------------------------------------------ capture
def test_shortlist_records_and_replays(gpu):
    G, Q, k = 20037, 4, 100
    idx = fresh_index(gpu, gallery(G))
    idx.remove(rows=torch.nonzero(coin("cap_dead", G, 10)).reshape(-1))
    qa = OF.randn("gsl:cap_a", (Q, 256), SEED).to(gpu)
    qb = OF.randn("gsl:cap_b", (Q, 256), SEED).to(gpu)
    ma, mb = coin("cap_ma", G).to(gpu), coin("cap_mb", G).to(gpu)
    buf, m = qa.clone(), ma.clone()
    idx.shortlist(buf, k=k, mask=m)  # (allocates the score buffer, the workspaces and the word buffer)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        vals, rows = idx.shortlist(buf, k=k, mask=m)
    g.replay()
    torch.cuda.synchronize()
    va, ra = idx.shortlist(qa, k=k, mask=ma)
    assert torch.equal(vals, va) and torch.equal(rows, ra)
    buf.copy_(qb)
    m.copy_(mb)
    g.replay()
    torch.cuda.synchronize()
    got_v, got_r = vals.clone(), rows.clone()
    vb, rb = idx.shortlist(qb, k=k, mask=mb)
    assert torch.equal(got_v, vb) and torch.equal(got_r, rb)
    assert not torch.equal(rb, ra)
    live = idx.live.cpu()
    same((got_v, got_r), reference(dense_product(idx, unit_rows(qb)), k, mb.cpu() & live), "replay against the host reference")
    # a recording with another k than any eager call used (another instantiation of the select kernel): still nothing but launches
    g16 = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g16):
        v16, r16 = idx.shortlist(buf, k=16, mask=m)
    g16.replay()
    torch.cuda.synchronize()
    same((v16, r16), reference(dense_product(idx, unit_rows(qb)), 16, mb.cpu() & live), "k = 16 recorded after an eager k = 100")
