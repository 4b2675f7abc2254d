"""Query expansion and database-side augmentation of GalleryIndex / GalleryShards on the GPU: trid_index_blend_rows_f32 alone against
gallery_expand_ref.blend (the whole output buffer compared bitwise, so that nothing outside [M, 256] moves), expand_queries /
search_expanded / search_expanded_pids against the reference built on the dense trid_gemm_p16 product of the index's OWN operands,
augmented against the blend of the index's own lists.  Nothing here needs a tolerance: values are compared as bit patterns, rows
exactly."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import gallery_expand_ref as XR  # noqa: E402
import oracle.fill as OF  # noqa: E402
import topk_deep_ref as TR  # noqa: E402
from gallery_support import dense_product, fresh_index, gpu, Inputs, same_bits as same, unit_rows  # noqa: E402,F401

SEED = 17
CLUSTER_SEED = 15  # (the clustered gallery of test_gallery_rerank_gpu.py: the same names, the same seed)
IN = Inputs("grr:", 13, graph_n=5)  # (the galleries, queries and coins of test_gallery_rerank_gpu.py, by name: the caches are shared with it)
coin, gallery, queries, shared_index = IN.coin_one_in, IN.gallery, IN.queries, IN.shared_index
INT_MAX = 0x7FFFFFFF


def bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def l2(gpu, x):
    """the library's own normalisation of a host float32 array -> a device tensor"""
    from textreid_amd import ops

    return ops.l2norm_rows(torch.from_numpy(np.ascontiguousarray(x)).to(gpu))[0]


# ------------------------------------------------------------------------------------------------------------------ the kernel alone
def _part_lengths(R, n_parts):
    return [R] if n_parts == 1 else [R, R // 2 + 2, R + 5]


_parts = {}


def _part_rows(gpu, R, n_parts):
    """the parts' unit rows on the host and their device copies with the two tables, once per shape"""
    if (R, n_parts) not in _parts:
        lens = _part_lengths(R, n_parts)
        host = [torch.nn.functional.normalize(OF.randn("gxp:part%d_%d_%d" % (R, n_parts, s), (n, 256), SEED), dim=1).numpy() for s, n in enumerate(lens)]
        dev = [torch.from_numpy(h).to(gpu) for h in host]
        tab = torch.tensor([[d.data_ptr() for d in dev], lens], dtype=torch.int64, device=gpu)
        _parts[R, n_parts] = (host, dev, tab)
    return _parts[R, n_parts]


def _kernel_inputs(R, n_parts, M, m, ld_list, seed):
    """ids int64 [M, ld_list] and vals float32 [M, ld_list] with the planted rows (by i % 8; every id also fits int32):
    0: -1 in the first, a middle and the last slot; 1: a list that is all -1; 2: an id equal to the part length first, INT_MAX last;
    3: a part number beyond the table (one part: a row beyond the length); 4: a duplicate id; 5: negative, zero and -inf values on
    present ids.  The columns behind m hold valid ids and weights: reading them would show."""
    rng = np.random.RandomState(seed)
    lens = np.array(_part_lengths(R, n_parts))
    shift = 0 if n_parts == 1 else 21
    part = rng.randint(0, n_parts, size=(M, ld_list))
    row = (rng.randint(0, 1 << 30, size=(M, ld_list)) % lens[part]).astype(np.int64)
    ids = (part.astype(np.int64) << shift) | row
    vals = rng.uniform(-0.2, 1.0, size=(M, ld_list)).astype(np.float32)
    for i in range(M):
        kind = i % 8
        if kind == 0:
            ids[i, [0, m // 2, m - 1]] = -1
        elif kind == 1:
            ids[i, :m] = -1
        elif kind == 2:
            ids[i, 0] = lens[0]  # (part 0, row = its length)
            ids[i, m - 1] = INT_MAX
        elif kind == 3:
            ids[i, 0] = (n_parts << shift) if shift else lens[0] + 7
        elif kind == 4:
            ids[i, m - 1] = ids[i, 0]
        elif kind == 5:
            vals[i, : min(m, 3)] = np.array([-0.5, 0.0, -np.inf], dtype=np.float32)[: min(m, 3)]
    return ids, vals, shift


@pytest.mark.parametrize("n_parts", [1, 3])
@pytest.mark.parametrize("R", [1, 63, 5000])
def test_kernel_equals_the_reference_and_writes_nothing_else(gpu, R, n_parts):
    from textreid_amd import ops
    from textreid_amd.ops import _p

    host, dev, tab = _part_rows(gpu, R, n_parts)
    case = 0
    for M in (1, 31, 33, 300):
        base_h = torch.nn.functional.normalize(OF.randn("gxp:base%d" % M, (M, 256), SEED), dim=1).numpy()
        for m in (1, 5, 8, 32):
            for ld_list in (m, m + 3):
                case += 1
                ids, vals, shift = _kernel_inputs(R, n_parts, M, m, ld_list, 100000 * n_parts + 10 * R + case)
                d_vals = torch.from_numpy(vals).to(gpu)
                d_ids = {8: torch.from_numpy(ids).to(gpu), 4: torch.from_numpy(ids.astype(np.int32)).to(gpu)}
                ld_base = 256 if ld_list == m else 260
                base_buf = np.zeros((M, ld_base), dtype=np.float32)
                base_buf[:, :256] = base_h
                base_buf[:, 256:] = 7.0
                d_base = torch.from_numpy(base_buf).to(gpu)
                for power in (0, 1, 3):
                    for with_base in (True, False):
                        ref = XR.blend(host, ids, vals, m, power, base=base_h if with_base else None, shift=shift)
                        # the buffer: larger than the extent on both sides, a recognisable pattern outside it
                        size = M * 256 + 512
                        want = (0x5A5A0000 + (np.arange(size) & 0xFFFF)).astype(np.uint32)
                        pattern = torch.from_numpy(want.view(np.int32).copy()).to(gpu)
                        want[256 : 256 + M * 256] = ref.reshape(-1).view(np.uint32)
                        for id_bytes in (4, 8):
                            buf = pattern.clone()
                            ops.call("trid_index_blend_rows_f32", _p(tab[0]), _p(tab[1]), n_parts, shift, _p(d_ids[id_bytes]), id_bytes, _p(d_vals),
                                     ld_list, M, m, power, _p(d_base) if with_base else None, ld_base if with_base else 0,
                                     buf.data_ptr() + 1024, ops.stream())
                            got = buf.cpu().numpy().view(np.uint32)
                            bad = np.nonzero(got != want)[0]
                            assert bad.size == 0, "R=%d parts=%d M=%d m=%d ld=%d power=%d base=%s id_bytes=%d: %d words differ, first at %d" % (
                                R, n_parts, M, m, ld_list, power, with_base, id_bytes, bad.size, bad[0])


# ------------------------------------------------------------------------------------------------------------------ expand_queries
def reference_expanded(gpu, idx, q_unit, m, power, allow=None):
    """-> (the reference's expanded queries on the device, their dense product with the index [Q, len] on the host, the phase-1
    product): phase 1 = topk_deep_ref.topk on the dense product of the index's own operands, the blend = gallery_expand_ref.blend on
    idx.rows, the norm = the library's own"""
    sim = dense_product(idx, q_unit).numpy()
    blend, _, _ = XR.expand(idx.rows.cpu().numpy(), q_unit.cpu().numpy(), sim, m, power, None if allow is None else allow.numpy())
    new = l2(gpu, blend)
    return new, dense_product(idx, new).numpy(), sim


@pytest.mark.parametrize("G", [20, 65, 2000])
def test_expand_queries_equals_the_reference(gpu, G):
    idx = shared_index(gpu, G)
    for Q in (1, 5, 32, 40):
        qu = queries(gpu, Q, "xq")
        for m, power in ((1, 1), (5, 1), (5, 0), (5, 3), (16, 1), (32, 1), (32, 4)):
            if m > G:
                with pytest.raises(ValueError, match="expand_queries: m must be in"):
                    idx.expand_queries(qu, m=m, power=power, normalize=False)
                continue
            want = reference_expanded(gpu, idx, qu, m, power)[0]
            got = idx.expand_queries(qu, m=m, power=power, normalize=False)
            assert got.dtype == torch.float32 and bits_equal(got, want), (G, Q, m, power)
    # raw queries: normalised by the same kernel search uses; the defaults are m = 5, power = 1
    raw = OF.randn("gxp:raw", (5, 256), SEED).to(gpu)
    assert bits_equal(idx.expand_queries(raw), reference_expanded(gpu, idx, unit_rows(raw), 5, 1)[0])
    norms = idx.expand_queries(raw).double().norm(dim=1).cpu()
    assert bool(((norms - 1).abs() < 1e-6).all())


# ------------------------------------------------------------------------------------------------------------------ search_expanded
@pytest.mark.parametrize("G,Qs,ks", [(2000, (1, 5, 40), (1, 10, 100, 1024)), (20037, (5,), (100,))])
def test_search_expanded_equals_the_reference_and_the_composition(gpu, G, Qs, ks):
    idx = shared_index(gpu, G)
    for Q in Qs:
        qu = queries(gpu, Q, "xs")
        for m, power in ((5, 1), (16, 3)):
            new, sim2, _ = reference_expanded(gpu, idx, qu, m, power)
            for k in ks:
                got = idx.search_expanded(qu, k=k, m=m, power=power, normalize=False)
                assert got[0].shape == (Q, k) and got[1].dtype == torch.int64 and got[0].dtype == torch.float32
                same(got, XR.expanded_topk(sim2, k), "G=%d Q=%d m=%d power=%d k=%d" % (G, Q, m, power, k))
                two = idx.shortlist(idx.expand_queries(qu, m=m, power=power, normalize=False), k=k, normalize=False)
                assert bits_equal(got[0], two[0]) and torch.equal(got[1], two[1]), (G, Q, m, power, k)
    raw = OF.randn("gxp:raw_s", (7, 256), SEED).to(gpu)
    _, sim2, _ = reference_expanded(gpu, idx, unit_rows(raw), 5, 1)
    same(idx.search_expanded(raw, k=10), XR.expanded_topk(sim2, 10), "normalize=True")
    got, two = idx.search_expanded(raw, k=10), idx.shortlist(idx.expand_queries(raw), k=10, normalize=False)
    assert bits_equal(got[0], two[0]) and torch.equal(got[1], two[1])
    assert idx.live_count == G and idx.neighbours_current


def test_tombstones_masks_and_short_lists(gpu):
    G, Q, k, m = 2000, 5, 100, 5
    idx = fresh_index(gpu, gallery(G))
    qu = queries(gpu, Q, "xm")
    gone = coin("x_gone", G, 4)
    idx.remove(rows=torch.nonzero(gone).reshape(-1))
    live = ~gone
    _, sim2, _ = reference_expanded(gpu, idx, qu, m, 1, live)
    same(idx.search_expanded(qu, k=k, m=m, normalize=False), XR.expanded_topk(sim2, k, live.numpy()), "tombstones")
    msk = coin("x_mask", G)
    allow = msk & live
    new, sim2, _ = reference_expanded(gpu, idx, qu, m, 1, allow)
    assert bits_equal(idx.expand_queries(qu, m=m, normalize=False, mask=msk.to(gpu)), new)
    got = idx.search_expanded(qu, k=k, m=m, normalize=False, mask=msk.to(gpu))
    same(got, XR.expanded_topk(sim2, k, allow.numpy()), "tombstones & mask")
    assert not bool(gone[got[1].cpu()].any()) and bool(msk[got[1].cpu()].all())
    # fewer than k allowed: real results first, then (-inf, -1)
    few = torch.zeros(G, dtype=torch.bool)
    few[OF.randint("gxp:few", 0, G, (k - 10,), SEED)] = True
    n_ok = int((few & live).sum())
    assert m < n_ok < k
    _, sim2, _ = reference_expanded(gpu, idx, qu, m, 1, few & live)
    got = idx.search_expanded(qu, k=k, m=m, normalize=False, mask=few.to(gpu))
    same(got, XR.expanded_topk(sim2, k, (few & live).numpy()), "fewer than k allowed")
    assert bool((got[1][:, n_ok:] == -1).all()) and bool((got[1][:, :n_ok] >= 0).all()) and bool(torch.isneginf(got[0][:, n_ok:]).all())
    # fewer than m allowed: the query blends what it has
    live_rows = torch.nonzero(live).reshape(-1)
    for left in (3, 1, 0):
        mk = torch.zeros(G, dtype=torch.bool)
        mk[live_rows[torch.unique(OF.randint("gxp:left%d" % left, 0, live_rows.numel(), (40,), SEED))[:left]]] = True
        mk |= gone  # (removed rows the mask allows stay removed: live & mask)
        assert int((mk & live).sum()) == left
        new, sim2, _ = reference_expanded(gpu, idx, qu, m, 1, mk & live)
        assert bits_equal(idx.expand_queries(qu, m=m, normalize=False, mask=mk.to(gpu)), new), left
        if left == 0:  # (nothing to blend: the unit query, normalised once more)
            assert bits_equal(new, unit_rows(qu))
        got = idx.search_expanded(qu, k=10, m=m, normalize=False, mask=mk.to(gpu))
        same(got, XR.expanded_topk(sim2, 10, (mk & live).numpy()), "%d allowed" % left)
        assert bool((got[1][:, :left] >= 0).all()) and bool((got[1][:, left:] == -1).all())
    # m and k beyond the live rows without a mask are refused on the host
    idx.remove(rows=torch.nonzero(~few).reshape(-1))
    assert idx.live_count == n_ok
    with pytest.raises(ValueError, match="search_expanded: k must be <= live_count"):
        idx.search_expanded(qu, k=k, m=m, normalize=False)
    idx.remove(rows=live_rows[3:])
    with pytest.raises(ValueError, match="expand_queries: m must be <= live_count"):
        idx.expand_queries(qu, m=m, normalize=False)


def test_search_expanded_pids_equals_the_distinct_reference(gpu):
    from textreid_amd import GalleryIndex

    G, m = 2000, 5
    pids = OF.randint("gxp:pids", 0, 300, (G,), SEED).long()
    idx = GalleryIndex()
    idx.add(gallery(G).to(gpu), pids=pids)
    gone = coin("xp_gone", G, 5)
    idx.remove(rows=torch.nonzero(gone).reshape(-1))
    msk = coin("xp_mask", G)
    for Q in (5, 40):
        qu = queries(gpu, Q, "xp")
        for mask, allow in ((None, ~gone), (msk, msk & ~gone)):
            _, sim2, _ = reference_expanded(gpu, idx, qu, m, 1, allow)
            for k in (1, 10, 100, 290):
                got = idx.search_expanded_pids(qu, k=k, m=m, normalize=False, mask=None if mask is None else mask.to(gpu))
                assert len(got) == 3 and got[2].dtype == torch.int64
                want = XR.expanded_topk(sim2, k, allow.numpy(), groups=pids.numpy())
                same(got[:2], want, "Q=%d k=%d mask=%s" % (Q, k, mask is not None))
                rows = got[1].cpu()
                assert torch.equal(got[2].cpu(), torch.where(rows < 0, rows, pids[rows.clamp(min=0)]))
                two = idx.shortlist_pids(idx.expand_queries(qu, m=m, normalize=False, mask=None if mask is None else mask.to(gpu)), k=k, normalize=False,
                                         mask=None if mask is None else mask.to(gpu))
                assert bits_equal(got[0], two[0]) and torch.equal(got[1], two[1]) and torch.equal(got[2], two[2])


# ------------------------------------------------------------------------------------------------------------------ the feature bites
_clustered = {}


def clustered(gpu):
    """the clustered gallery of test_clustered_gallery_where_the_term_bites: 250 centres x 8 rows, noise 2.0, seed 15, 40 queries ->
    (an index with the n = 5 graph, never modified; the unit queries)"""
    if not _clustered:
        noise = 2.0
        centres = OF.randn("grr:centres", (250, 256), CLUSTER_SEED)
        rows = centres.repeat_interleave(8, dim=0) + noise * OF.randn("grr:cnoise", (2000, 256), CLUSTER_SEED)
        rows = rows[torch.from_numpy(np.argsort(OF.randn("grr:cperm", (2000,), CLUSTER_SEED).numpy(), kind="stable"))]
        qu = unit_rows((centres[:40] + noise * OF.randn("grr:cq", (40, 256), CLUSTER_SEED)).to(gpu))
        _clustered["idx"], _clustered["qu"] = fresh_index(gpu, rows, n=5), qu
    return _clustered["idx"], _clustered["qu"]


def changed_sets(a, b):
    return sum(set(a[q].tolist()) != set(b[q].tolist()) for q in range(a.shape[0]))


@pytest.mark.parametrize("m,power", [(1, 3), (5, 0), (5, 1), (5, 3), (16, 3)])
def test_clustered_gallery_where_expansion_bites(gpu, m, power):
    idx, qu = clustered(gpu)
    _, sim2, sim = reference_expanded(gpu, idx, qu, m, power)
    want, plain = XR.expanded_topk(sim2, 10), TR.topk(sim, 10)
    moved = changed_sets(want[1], plain[1])
    print("m = %d, power = %d: queries whose top-10 row set changes: %d of 40" % (m, power, moved))
    # on the REFERENCE's output: an expansion that does nothing cannot pass
    assert moved >= 10
    same(idx.search_expanded(qu, k=10, m=m, power=power, normalize=False), want, "m=%d power=%d" % (m, power))
    same(idx.shortlist(qu, k=10, normalize=False), plain, "shortlist next to it")


# ------------------------------------------------------------------------------------------------------------------ augmented
def check_augmented(gpu, idx, qu, m, power=1):
    """aug = idx.augmented(m, power) against the reference built on idx's own rows, lists and values -> (aug, the fresh index built
    from the reference's rows)"""
    from textreid_amd import GalleryIndex

    G = len(idx)
    blend = XR.augment(idx.rows.cpu().numpy(), idx.neighbours.cpu().numpy(), idx.neighbour_values.cpu().numpy(), m, power)
    want_rows = l2(gpu, blend)
    aug = idx.augmented(m=m, power=power)
    assert isinstance(aug, GalleryIndex) and aug is not idx and len(aug) == G
    assert bits_equal(aug.rows, want_rows), m
    ref = GalleryIndex()
    ref.add(want_rows, pids=idx.pids, normalize=False)
    assert torch.equal(aug.rows_p16.view(torch.int32), ref.rows_p16.view(torch.int32))
    assert (aug.pids is None and idx.pids is None) or torch.equal(aug.pids, idx.pids)
    assert torch.equal(aug.live, idx.live) and aug.live_count == idx.live_count
    assert aug.neighbours is None and not aug.neighbours_current
    live = idx.live.cpu()
    if not bool(live.all()):
        assert bool((aug.rows[~live.to(gpu)] == 0).all())  # (a removed row's list is all -1: a zero blend)
    k = min(100, idx.live_count)
    for got in (aug.shortlist(qu, k=k, normalize=False), aug.search(qu, k=10, normalize=False)):
        assert bool((got[1] >= 0).all()) and bool(live[got[1].cpu()].all())
    same(aug.shortlist(qu, k=k, normalize=False), TR.topk(dense_product(ref, qu).numpy(), k, live.numpy()), "a search on the augmented index")
    return aug, ref


def test_augmented_with_removed_rows(gpu):
    from textreid_amd import GalleryIndex

    G, n = 2000, 5
    idx = GalleryIndex()
    idx.add(gallery(G).to(gpu), pids=torch.arange(G) // 4)
    with pytest.raises(RuntimeError, match="augmented: the neighbour graph is absent.*build_neighbours"):
        idx.augmented()
    gone = coin("xa_gone", G, 3)
    idx.remove(rows=torch.nonzero(gone).reshape(-1))
    idx.build_neighbours(n)
    qu = queries(gpu, 40, "xa")
    before = (idx.rows.clone(), idx.rows_p16.clone(), idx.neighbours.clone(), idx.neighbour_values.clone(), idx.shortlist(qu, k=100, normalize=False),
              idx.search_reranked(qu, k=100, normalize=False), idx.search(qu[:7], k=10, normalize=False))
    for m in (2, 5):
        check_augmented(gpu, idx, qu, m)
    aug0, _ = check_augmented(gpu, idx, qu, 5, power=0)
    assert not bits_equal(aug0.rows, idx.augmented().rows)  # (m defaults to n = 5, power to 1)
    for bad in (0, 6):
        with pytest.raises(ValueError, match="augmented: m must be in"):
            idx.augmented(m=bad)
    # the original: rows, graph and searches as before
    assert bits_equal(idx.rows, before[0]) and torch.equal(idx.rows_p16.view(torch.int32), before[1].view(torch.int32))
    assert idx.neighbours_current and torch.equal(idx.neighbours, before[2]) and bits_equal(idx.neighbour_values, before[3])
    for got, want in ((idx.shortlist(qu, k=100, normalize=False), before[4]), (idx.search_reranked(qu, k=100, normalize=False), before[5]),
                      (idx.search(qu[:7], k=10, normalize=False), before[6])):
        assert bits_equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert idx.live_count == G - int(gone.sum())
    # the result is an ordinary index: it takes a graph of its own
    aug = idx.augmented(m=2)
    aug.build_neighbours(n)
    assert aug.neighbours_current and bool((aug.neighbours[~idx.live] == -1).all())
    # a stale graph raises
    idx.add(gallery(65).to(gpu), pids=torch.arange(65) + G)
    with pytest.raises(RuntimeError, match="augmented: the neighbour graph is stale.*build_neighbours"):
        idx.augmented()
    idx.refresh_neighbours()
    assert len(idx.augmented()) == G + 65


def test_augmented_bites_on_the_clustered_gallery(gpu):
    idx, qu = clustered(gpu)
    plain = TR.topk(dense_product(idx, qu).numpy(), 10)
    for m in (2, 5):
        aug, ref = check_augmented(gpu, idx, qu, m)
        want = TR.topk(dense_product(ref, qu).numpy(), 10)  # (the REFERENCE's rows: an augmentation that does nothing cannot pass)
        moved = changed_sets(want[1], plain[1])
        print("m = %d: queries whose plain top-10 row set changes against the augmented gallery: %d of 40" % (m, moved))
        assert moved >= 10
        same(aug.shortlist(qu, k=10, normalize=False), want, "m=%d" % m)
    assert idx.neighbours_current and idx.live_count == 2000


# ------------------------------------------------------------------------------------------------------------------ shards
@pytest.mark.parametrize("shard_rows", [7, 64])
def test_shards_equal_one_index(gpu, shard_rows):
    from textreid_amd import GalleryIndex, GalleryShards

    G = 200
    rows = gallery(2000)[:G].to(gpu)
    pids = OF.randint("gxp:spids", 0, 40, (G,), SEED).long()
    one, sh = GalleryIndex(), GalleryShards(shard_rows=shard_rows)
    one.add(rows, pids=pids)
    sh.add(rows, pids=pids)
    assert sh.n_shards == -(-G // shard_rows)
    at = torch.arange(G)
    to_global = (at // shard_rows) * (1 << 21) + at % shard_rows

    def mapped(r):
        shard, local = sh.locate(r.cpu())
        return torch.where(r.cpu() < 0, r.cpu(), shard * shard_rows + local)

    def check(mask_one, mask_parts, tag):
        for Q in (5, 40):
            qu = queries(gpu, Q, "xsh")
            raw = OF.randn("gxp:shraw%d" % Q, (Q, 256), SEED).to(gpu)
            for m, power in ((5, 1), (32, 3)):
                assert bits_equal(sh.expand_queries(qu, m=m, power=power, normalize=False, mask=mask_parts),
                                  one.expand_queries(qu, m=m, power=power, normalize=False, mask=mask_one)), (tag, Q, m)
                for k in (10, 100):
                    a = sh.search_expanded(qu, k=k, m=m, power=power, normalize=False, mask=mask_parts)
                    b = one.search_expanded(qu, k=k, m=m, power=power, normalize=False, mask=mask_one)
                    assert bits_equal(a[0], b[0]) and torch.equal(mapped(a[1]), b[1].cpu()), (tag, Q, m, k)
            a, b = sh.search_expanded(raw, k=10, mask=mask_parts), one.search_expanded(raw, k=10, mask=mask_one)
            assert bits_equal(a[0], b[0]) and torch.equal(mapped(a[1]), b[1].cpu()), (tag, Q, "normalize=True")
            a = sh.search_expanded_pids(qu, k=30, m=5, normalize=False, mask=mask_parts)
            b = one.search_expanded_pids(qu, k=30, m=5, normalize=False, mask=mask_one)
            assert bits_equal(a[0], b[0]) and torch.equal(mapped(a[1]), b[1].cpu()) and torch.equal(a[2], b[2]), (tag, Q, "pids")

    check(None, None, "plain")
    gone = torch.nonzero(coin("xsh_gone", G, 4)).reshape(-1)
    assert one.remove(rows=gone) == sh.remove(rows=to_global[gone])
    msk = coin("xsh_mask", G).to(gpu)
    check(msk, [msk[s * shard_rows : (s + 1) * shard_rows] for s in range(sh.n_shards)], "tombstones & mask")
    with pytest.raises(RuntimeError, match="search_expanded: query expansion is not built for the by-rank form"):
        GalleryShards(collective=True).search_expanded(queries(gpu, 5, "xsh"))


# ------------------------------------------------------------------------------------------------------------------ capture
def test_search_expanded_records_and_replays(gpu):
    G, Q, k = 20037, 4, 100
    idx = fresh_index(gpu, gallery(G))
    idx.remove(rows=torch.nonzero(coin("xcap_dead", G, 10)).reshape(-1))
    qa = OF.randn("gxp:cap_a", (Q, 256), SEED).to(gpu)
    qb = OF.randn("gxp:cap_b", (Q, 256), SEED).to(gpu)
    ma, mb = coin("xcap_ma", G).to(gpu), coin("xcap_mb", G).to(gpu)
    buf, m = qa.clone(), ma.clone()
    idx.search_expanded(buf, k=k, mask=m)  # (allocates the score buffer, the workspaces, the word buffer and the blend's tables)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        vals, rows = idx.search_expanded(buf, k=k, mask=m)
    g.replay()
    torch.cuda.synchronize()
    va, ra = idx.search_expanded(qa, k=k, mask=ma)
    assert torch.equal(vals, va) and torch.equal(rows, ra)
    buf.copy_(qb)
    m.copy_(mb)
    g.replay()
    torch.cuda.synchronize()
    got_v, got_r = vals.clone(), rows.clone()
    vb, rb = idx.search_expanded(qb, k=k, mask=mb)
    assert torch.equal(got_v, vb) and torch.equal(got_r, rb)
    assert not torch.equal(rb, ra)
    allow = mb.cpu() & idx.live.cpu()
    _, sim2, _ = reference_expanded(gpu, idx, unit_rows(qb), 5, 1, allow)
    same((got_v, got_r), XR.expanded_topk(sim2, k, allow.numpy()), "replay against the host reference")


# ------------------------------------------------------------------------------------------------------------------ nothing else moved
def test_the_other_searches_after_an_expanded_search_are_unchanged(gpu):
    idx = shared_index(gpu, 2000)
    qu = queries(gpu, 40)
    sim = dense_product(idx, qu)
    want = TR.topk(sim.numpy(), 100)
    before = (idx.shortlist(qu, k=100, normalize=False), idx.search(qu[:7], k=10, normalize=False), idx.search_reranked(qu, k=100, normalize=False))
    idx.search_expanded(qu, k=100, m=16, power=3, normalize=False)  # (the score buffer, the panel and the select workspace are shared)
    after = (idx.shortlist(qu, k=100, normalize=False), idx.search(qu[:7], k=10, normalize=False), idx.search_reranked(qu, k=100, normalize=False))
    for a, b in zip(after, before):
        assert bits_equal(a[0], b[0]) and torch.equal(a[1], b[1])
    same(after[0], want, "shortlist after")
    same(after[1], TR.topk(sim[:7].numpy(), 10), "search after")
    idx.expand_queries(qu[:3], m=32, normalize=False)
    same(idx.shortlist(qu[:9], k=100, normalize=False), TR.topk(sim[:9].numpy(), 100), "a smaller panel next")
    assert idx.neighbours_current and idx.live_count == 2000
