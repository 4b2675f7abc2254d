"""The incremental neighbour-graph refresh of GalleryIndex on the GPU: trid_index_nn_merge_f32 alone (over-allocated buffers compared
whole, so that nothing outside the named slots moves), the wide [32, n0] candidate product against the narrow dense product of the
build, and refresh_neighbours against a from-scratch build_neighbours on the same contents and against gallery_rerank_ref.graph of
the dense product.  Nothing here needs a tolerance: values are compared as bit patterns, rows exactly."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import gallery_nn_update_ref as NU  # noqa: E402
import gallery_rerank_ref as RR  # noqa: E402
import oracle.fill as OF  # noqa: E402
import topk_deep_ref as TR  # noqa: E402
from gallery_support import dense_product, gpu, Inputs  # noqa: E402,F401

SEED = 13
IN = Inputs("grr:", SEED)  # (the galleries and queries of test_gallery_rerank_gpu.py, by name: the cached galleries are shared with it)
gallery, queries, product_of = IN.gallery, IN.queries, IN.product_of


def built_index(gpu, rows, n, capacity=0):
    from textreid_amd import GalleryIndex

    idx = GalleryIndex(capacity=capacity)
    idx.add(rows.to(gpu))
    idx.build_neighbours(n)
    return idx


def rebuilt(idx):
    """a fresh index with the same contents (rows bit for bit, the same tombstones) and a from-scratch graph of the same n"""
    from textreid_amd import GalleryIndex

    new = GalleryIndex()
    new.add(idx.rows.clone(), normalize=False)
    assert torch.equal(new.rows_p16.view(torch.int32), idx.rows_p16.view(torch.int32))
    dead = torch.nonzero(~idx.live).reshape(-1)
    if dead.numel():
        new.remove(rows=dead)
    new.build_neighbours(idx.neighbours.shape[1])
    return new


def same_graph(idx, other, what=""):
    assert idx.neighbours_current and idx.neighbours_refreshable, what
    assert torch.equal(idx.neighbours, other.neighbours), what
    assert torch.equal(idx.neighbour_values.view(torch.int32), other.neighbour_values.view(torch.int32)), what
    dead = ~idx.live
    assert bool((idx.neighbours[dead] == -1).all()) and bool(torch.isneginf(idx.neighbour_values[dead]).all()), what


def flagged(old_nn, old_val, n0, live_now):
    """rows the reference flags: live old rows whose list, as it was last current, holds a row that is dead now"""
    live = np.asarray(live_now)[:n0]
    return int(NU.merge(None, 0, n0, n0, live, old_nn[:n0], old_val[:n0])[2].sum())


def refresh_and_check(idx, what=""):
    """refresh_neighbours on a stale index: the counts against the reference, lists and values against the rebuild -> the rebuild"""
    n0 = idx._nn_rows
    old_nn, old_val = idx.neighbours[:n0].cpu().numpy(), idx.neighbour_values[:n0].cpu().numpy()
    live = idx.live.cpu().numpy()
    assert not idx.neighbours_current
    got = idx.refresh_neighbours()
    assert got == (int(live[n0:].sum()), flagged(old_nn, old_val, n0, live)), what
    other = rebuilt(idx)
    same_graph(idx, other, what)
    return other


# ------------------------------------------------------------------------------------------------------------------ the kernel alone
def _merge_case(gpu, rows, m, n, ld, seed):
    from textreid_amd import ops
    from textreid_amd.ops import _p

    rng = np.random.RandomState(seed)
    first = rows + 3  # (rows <= cand_first: rows between them are neither merged nor candidates)
    total = first + m
    live = rng.randint(0, 6, size=total) != 0
    live[0] = True
    if m >= 2:
        live[first], live[first + 1] = True, True
    if m >= 4:
        live[first + 2] = False  # a dead candidate
    if rows >= 63:
        live[5], live[9] = False, True  # a dead row; row 9 is live and, below, uncovered
    grid = lambda *shape: (rng.randint(-12, 13, size=shape) / 8).astype(np.float32)  # noqa: E731  (coarse: equal values everywhere)
    vals = np.sort(grid(rows, n), axis=1)[:, ::-1].copy()
    nn = rng.randint(0, first, size=(rows, n)).astype(np.int32)
    nn[0] = 0  # (row 0: a list without dead entries and n distinct values, so the planted ties below are merged where expected)
    vals[0] = (np.arange(n, 0, -1) / 8).astype(np.float32)
    if rows >= 63:
        nn[9] = -1
        nn[11, n - 1], live[11], live[3] = 3, True, False  # a dead list entry in the last slot
        nn[12, 0], live[12], live[5] = 5, True, False
    cand2d = grid(m, ld)
    if m >= 1:
        cand2d[:, 0] = -2.0
        cand2d[0, 0] = vals[0, n // 2]  # old against candidate: the candidate stays behind
    if m >= 2:
        cand2d[1, 0] = cand2d[0, 0]     # candidate against candidate: the lower one stays in front
    want_nn, want_val, want_redo = NU.merge(cand2d if m else None, m, first, rows, live, nn, vals)
    if m >= 2 and n >= 5:
        assert want_nn[0].tolist()[n // 2 : n // 2 + 3] == [0, first, first + 1]
    if rows >= 63:
        assert want_redo[9] == 1 and want_redo[11] == 1 and want_redo[12] == 1 and want_redo[5] == 0 and (want_nn[5] == -1).all()
    # over-allocated buffers with a recognisable pattern outside the extents
    cand_buf = (0x5A5A0000 + (np.arange((m + 1) * ld + 7) & 0xFFFF)).astype(np.uint32).view(np.float32).copy()
    cand_buf[: m * ld] = cand2d.reshape(-1)
    nn_buf = np.full((rows + 2) * n + 3, 0x7A7A7A7A, dtype=np.int32)
    nn_buf[: rows * n] = nn.reshape(-1)
    val_buf = np.full((rows + 2) * n + 3, 0x6B6B6B6B, dtype=np.uint32).view(np.float32).copy()
    val_buf[: rows * n] = vals.reshape(-1)
    redo_buf = np.full(rows + 9, 0xAB, dtype=np.uint8)
    w_nn, w_val, w_redo = nn_buf.copy(), val_buf.copy(), redo_buf.copy()
    w_nn[: rows * n], w_val[: rows * n], w_redo[:rows] = want_nn.reshape(-1), want_val.reshape(-1), want_redo
    d_cand, d_nn, d_val = torch.from_numpy(cand_buf).to(gpu), torch.from_numpy(nn_buf).to(gpu), torch.from_numpy(val_buf).to(gpu)
    d_redo, d_live = torch.from_numpy(redo_buf).to(gpu), torch.from_numpy(live.astype(np.uint8)).to(gpu)
    ops.call("trid_index_nn_merge_f32", _p(d_cand) if m else None, ld, m, first, rows, _p(d_live), _p(d_nn), _p(d_val), n, _p(d_redo), ops.stream())
    what = "rows=%d m=%d n=%d ld=%d" % (rows, m, n, ld)
    assert np.array_equal(d_redo.cpu().numpy(), w_redo), what
    assert np.array_equal(d_nn.cpu().numpy(), w_nn), what
    assert np.array_equal(d_val.cpu().numpy().view(np.uint32), w_val.view(np.uint32)), what
    assert np.array_equal(d_cand.cpu().numpy().view(np.uint32), cand_buf.view(np.uint32)), what
    assert np.array_equal(d_live.cpu().numpy(), live.astype(np.uint8)), what


@pytest.mark.parametrize("n", [1, 5, 8])
@pytest.mark.parametrize("m", [0, 1, 31, 32])
@pytest.mark.parametrize("rows", [1, 63, 64, 65, 257, 5000])
def test_merge_kernel_equals_the_reference_and_touches_nothing_else(gpu, rows, m, n):
    _merge_case(gpu, rows, m, n, rows, 100000 * n + 100 * rows + m)
    _merge_case(gpu, rows, m, n, rows + 5, 100000 * n + 100 * rows + m + 50)  # ld_cand > rows


# ------------------------------------------------------------------------------------------------------------------ the wide product
@pytest.mark.parametrize("n0", [20, 60, 65, 2000, 2048])  # (20 / 60 / 65: the 256x32, 128x64 and 128x128 tiles; 2048: the streaming kernel's shape)
def test_wide_candidate_product_equals_the_narrow_dense_product(gpu, n0):
    from textreid_amd import GalleryIndex

    idx = GalleryIndex()
    idx.add(gallery(n0 + 32).to(gpu))
    sim = product_of(idx, ("wide", n0))  # sim[i, g]: row i as the query (B panel), row g as the gallery (A)
    cand = idx._candidate_scores(n0, 32, n0)
    wide = cand.reshape(-1)[: 32 * n0].reshape(32, n0).cpu().numpy()
    want = np.ascontiguousarray(sim[:n0, n0:].T)
    assert np.array_equal(wide.view(np.uint32), want.view(np.uint32)), n0
    # the direction matters: the transposed entries are not the same fp32 numbers
    if n0 >= 2000:
        assert (sim[:n0, n0:] != sim[n0:, :n0].T).any()
    # a ragged group: 5 rows from n0 + 27
    part = idx._candidate_scores(n0 + 27, 5, n0).reshape(-1)[: 5 * n0].reshape(5, n0).cpu().numpy()
    assert np.array_equal(part.view(np.uint32), want[27:].view(np.uint32)), n0


# ------------------------------------------------------------------------------------------------------------------ refresh = rebuild
@pytest.mark.parametrize("added", [1, 32, 35, 100])
@pytest.mark.parametrize("n0", [20, 65, 2000])
def test_refresh_after_add_equals_rebuild_and_the_dense_product(gpu, n0, added):
    rows = gallery(2100)[: n0 + added]
    sim = None
    for n in (5, 1, 8):
        idx = built_index(gpu, rows[:n0], n)
        assert idx.neighbours_refreshable and idx.add(rows[n0:].to(gpu)) == n0
        assert not idx.neighbours_current and bool((idx.neighbours[n0:] == -1).all()) and bool(torch.isneginf(idx.neighbour_values[n0:]).all())
        assert idx.refresh_neighbours() == (added, 0)
        fresh = built_index(gpu, rows, n)
        same_graph(idx, fresh, (n0, added, n))
        if sim is None:
            sim = product_of(idx, ("add", n0, added))
        want = RR.graph(sim, n)
        assert np.array_equal(idx.neighbours.cpu().numpy(), want), (n0, added, n)
        want_val = np.take_along_axis(sim, want.astype(np.int64), axis=1)  # the product's own entries: s(query i, gallery g)
        assert np.array_equal(idx.neighbour_values.cpu().numpy().view(np.uint32), want_val.view(np.uint32)), (n0, added, n)
        assert idx.refresh_neighbours() == (0, 0)


# ------------------------------------------------------------------------------------------------------------------ scenarios
def test_added_duplicates_follow_the_old_copy_in_both_lists(gpu):
    base = gallery(2100)[:300]
    idx = built_index(gpu, base, 5)
    idx.add(base[:40].to(gpu))  # row 300 + r is the image of row r
    refresh_and_check(idx, "duplicates")
    nn = idx.neighbours.cpu().long()
    r = torch.arange(40)
    assert torch.equal(nn[:40, 0], r) and torch.equal(nn[:40, 1], r + 300)
    assert torch.equal(nn[300:, 0], r) and torch.equal(nn[300:, 1], r + 300)
    v = idx.neighbour_values.cpu()
    assert torch.equal(v[:40, 0].view(torch.int32), v[:40, 1].view(torch.int32))


def test_remove_only(gpu):
    idx = built_index(gpu, gallery(2000), 5)
    gone = OF.randint("grf:gone", 0, 10, (2000,), SEED) == 0
    assert idx.remove(rows=torch.nonzero(gone).reshape(-1)) == int(gone.sum())
    before = idx.neighbours.clone()
    other = refresh_and_check(idx, "remove only")
    changed = (idx.neighbours != before).any(dim=1).cpu()
    assert bool(changed[gone].all()) and 0 < int(changed[~gone].sum()) < int((~gone).sum())
    # searches: after the refresh = on the rebuilt index
    q = queries(gpu, 7)
    a, b = idx.search_reranked(q, k=50, normalize=False), other.search_reranked(q, k=50, normalize=False)
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1], b[1])


def test_add_and_remove_mixed_with_a_capacity_growth(gpu):
    rows = gallery(2100)
    idx = built_index(gpu, rows[:60], 5)
    assert idx.capacity == 64
    idx.remove(rows=[3, 17])
    idx.add(rows[60:300].to(gpu))  # growth: lists and values move with the storage
    assert idx.capacity > 64 and tuple(idx.neighbour_values.shape) == (300, 5)
    idx.remove(rows=[5, 100, 101, 299])  # old and just-added rows
    idx.add(rows[300:345].to(gpu))
    idx.remove(rows=[344, 20])
    other = refresh_and_check(idx, "mixed")
    q = queries(gpu, 40)
    a, b = idx.search_reranked(q, k=100, normalize=False), other.search_reranked(q, k=100, normalize=False)
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1], b[1])
    m = OF.randint("grf:mask", 0, 2, (345,), SEED).to(gpu) != 0
    a, b = idx.search_reranked(q, k=100, normalize=False, mask=m), other.search_reranked(q, k=100, normalize=False, mask=m)
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1], b[1])
    # a second round on the refreshed graph, then nothing to do
    idx.add(rows[345:346].to(gpu))
    idx.remove(rows=[0, 345])
    refresh_and_check(idx, "second round")
    assert idx.refresh_neighbours() == (0, 0) and idx.neighbours_current


def test_rows_added_and_removed_before_the_refresh(gpu):
    rows = gallery(2100)
    idx = built_index(gpu, rows[:65], 8)
    idx.add(rows[65:105].to(gpu))
    idx.remove(rows=list(range(65, 105)))
    before = idx.neighbours[:65].clone()
    assert idx._nn_rows == 65
    refresh_and_check(idx, "added and removed")
    assert torch.equal(idx.neighbours[:65], before) and bool((idx.neighbours[65:] == -1).all())


def test_sampled_rows_at_20037_plus_40(gpu):
    G, add, n = 20037, 40, 5
    rows = gallery(G + add)
    idx = built_index(gpu, rows[:G], n)
    idx.add(rows[G:].to(gpu))
    idx.remove(rows=[31, 20036, G + 7])
    assert idx.refresh_neighbours()[0] == add - 1
    fixed = [0, 32, 20032, 20035, G, G + 1, G + 8, G + 31, G + 32, G + 39]
    rest = [int(r) for r in OF.randint("grf:sample", 0, G + add, (200,), SEED).tolist() if r not in fixed + [31, 20036, G + 7]]
    sample = torch.tensor(fixed + list(dict.fromkeys(rest))[: 64 - len(fixed)])
    assert sample.numel() == 64
    sim = dense_product(idx, idx.rows[sample.to(gpu)].contiguous()).numpy()
    want_val, want = TR.topk(sim, n, idx.live.cpu().numpy())
    assert np.array_equal(idx.neighbours.cpu()[sample].numpy(), want.astype(np.int32))
    assert np.array_equal(idx.neighbour_values.cpu()[sample].numpy().view(np.uint32), want_val.view(np.uint32))
    for r in (31, 20036, G + 7):
        assert bool((idx.neighbours[r] == -1).all()) and bool(torch.isneginf(idx.neighbour_values[r]).all())


# ------------------------------------------------------------------------------------------------------------------ persistence, compact, limits
def test_state_dict_round_trip_with_and_without_values(gpu):
    from textreid_amd import GalleryIndex

    rows = gallery(2100)
    idx = built_index(gpu, rows[:300], 5)
    idx.remove(rows=[4, 250])
    assert idx.state_dict()["neighbour_values"] is None  # (stale: neither lists nor values are saved)
    idx.refresh_neighbours()
    sd = idx.state_dict()
    assert sd["neighbour_values"].dtype == torch.float32 and tuple(sd["neighbour_values"].shape) == (300, 5)
    assert torch.equal(sd["neighbour_values"].view(torch.int32), idx.neighbour_values.view(torch.int32))
    sd["neighbour_values"][0, 0] = 7.0  # (a clone: the index does not see this)
    assert float(idx.neighbour_values[0, 0]) != 7.0
    sd = idx.state_dict()
    back = GalleryIndex()
    back.load_state_dict(sd)
    assert back.neighbours_current and back.neighbours_refreshable and back._nn_rows == 300
    same_graph(back, idx, "loaded")
    back.add(rows[300:340].to(gpu))
    back.remove(rows=[7])
    refresh_and_check(back, "add + refresh on the loaded index")
    # a dict without values: the graph is current, search_reranked works, refresh raises
    q = queries(gpu, 5)
    bare = GalleryIndex()
    bare.load_state_dict({k: v for k, v in sd.items() if k != "neighbour_values"})
    assert bare.neighbours_current and not bare.neighbours_refreshable and bare.neighbour_values is None
    a, b = bare.search_reranked(q, k=20, normalize=False), idx.search_reranked(q, k=20, normalize=False)
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1], b[1])
    assert bare.state_dict()["neighbours"] is not None and bare.state_dict()["neighbour_values"] is None
    with pytest.raises(RuntimeError, match="refresh_neighbours: .*build_neighbours"):
        bare.refresh_neighbours()
    bare.add(rows[300:301].to(gpu))
    with pytest.raises(RuntimeError, match="refresh_neighbours: .*build_neighbours"):
        bare.refresh_neighbours()
    bare.build_neighbours(5)
    assert bare.neighbours_refreshable


def test_compact_keeps_the_graph_on_request(gpu):
    rows = gallery(2100)
    idx = built_index(gpu, rows[:300], 5)
    idx.remove(rows=[0, 9, 150, 299])
    # a stale graph is dropped whatever was asked
    stale = built_index(gpu, rows[:300], 5)
    stale.remove(rows=[0, 9])
    stale.compact(keep_neighbours=True)
    assert stale.neighbours is None and not stale.neighbours_refreshable
    with pytest.raises(RuntimeError, match="refresh_neighbours: .*build_neighbours"):
        stale.refresh_neighbours()
    idx.refresh_neighbours()
    new_of = idx.compact(keep_neighbours=True)
    assert len(idx) == 296 and int(new_of[0]) == -1 and int(new_of[1]) == 0 and idx._nn_rows == 296
    same_graph(idx, rebuilt(idx), "compact(keep_neighbours=True)")
    idx.add(rows[300:333].to(gpu))
    refresh_and_check(idx, "refresh after a keeping compact")
    # the default still drops
    idx.remove(rows=[1])
    idx.refresh_neighbours()
    idx.compact()
    assert idx.neighbours is None and idx.neighbour_values is None and not idx.neighbours_current and not idx.neighbours_refreshable


def test_n_beyond_live_count_raises_and_leaves_the_lists(gpu):
    idx = built_index(gpu, gallery(2100)[:20], 5)
    idx.remove(rows=list(range(3, 20)))
    nn, val = idx.neighbours.clone(), idx.neighbour_values.clone()
    with pytest.raises(ValueError, match="build_neighbours: n must be <= live_count = 3"):
        idx.refresh_neighbours()
    assert not idx.neighbours_current and torch.equal(idx.neighbours, nn) and torch.equal(idx.neighbour_values.view(torch.int32), val.view(torch.int32))
