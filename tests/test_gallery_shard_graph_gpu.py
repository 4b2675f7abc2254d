"""The neighbour graph and the re-ranked search of GalleryShards on the GPU: trid_index_nn_merge_sharded_f32 alone against the numpy
reference (gallery_shard_graph_ref.merge; over-allocated buffers compared whole, so that nothing outside the named slots moves), the
in-process form against ONE GalleryIndex over the same rows (build_neighbours, search_reranked, search_reranked_pids,
refresh_neighbours against a fresh build, state_dict, capture), and the by-rank form on two gloo ranks sharing the GPU
(tests/gallery_shard_graph_worker.py, started by rank_launch.run_ranks).  The pair of the two is gallery_support.ShardPair with add /
remove / same_graph / build on top.  Nothing here needs a tolerance: values are compared as bit patterns, ids exactly."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import gallery_shard_graph_ref as SG  # noqa: E402
from gallery_support import ShardPair, gpu, shard_inputs  # noqa: E402,F401
from rank_launch import run_ranks  # noqa: E402

STRIDE = SG.SHARD_STRIDE


# ------------------------------------------------------------------------------------------------------------------ the kernel alone
def _sorted_lists(rng, pool, rows, n):
    """[rows, n] distinct ids from ``pool`` with values on the 1/8 grid, each list in the order value descending, id ascending"""
    nn = np.stack([rng.choice(pool, size=n, replace=False) for _ in range(rows)]).astype(np.int64)
    vals = (rng.randint(-8, 9, size=(rows, n)) / 8).astype(np.float32)
    vals[rng.randint(0, 5, size=(rows, n)) == 0] *= np.float32(-1.0)  # (both zeros)
    for i in range(rows):
        order = np.lexsort((nn[i], -vals[i].astype(np.float64)))
        nn[i], vals[i] = nn[i][order], vals[i][order]
    return nn.astype(np.int32), vals


def _kernel_case(gpu, rows, m, n, n_shards, ld, seed):
    from textreid_amd import ops
    from textreid_amd.ops import _p

    rng = np.random.RandomState(seed)
    if n_shards == 1:
        # one shard: the candidates are numbered above every merged row, eight unmerged rows between them
        self_shard, cand_shard, first_local = 0, 0, rows + 8
        lens = [rows + 8 + m]
        pool = np.arange(rows + 8)
    else:
        # three shards, the middle one empty: the rows of shard 2 are merged, their lists hold rows of shard 0 (below the
        # candidates) and of shard 2 (above them); the candidates are the last m rows of shard 0
        self_shard, cand_shard, first_local = 2, 0, 37
        lens = [37 + m, 0, rows + 9]
        pool = np.concatenate([np.arange(37), 2 * STRIDE + np.arange(rows + 9)])
    cand_first = cand_shard * STRIDE + first_local
    lives = [(rng.randint(0, 12, size=g) != 0).astype(np.uint8) for g in lens]
    own = lives[self_shard]
    own[0] = 1
    if m >= 2:
        lives[cand_shard][first_local], lives[cand_shard][first_local + 1] = 1, 1
    if m >= 4:
        lives[cand_shard][first_local + 2] = 0  # a dead candidate
    nn, vals = _sorted_lists(rng, pool, rows, n)
    live_len = list(lens)
    if rows >= 63:
        own[5], own[9], own[11], own[12], own[13], own[14] = 0, 1, 1, 1, 1, 1  # a dead own row; row 9 is live and, below, uncovered
        nn[9] = -1
        dead = int(pool[3])
        lives[dead >> SG.SHARD_BITS][dead & SG.LOCAL_MASK] = 0
        nn[11, n - 1] = dead                                # an entry that points at a removed row, in the last slot
        nn[12, 0] = n_shards * STRIDE + 1                   # at a shard >= n_shards
        nn[13, n // 2] = self_shard * STRIDE + lens[self_shard] + 2  # at a local row >= live_len
        if n_shards == 3:
            nn[14, 0] = STRIDE                              # at the empty shard
        live_len[self_shard] = lens[self_shard] - (2 if n_shards == 3 else 0)  # (uneven: the recorded length is below the bytes held)
    # row 0: a list of live rows with n distinct values, so the planted ties below are merged where expected
    fine = [int(e) for e in pool if SG.is_live(e, [lv[:g] for lv, g in zip(lives, live_len)]) and not cand_first <= e < cand_first + m][:n]
    if len(fine) == n:
        nn[0], vals[0] = np.sort(fine), (np.arange(n, 0, -1) / 8).astype(np.float32)
    cand2d = (rng.randint(-8, 9, size=(m, ld)) / 8).astype(np.float32)
    if m >= 1:
        cand2d[:, 0] = -2.0
        cand2d[0, 0] = vals[0, n // 2]  # a tie between a stored row and a candidate: the lower id goes first
    if m >= 2:
        cand2d[1, 0] = cand2d[0, 0]     # a tie between two candidates
    ref_lives = [lv[:g] for lv, g in zip(lives, live_len)]
    want_nn, want_val, want_redo = SG.merge(cand2d if m else None, m, cand_first, rows, ref_lives, self_shard, nn, vals)
    if rows >= 63:
        assert want_redo[9] == 1 and want_redo[11] == 1 and want_redo[12] == 1 and want_redo[13] == 1 and want_redo[5] == 0 and (want_nn[5] == -1).all()
        assert n_shards == 1 or want_redo[14] == 1
    if m >= 2 and n >= 5 and len(fine) == n:
        assert cand_first in want_nn[0] and want_redo[0] == 0
    # the liveness bytes: three pad bytes, then the shards one after the other
    live_all = np.concatenate([np.full(3, 1, dtype=np.uint8)] + lives)
    live_off = np.array([3 + sum(lens[:s]) for s in range(n_shards)], dtype=np.int64)
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
    d_redo, d_live = torch.from_numpy(redo_buf).to(gpu), torch.from_numpy(live_all).to(gpu)
    d_off, d_len = torch.from_numpy(live_off).to(gpu), torch.tensor(live_len, dtype=torch.int32, device=gpu)
    ops.call("trid_index_nn_merge_sharded_f32", _p(d_cand) if m else None, ld, m, cand_first, rows, _p(d_live), _p(d_off), _p(d_len), live_all.size,
             n_shards, self_shard, _p(d_nn), _p(d_val), n, _p(d_redo), ops.stream())
    what = "rows=%d m=%d n=%d shards=%d ld=%d" % (rows, m, n, n_shards, ld)
    assert np.array_equal(d_redo.cpu().numpy(), w_redo), what
    assert np.array_equal(d_nn.cpu().numpy(), w_nn), what
    assert np.array_equal(d_val.cpu().numpy().view(np.uint32), w_val.view(np.uint32)), what
    assert np.array_equal(d_cand.cpu().numpy().view(np.uint32), cand_buf.view(np.uint32)), what
    assert np.array_equal(d_live.cpu().numpy(), live_all), what


@pytest.mark.parametrize("n_shards", [1, 3])
@pytest.mark.parametrize("n", [1, 5, 8])
@pytest.mark.parametrize("m", [0, 1, 31, 32])
@pytest.mark.parametrize("rows", [1, 63, 64, 65, 300])
def test_merge_kernel_equals_the_reference_and_touches_nothing_else(gpu, rows, m, n, n_shards):
    _kernel_case(gpu, rows, m, n, n_shards, rows, 100000 * n + 100 * rows + m + 7 * n_shards)
    _kernel_case(gpu, rows, m, n, n_shards, rows + 5, 100000 * n + 100 * rows + m + 7 * n_shards + 50)  # ld_cand > rows


# ------------------------------------------------------------------------------------------------------------------ the host path
class Pair(ShardPair):
    """ONE GalleryIndex and one GalleryShards over the same rows, appended in the same order (so every part but the last is full),
    and the comparisons between them"""

    def __init__(self, kind, gpu, G, shard_rows, extra=100):
        # G + extra gallery rows, 40 queries, about four rows per pid: the exact-level rows of test_gallery_shards_gpu or unit random rows
        super().__init__(gpu, shard_inputs(kind, 41 + G, 40, G + extra, (G + extra) // 4), shard_rows)
        self.at = 0
        self.add(G)

    def add(self, count):
        lo, hi = self.at, self.at + count
        self.one.add(self.g[lo:hi], self.pids[lo:hi], normalize=self.normalize)
        self.sh.add(self.g[lo:hi], self.pids[lo:hi], normalize=self.normalize)
        self.at = hi

    def remove(self, rows=None, pids=None):
        if pids is not None:
            assert self.sh.remove(pids=pids) == self.one.remove(pids=pids)
        else:
            rows = torch.as_tensor(rows, dtype=torch.int64)
            assert self.sh.remove(rows=self.to_global(rows)) == self.one.remove(rows=rows)
        assert self.sh.live_count == self.one.live_count

    def same_graph(self, what=""):
        """the shards' lists and values against the ONE index's, as they stand"""
        sh, one = self.sh, self.one
        assert sh.neighbours_current and sh.neighbours_refreshable and one.neighbours_current, what
        assert [tuple(t.shape) for t in sh.neighbours] == [(len(p), one.neighbours.shape[1]) for p in sh.parts], what
        nn, val = torch.cat(sh.neighbours), torch.cat(sh.neighbour_values)
        assert nn.dtype == torch.int32 and torch.equal(nn.long(), self.to_global(one.neighbours)), what
        assert torch.equal(val.view(torch.int32), one.neighbour_values.view(torch.int32)), what
        dead = ~one.live
        assert bool((nn[dead] == -1).all()) and bool(torch.isneginf(val[dead]).all()), what

    def build(self, n):
        self.sh.build_neighbours(n)
        self.one.build_neighbours(n)
        self.same_graph(("build", n))

    def check(self, name, Q, k, alpha=0.05, mask=None):
        """sh.<name>(k) against the one index at k' = min(k, what it can give), padded with absent slots"""
        one, sh = self.one, self.sh
        q = self.q[:Q]
        kk = min(k, len(one) if mask is not None else one.live_count)
        got = getattr(sh, name)(q, k=k, alpha=alpha, normalize=self.normalize, mask=None if mask is None else self.split(mask))
        want = getattr(one, name)(q, k=kk, alpha=alpha, normalize=self.normalize, mask=mask)
        what = (name, Q, k, alpha)
        assert len(got) == len(want) and all(tuple(t.shape) == (Q, k) for t in got), what
        self.compare(got, want, kk, what)
        return got


SHAPES = {99: 32, 300: 96}  # 99 rows in parts of 32 / 32 / 32 / 3 (the last part is shorter than n = 5 and n = 8); 300 in 96 / 96 / 96 / 12


@pytest.fixture(scope="module", params=[("ties", 99), ("random", 99), ("ties", 300), ("random", 300)], ids=lambda p: "%s-%d" % p)
def pair(request, gpu):
    kind, G = request.param
    p = Pair(kind, gpu, G, SHAPES[G])
    assert [len(x) for x in p.sh.parts] == ([32, 32, 32, 3] if G == 99 else [96, 96, 96, 12])
    p.build(5)
    return p


@pytest.mark.parametrize("kind", ["ties", "random"])
@pytest.mark.parametrize("G", [99, 300])
def test_build_equals_the_one_index(gpu, kind, G):
    p = Pair(kind, gpu, G, SHAPES[G])
    assert p.sh.neighbours is None and not p.sh.neighbours_current
    for n in (1, 5, 8):
        p.build(n)
    if kind == "ties":  # exact duplicates across the cuts: equal values, ordered by global row
        nn, val = torch.cat(p.sh.neighbours).long(), torch.cat(p.sh.neighbour_values)
        tied = val[:, 1:] == val[:, :-1]
        assert bool(tied.any()) and bool((nn[:, 1:][tied] > nn[:, :-1][tied]).all())
        assert bool(((nn >> SG.SHARD_BITS) != (nn[:, :1] >> SG.SHARD_BITS)).any())


@pytest.mark.parametrize("Q", [1, 3, 32, 33])
def test_reranked_searches_equal_the_one_index(pair, Q):
    G = len(pair.one)
    for k in (1, 10, 100, G):
        pair.check("search_reranked", Q, k)
        pair.check("search_reranked_pids", Q, k)
    pair.check("search_reranked", Q, 10, alpha=0.3)
    pair.check("search_reranked_pids", Q, 10, alpha=0.3)


def test_the_bonus_changes_the_order_somewhere(pair):
    plain = pair.sh.shortlist(pair.q, k=10, normalize=pair.normalize)
    got = pair.sh.search_reranked(pair.q, k=10, alpha=0.3, normalize=pair.normalize)
    assert not torch.equal(plain[0].view(torch.int32), got[0].view(torch.int32))


@pytest.mark.parametrize("Q", [3, 33])
def test_masks_per_part(pair, Q):
    G = len(pair.one)
    gen = torch.Generator().manual_seed(3)
    mask = (torch.rand(G, generator=gen) < 0.5).to(pair.q.device)
    for k in (1, 10, 100, G):
        pair.check("search_reranked", Q, k, mask=mask)
        pair.check("search_reranked_pids", Q, k, mask=mask.to(torch.uint8))
    few = torch.zeros(G, dtype=torch.bool, device=pair.q.device)
    few[G - 2 :] = True  # fewer allowed rows than n, all in the last part: the query's own list is short
    pair.check("search_reranked", Q, 10, mask=few)
    pair.check("search_reranked_pids", Q, 10, mask=few)


@pytest.mark.parametrize("Q", [1, 33])
def test_alpha_zero_is_the_shortlist_bit_for_bit(pair, Q):
    q = pair.q[:Q]
    gen = torch.Generator().manual_seed(5)
    mask = (torch.rand(len(pair.one), generator=gen) < 0.6).to(q.device)
    for m in (None, pair.split(mask)):
        for k in (10, 100):
            a, b = pair.sh.search_reranked(q, k=k, alpha=0.0, normalize=pair.normalize, mask=m), pair.sh.shortlist(q, k=k, normalize=pair.normalize, mask=m)
            assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1], b[1])
            a, b = pair.sh.search_reranked_pids(q, k=k, alpha=0.0, normalize=pair.normalize, mask=m), pair.sh.shortlist_pids(q, k=k, normalize=pair.normalize, mask=m)
            assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    pair.check("search_reranked", Q, 10, alpha=0.0)


@pytest.mark.parametrize("G", [99, 300])
def test_n_8_with_a_part_shorter_than_n(gpu, G):
    p = Pair("random", gpu, G, SHAPES[G])
    p.build(8)
    for Q in (3, 33):
        for k in (10, G):
            p.check("search_reranked", Q, k)
            p.check("search_reranked_pids", Q, k)


@pytest.mark.parametrize("kind", ["ties", "random"])
@pytest.mark.parametrize("G", [99, 300])
def test_removal_in_two_parts_of_a_whole_part_and_by_pid(gpu, kind, G):
    p = Pair(kind, gpu, G, SHAPES[G])
    S = SHAPES[G]
    p.build(5)
    p.remove(rows=[3, S - 1, 2 * S + 5, 2 * S + 6, 3 * S])  # parts 0 and 2 (and 3: its first row)
    assert not p.sh.neighbours_current
    with pytest.raises(RuntimeError, match="search_reranked: the neighbour graph is stale.*build_neighbours"):
        p.sh.search_reranked(p.q[:3], k=5, normalize=p.normalize)
    p.build(5)
    for Q in (3, 33):
        p.check("search_reranked", Q, 10)
        p.check("search_reranked_pids", Q, G)
    p.remove(rows=torch.arange(S, 2 * S))  # part 1 entirely: it contributes absent lists
    assert p.sh.parts[1].live_count == 0
    p.build(5)
    p.check("search_reranked", 33, 100)
    p.check("search_reranked_pids", 1, 10)
    p.remove(pids=p.pids[[0, S + 4, 2 * S + 50 if G == 300 else 2 * S + 9, G - 1]])
    p.build(8)
    gen = torch.Generator().manual_seed(8)
    mask = (torch.rand(G, generator=gen) < 0.6).to(gpu)
    p.check("search_reranked", 33, G)
    p.check("search_reranked_pids", 3, 10, mask=mask)


def _refresh_and_check(p, what, counts=None):
    """refresh_neighbours on the stale shards: against a fresh build of the ONE index on the same contents, against a fresh build of
    the shards themselves, and the counts"""
    n = p.sh.neighbours[0].shape[1]
    assert not p.sh.neighbours_current and p.sh.neighbours_refreshable, what
    got = p.sh.refresh_neighbours()
    p.one.build_neighbours(n)
    p.same_graph(what)
    nn, val = [t.clone() for t in p.sh.neighbours], [t.clone() for t in p.sh.neighbour_values]
    p.sh.build_neighbours(n)
    assert all(torch.equal(a, b) for a, b in zip(nn, p.sh.neighbours)), what
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(val, p.sh.neighbour_values)), what
    if counts is not None:
        assert got == counts, (what, got)
    assert p.sh.refresh_neighbours() == (0, 0)
    return got


@pytest.mark.parametrize("n", [5, 8])
@pytest.mark.parametrize("kind", ["ties", "random"])
@pytest.mark.parametrize("G", [99, 300])
def test_refresh_equals_a_fresh_build(gpu, kind, G, n):
    p = Pair(kind, gpu, G, SHAPES[G])
    S = SHAPES[G]
    p.build(n)
    # one row
    p.add(1)
    assert not p.sh.neighbours_current and bool((p.sh.neighbours[-1][-1] == -1).all()) and bool(torch.isneginf(p.sh.neighbour_values[-1][-1]).all())
    _refresh_and_check(p, "add 1", (1, 0))
    # 40 rows that spill into a newly opened part (99 rows: they fill the last part and open the next; 300 rows: 90 rows do)
    before = p.sh.n_shards
    p.add(40 if G == 99 else 90)
    assert p.sh.n_shards == before + 1
    _refresh_and_check(p, "add with a new part", (40 if G == 99 else 90, 0))
    p.check("search_reranked", 33, 10)
    # rows that other rows' lists hold
    nn = p.to_global(p.one.neighbours)  # (the one index is current: its lists, as global ids)
    own = p.to_global(torch.arange(len(p.one), device=nn.device))
    others = nn[(nn != own[:, None]) & (nn >= 0)]
    held = torch.unique(others)[:: max(1, torch.unique(others).numel() // 4)][:4]
    back = {g: r for r, g in enumerate(own.tolist())}
    p.remove(rows=[back[int(h)] for h in held])
    got = _refresh_and_check(p, "remove held rows")
    assert got[0] == 0 and got[1] > 0
    # rows that no other row's list holds
    nn = p.to_global(p.one.neighbours)
    others = set(nn[(nn != own[:, None]) & (nn >= 0)].tolist())
    free = [r for r in range(len(p.one)) if int(own[r]) not in others and bool(p.one.live[r])][:3]
    if free:
        p.remove(rows=free)
        _refresh_and_check(p, "remove rows no list holds", (0, 0))
    # an add and a remove together: old rows and just-added ones, in several parts
    p.add(7)
    p.remove(rows=[1, S + 2, len(p.one) - 2])
    got = _refresh_and_check(p, "add and remove")
    assert got[0] == 6
    p.check("search_reranked", 33, 100)
    p.check("search_reranked_pids", 3, 10)


def test_state_dict_round_trip(gpu):
    from textreid_amd import GalleryShards

    p = Pair("ties", gpu, 99, 32)
    p.build(5)
    p.remove(rows=[4, 70])
    sd = p.sh.state_dict()
    assert sd["neighbours"] is None and sd["neighbour_values"] is None  # (stale: neither lists nor values are saved)
    p.sh.refresh_neighbours()
    p.one.build_neighbours(5)
    sd = p.sh.state_dict()
    assert [tuple(t.shape) for t in sd["neighbours"]] == [(32, 5), (32, 5), (32, 5), (3, 5)] and sd["neighbours"][0].dtype == torch.int32
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(sd["neighbour_values"], p.sh.neighbour_values))
    back = GalleryShards()
    back.load_state_dict(sd)
    assert back.neighbours_current and back.neighbours_refreshable and back.shard_rows == 32
    assert all(torch.equal(a, b) for a, b in zip(back.neighbours, p.sh.neighbours))
    mine, p.sh = p.sh, back
    p.check("search_reranked", 33, 10)
    p.check("search_reranked_pids", 3, 100)
    p.add(40)  # (the loaded shards go on: an add that opens parts, then a refresh)
    _refresh_and_check(p, "refresh on the loaded shards", (40, 0))
    # a dict written before the graph existed: no graph; lists without values: current, not refreshable
    old = {k: v for k, v in sd.items() if k not in ("neighbours", "neighbour_values")}
    bare = GalleryShards()
    bare.load_state_dict(old)
    assert bare.neighbours is None and not bare.neighbours_current and bare.live_count == mine.live_count
    bare.load_state_dict({k: v for k, v in sd.items() if k != "neighbour_values"})
    assert bare.neighbours_current and not bare.neighbours_refreshable
    a, b = bare.search_reranked(p.q[:5], k=20, normalize=p.normalize), mine.search_reranked(p.q[:5], k=20, normalize=p.normalize)
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1], b[1])


def test_recorded_search_reranked_replays_against_new_queries(pair):
    """a torch.cuda.graph recording of search_reranked and of search_reranked_pids (after one eager call each), replayed after the
    contents of the queries and of the masks changed"""
    G = len(pair.one)
    q = pair.q[:3].clone()
    mask = torch.ones(G, dtype=torch.bool, device=q.device)
    for name, k in (("search_reranked", 10), ("search_reranked_pids", 100)):
        fn = getattr(pair.sh, name)
        fn(q, k=k, alpha=0.2, normalize=pair.normalize, mask=pair.split(mask))
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = fn(q, k=k, alpha=0.2, normalize=pair.normalize, mask=pair.split(mask))
        q.copy_(pair.q[5:8])
        mask[::3] = False
        graph.replay()
        torch.cuda.synchronize()
        kk = min(k, G)
        want = getattr(pair.one, name)(pair.q[5:8], k=kk, alpha=0.2, normalize=pair.normalize, mask=mask)
        assert torch.equal(out[0][:, :kk].view(torch.int32), want[0].view(torch.int32)), name
        assert torch.equal(out[1][:, :kk], pair.to_global(want[1])) and (len(out) == 2 or torch.equal(out[2][:, :kk], want[2])), name
        q.copy_(pair.q[:3])
        mask[:] = True


# ------------------------------------------------------------------------------------------------------------------ two ranks
def test_two_ranks():
    """200 | 100 rows and 300 | 0 rows: build_neighbours and both re-ranked searches equal the one-process GalleryIndex on both ranks -
    see tests/gallery_shard_graph_worker.py"""
    run_ranks(2, "gallery_shard_graph_worker.py", ("SHARD_GRAPH_UNEVEN_OK", "SHARD_GRAPH_EMPTY_OK"), 240, TRID_DIST_BACKEND="gloo")
