"""GalleryShards on the GPU: trid_index_merge_lists_f32 against the numpy reference (gallery_shards_ref) bit for bit, the in-process
form against ONE GalleryIndex over the same rows (values bit for bit, rows after mapping, pids), and the by-rank form on two gloo
ranks sharing the GPU (tests/gallery_shards_worker.py, started by rank_launch.run_ranks).  The pair of the two is
gallery_support.ShardPair with this file's order of adds and its choice of comparator method.  Nothing here needs a tolerance."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import gallery_shards_ref as SR  # noqa: E402
from gallery_support import ShardPair, gpu, shard_inputs  # noqa: E402,F401
from rank_launch import run_ranks  # noqa: E402

G, SHARD = 300, 96  # parts of 96, 96, 96 and 12 rows


# ------------------------------------------------------------------ the kernel
_REF = {}


def kernel_case(S, kin, k, Q, n_pids, sort_lists):
    """inputs and the four reference results (rows / distinct form, with and without bases), computed once per shape"""
    key = (S, kin, k, Q, n_pids, sort_lists)
    if key not in _REF:
        val, row, base, pid = SR.special_inputs(Q, S, kin, 31 * S + kin + Q, n_pids=n_pids, sort_lists=sort_lists)
        _REF[key] = (val, row, base, pid, {(b, d): SR.merge(val, row, k, base if b else None, pid if d else None) for b in (0, 1) for d in (0, 1)})
    return _REF[key]


@pytest.mark.parametrize("Q", [1, 33])
@pytest.mark.parametrize("S,kin,k", [(1, 1, 1), (2, 16, 16), (3, 17, 17), (8, 1024, 1024), (5, 100, 7), (64, 16, 16)])
@pytest.mark.parametrize("n_pids,sort_lists", [(None, False), (5, False), (None, True)])
def test_merge_kernel_equals_the_reference_bit_for_bit(gpu, S, kin, k, Q, n_pids, sort_lists):
    """heavy ties, both zeros, real -inf on present rows, absent slots with junk values, an all-absent list, one pid in every list
    with equal values; n_pids = 5: fewer than k distinct pids; unsorted and sorted lists; with list_base and with NULL"""
    from textreid_amd.index_shards import merge_lists

    val, row, base, pid, want = kernel_case(S, kin, k, Q, n_pids, sort_lists)
    dv, dr, db, dp = (torch.from_numpy(a).to(gpu) for a in (val, row, base, pid))
    for b in (0, 1):
        for d in (0, 1):
            got = merge_lists(dv, dr, k, db if b else None, dp if d else None)
            assert len(got) == (3 if d else 2) and all(tuple(t.shape) == (Q, k) for t in got)
            assert SR.same([t.cpu().numpy() for t in got], want[(b, d)]), ("base" if b else "no base", "distinct" if d else "rows")


def test_merge_kernel_all_absent_and_outputs_only(gpu):
    """every slot absent: all fills; and the launch writes its [Q, k] outputs and nothing behind them"""
    from textreid_amd import lib as L
    from textreid_amd.ops import _p, stream

    Q, S, kin, k = 3, 4, 9, 11
    val = torch.full((Q, S, kin), float("inf"), device=gpu)
    row = torch.full((Q, S, kin), -7, dtype=torch.int64, device=gpu)
    pid = torch.zeros(Q, S, kin, dtype=torch.int64, device=gpu)
    for p in (None, pid):
        ov = torch.full((Q * k + 5,), 123.0, device=gpu)
        orow = torch.full((Q * k + 5,), 99, dtype=torch.int64, device=gpu)
        opid = torch.full((Q * k + 5,), 98, dtype=torch.int64, device=gpu)
        L.call("trid_index_merge_lists_f32", _p(val), _p(row), None, _p(p), Q, S, kin, k, _p(ov), _p(orow), _p(opid), stream())
        assert bool(torch.isneginf(ov[: Q * k]).all()) and bool((orow[: Q * k] == -1).all())
        assert bool((ov[Q * k :] == 123.0).all()) and bool((orow[Q * k :] == 99).all())
        assert bool((opid[: Q * k] == (-1 if p is not None else 98)).all()) and bool((opid[Q * k :] == 98).all())


def test_merge_in_rounds_equals_one_merge(gpu):
    """more candidates than one launch takes (20 lists of 512): groups of lists, then the groups' results"""
    from textreid_amd import GalleryShards

    Q, S, kin, k = 3, 20, 512, 600
    val, row, base, pid = SR.special_inputs(Q, S, kin, 5)
    dv, dr, db, dp = (torch.from_numpy(a).to(gpu) for a in (val, row, base, pid))
    sh = GalleryShards()
    assert SR.same([t.cpu().numpy() for t in sh._merge(dv, dr, None, db, k)], SR.merge(val, row, k, base))
    assert SR.same([t.cpu().numpy() for t in sh._merge(dv, dr, dp, db, k)], SR.merge(val, row, k, base, pid))


# ------------------------------------------------------------------ the in-process form
class Pair(ShardPair):
    """one GalleryIndex and one GalleryShards (shard_rows = 96) over the same 300 rows, and the comparison between them"""

    def __init__(self, kind, gpu, shard_rows=SHARD):
        # 33 queries, pids in [0, 70): every pid about four times, reused across the parts
        super().__init__(gpu, shard_inputs(kind, 19, 33, G, 70), shard_rows)
        self.one.add(self.g, self.pids, normalize=self.normalize)
        # (one add call spanning three parts, then one that fills the third and opens the fourth)
        self.first = [self.sh.add(self.g[:250], self.pids[:250], normalize=self.normalize), self.sh.add(self.g[250:], self.pids[250:], normalize=self.normalize)]

    def check(self, name, Q, k, mask=None, sh=None):
        """sh.<name>(k) against the plain index at k' = min(k, what it can give), padded with absent slots"""
        one, sh = self.one, sh or self.sh
        q = self.q[:Q]
        limit = G if mask is not None else one.live_count
        kk = min(k, limit)
        got = getattr(sh, name)(q, k=k, normalize=self.normalize, mask=None if mask is None else self.split(mask))
        distinct = name.endswith("pids")
        assert len(got) == (3 if distinct else 2) and all(tuple(t.shape) == (Q, k) for t in got), (name, Q, k)
        if kk == 0:
            want = None
        elif Q > 32 or k > 16:  # (the panelled comparators: bit-identical to search / search_pids at k <= 16)
            want = getattr(one, "shortlist_pids" if distinct else "shortlist")(q, k=kk, normalize=self.normalize, mask=mask)
        else:
            want = getattr(one, name)(q, k=kk, normalize=self.normalize, mask=mask)
        self.compare(got, want, kk, (name, Q, k))
        return got


@pytest.fixture(scope="module", params=["ties", "random"])
def pair(request, gpu):
    return Pair(request.param, gpu)


def test_add_spans_parts_and_rows_are_global(pair):
    from textreid_amd.index_shards import SHARD_STRIDE

    sh = pair.sh
    assert [len(p) for p in sh.parts] == [96, 96, 96, 12] and sh.n_shards == 4 and len(sh) == G and sh.live_count == G
    assert pair.first == [0, 2 * SHARD_STRIDE + 58]
    for s, part in enumerate(sh.parts):
        assert torch.equal(part.rows, pair.one.rows[s * 96 : s * 96 + len(part)]) and torch.equal(part.pids, pair.pids[s * 96 : s * 96 + len(part)])
        assert torch.equal(part.rows_p16.view(torch.int32), pair.one.rows_p16[s * 96 : s * 96 + len(part)].view(torch.int32))


@pytest.mark.parametrize("Q", [1, 3, 32, 33])
def test_search_and_search_pids_equal_the_plain_index(pair, Q):
    for k in (1, 10, 16):
        pair.check("search", Q, k)
        pair.check("search_pids", Q, k)


@pytest.mark.parametrize("Q", [1, 3, 32, 33])
def test_shortlists_equal_the_plain_index(pair, Q):
    """k greater than a part (100, 301, 1024) and greater than the total (301, 1024)"""
    for k in (1, 17, 100, 301, 1024):
        pair.check("shortlist", Q, k)
        pair.check("shortlist_pids", Q, k)


@pytest.mark.parametrize("left", ["0", "k-1", "k", "k+1"])
def test_masks_that_leave_few_rows_all_in_the_last_part(pair, left):
    k = 10
    n = {"0": 0, "k-1": k - 1, "k": k, "k+1": k + 1}[left]
    mask = torch.zeros(G, dtype=torch.bool, device=pair.q.device)
    mask[G - n :] = True
    for name in ("search", "search_pids", "shortlist", "shortlist_pids"):
        for Q in (3, 33):
            got = pair.check(name, Q, k, mask=mask)
            if not name.endswith("pids"):
                assert bool((got[1][:, : min(n, k)] >= 0).all()) and bool((got[1][:, min(n, k) :] == -1).all())


def test_random_masks_over_every_part(pair):
    gen = torch.Generator().manual_seed(3)
    mask = (torch.rand(G, generator=gen) < 0.5).to(pair.q.device)
    for name, k in (("search", 16), ("search_pids", 10), ("shortlist", 100), ("shortlist", 301), ("shortlist_pids", 100)):
        pair.check(name, 33, k, mask=mask)
        pair.check(name, 3, k, mask=mask.to(torch.uint8))
    parts = pair.split(mask)
    parts[1] = None  # (no mask for one part: all of its live rows)
    whole = mask.clone()
    whole[96:192] = True
    got = pair.sh.shortlist(pair.q[:3], k=50, normalize=pair.normalize, mask=parts)
    want = pair.one.shortlist(pair.q[:3], k=50, normalize=pair.normalize, mask=whole)
    assert torch.equal(got[0].view(torch.int32), want[0].view(torch.int32)) and torch.equal(got[1], pair.to_global(want[1]))


def test_removal_in_two_parts_a_whole_part_and_by_pid(gpu):
    from textreid_amd import GalleryShards

    for kind in ("ties", "random"):
        p = Pair(kind, gpu)
        gone = torch.tensor([3, 50, 95, 200, 201, 288])  # parts 0 and 2 (and 3: its first row)
        assert p.sh.remove(rows=p.to_global(gone)) == 6 and p.one.remove(rows=gone) == 6
        assert p.sh.remove(rows=p.to_global(gone[:2]).tolist()) == 0  # (already removed: ignored)
        assert p.sh.live_count == p.one.live_count == G - 6 and len(p.sh) == G
        for name, k in (("search", 16), ("search_pids", 16), ("shortlist", 100), ("shortlist", 301), ("shortlist_pids", 100)):
            p.check(name, 33, k)
        whole = torch.arange(96, 192)  # part 1 entirely: it contributes an absent list
        assert p.sh.remove(rows=p.to_global(whole)) == 96 and p.one.remove(rows=whole) == 96 and p.sh.parts[1].live_count == 0
        for name, k in (("search", 10), ("search_pids", 10), ("shortlist", 100), ("shortlist", 301), ("shortlist_pids", 1024)):
            p.check(name, 33, k)
            p.check(name, 1, k)
        pids = p.pids[[0, 100, 250, 299]]
        assert p.sh.remove(pids=pids) == p.one.remove(pids=pids) and p.sh.live_count == p.one.live_count
        gen = torch.Generator().manual_seed(8)
        mask = (torch.rand(G, generator=gen) < 0.6).to(gpu)
        for name, k in (("search", 16), ("search_pids", 10), ("shortlist", 17), ("shortlist", 301), ("shortlist_pids", 100)):
            p.check(name, 33, k)
            p.check(name, 3, k, mask=mask)
        # persistence: the parts' own dicts plus shard_rows; row ids and tombstones survive
        back = GalleryShards()
        back.load_state_dict(p.sh.state_dict())
        assert back.shard_rows == 96 and [len(x) for x in back.parts] == [96, 96, 96, 12] and back.live_count == p.sh.live_count
        for name, k in (("search", 16), ("shortlist_pids", 100)):
            p.check(name, 33, k, sh=back)


def test_one_shard_is_the_plain_index_without_a_merge(gpu):
    from textreid_amd import lib as L

    p = Pair("ties", gpu, shard_rows=G)
    assert p.sh.n_shards == 1 and p.first == [0, 250]
    L.TRACE = []
    try:
        for name, k in (("search", 16), ("search_pids", 10), ("shortlist", 100), ("shortlist", 301), ("shortlist_pids", 1024)):
            p.check(name, 33, k)
        names = {t[0] for t in L.TRACE}
    finally:
        L.TRACE = None
    assert "trid_gemm_p16" in names and "trid_index_merge_lists_f32" not in names


def test_many_shards_at_deep_k_merge_in_rounds(gpu):
    """9 parts of 1024 rows at k = 1024: 9216 candidates per query, more than one launch takes"""
    from textreid_amd import GalleryIndex, GalleryShards
    from textreid_amd.index_shards import SHARD_STRIDE

    gen = torch.Generator().manual_seed(2)
    g = torch.randn(9216, 256, generator=gen).to(gpu)
    g[5000:5400] = g[100:500]  # (exact duplicates across parts)
    q = torch.randn(3, 256, generator=gen).to(gpu)
    pids = torch.randint(0, 3000, (9216,), generator=gen).to(gpu)
    one, sh = GalleryIndex(), GalleryShards(shard_rows=1024)
    one.add(g, pids)
    sh.add(g, pids)
    assert sh.n_shards == 9
    for name in ("shortlist", "shortlist_pids"):
        got, want = getattr(sh, name)(q, k=1024), getattr(one, name)(q, k=1024)
        assert torch.equal(got[0].view(torch.int32), want[0].view(torch.int32)), name
        assert torch.equal(got[1], (want[1] // 1024) * SHARD_STRIDE + want[1] % 1024), name
        assert len(got) == 2 or torch.equal(got[2], want[2]), name


def test_recorded_searches_replay_against_new_queries(pair):
    """torch.cuda.graph recordings of search and shortlist_pids (after one eager call each), replayed after the queries' contents changed"""
    q = pair.q[:3].clone()
    mask = torch.ones(G, dtype=torch.bool, device=q.device)
    for name, k in (("search", 10), ("shortlist_pids", 100)):
        fn = getattr(pair.sh, name)
        fn(q, k=k, normalize=pair.normalize, mask=pair.split(mask))
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = fn(q, k=k, normalize=pair.normalize, mask=pair.split(mask))
        q.copy_(pair.q[5:8])
        mask[::3] = False
        graph.replay()
        torch.cuda.synchronize()
        want = getattr(pair.one, name)(pair.q[5:8], k=k, normalize=pair.normalize, mask=mask)
        assert torch.equal(out[0].view(torch.int32), want[0].view(torch.int32)), name
        assert torch.equal(out[1], pair.to_global(want[1])) and (len(out) == 2 or torch.equal(out[2], want[2])), name
        q.copy_(pair.q[:3])
        mask[:] = True


# ------------------------------------------------------------------ two ranks
def test_two_ranks():
    """200 | 100 rows and 300 | 0 rows: the four searches equal the one-process GalleryIndex on both ranks - see tests/gallery_shards_worker.py"""
    run_ranks(2, "gallery_shards_worker.py", ("SHARDS_UNEVEN_OK", "SHARDS_EMPTY_OK"), 240, TRID_DIST_BACKEND="gloo")
