"""GPU: the sharded matrix-free rank metrics.  One process through the C ABI (the `offset` contract of trid_rank_stream_p16 /
trid_rank_stream_f32 and trid_rank_rerank_fix_shard, isolated from the collectives): the gallery of test_rank_stream_gpu's tie
inputs is cut into shards that stream one after the other, with the GLOBAL list and their offsets, into one counts buffer, and
the ranks equal the fp64 restatement tests/rank_stream_ref.py exactly.  Two ranks (tests/rank_shard_worker.py, sharing the one
GPU over gloo): evaluation.positive_ranks_sharded / rank_from_embeddings_sharded / tables_sharded against the one-process
results."""

import pytest
import torch

import rank_stream_ref as R
from gallery_support import gpu  # noqa: F401
from rank_launch import run_ranks

pytestmark = pytest.mark.gpu
G = 20011


def _tie_inputs(G):
    """_tie_inputs of test_rank_stream_gpu.py, restated: every product and sum exact in every arithmetic"""
    gen = torch.Generator().manual_seed(11)
    lv = torch.tensor([-1.0, -0.5, 0.0, 0.5, 1.0]) / 8
    q = lv[torch.randint(0, 5, (37, 256), generator=gen)]
    base = lv[torch.randint(0, 5, (40, 256), generator=gen)]
    g = base[torch.randint(0, 40, (G,), generator=gen)]  # every row repeated G / 40 times: hundreds of exact ties per query
    q[0, 0] = 1 / 8
    qp = torch.randint(0, 600, (37,), generator=gen)
    gp = torch.randint(0, 600, (G,), generator=gen)
    gp[:37] = qp  # (every query has a positive)
    return q, g, qp, gp


def _top5(a, b):
    """fp64 top-5 rows of b per row of a, ties to the lower row (the products are exact: any arithmetic gives these)"""
    out = []
    for r0 in range(0, a.shape[0], 4096):
        s = a[r0:r0 + 4096].double() @ b.double().t()
        out.append(torch.sort(s, dim=1, descending=True, stable=True)[1][:, :5])
    return torch.cat(out).contiguous()


@pytest.fixture(scope="module")
def ties(gpu):
    q, g, qp, gp = _tie_inputs(G)
    dq, dg = q.to(gpu), g.to(gpu)
    ref = R.ranks_ref(q, g, qp, gp)
    # neighbour lists: "top5" the fp64 top-5 at the reference's alpha (the term moves few ranks of these inputs); "dense" lists
    # that intersect for almost every pair, alpha = 1/4: J = 1/4 and J = 1 add 1/16 and 1/4 EXACTLY, so the re-ranked values tie
    # exactly too, across the cut, and every other pair of values stays > 4e-4 apart (far beyond fp32 rounding)
    u = torch.arange(5, device=gpu).view(1, -1)
    nn = {"top5": (_top5(dq, dg), _top5(dg, dg), 0.05),
          "dense": ((torch.arange(37, device=gpu).view(-1, 1) % 3 + u).contiguous(), (torch.arange(G, device=gpu).view(-1, 1) % 7 + u).contiguous(), 0.25)}
    ref_re = {k: R.ranks_ref(q, g, qp, gp, a.cpu(), b.cpu(), alpha) for k, (a, b, alpha) in nn.items()}
    return dict(q=dq, g=dg, nn=nn, ref=ref, ref_re=ref_re)


def _own(ptr, idx, lo, n):
    """the entries of the global list whose row lies in [lo, lo + n): (sub-list ptr, LOCAL rows, positions in the list)"""
    own = (idx >= lo) & (idx < lo + n)
    csum = torch.cat([torch.zeros(1, dtype=torch.int64, device=idx.device), own.long().cumsum(0)])
    pos = own.nonzero().reshape(-1)
    return csum[ptr].contiguous(), (idx[pos] - lo).contiguous(), pos


def _bounds(cuts):
    assert sum(cuts) == G
    return [(sum(cuts[:w]), cuts[w]) for w in range(len(cuts))]


def _p16_counts(t, cuts, rerank=None):
    from textreid_amd import ops
    from textreid_amd.evaluation import _neighbour_list
    from textreid_amd.ops import _p, call, stream

    q, g, dev = t["q"], t["g"], t["q"].device
    ptr, idx = (x.to(dev).contiguous() for x in t["ref"][:2])
    if rerank:
        qnn, gnn, alpha = t["nn"][rerank]
    Q, NP = q.shape[0], idx.numel()
    max_list = int((ptr[1:] - ptr[:-1]).max())
    qa, ga = ops.amax(q), ops.amax(g)  # the GLOBAL gallery scale: every shard is packed with it
    q16 = torch.zeros((Q + 31) // 32 * 32, 256, dtype=torch.float32, device=dev)
    call("trid_p16_pack_f32", _p(q), Q, 256, 256, _p(qa), _p(q16), 1, stream())
    shards = []
    for lo, n in _bounds(cuts):
        gs = g[lo:lo + n].contiguous()
        g16 = torch.empty_like(gs)
        call("trid_p16_pack_f32", _p(gs), n, 256, 256, _p(ga), _p(g16), 1, stream())
        shards.append((lo, n, g16))

    def values(g16, p, i):  # mode 0: the gathered rows of a list of LOCAL rows
        v = torch.empty(i.numel(), dtype=torch.float32, device=dev)
        a16 = g16[i]
        call("trid_rank_stream_p16", _p(q16), _p(a16), _p(qa), _p(ga), _p(p), _p(i), _p(v), None, Q, i.numel(), i.numel(), 0, 0, 0, stream())
        return v

    thr = torch.zeros(NP, dtype=torch.float32, device=dev)
    for lo, n, g16 in shards:  # thresholds: per owner
        op, oi, pos = _own(ptr, idx, lo, n)
        v = values(g16, op, oi)
        if rerank:
            gl = gnn[lo:lo + n].contiguous()
            call("trid_rank_pairs_jaccard_f32", _p(op), _p(oi), _p(v), _p(qnn), _p(gl), 5, alpha, Q, oi.numel(), stream())
        thr[pos] = v
    counts = torch.zeros(NP, dtype=torch.int32, device=dev)
    for lo, n, g16 in shards:  # each shard in turn: the GLOBAL list, its offset, one counts buffer
        call("trid_rank_stream_p16", _p(q16), _p(g16), _p(qa), _p(ga), _p(ptr), _p(idx), _p(thr), _p(counts), Q, n, NP, max_list, lo, 1, stream())
        if rerank:
            gl = gnn[lo:lo + n].contiguous()
            nb_ptr, nb_idx = _neighbour_list(qnn, gl)  # pairs (q, LOCAL row)
            assert nb_idx.numel() > 0
            nb_val = values(g16, nb_ptr, nb_idx)
            call("trid_rank_rerank_fix_shard", _p(ptr), _p(idx), _p(thr), _p(counts), _p(nb_ptr), _p(nb_idx), _p(nb_val), _p(qnn),
                 _p(gl), 5, alpha, Q, nb_idx.numel(), lo, stream())
    return counts.cpu().long()


def test_p16_shards_count_exact_ties_across_the_cut(ties):
    """9001 | 11010, both beyond the first panel: the streaming kernel.  Hundreds of exact ties per query straddle the cut; a
    kernel that ignores `offset` breaks them by the LOCAL row and misses the ranks"""
    assert torch.equal(_p16_counts(ties, [9001, 11010]) + 1, ties["ref"][2])


def test_f32_shards_count_exact_ties_across_cut_and_panel(ties):
    """700 | 8192 | 11119 through trid_rank_stream_f32: ties cross the shard boundaries and the 8192-column panel boundary inside
    the last shard.  Pair values: the GLOBAL list and a zero-filled val - a shard writes the entries it owns and no other"""
    from textreid_amd import ops
    from textreid_amd.ops import _p, call, stream

    q, g, dev = ties["q"], ties["g"], ties["q"].device
    ptr, idx = (x.to(dev).contiguous() for x in ties["ref"][:2])
    Q, NP = q.shape[0], idx.numel()
    max_list = int((ptr[1:] - ptr[:-1]).max())
    qa, ga = ops.amax(q), ops.amax(g)
    ws = torch.empty(ops.L.load().trid_rank_ws_floats(Q, 11119), dtype=torch.float32, device=dev)
    thr = torch.zeros(NP, dtype=torch.float32, device=dev)
    shards = [(lo, n, g[lo:lo + n].contiguous()) for lo, n in _bounds([700, 8192, 11119])]
    owned = torch.zeros(NP, dtype=torch.int64, device=dev)
    for lo, n, gs in shards:
        before = thr.clone()
        call("trid_rank_stream_f32", _p(q), _p(gs), _p(ptr), _p(idx), _p(thr), None, Q, n, 256, NP, 0, lo, 16, _p(qa), _p(ga), _p(ws), 0, stream())
        out = (idx < lo) | (idx >= lo + n)
        assert torch.equal(thr[out], before[out])  # entries of other shards: untouched
        owned += (~out).long()
    assert bool((owned == 1).all())
    want = (q.double() @ g.double().t())[torch.repeat_interleave(torch.arange(Q, device=dev), ptr[1:] - ptr[:-1]), idx]
    assert torch.equal(thr.double(), want)  # (exact products)
    counts = torch.zeros(NP, dtype=torch.int32, device=dev)
    for lo, n, gs in shards:
        call("trid_rank_stream_f32", _p(q), _p(gs), _p(ptr), _p(idx), _p(thr), _p(counts), Q, n, 256, NP, max_list, lo, 16, _p(qa), _p(ga),
             _p(ws), 1, stream())
    assert torch.equal(counts.cpu().long() + 1, ties["ref"][2])


@pytest.mark.parametrize("nn", ["top5", "dense"])
def test_sharded_rerank_fix(ties, nn):
    """thresholds with their owner's Jaccard term, the plain count per shard, then trid_rank_rerank_fix_shard over each shard's
    LOCAL neighbour list against the GLOBAL positives: the ranks of s' = s + alpha J exactly"""
    want = ties["ref_re"][nn]
    assert torch.equal(want[0], ties["ref"][0]) and torch.equal(want[1], ties["ref"][1])
    moved = int((want[2] != ties["ref"][2]).sum())
    assert moved > (0 if nn == "top5" else want[2].numel() // 2), moved  # (the term moves ranks on these inputs)
    assert torch.equal(_p16_counts(ties, [9001, 11010], nn) + 1, want[2])


def test_two_ranks():
    """(a) ties over 9001 | 11010, plain and re-ranked; (d) 20011 | 0; (b) random unit rows inside the fp64 brackets and equal to
    the one-process ranks; (c) 9001 | 5000 on the panel path; (e) the four tables on the golden embeddings; (f) no [Q, G_local]
    allocation - see tests/rank_shard_worker.py"""
    run_ranks(2, "rank_shard_worker.py", ("SHARD_TIES_OK", "SHARD_EMPTY_OK", "SHARD_RANDOM_OK", "SHARD_PANEL_OK", "SHARD_TABLES_OK",
                                          "SHARD_ALLOC_OK"), 300, TRID_DIST_BACKEND="gloo")
