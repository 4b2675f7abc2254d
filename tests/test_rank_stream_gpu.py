"""GPU: matrix-free rank metrics (evaluation.positive_ranks / rank_from_embeddings / evaluation(matrix_free=True); csrc
rank_stream.hip, gemm_stream.hip FUSE 5) against the fp64 restatement tests/rank_stream_ref.py and the recorded reference
values (lib/data/metrics/evaluation.py:11-37, 40-65, 144-163)."""

import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import rank_stream_ref as R

pytestmark = pytest.mark.gpu

# fp32-class similarity of unit rows: 3 * 2^-22 for the split + fp32 accumulation over <= 256 terms, with margin (the bound the
# brackets are built with).  The worst |s_gpu - s_fp64| on these inputs has NOT been measured yet; if it exceeds 2e-6, DELTA
# becomes twice the measured value and the figure is recorded here.
DELTA = 4e-6


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda")


def _golden(golden_dir):
    g = np.load(os.path.join(golden_dir, "rank.npz"))
    return g, torch.from_numpy(g["te"]), torch.from_numpy(g["ie"]), torch.from_numpy(g["tp"]), torch.from_numpy(g["ip"])


@pytest.mark.parametrize("rerank", [False, True])
def test_golden(gpu, golden_dir, rerank):
    """C = 32: the panel path.  No value is within 1.6e-4 of a positive's in any table, so cmc is exact."""
    from textreid_amd.evaluation import rank_from_embeddings

    g, te, ie, tp, ip = _golden(golden_dir)
    tn, im = F.normalize(te.double(), dim=1), F.normalize(ie.double(), dim=1)
    for q, gal, qp, gp, tag in ((te, ie, tp, ip, "t2i"), (ie, te, ip, tp, "i2t")):
        cmc, mAP = rank_from_embeddings(q.to(gpu), gal.to(gpu), qp.to(gpu), gp.to(gpu), (1, 5, 10), rerank=rerank)
        if rerank:
            ref_cmc, ref_map = g["re_%s_cmc" % tag], float(g["re_%s_map" % tag])
        else:
            qq, gg = (tn, im) if tag == "t2i" else (im, tn)
            ptr, _, ranks = R.ranks_ref(qq, gg, qp, gp)
            c, _, m = R.ap_cmc_from_ranks(ptr, ranks, (1, 5, 10))
            ref_cmc, ref_map = c.numpy(), float(m)
        assert np.allclose(cmc.cpu().numpy(), ref_cmc, rtol=1e-6, atol=0), (tag, cmc, ref_cmc)
        assert abs(float(mAP) - ref_map) <= 1e-5 * ref_map, (tag, float(mAP), ref_map)
    assert len(rank_from_embeddings(te.to(gpu), ie.to(gpu), tp.to(gpu), ip.to(gpu), (1, 30), get_mAP=False)) == 1


def _tie_inputs(G):
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


@pytest.fixture(scope="module")
def ties():
    q, g, qp, gp = _tie_inputs(9001)
    return q, g, qp, gp, R.ranks_ref(q, g, qp, gp)


@pytest.mark.parametrize("G,path", [(9001, "p16"), (20011, "p16"), (9001, "panel"), (9001, "p16-chunked")])
def test_exact_ties(gpu, ties, G, path, monkeypatch):
    """products and sums exact in every arithmetic: the ranks equal the restatement's, tie rule included.  panel: the same
    inputs through the [Q, 8192] panel path (ties across the chunk boundary at column 8192); p16-chunked: the gathered pair
    list cut into several launches"""
    import textreid_amd.evaluation as E
    from textreid_amd.evaluation import positive_ranks, rank_from_embeddings

    if path == "panel":
        monkeypatch.setattr(E, "USE_SIM_P16", False)
    if path == "p16-chunked":
        monkeypatch.setattr(E, "PAIR_CHUNK", 100)
    if G == 9001:
        q, g, qp, gp, (ptr, gi, ranks) = ties
    else:
        q, g, qp, gp = _tie_inputs(G)
        ptr, gi, ranks = R.ranks_ref(q, g, qp, gp)
    p2, i2, r2 = positive_ranks(q.to(gpu), g.to(gpu), qp.to(gpu), gp.to(gpu))
    assert torch.equal(p2.cpu(), ptr) and torch.equal(i2.cpu(), gi)
    assert r2.dtype == torch.int64 and torch.equal(r2.cpu(), ranks)
    cmc, _, mAP = R.ap_cmc_from_ranks(ptr, ranks, (1, 5, 10))
    c2, m2 = rank_from_embeddings(q.to(gpu), g.to(gpu), qp.to(gpu), gp.to(gpu), (1, 5, 10), normalize=False)
    assert np.allclose(c2.cpu().numpy(), cmc.numpy(), rtol=1e-6) and abs(float(m2) - float(mAP)) <= 1e-6 * float(mAP)


def _random_inputs(C):
    gen = torch.Generator().manual_seed(5 + C)
    Q, G = 48, 20011
    q = F.normalize(torch.randn(Q, C, generator=gen), dim=1)
    g = F.normalize(torch.randn(G, C, generator=gen), dim=1)
    qp = torch.randint(0, 600, (Q,), generator=gen)
    gp = torch.randint(0, 600, (G,), generator=gen)
    qp[3], qp[7] = 700, 701         # query 3: no positive; query 7: 150 positives at rows 0..149 (many passes of the list)
    gp[:150] = 701
    return q, g, qp, gp


@pytest.fixture(scope="module", params=[256, 64])
def rnd(request):
    q, g, qp, gp = _random_inputs(request.param)
    return q, g, qp, gp, R.rank_brackets(q, g, qp, gp, delta=DELTA)


def test_random_ranks_within_brackets(gpu, rnd):
    from textreid_amd.evaluation import positive_ranks, rank_from_embeddings

    q, g, qp, gp, (ptr, gi, lo, hi) = rnd
    assert float((hi - lo).double().mean()) <= 2.0  # (the bracket is a few ranks wide: it cannot quietly become vacuous)
    dq, dg, dqp, dgp = q.to(gpu), g.to(gpu), qp.to(gpu), gp.to(gpu)
    p2, i2, r = positive_ranks(dq, dg, dqp, dgp)
    assert torch.equal(p2.cpu(), ptr) and torch.equal(i2.cpu(), gi) and r.numel() == lo.numel()
    assert int(ptr[4] - ptr[3]) == 0 and int(ptr[8] - ptr[7]) == 150
    r = r.cpu()
    bad = ~((lo + 1 <= r) & (r <= hi + 1))
    assert not bool(bad.any()), (int(bad.sum()), r[bad][:5], lo[bad][:5], hi[bad][:5])
    # run-to-run: integer counts, bit-identical
    assert torch.equal(positive_ranks(dq, dg, dqp, dgp)[2].cpu(), r)
    topk = (1, 5, 10, 50)
    cmc, ap, mAP = R.ap_cmc_from_ranks(ptr, r, topk)
    c2, m2 = rank_from_embeddings(dq, dg, dqp, dgp, topk, normalize=False)
    assert np.allclose(c2.cpu().numpy(), cmc.numpy(), rtol=1e-6)
    assert torch.isnan(ap[3]) and torch.isnan(m2)  # the empty query's AP is NaN, as the reference; so is the mean
    # AP per query from the finalise kernel on the returned ranks, elementwise: NaN exactly at the empty query 3, the query
    # with 150 positives (more than a wave's worth) included
    from textreid_amd import ops

    counts = (p2.new_tensor(r.tolist()) - 1).to(torch.int32).contiguous()
    topk_t = torch.tensor(topk, dtype=torch.int64, device=gpu)
    first = torch.empty(48, dtype=torch.int32, device=gpu)
    gap = torch.empty(48, dtype=torch.float32, device=gpu)
    gcmc = torch.empty(4, dtype=torch.float32, device=gpu)
    ops.call("trid_rank_finalize", ops._p(counts), ops._p(p2), 48, ops._p(first), ops._p(gap), ops._p(topk_t), 4, ops._p(gcmc), ops.stream())
    gap = gap.cpu().double()
    nan = torch.isnan(gap)
    assert nan.tolist() == [i == 3 for i in range(48)]
    assert bool(((gap[~nan] - ap[~nan]).abs() <= 1e-5 * ap[~nan]).all()), (gap - ap).abs().max()
    first = first.cpu().long()
    want_first = torch.tensor([int(r[ptr[i]:ptr[i + 1]].min()) - 1 if ptr[i + 1] > ptr[i] else 0x7FFFFFFF for i in range(48)])
    assert torch.equal(first, want_first)
    keep = torch.ones(48, dtype=torch.bool)
    keep[3] = False
    c3, m3 = rank_from_embeddings(dq[keep], dg, dqp[keep], dgp, topk, normalize=False)
    ref = float(ap[keep].mean() * 100)
    assert abs(float(m3) - ref) <= 1e-5 * ref


def test_duplicates_rank_consecutively(gpu, rnd):
    """a positive row copied to further positions compares EQUAL to itself in both sub-passes: consecutive ranks in index order"""
    from textreid_amd.evaluation import positive_ranks

    q, g, qp, gp, _ = rnd
    g, gp = g.clone(), gp.clone()
    gen = torch.Generator().manual_seed(1)
    cases = []
    for qq in (0, 11, 30):
        src = int((gp == qp[qq]).nonzero()[0])
        dst = torch.randperm(g.shape[0] - 200, generator=gen)[:5] + 200
        dst = dst[(gp[dst] != qp[qq])]
        g[dst] = g[src].clone()
        gp[dst[:3]] = qp[qq]
        gp[dst[3:]] = 900 + qq
        cases.append((qq, src, dst[:3].tolist(), dst[3:].tolist()))
    ptr, idx, r = (t.cpu() for t in positive_ranks(q.to(gpu), g.to(gpu), qp.to(gpu), gp.to(gpu)))
    for qq, src, same, foreign in cases:
        rows = idx[ptr[qq]:ptr[qq + 1]].tolist()
        rk = r[ptr[qq]:ptr[qq + 1]].tolist()
        group = sorted([src] + same)
        got = [rk[rows.index(j)] for j in group]
        want = [got[0] + k + sum(1 for f in foreign if group[0] < f < j) for k, j in enumerate(group)]
        assert got == want, (qq, group, foreign, got)


def test_matches_the_matrix_path(gpu, ties, golden_dir, tmp_path):
    from textreid_amd import ops
    from textreid_amd.evaluation import evaluation, rank, rank_from_embeddings

    q, g, qp, gp, _ = ties
    dq, dg = q.to(gpu), g.to(gpu)
    cmc, mAP, _ = rank(ops.linear(dq, dg), qp.to(gpu), gp.to(gpu), (1, 5, 10), get_mAP=True)
    c2, m2 = rank_from_embeddings(dq, dg, qp.to(gpu), gp.to(gpu), (1, 5, 10), normalize=False)
    assert torch.equal(c2, cmc) and abs(float(m2) - float(mAP)) <= 1e-6 * float(mAP)

    _, te, ie, _, ip = _golden(golden_dir)
    image_ids = [i * 25 // 40 for i in range(40)]
    pids = [int(ip[k]) for k in image_ids]  # (a caption carries its image's identity: every query has a positive)

    class DS:
        def get_id_info(self, idx):
            return image_ids[idx], pids[idx]

    preds = {i: [ie[image_ids[i]].to(gpu), te[i].to(gpu)] for i in range(40)}
    evaluation(DS(), preds, str(tmp_path), [1, 5, 10], save_data=False, rerank=True)
    want = {k: (v[0].cpu().numpy().copy(), float(v[1])) for k, v in evaluation.last_results.items()}
    evaluation(DS(), preds, str(tmp_path), [1, 5, 10], save_data=True, rerank=True, matrix_free=True)
    saved = np.load(os.path.join(str(tmp_path), "inference_embed.npz"))
    assert set(saved.files) == {"image_pid", "text_pid", "image_embed", "text_embed"}
    for rnd_ in range(2):
        got = evaluation.last_results
        assert set(got) == set(want)
        for k, (c0, m0) in want.items():
            assert np.array_equal(got[k][0].cpu().numpy(), c0), k
            assert abs(float(got[k][1]) - m0) <= 1e-5 * m0, k
        evaluation(DS(), None, str(tmp_path), [1, 5, 10], save_data=False, rerank=True, matrix_free=True)


def test_no_query_by_gallery_allocation(gpu):
    from textreid_amd.evaluation import rank_from_embeddings

    Q, G = 1024, 40960
    gen = torch.Generator().manual_seed(2)
    q = F.normalize(torch.randn(Q, 256, generator=gen), dim=1).to(gpu)
    g = F.normalize(torch.randn(G, 256, generator=gen), dim=1).to(gpu)
    qp = torch.arange(Q, device=gpu)
    gp = (torch.arange(G, device=gpu) * 7919) % 20000
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    cmc, mAP = rank_from_embeddings(q, g, qp, gp, (1, 5, 10), normalize=False)
    torch.cuda.synchronize()
    assert torch.cuda.max_memory_allocated() - before < Q * G * 4
    assert bool(torch.isfinite(mAP))


def test_declines_inside_a_capture(gpu):
    """the list lengths are host values: the call refuses a capturing stream instead of reading the device in it"""
    from textreid_amd.evaluation import positive_ranks

    q, g = torch.randn(8, 32, device=gpu), torch.randn(64, 32, device=gpu)
    qp, gp = torch.arange(8, device=gpu), torch.arange(64, device=gpu) % 8
    assert positive_ranks(q, g, qp, gp)[2].numel() == 64
    s = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            with pytest.raises(RuntimeError, match="stream capture"):
                positive_ranks(q, g, qp, gp)
            _ = q * 2.0
