"""One rank of tests/test_rank_shard_gpu.py::test_two_ranks: the sharded matrix-free rank metrics (evaluation.*_sharded) on this
rank's gallery shard against the one-process results, which are computed on the whole gallery BEFORE init_process_group (the
unsharded entry points refuse under a process group), and against the fp64 restatement tests/rank_stream_ref.py.  Every rank
checks its own results (they must be identical on every rank); rank 0 prints one tag per case."""

import os
import sys
import tempfile

import numpy as np
import torch
import torch.distributed as dist
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import rank_stream_ref as R  # noqa: E402

# fp32-class similarity of unit rows: 3 * 2^-22 for the split + fp32 accumulation over <= 256 terms, with margin (the bound the
# brackets are built with).  The worst |s_gpu - s_fp64| on these inputs has NOT been measured yet; if it exceeds 2e-6, DELTA
# becomes twice the measured value and the figure is recorded here.
DELTA = 4e-6
TOPK = (1, 5, 10)


def tie_inputs(G):
    """_tie_inputs of tests/test_rank_stream_gpu.py, restated"""
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


def random_inputs(C):
    """_random_inputs of tests/test_rank_stream_gpu.py, restated"""
    gen = torch.Generator().manual_seed(5 + C)
    Q, G = 48, 20011
    q = F.normalize(torch.randn(Q, C, generator=gen), dim=1)
    g = F.normalize(torch.randn(G, C, generator=gen), dim=1)
    qp = torch.randint(0, 600, (Q,), generator=gen)
    gp = torch.randint(0, 600, (G,), generator=gen)
    qp[3], qp[7] = 700, 701         # query 3: no positive; query 7: 150 positives at rows 0..149 (many passes of the list)
    gp[:150] = 701
    return q, g, qp, gp


def same_metrics(got, want_cmc, want_map):
    return np.allclose(got[0].cpu().numpy(), np.asarray(want_cmc), rtol=1e-6, atol=0) and abs(float(got[1]) - float(want_map)) <= 1e-6 * float(want_map)


def main():
    r, W = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    assert W == 2
    dev = torch.device("cuda", r % torch.cuda.device_count())
    torch.cuda.set_device(dev)
    import textreid_amd.evaluation as E

    def cut(sizes):
        lo = sum(sizes[:r])
        return lo, lo + sizes[r]

    # ---------------- one process, the whole gallery: before the process group exists
    one = {}
    q, g, qp, gp = tie_inputs(20011)
    dq, dg, dqp, dgp = q.to(dev), g.to(dev), qp.to(dev), gp.to(dev)
    qnn, gnn = E._topk_neighbours(dq, dg, 5), E._topk_neighbours(dg, dg, 5)
    one["tie"] = dict(
        t=(dq, dg, dqp, dgp), nn=(qnn, gnn),
        plain=E.positive_ranks(dq, dg, dqp, dgp), re=E.positive_ranks(dq, dg, dqp, dgp, qnn, gnn),
        m_plain=E.rank_from_embeddings(dq, dg, dqp, dgp, TOPK, normalize=False),
        m_re=E.rank_from_embeddings(dq, dg, dqp, dgp, TOPK, normalize=False, rerank=True),
        ref=R.ranks_ref(q, g, qp, gp), ref_re=R.ranks_ref(q, g, qp, gp, qnn.cpu(), gnn.cpu()))
    q, g, qp, gp = random_inputs(256)
    dq, dg, dqp, dgp = q.to(dev), g.to(dev), qp.to(dev), gp.to(dev)
    qnn, gnn = E._topk_neighbours(dq, dg, 5), E._topk_neighbours(dg, dg, 5)
    one["rnd"] = dict(
        t=(dq, dg, dqp, dgp), nn=(qnn, gnn),
        plain=E.positive_ranks(dq, dg, dqp, dgp), re=E.positive_ranks(dq, dg, dqp, dgp, qnn, gnn),
        br=R.rank_brackets(q, g, qp, gp, delta=DELTA), br_re=R.rank_brackets(q, g, qp, gp, qnn.cpu(), gnn.cpu(), delta=DELTA))
    q, g, qp, gp = tie_inputs(14001)
    one["panel"] = dict(t=(q.to(dev), g.to(dev), qp.to(dev), gp.to(dev)), ref=R.ranks_ref(q, g, qp, gp))
    gold = np.load(os.path.join(ROOT, "tests", "golden", "rank.npz"))
    ie, te = E.l2_normalize_rows(torch.from_numpy(gold["ie"]).to(dev)), E.l2_normalize_rows(torch.from_numpy(gold["te"]).to(dev))
    ip, tp = torch.from_numpy(gold["ip"]).to(dev), torch.from_numpy(gold["tp"]).to(dev)
    tables = {}
    with tempfile.TemporaryDirectory() as tmp:
        np.savez(os.path.join(tmp, "inference_embed.npz"), image_pid=ip.cpu().numpy(), text_pid=tp.cpu().numpy(),
                 image_embed=ie.cpu().numpy(), text_embed=te.cpu().numpy())
        for re in (True, False):
            E.evaluation(None, None, tmp, list(TOPK), save_data=False, rerank=re, matrix_free=True)
            tables[re] = {k: (v[0].cpu().numpy().copy(), None if v[1] is None else float(v[1])) for k, v in E.evaluation.last_results.items()}
    torch.cuda.synchronize()

    dist.init_process_group(os.environ.get("TRID_DIST_BACKEND", "gloo"), init_method="env://")
    assert dist.get_world_size() == 2 and dist.get_rank() == r

    def tag(name):
        dist.barrier()
        if r == 0:
            print(name, flush=True)

    def eq3(a, b):
        return all(torch.equal(x.cpu(), y.cpu()) for x, y in zip(a, b))

    # ---------------- (a) exact ties straddling the cut 9001 | 11010: the streaming P16 kernel on both ranks
    o = one["tie"]
    dq, dg, dqp, dgp = o["t"]
    lo, hi = cut([9001, 11010])
    got = E.positive_ranks_sharded(dq, dg[lo:hi], dqp, dgp[lo:hi])
    assert got[2].dtype == torch.int64 and eq3(got, o["plain"]) and eq3(got, o["ref"]), "tie ranks"
    cmc, _, mAP = R.ap_cmc_from_ranks(o["ref"][0], o["ref"][2], TOPK)
    m = E.rank_from_embeddings_sharded(dq, dg[lo:hi], dqp, dgp[lo:hi], TOPK, normalize=False)
    assert same_metrics(m, cmc.numpy(), mAP) and same_metrics(m, o["m_plain"][0].cpu().numpy(), o["m_plain"][1]), "tie metrics"
    qnn, gnn = o["nn"]
    got = E.positive_ranks_sharded(dq, dg[lo:hi], dqp, dgp[lo:hi], qnn, gnn[lo:hi])
    assert eq3(got, o["re"]) and eq3(got, o["ref_re"]), "tie re-ranked ranks"
    sh = E._Shards(dq, dg[lo:hi].contiguous())
    assert sh.p16 and sh.offset == lo and sh.G == 20011
    sq, sg = sh.neighbours(5)  # (ties in the neighbour match go to the lower GLOBAL row, whatever the shard)
    assert torch.equal(sq, qnn) and torch.equal(sg, gnn[lo:hi]), "sharded neighbour lists"
    cmc, _, mAP = R.ap_cmc_from_ranks(o["ref_re"][0], o["ref_re"][2], TOPK)
    m = E.rank_from_embeddings_sharded(dq, dg[lo:hi], dqp, dgp[lo:hi], TOPK, normalize=False, rerank=True)
    assert same_metrics(m, cmc.numpy(), mAP) and same_metrics(m, o["m_re"][0].cpu().numpy(), o["m_re"][1]), "tie re-ranked metrics"
    tag("SHARD_TIES_OK")

    # ---------------- (d) shards 20011 | 0: the empty rank joins every collective and launches no rank kernel
    lo, hi = cut([20011, 0])
    names = []
    orig_call = E.call
    E.call = lambda name, *a: (names.append(name), orig_call(name, *a))[1]
    try:
        got = E.positive_ranks_sharded(dq, dg[lo:hi], dqp, dgp[lo:hi])
        got_re = E.positive_ranks_sharded(dq, dg[lo:hi], dqp, dgp[lo:hi], qnn, gnn[lo:hi])
        m = E.rank_from_embeddings_sharded(dq, dg[lo:hi], dqp, dgp[lo:hi], TOPK, normalize=False, rerank=True)
    finally:
        E.call = orig_call
    assert eq3(got, o["plain"]) and eq3(got_re, o["re"]) and same_metrics(m, o["m_re"][0].cpu().numpy(), o["m_re"][1]), "empty shard"
    if r == 1:
        assert not [n for n in names if n.startswith(("trid_rank_stream", "trid_rank_rerank", "trid_rank_pairs", "trid_sim_topk"))], names
    tag("SHARD_EMPTY_OK")

    # ---------------- (b) random unit rows, 9001 | 11010: the one-process bits (global scale), inside the fp64 brackets
    o = one["rnd"]
    dq, dg, dqp, dgp = o["t"]
    lo, hi = cut([9001, 11010])
    for key, nn, br in (("plain", (None, None), o["br"]), ("re", o["nn"], o["br_re"])):
        ptr, gi, blo, bhi = br
        assert float((bhi - blo).double().mean()) <= 2.0  # (the bracket is a few ranks wide: it cannot quietly become vacuous)
        got = E.positive_ranks_sharded(dq, dg[lo:hi], dqp, dgp[lo:hi], nn[0], None if nn[1] is None else nn[1][lo:hi])
        assert torch.equal(got[0].cpu(), ptr) and torch.equal(got[1].cpu(), gi) and got[2].numel() == blo.numel(), key
        assert int(ptr[4] - ptr[3]) == 0 and int(ptr[8] - ptr[7]) == 150
        rk = got[2].cpu()
        bad = ~((blo + 1 <= rk) & (rk <= bhi + 1))  # every positive, none left out
        assert not bool(bad.any()), (key, int(bad.sum()), rk[bad][:5], blo[bad][:5], bhi[bad][:5])
        assert eq3(got, o[key]), "random ranks differ from the one-process ranks: " + key
    tag("SHARD_RANDOM_OK")

    # ---------------- (c) ties, 9001 | 5000: one shard fits the first panel, so BOTH ranks take the panel path
    o = one["panel"]
    dq, dg, dqp, dgp = o["t"]
    lo, hi = cut([9001, 5000])
    names = []
    E.call = lambda name, *a: (names.append(name), orig_call(name, *a))[1]
    try:
        got = E.positive_ranks_sharded(dq, dg[lo:hi], dqp, dgp[lo:hi])
    finally:
        E.call = orig_call
    assert "trid_rank_stream_f32" in names and "trid_rank_stream_p16" not in names, names
    assert eq3(got, o["ref"]), "panel path ranks"
    tag("SHARD_PANEL_OK")

    # ---------------- (e) the four tables of evaluation(matrix_free=True), images and texts both split two ways
    ni, nt = ie.shape[0], te.shape[0]
    ilo, ihi = cut([ni // 2 + 1, ni - ni // 2 - 1])
    tlo, thi = cut([nt // 2, nt - nt // 2])
    for re in (True, False):
        res = E.tables_sharded(ie[ilo:ihi], ip[ilo:ihi], te[tlo:thi], tp[tlo:thi], TOPK, rerank=re)
        assert set(res) == set(tables[re]) == ({"t2i", "i2t", "re-t2i", "re-i2t"} if re else {"t2i", "i2t"})
        for k, (c0, m0) in tables[re].items():
            assert np.allclose(res[k][0].cpu().numpy(), c0, rtol=1e-6, atol=0), (k, res[k][0], c0)
            if re:
                assert abs(float(res[k][1]) - m0) <= 1e-5 * m0, (k, float(res[k][1]), m0)
            else:
                assert res[k][1] is None and m0 is None
    tag("SHARD_TABLES_OK")

    # ---------------- (f) nothing of the size of [Q, G_local] is allocated
    Q, G = 1024, 40960
    gen = torch.Generator().manual_seed(2)
    q = F.normalize(torch.randn(Q, 256, generator=gen), dim=1).to(dev)
    g = F.normalize(torch.randn(G, 256, generator=gen), dim=1)
    lo, hi = cut([G // 2, G // 2])
    gl = g[lo:hi].to(dev)
    qp = torch.arange(Q, device=dev)
    gpl = ((torch.arange(G, device=dev) * 7919) % 20000)[lo:hi].contiguous()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    cmc, mAP = E.rank_from_embeddings_sharded(q, gl, qp, gpl, TOPK, normalize=False)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    assert peak < Q * (hi - lo) * 4, (peak, Q * (hi - lo) * 4)
    assert bool(torch.isfinite(mAP))
    tag("SHARD_ALLOC_OK")
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
