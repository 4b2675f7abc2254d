#!/usr/bin/env python3
"""Bits and library calls of the retrieval host paths (textreid_amd/evaluation.py, index.GalleryIndex.search for Q > 32), recorded
at the commit BEFORE the top-k launch sequence, the shard merge, the count pass and the table loop were each reduced to one copy
(tests/test_retrieval_flow_gpu.py holds every later commit to them).

Run on the GPU in a checkout of that parent commit, twice, in two processes; the two files must be identical:

    python tests/golden/make_retrieval_parent.py /tmp/a.json && python tests/golden/make_retrieval_parent.py /tmp/b.json
    cmp /tmp/a.json /tmp/b.json && cp /tmp/a.json tests/golden/retrieval_parent.json

Only names that exist on both sides of that change are used: similarity_topk, _topk_neighbours, positive_ranks[_sharded],
rank_from_embeddings[_sharded], evaluation, the module globals USE_SIM_P16 / DEVICE_GATED_FALLBACK / PAIR_CHUNK, GalleryIndex and
textreid_amd.lib.TRACE.  Per case (``compute(case, device)``):

* ``<result>``: sha256 of every returned tensor (integer counts or the outcome of a deterministic merge: equality holds);
* ``calls``: the sorted MULTISET of (entry-point name, scalar arguments) of the case, as {"name(args)": count} - everything runs
  on one stream, so the order of independent calls is free.  One rename is applied before counting: ``trid_rank_rerank_fix`` is
  recorded as ``trid_rank_rerank_fix_shard`` with offset 0 (the entry point every path calls after the change).
"""

import collections
import hashlib
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import oracle.fill as OF  # noqa: E402

SEED = 23
TOPK = (1, 5, 10)
TOPK_SHAPES = [(256, 1, 8193, 3), (256, 70, 8261, 10), (256, 33, 8255, 1), (64, 5, 8192, 10), (64, 5, 8193, 3)]
RANK_INPUTS = ["ties9001", "ties20011", "ties9001:panel", "ties9001:chunk", "rnd256", "rnd64"]
CASES = (["topk:%d:%dx%dx%d" % s for s in TOPK_SHAPES] + ["topk:overflow:host", "topk:overflow:gated", "index:9001", "index:5000"]
         + ["rank:" + n for n in RANK_INPUTS] + ["sharded:ties9001", "sharded:rnd256"]
         + ["evaluation:free:re", "evaluation:free:plain", "evaluation:matrix:re", "evaluation:matrix:plain"])


def _sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def _traced(fn):
    """(fn(), {"name(scalar arguments)": count})"""
    from textreid_amd import lib

    lib.TRACE = []
    try:
        out = fn()
        torch.cuda.synchronize()
        entries = [(e[0], tuple(e[1])) for e in lib.TRACE]
    finally:
        lib.TRACE = None
    calls = collections.Counter()
    for name, scal in entries:
        if name == "trid_rank_rerank_fix":  # (n, alpha, Q, NB[, stream]) -> (n, alpha, Q, NB, offset 0[, stream])
            name, scal = "trid_rank_rerank_fix_shard", scal[:4] + (0,) + scal[4:]
        calls["%s(%s)" % (name, ", ".join(repr(v) for v in scal))] += 1
    return out, dict(sorted(calls.items()))


def tie_inputs(G):
    """_tie_inputs of tests/test_rank_stream_gpu.py, restated"""
    gen = torch.Generator().manual_seed(11)
    lv = torch.tensor([-1.0, -0.5, 0.0, 0.5, 1.0]) / 8
    q = lv[torch.randint(0, 5, (37, 256), generator=gen)]
    base = lv[torch.randint(0, 5, (40, 256), generator=gen)]
    g = base[torch.randint(0, 40, (G,), generator=gen)]
    q[0, 0] = 1 / 8
    qp = torch.randint(0, 600, (37,), generator=gen)
    gp = torch.randint(0, 600, (G,), generator=gen)
    gp[:37] = qp
    return q, g, qp, gp


def random_inputs(C):
    """_random_inputs of tests/test_rank_stream_gpu.py, restated"""
    gen = torch.Generator().manual_seed(5 + C)
    Q, G = 48, 20011
    q = F.normalize(torch.randn(Q, C, generator=gen), dim=1)
    g = F.normalize(torch.randn(G, C, generator=gen), dim=1)
    qp = torch.randint(0, 600, (Q,), generator=gen)
    gp = torch.randint(0, 600, (G,), generator=gen)
    qp[3], qp[7] = 700, 701
    gp[:150] = 701
    return q, g, qp, gp


def overflow_inputs():
    """the inputs of test_fused_similarity_topk_presplit_overflow_and_negative_thresholds (tests/test_match_state_gpu.py), restated"""
    G, Q, C = 8192 * 2 + 1234, 96, 256
    gen = torch.Generator().manual_seed(3)
    gal = torch.zeros(G, C)
    gal[:, 0] = torch.arange(G, dtype=torch.float32) * 1e-4
    gal[:, 1] = torch.randn(G, generator=gen)
    gal[:, 2] = -torch.rand(G, generator=gen) - 0.5
    q = torch.zeros(Q, C)
    q[:32, 0] = 1.0
    q[32:64, 1] = 1.0
    q[64:, 2] = 1.0
    return q, gal


def _rank_inputs(name, dev):
    kind = name.split(":")[0]
    t = tie_inputs(int(kind[4:])) if kind.startswith("ties") else random_inputs(int(kind[3:]))
    return tuple(x.to(dev) for x in t)


def _rank_results(E, t, sharded):
    """the plain and the re-ranked ranks and metrics of one input set -> {key: tensor}"""
    q, g, qp, gp = t
    ranks = E.positive_ranks_sharded if sharded else E.positive_ranks
    metrics = E.rank_from_embeddings_sharded if sharded else E.rank_from_embeddings
    qnn, gnn = E._topk_neighbours(q, g, 5), E._topk_neighbours(g, g, 5)
    out = {"qnn": qnn, "gnn": gnn}
    for tag, nn in (("plain", ()), ("re", (qnn, gnn))):
        for name, x in zip(("ptr", "idx", "ranks"), ranks(q, g, qp, gp, *nn)):
            out["%s:%s" % (tag, name)] = x
        for name, x in zip(("cmc", "mAP"), metrics(q, g, qp, gp, TOPK, normalize=False, rerank=bool(nn))):
            out["%s:%s" % (tag, name)] = x
    return out


def _predictions(dev):
    """the predictions of test_matches_the_matrix_path (tests/test_rank_stream_gpu.py), restated"""
    g = np.load(os.path.join(ROOT, "tests", "golden", "rank.npz"))
    te, ie, ip = torch.from_numpy(g["te"]), torch.from_numpy(g["ie"]), torch.from_numpy(g["ip"])
    image_ids = [i * 25 // 40 for i in range(40)]
    pids = [int(ip[k]) for k in image_ids]

    class DS:
        def get_id_info(self, idx):
            return image_ids[idx], pids[idx]

    return DS(), {i: [ie[image_ids[i]].to(dev), te[i].to(dev)] for i in range(40)}


def compute(case, dev):
    import textreid_amd.evaluation as E
    from textreid_amd.index import GalleryIndex

    kind, _, rest = case.partition(":")
    saved = E.USE_SIM_P16, E.DEVICE_GATED_FALLBACK, E.PAIR_CHUNK
    try:
        if kind == "topk":
            if rest.startswith("overflow"):
                q, g = (x.to(dev) for x in overflow_inputs())
                E.DEVICE_GATED_FALLBACK = rest.endswith("gated")
                run = lambda: E.similarity_topk(q, g, 10, normalize=False)  # noqa: E731
            else:
                C, shape = rest.split(":")
                Q, G, k = (int(v) for v in shape.split("x"))
                q = OF.randn("retrieval:q:" + rest, (Q, int(C)), SEED).to(dev)
                g = OF.randn("retrieval:g:" + rest, (G, int(C)), SEED).to(dev)
                run = lambda: E.similarity_topk(q, g, k)  # noqa: E731
            (vals, idx), calls = _traced(run)
            res = {"vals": vals, "idx": idx}
        elif kind == "index":
            index = GalleryIndex()
            index.add(OF.randn("retrieval:index:" + rest, (int(rest), 256), SEED).to(dev))
            q = OF.randn("retrieval:index:q", (40, 256), SEED).to(dev)
            (vals, rows), calls = _traced(lambda: index.search(q, k=10))
            res = {"vals": vals, "rows": rows}
        elif kind in ("rank", "sharded"):
            t = _rank_inputs(rest, dev)
            E.USE_SIM_P16 = saved[0] and not rest.endswith(":panel")
            if rest.endswith(":chunk"):
                E.PAIR_CHUNK = 100
            res, calls = _traced(lambda: _rank_results(E, t, kind == "sharded"))
        elif kind == "evaluation":
            ds, preds = _predictions(dev)
            form, re = rest.split(":")
            _, calls = _traced(lambda: E.evaluation(ds, preds, None, list(TOPK), save_data=False, rerank=re == "re", matrix_free=form == "free"))
            res = {}
            for k, (cmc, mAP) in E.evaluation.last_results.items():
                res[k + ":cmc"] = cmc
                if mAP is not None:
                    res[k + ":mAP"] = mAP
        else:
            raise KeyError(case)
    finally:
        E.USE_SIM_P16, E.DEVICE_GATED_FALLBACK, E.PAIR_CHUNK = saved
    out = {k: _sha(v) for k, v in res.items()}
    out["calls"] = calls
    return out


if __name__ == "__main__":
    import textreid_amd  # noqa: F401

    dev = torch.device("cuda")
    out = {case: compute(case, dev) for case in CASES}
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print({k: len(v) for k, v in out.items()})
