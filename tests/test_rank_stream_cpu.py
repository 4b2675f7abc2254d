"""CPU: the comparator of the matrix-free rank metrics (tests/rank_stream_ref.py) against the values recorded from the
reference, the new entry points in the header, and the refusals of the Python surface."""

import os
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import oracle.evaluation as OE
import rank_stream_ref as R

NEW = ["trid_rank_ws_floats", "trid_rank_stream_p16", "trid_rank_stream_f32", "trid_rank_pairs_jaccard_f32", "trid_rank_rerank_fix",
       "trid_rank_finalize"]


def _golden(golden_dir):
    g = np.load(os.path.join(golden_dir, "rank.npz"))
    te, ie = F.normalize(torch.from_numpy(g["te"]).double(), dim=1), F.normalize(torch.from_numpy(g["ie"]).double(), dim=1)
    return g, te, ie, torch.from_numpy(g["tp"]), torch.from_numpy(g["ip"])


def _nn(a, b, k=5):
    return torch.argsort(a @ b.t(), dim=1, descending=True)[:, :k]


def test_restatement_reproduces_the_recorded_reference(golden_dir):
    g, te, ie, tp, ip = _golden(golden_dir)
    topk = (1, 5, 10)
    for q, gal, qp, gp, tag in ((te, ie, tp, ip, "re_t2i"), (ie, te, ip, tp, "re_i2t")):
        ptr, _, ranks = R.ranks_ref(q, gal, qp, gp, _nn(q, gal), _nn(gal, gal), 0.05)
        cmc, _, mAP = R.ap_cmc_from_ranks(ptr, ranks, topk)
        assert np.allclose(cmc.numpy(), g[tag + "_cmc"], rtol=1e-6), tag
        assert abs(float(mAP) - float(g[tag + "_map"])) <= 1e-6 * float(g[tag + "_map"]), tag
    ptr, _, ranks = R.ranks_ref(te, ie, tp, ip)
    cmc, _, mAP = R.ap_cmc_from_ranks(ptr, ranks, topk)
    ocmc, omap, _ = OE.rank(torch.from_numpy(g["sim_ti"]), tp, ip, topk, True)
    assert np.allclose(cmc.numpy(), ocmc.numpy(), rtol=1e-6) and abs(float(mAP) - float(omap)) <= 1e-6 * float(omap)


def test_brackets_contain_the_rank():
    gen = torch.Generator().manual_seed(3)
    q, g = torch.randn(7, 16, generator=gen), torch.randn(90, 16, generator=gen)
    qp, gp = torch.randint(0, 9, (7,), generator=gen), torch.randint(0, 9, (90,), generator=gen)
    _, _, r = R.ranks_ref(q, g, qp, gp)
    _, _, lo, hi = R.rank_brackets(q, g, qp, gp, delta=1e-3)
    assert bool(((lo + 1 <= r) & (r <= hi + 1)).all())
    _, _, lo0, hi0 = R.rank_brackets(q, g, qp, gp, delta=0.0)
    assert bool((lo0 + 1 == r).all()) and bool((hi0 + 1 >= r).all())


def test_new_entry_points_declared_and_exported():
    import textreid_amd.lib as L

    for name in NEW:
        assert name in L.EXPORTS, name
    assert L.DECLS["trid_rank_stream_p16"] == ("int", "ppppppppiililip")
    assert L.DECLS["trid_rank_finalize"] == ("int", "ppipppipp")
    assert L.DECLS["trid_rank_ws_floats"] == ("long long", "ii")
    out = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True).stdout
    syms = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    for name in NEW:
        assert name in syms, name
    text = open(L.HEADER_PATH).read()
    assert "evaluation.py:11-37" in text and ":40-65" in text and ":144-163" in text


def test_refusals():
    import textreid_amd.evaluation as E
    import textreid_amd.parallel as P

    q, g = torch.randn(4, 8), torch.randn(6, 8)
    qp, gp = torch.arange(4), torch.arange(6)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        E.positive_ranks(q, g, qp, gp)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        E.rank_from_embeddings(q, g, qp, gp)

    class Fake:
        is_cuda = True

    orig = P.dp_active
    P.dp_active = lambda: True
    try:
        with pytest.raises(NotImplementedError, match="sharded form"):
            E.positive_ranks(Fake(), Fake(), qp, gp)
        with pytest.raises(NotImplementedError, match="sharded form"):
            E.rank_from_embeddings(Fake(), Fake(), qp, gp)
    finally:
        P.dp_active = orig
