"""GalleryIndex on the GPU: storage, the one-pass small-batch search against the dense P16 product (gallery_support.dense_product;
exact: same arithmetic, same product order) and against the CPU oracle, adversarial orders, incremental adds, the large-batch route
and graph capture."""

import pytest
import torch

pytestmark = pytest.mark.gpu

import oracle.evaluation as OE  # noqa: E402
import oracle.fill as OF  # noqa: E402
from gallery_support import c_search, dense_product, gpu, Inputs, same_values as same  # noqa: E402,F401

SEED = 8  # every gap among the top k + 1 oracle values of every query is >= 2.1e-5 for the shapes below (checked on the CPU)
SHAPES = [(1, 1, 1), (2, 10, 10), (5, 63, 5), (32, 64, 16), (7, 65, 10), (5, 4099, 16), (3, 8193, 10), (32, 8255, 10), (17, 20037, 10)]
ADV_G = 20037


IN = Inputs("gix:", SEED)
raw = IN.raw


def top_k(sim, k):
    """stable descending sort of the dense product = (value descending, row ascending) -> (values [Q,k], rows [Q,k]) on the CPU"""
    order = torch.sort(sim, dim=1, descending=True, stable=True)
    return order.values[:, :k].contiguous(), order.indices[:, :k].contiguous()


def reference(idx, q_unit, k):
    """the comparator: the top k of gallery_support.dense_product"""
    return top_k(dense_product(idx, q_unit), k)


def built(gpu, Q, G, k):
    """index over the seed-8 gallery of G rows (shared, never modified), the unit queries, the dense reference"""
    idx, te, ie, qu, sim = IN.built(gpu, Q, G)
    return idx, te, ie, qu, top_k(sim, k)


# ----------------------------------------------------------------------------------------------------------- 1. storage
def test_storage_growth_pack_pids_and_state_dict(gpu):
    from textreid_amd import GalleryIndex, ops

    pieces = [1, 63, 64, 65, 700]
    n = sum(pieces)
    x = OF.randn("gix:store", (n, 256), SEED)
    x[5] = 0.0
    x[70] *= 1e20
    x[200] *= 1e-30
    pid = OF.randint("gix:pid", 0, 1000, (n,), SEED)
    xg = x.to(gpu)
    idx = GalleryIndex(dim=256, capacity=100)
    assert idx.capacity == 0  # storage is allocated on the first add
    at, caps = 0, []
    for m in pieces:
        assert idx.add(xg[at : at + m], pids=pid[at : at + m]) == at
        at += m
        caps.append(idx.capacity)
        assert len(idx) == at and idx.capacity >= at
    assert caps[0] == 100 and caps[-1] > caps[0] and len(set(caps)) >= 3  # grew, and more than once
    want = ops.l2norm_rows(xg)[0]
    assert torch.equal(idx.rows.view(torch.int32), want.view(torch.int32))
    ones = torch.ones(1, device=gpu)
    assert torch.equal(idx.rows_p16.view(torch.int32), ops.p16_pack(want, amax_=ones).data.view(torch.int32))
    assert float(idx.unit_amax) == 1.0
    assert idx.pids.dtype == torch.int64 and torch.equal(idx.pids.cpu(), pid)
    assert float(idx.rows[5].abs().max()) == 0.0

    bad = torch.zeros(2, 256, device=gpu)
    bad[1, 17] = 1.5
    with pytest.raises(ValueError, match="max"):
        idx.add(bad, pids=torch.zeros(2, dtype=torch.int64), normalize=False)
    assert len(idx) == n
    with pytest.raises(ValueError, match="every add or on none"):
        idx.add(xg[:2])
    ok = torch.zeros(2, 256, device=gpu)
    ok[0, 3], ok[1, 4] = 1.0, -0.5
    assert idx.add(ok, pids=torch.tensor([7, 8]), normalize=False) == n
    assert torch.equal(idx.rows[n:], ok) and idx.pids[-2:].tolist() == [7, 8]

    sd = idx.state_dict()
    other = GalleryIndex()
    other.load_state_dict(sd)
    assert len(other) == len(idx)
    assert torch.equal(other.rows, idx.rows) and torch.equal(other.pids, idx.pids)
    assert torch.equal(other.rows_p16.view(torch.int32), idx.rows_p16.view(torch.int32))
    v0, r0 = idx.search(xg[:3], k=5)
    v1, r1 = other.search(xg[:3], k=5)
    assert torch.equal(v0, v1) and torch.equal(r0, r1)


# ------------------------------------------------------------------------------------- 2. exact against the dense product
@pytest.mark.parametrize("Q,G,k", SHAPES)
def test_search_equals_dense_p16_product(gpu, Q, G, k):
    idx, te, ie, qu, ref = built(gpu, Q, G, k)
    same(idx.search(te.to(gpu), k=k), ref, "search")
    same(idx.search(qu, k=k, normalize=False), ref, "search, unit queries")
    for wg in (0, 1, 3):
        same(c_search(idx, qu, k, wg), ref, "workgroups=%d" % wg)


# --------------------------------------------------------------------------- 3. orders a running threshold is weakest on
def _adversarial(kind):
    G = ADV_G
    q = OF.randn("gix:advq", (5, 256), SEED)
    g = OF.randn("gix:advg:" + kind, (G, 256), SEED)
    if kind in ("rising", "falling"):
        # query 0 = e_0, gallery row i = c_i e_0 + (noise in the other coordinates): similarity to query 0 is c_i exactly
        q[0] = 0.0
        q[0, 0] = 1.0
        g[:, 0] = 0.0
        g = 0.5 * g / g.norm(dim=1, keepdim=True)
        c = (torch.arange(G, dtype=torch.float32) + 1.0) / G
        g[:, 0] = 0.75 * (c if kind == "rising" else c.flip(0))
    elif kind == "ties":
        g[10000:20000] = g[:10000]
    elif kind == "negative":
        q, g = q.abs(), -g.abs()
    q = q / q.norm(dim=1, keepdim=True)
    if kind in ("ties", "negative"):
        g = g / g.norm(dim=1, keepdim=True)
    # (fp32 rounding of the normalisation may leave a norm a last bit above 1; the components stay below 1, which is what add checks)
    return q, g


@pytest.mark.parametrize("kind", ["rising", "falling", "ties", "negative"])
def test_adversarial_orders(gpu, kind):
    from textreid_amd import GalleryIndex

    q, g = _adversarial(kind)
    qg = q.to(gpu)
    idx = GalleryIndex()
    idx.add(g.to(gpu), normalize=False)
    assert torch.equal(idx.rows.cpu(), g)
    k = 10
    ref = reference(idx, qg, k)
    if kind == "rising":
        assert ref[1][0].tolist() == list(range(ADV_G - 1, ADV_G - 1 - k, -1))
    if kind == "falling":
        assert ref[1][0].tolist() == list(range(k))
    if kind == "ties":  # the best rows below 10000 come as (i, i + 10000) pairs, the lower row first
        r = ref[1]
        pairs = (r[:, :-1] < 10000) & (r[:, 1:] == r[:, :-1] + 10000)
        assert int(pairs.sum()) >= 5
    if kind == "negative":
        assert float(ref[0].max()) < 0.0
    same(idx.search(qg, k=k, normalize=False), ref, kind)
    for wg in (1, 0):
        same(c_search(idx, qg, k, wg), ref, "%s workgroups=%d" % (kind, wg))


# ------------------------------------------------------------------------------------------------------ 4. against the oracle
def oracle_check(got, te, ie, k):
    rv, ri = torch.topk(OE.similarity(te, ie), k, dim=1)
    assert torch.equal(got[1].cpu(), ri)
    assert torch.allclose(got[0].cpu(), rv, atol=2e-6, rtol=0), float((got[0].cpu() - rv).abs().max())


@pytest.mark.parametrize("Q,G,k", [s for s in SHAPES if s[1] >= 10])
def test_search_matches_oracle(gpu, Q, G, k):
    idx, te, ie, qu, ref = built(gpu, Q, G, k)
    oracle_check(idx.search(te.to(gpu), k=k), te, ie, k)


# ------------------------------------------------------------------------------------------------------------ 5. incremental
def test_incremental_adds(gpu):
    from textreid_amd import GalleryIndex

    Q, G, k = 5, 4099, 16
    idx, te, ie, qu, ref = built(gpu, Q, G, k)
    parts = GalleryIndex(capacity=500)
    at = 0
    for m in (1000, 2099, 1000):
        assert parts.add(ie[at : at + m].to(gpu)) == at
        at += m
    assert torch.equal(parts.rows, idx.rows) and torch.equal(parts.rows_p16.view(torch.int32), idx.rows_p16.view(torch.int32))
    v0, r0 = idx.search(te.to(gpu), k=k)
    v1, r1 = parts.search(te.to(gpu), k=k)
    assert torch.equal(v0, v1) and torch.equal(r0, r1)
    same((v1, r1), ref, "three adds")
    assert parts.add(te[:1].to(gpu)) == G
    v2, r2 = parts.search(te.to(gpu), k=k)
    assert int(r2[0, 0]) == G and abs(float(v2[0, 0]) - 1.0) <= 2e-6
    assert torch.equal(r2[0, 1:].cpu(), ref[1][0, : k - 1]) and torch.equal(v2[0, 1:].cpu(), ref[0][0, : k - 1])


# ------------------------------------------------------------------------------------------------------------ 6. large batch
def test_large_batch_uses_the_index_operands(gpu, monkeypatch):
    import textreid_amd.evaluation as E
    from textreid_amd import GalleryIndex

    Q, G, k = 70, 8192 + 69, 10
    te, ie = raw(Q, G)
    idx = GalleryIndex()
    idx.add(ie.to(gpu))
    packs = []
    real = E.call

    def counting(name, *args):
        if name == "trid_p16_pack_f32":
            packs.append(args[1])
        return real(name, *args)

    monkeypatch.setattr(E, "call", counting)
    got = idx.search(te.to(gpu), k=k)
    monkeypatch.undo()
    assert E.USE_SIM_P16 and packs == [Q], packs  # the queries are packed; the gallery (G rows) is not
    oracle_check(got, te, ie, k)


# ---------------------------------------------------------------------------------------------------------------- 7. capture
def test_search_records_and_replays(gpu):
    Q, G, k = 4, 4099, 10
    idx, te5, ie, qu, ref = built(gpu, 5, G, 16)
    qa = OF.randn("gix:cap_a", (Q, 256), SEED).to(gpu)
    qb = OF.randn("gix:cap_b", (Q, 256), SEED).to(gpu)
    buf = qa.clone()
    idx.search(buf, k=k)  # (allocates the cached workspace)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        vals, rows = idx.search(buf, k=k)
    g.replay()
    torch.cuda.synchronize()
    va, ra = idx.search(qa, k=k)
    assert torch.equal(vals, va) and torch.equal(rows, ra)
    buf.copy_(qb)
    g.replay()
    torch.cuda.synchronize()
    got_v, got_r = vals.clone(), rows.clone()
    vb, rb = idx.search(qb, k=k)
    assert torch.equal(got_v, vb) and torch.equal(got_r, rb)
    assert not torch.equal(rb, ra)
