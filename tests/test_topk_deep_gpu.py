"""trid_topk_rows_deep_f32 on the GPU against topk_deep_ref on the CPU copy of the same matrix.  The select moves values and never
computes one: values are compared as bit patterns, columns exactly, and CMC as the integer hit counts behind the percentages - no
tolerance anywhere."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import oracle.evaluation as OE  # noqa: E402
import topk_deep_ref as TR  # noqa: E402
from gallery_support import gpu, words_tensor  # noqa: E402,F401


def lib():
    from textreid_amd import lib as L

    return L


def default_chunk(k):
    return lib().load().trid_topk_rows_deep_chunk(k)


def matrix(Q, G, seed, ties=False):
    """seeded scores; ties: a few distinct values only, both zeros among them"""
    rng = np.random.RandomState(seed)
    if ties:
        pool = np.array([0.0, -0.0, 0.25, -0.25, 1.0, 3.5, -2.0], dtype=np.float32)
        return pool[rng.randint(0, pool.size, size=(Q, G))]
    return rng.standard_normal((Q, G)).astype(np.float32)


def deep(dev_sim, Q, G, k, ld_q, ld_g, words=None, offset=0, chunk=0):
    """the C entry itself on a device buffer -> (values, columns) as numpy; the outputs start as garbage"""
    from textreid_amd.ops import _p, stream

    L = lib()
    nws = L.load().trid_topk_rows_deep_ws_bytes(Q, G, k, chunk)
    assert nws > 0
    ws = torch.empty(nws, dtype=torch.uint8, device=dev_sim.device)
    vals = torch.full((Q, k), float("nan"), device=dev_sim.device)
    cols = torch.full((Q, k), -7, dtype=torch.int64, device=dev_sim.device)
    L.call("trid_topk_rows_deep_f32", _p(dev_sim), ld_q, ld_g, Q, G, k, _p(words), offset, _p(vals), _p(cols), _p(ws), nws, chunk, stream())
    return vals.cpu().numpy(), cols.cpu().numpy()


def row_major(sim, dev, pad=0):
    """-> (device buffer [Q, G + pad] with NaN in the padding, ld_q)"""
    Q, G = sim.shape
    buf = torch.full((Q, G + pad), float("nan"), device=dev)
    buf[:, :G] = torch.from_numpy(sim).to(dev)
    return buf, G + pad


def query_minor(sim, dev):
    """-> (device buffer [G, cols] as trid_gemm_p16 writes it with the gallery as A, cols): ld_q = 1, ld_g = cols"""
    Q, G = sim.shape
    cols = 32 if Q <= 32 else 64
    assert Q <= cols
    buf = torch.full((G, cols), float("nan"), device=dev)
    buf[:, :Q] = torch.from_numpy(sim).to(dev).t()
    return buf, cols


@pytest.mark.parametrize("k", [1, 16, 17, 100, 1024])
def test_shapes_around_the_chunk(gpu, k):
    C = default_chunk(k)
    for G in (1, 17, 63, 64, 65, 1000, C - 1, C, C + 1, 2 * C + 3):
        if k > G:
            continue
        full = matrix(33, G, 100 + G % 97, ties=(G % 2 == 0))
        for Q in (1, 5, 33):
            sim = full[:Q]
            buf, ld = row_major(sim, gpu)
            got = deep(buf, Q, G, k, ld, 1)
            assert TR.same(got, TR.topk(sim, k)), (Q, G, k)


def test_k_equals_g_equals_1024_padded_rows_and_an_offset(gpu):
    sim = matrix(5, 1024, 7)
    buf, ld = row_major(sim, gpu)
    assert TR.same(deep(buf, 5, 1024, 1024, ld, 1), TR.topk(sim, 1024))
    sim = matrix(5, 1000, 8, ties=True)
    buf, ld = row_major(sim, gpu, pad=13)  # ld_q > G
    assert ld > 1000
    assert TR.same(deep(buf, 5, 1000, 100, ld, 1, offset=123456789012), TR.topk(sim, 100, None, 123456789012))
    allowed = np.zeros(1000, dtype=bool)
    allowed[::50] = True  # 20 allowed: the short slots stay -1 whatever the offset
    got = deep(buf, 5, 1000, 100, ld, 1, words=words_tensor(allowed, gpu), offset=1 << 40)
    assert TR.same(got, TR.topk(sim, 100, allowed, 1 << 40))
    assert (got[1][:, 20:] == -1).all() and (got[1][:, :20] >= 1 << 40).all()


@pytest.mark.parametrize("chunk,k,G", [(256, 100, 3000), (64, 17, 5000)])
def test_forced_small_chunks_take_several_merge_levels(gpu, chunk, k, G):
    # (256, 100, 3000): 12 lists -> 6 -> 3 -> 2 -> 1; (64, 17, 5000): 79 lists -> 27 -> 9 -> 3 -> 1
    for ties in (False, True):
        sim = matrix(5, G, 21, ties=ties)
        buf, ld = row_major(sim, gpu)
        want = TR.topk(sim, k)
        auto = deep(buf, 5, G, k, ld, 1)
        forced = deep(buf, 5, G, k, ld, 1, chunk=chunk)
        assert TR.same(auto, want) and TR.same(forced, want) and TR.same(forced, auto)


def test_ties(gpu):
    k, chunk, G = 17, 64, 640
    check = lambda sim, kk=k, ch=chunk: TR.same(deep(row_major(sim, gpu)[0], sim.shape[0], sim.shape[1], kk, sim.shape[1], 1, chunk=ch), TR.topk(sim, kk))  # noqa: E731
    # all equal: columns 0 .. k-1
    sim = np.full((3, G), 0.5, dtype=np.float32)
    got = deep(row_major(sim, gpu)[0], 3, G, k, G, 1, chunk=chunk)
    assert (got[1] == np.arange(k)[None, :]).all() and (got[0] == 0.5).all()
    assert check(sim, 100, 0)
    # every value twice, the copies in different chunks
    half = matrix(3, G // 2, 31)
    assert check(np.concatenate([half, half], axis=1))
    assert check(np.concatenate([half, half], axis=1), 100, 256)
    # a row of zeros of both signs: columns 0 .. k-1 with their own sign bits
    z = np.where(np.random.RandomState(5).randint(0, 2, size=(3, G)) == 1, np.float32(0.0), np.float32(-0.0)).astype(np.float32)
    got = deep(row_major(z, gpu)[0], 3, G, k, G, 1, chunk=chunk)
    assert (got[1] == np.arange(k)[None, :]).all() and np.array_equal(np.signbit(got[0]), np.signbit(z[:, :k]))
    assert check(z)
    # real -inf among finite values, k reaching into them
    s = matrix(3, G, 32)
    s[:, np.random.RandomState(6).permutation(G)[: G - 9]] = -np.inf  # 9 finite values per row, k = 17
    got = deep(row_major(s, gpu)[0], 3, G, k, G, 1, chunk=chunk)
    assert TR.same(got, TR.topk(s, k)) and (got[1] >= 0).all() and np.isneginf(got[0][:, 9:]).all()
    # sorted rows, both ways
    asc = np.sort(matrix(3, G, 33), axis=1)
    assert check(asc) and check(asc[:, ::-1].copy()) and check(asc, 100, 0) and check(asc[:, ::-1].copy(), 100, 0)


def test_masks(gpu):
    k, chunk, G = 17, 64, 1000  # G % 32 == 8: the last word has 24 tail bits
    sim = matrix(5, G, 41, ties=True)
    buf, ld = row_major(sim, gpu)
    rng = np.random.RandomState(42)

    def run(allowed, ch=chunk, garbage=True):
        got = deep(buf, 5, G, k, ld, 1, words=words_tensor(allowed, gpu, garbage=garbage), chunk=ch)
        assert TR.same(got, TR.topk(sim, k, allowed)), int(allowed.sum())
        return got

    everything = np.ones(G, dtype=bool)
    assert TR.same(run(everything), deep(buf, 5, G, k, ld, 1, chunk=chunk))
    none = run(np.zeros(G, dtype=bool))
    assert (none[1] == -1).all() and np.isneginf(none[0]).all()
    few = np.zeros(G, dtype=bool)
    few[rng.permutation(G)[: k - 1]] = True
    got = run(few)
    assert (got[1][:, k - 1] == -1).all() and (got[1][:, : k - 1] >= 0).all()
    chunk_off = everything.copy()
    chunk_off[2 * chunk : 3 * chunk] = False  # a whole first-level chunk
    run(chunk_off)
    best_off = everything.copy()
    best_off[np.unique(TR.topk(sim, 1)[1])] = False  # the best column of every row
    got = run(best_off)
    assert not np.isin(got[1], np.nonzero(~best_off)[0]).any()
    random = rng.randint(0, 2, size=G).astype(bool)
    run(random)
    run(random, ch=0, garbage=False)
    # the library's own packing of a byte mask gives the same words
    from textreid_amd.ops import _p, stream

    m = torch.from_numpy(random).to(gpu)
    words = torch.full(((G + 31) // 32,), -1, dtype=torch.int32, device=gpu)
    lib().call("trid_index_pack_mask_u32", None, _p(m), G, _p(words), words.numel(), stream())
    assert TR.same(deep(buf, 5, G, k, ld, 1, words=words), TR.topk(sim, k, random))


@pytest.mark.parametrize("Q", [5, 33])
def test_row_major_and_query_minor_layouts_agree(gpu, Q):
    for G, k, chunk in ((1000, 100, 0), (20037, 100, 0), (3000, 17, 64)):
        sim = matrix(Q, G, 50 + Q, ties=(G == 1000))
        want = TR.topk(sim, k)
        a, ld = row_major(sim, gpu)
        b, cols = query_minor(sim, gpu)
        got_a = deep(a, Q, G, k, ld, 1, chunk=chunk)
        got_b = deep(b, Q, G, k, 1, cols, chunk=chunk)
        assert TR.same(got_a, want) and TR.same(got_b, want)


def test_agrees_with_the_register_list_kernel_up_to_16(gpu):
    from textreid_amd.ops import _p, stream

    for G, ties in ((65, True), (8195, False), (8195, True)):
        sim = matrix(7, G, 60, ties=ties)
        buf, ld = row_major(sim, gpu)
        for k in (1, 10, 16):
            vals = torch.empty(7, k, device=gpu)
            cols = torch.empty(7, k, dtype=torch.int64, device=gpu)
            lib().call("trid_topk_rows_f32", _p(buf), ld, 7, G, k, _p(vals), _p(cols), stream())
            assert TR.same(deep(buf, 7, G, k, ld, 1), (vals.cpu().numpy(), cols.cpu().numpy()))


def test_evaluation_topk_rows(gpu):
    from textreid_amd import evaluation as E

    sim = matrix(6, 2000, 70, ties=True)
    dev = torch.from_numpy(sim).to(gpu)
    vals, cols = E.topk_rows(dev, 300)
    assert vals.shape == (6, 300) and cols.dtype == torch.int64
    assert TR.same((vals.cpu().numpy(), cols.cpu().numpy()), TR.topk(sim, 300))
    view = dev[:, ::2]  # rows that are not contiguous: read in place
    assert not view.is_contiguous()
    allowed = np.random.RandomState(71).randint(0, 3, size=1000) > 0
    vals, cols = E.topk_rows(view, 100, mask=torch.from_numpy(allowed).to(gpu))
    assert TR.same((vals.cpu().numpy(), cols.cpu().numpy()), TR.topk(sim[:, ::2], 100, allowed))
    vals, cols = E.topk_rows(dev.t(), 6, mask=torch.ones(6, dtype=torch.uint8, device=gpu))  # a transposed view: [2000, 6]
    assert TR.same((vals.cpu().numpy(), cols.cpu().numpy()), TR.topk(sim.T, 6))
    with pytest.raises(ValueError, match="k must be"):
        E.topk_rows(dev, 1025)
    with pytest.raises(ValueError, match="mask"):
        E.topk_rows(dev, 10, mask=torch.ones(1999, dtype=torch.bool, device=gpu))


def host_rank(sim, q_pids, g_pids, topk):
    """the reference's formula (lib/data/metrics/evaluation.py:20-26) on the stable descending sort -> (hits per k, indices); the
    reference's cmc is 100 * hits / Q"""
    max_rank = max(topk)
    indices = torch.sort(sim, dim=1, descending=True, stable=True).indices[:, :max_rank]
    matches = g_pids[indices].eq(q_pids.view(-1, 1))
    all_cmc = matches[:, :max_rank].cumsum(1)
    all_cmc[all_cmc > 1] = 1
    return all_cmc.sum(0)[torch.as_tensor(topk) - 1], indices


def hit_counts(cmc, Q):
    """CMC percentages -> the integer hit counts they stand for (cmc = 100 * hits / Q: the counts are what is compared, exactly)"""
    return torch.round(cmc.cpu().double() * Q / 100).long()


def check_rank(gpu, Q, G, topk, seed):
    from textreid_amd import evaluation as E

    rng = np.random.RandomState(seed)
    sim = torch.from_numpy((rng.randint(-40, 40, size=(Q, G)) / 16.0).astype(np.float32))  # (ties: the order rule decides)
    g_pids = torch.from_numpy(rng.randint(0, 60, size=G).astype(np.int64))  # duplicated pids
    q_pids = torch.from_numpy(rng.randint(0, 60, size=Q).astype(np.int64))
    cmc, indices = E.rank(sim.to(gpu), q_pids.to(gpu), g_pids.to(gpu), topk=topk, get_mAP=False)
    hits, want_idx = host_rank(sim, q_pids, g_pids, topk)
    assert indices.shape == (Q, max(topk)) and indices.dtype == torch.int64
    assert torch.equal(indices.cpu(), want_idx)
    assert torch.equal(hit_counts(cmc, Q), hits)


def test_rank_with_deep_topk(gpu):
    check_rank(gpu, 50, 300, (1, 5, 10, 20, 100), 80)


def test_rank_beyond_1024_takes_the_argsort_slice(gpu):
    check_rank(gpu, 3, 2500, (1, 2000), 81)


def test_rank_up_to_16_is_unchanged_against_the_oracle(gpu):
    from textreid_amd import evaluation as E

    rng = np.random.RandomState(82)
    sim = torch.from_numpy(rng.standard_normal((50, 300)).astype(np.float32))
    g_pids = torch.from_numpy(rng.randint(0, 60, size=300).astype(np.int64))
    q_pids = torch.from_numpy(rng.randint(0, 60, size=50).astype(np.int64))
    cmc, indices = E.rank(sim.to(gpu), q_pids.to(gpu), g_pids.to(gpu), topk=(1, 5, 10), get_mAP=False)
    want_cmc, want_idx = OE.rank(sim, q_pids, g_pids, topk=(1, 5, 10), get_mAP=False)
    assert torch.equal(indices.cpu(), want_idx)
    assert torch.equal(hit_counts(cmc, 50), hit_counts(want_cmc, 50))
