"""CPU restatement of the neighbour graph and the re-ranked search of GalleryIndex (build_neighbours, search_reranked,
trid_index_rerank_add_f32): numpy on the host.  Both selects go through topk_deep_ref.topk; the bonus is formed step by step in
np.float32, as the library's host entry forms its table, so everything downstream compares bit patterns."""

import numpy as np

import topk_deep_ref as TR


def counts(qnn, gnn):
    """qnn [Q, a], gnn [G, b] integer lists of distinct rows, entries below 0 absent -> int64 [Q, G]: the number of equal pairs
    qnn[q, t] == gnn[g, u] >= 0"""
    qnn = np.asarray(qnn, dtype=np.int64)
    gnn = np.asarray(gnn, dtype=np.int64)
    out = np.zeros((qnn.shape[0], gnn.shape[0]), dtype=np.int64)
    for t in range(qnn.shape[1]):
        a = qnn[:, t]
        for u in range(gnn.shape[1]):
            out += (a[:, None] == gnn[None, :, u]) & (a[:, None] >= 0)
    return out


def bonus(nq, c, n, alpha):
    """(alpha * (float)c) / (float)(nq + n - c), every step rounded to float32; nq, c: integer arrays (or scalars) with
    c <= nq <= n, so the divisor is >= n >= 1"""
    nq = np.asarray(nq, dtype=np.int64)
    c = np.asarray(c, dtype=np.int64)
    num = np.float32(alpha) * c.astype(np.float32)
    den = (nq + n - c).astype(np.float32)
    out = (num.astype(np.float32) / den).astype(np.float32)
    assert out.dtype == np.float32
    return out


def rerank_scores(sim, qnn, gnn, n, alpha, allow=None):
    """sim [Q, G] float32 -> a copy with sim[q, g] + bonus(nq(q), c(q, g)) (one float32 add) where row g is allowed and c > 0; every
    other element keeps its bits"""
    sim = np.ascontiguousarray(np.asarray(sim, dtype=np.float32))
    qnn = np.asarray(qnn, dtype=np.int64)
    c = counts(qnn, gnn)
    nq = (qnn >= 0).sum(axis=1)
    hit = c > 0
    if allow is not None:
        hit &= (np.asarray(allow).reshape(-1) != 0)[None, :]
    out = sim.copy()
    b = bonus(np.broadcast_to(nq[:, None], c.shape)[hit], c[hit], n, alpha)
    out[hit] = (sim[hit] + b).astype(np.float32)
    return out


def reranked_topk(sim, gnn, n, alpha, k, allow=None):
    """-> (values [Q, k] float32, rows [Q, k] int64) of search_reranked: the query's own list = its n best allowed rows (-1 slots
    when fewer are allowed), the bonus, then the k best allowed rows of the modified scores"""
    qnn = TR.topk(sim, n, allow)[1]
    return TR.topk(rerank_scores(sim, qnn, gnn, n, alpha, allow), k, allow)


def graph(sim_gg, n, live=None):
    """sim_gg [G, G] float32 = every row's similarity to every row -> int32 [G, n] of build_neighbours: the n best LIVE rows of every
    live row, -1 in every slot of a dead row"""
    out = TR.topk(sim_gg, n, live)[1].astype(np.int32)
    if live is not None:
        out[np.asarray(live).reshape(-1) == 0] = -1
    return out
