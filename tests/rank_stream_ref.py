"""fp64 restatement, from features, of the rank metric (reference lib/data/metrics/evaluation.py:11-37) with the k-reciprocal
term (:40-65) as part of the compared value: s'(q,i) = q . g_i + alpha * Jaccard(qnn[q], gnn[i]).  Test infrastructure only.

rank r(q,j) = 1 + #{ i : s'(q,i) > s'(q,j), or s'(q,i) == s'(q,j) and i < j } (descending, ties lower index first); with a
query's P ranks ascending AP = (1/P) sum_k k / r_(k) and the first hit is r_(1) - 1."""

import torch


def scores(q, g, qnn=None, gnn=None, alpha=0.05):
    s = q.double() @ g.double().t()
    if qnn is not None:
        n = qnn.shape[1]
        eq = (qnn[:, None, :, None] == gnn[None, :, None, :]).sum(dim=(2, 3)).double()
        s = s + alpha * eq / (2 * n - eq)
    return s


def positives(qp, gp):
    """CSR list of the relevant gallery rows, ascending per query"""
    m = gp.view(1, -1) == qp.view(-1, 1)
    qi, gi = m.nonzero(as_tuple=True)
    ptr = torch.zeros(qp.numel() + 1, dtype=torch.int64)
    ptr[1:] = m.sum(1).cumsum(0)
    return ptr, gi, qi


def _per_positive(q, g, qp, gp, qnn, gnn, alpha, fn):
    s = scores(q, g, qnn, gnn, alpha)
    ptr, gi, qi = positives(qp, gp)
    col = torch.arange(g.shape[0])
    out = [fn(s[int(a)], s[int(a), int(j)], col, int(j)) for a, j in zip(qi, gi)]  # (one row at a time: no [NP, G] temporary)
    return ptr, gi, torch.tensor(out, dtype=torch.int64).reshape(len(out), -1)


def ranks_ref(q, g, qp, gp, qnn=None, gnn=None, alpha=0.05):
    ptr, gi, r = _per_positive(q, g, qp, gp, qnn, gnn, alpha,
                               lambda row, t, col, j: [int(((row > t) | ((row == t) & (col < j))).sum()) + 1])
    return ptr, gi, r.reshape(-1)


def rank_brackets(q, g, qp, gp, qnn=None, gnn=None, alpha=0.05, delta=0.0):
    """per positive: lo = #{i : s' > s'_j + delta}, hi = #{i : s' >= s'_j - delta} - 1"""
    ptr, gi, r = _per_positive(q, g, qp, gp, qnn, gnn, alpha,
                               lambda row, t, col, j: [int((row > t + delta).sum()), int((row >= t - delta).sum()) - 1])
    return ptr, gi, r[:, 0], r[:, 1]


def ap_cmc_from_ranks(ptr, ranks, topk):
    """(cmc [len(topk)] in percent, AP [Q] (NaN without positives), mAP in percent)"""
    Q = ptr.numel() - 1
    ap = torch.full((Q,), float("nan"), dtype=torch.float64)
    first = torch.full((Q,), 2**62, dtype=torch.int64)
    for qq in range(Q):
        r = torch.sort(ranks[ptr[qq]:ptr[qq + 1]].long())[0]
        if r.numel():
            ap[qq] = (torch.arange(1, r.numel() + 1).double() / r.double()).mean()
            first[qq] = r[0] - 1
    cmc = torch.stack([(first < k).double().mean() * 100 for k in topk])
    return cmc, ap, ap.mean() * 100
