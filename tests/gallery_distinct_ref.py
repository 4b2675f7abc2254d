"""CPU restatement of GalleryIndex.search_pids: the top-k over distinct groups of a given similarity matrix.  Plain torch on the host,
checked against a dict-based brute force in test_gallery_distinct_cpu.py."""

import torch

NEG = float("-inf")


def distinct_topk(sim, gid, allow, k):
    """sim [Q, G] f32, gid int [G] (equal = one group), allow bool [G] -> (values [Q, k], rows [Q, k] int64).  Pairs are ordered value
    descending, then row ascending; the representative of a group is its first ALLOWED row in that order; the result is the first k
    representatives in the same order.  Slots beyond the number of allowed groups are (-inf, -1)."""
    sim = sim.clone()
    gid = torch.as_tensor(gid).reshape(-1).long()
    allow = torch.as_tensor(allow).reshape(-1) != 0
    sim[:, ~allow] = NEG
    Q, G = sim.shape
    order = torch.sort(sim, dim=1, descending=True, stable=True)
    vals = torch.full((Q, k), NEG, dtype=sim.dtype)
    rows = torch.full((Q, k), -1, dtype=torch.int64)
    for q in range(Q):
        v, r = order.values[q], order.indices[q]
        by_group = torch.sort(gid[r], stable=True)  # inside a group the positions stay ascending: a run starts at the first occurrence
        start = torch.ones(G, dtype=torch.bool)
        start[1:] = by_group.values[1:] != by_group.values[:-1]
        first = torch.zeros(G, dtype=torch.bool)
        first[by_group.indices[start]] = True
        at = torch.nonzero(first & (v > NEG)).reshape(-1)[:k]  # (a group whose first occurrence is -inf has no allowed row)
        vals[q, : at.numel()] = v[at]
        rows[q, : at.numel()] = r[at]
    return vals, rows
