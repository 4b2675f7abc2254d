"""CPU restatement of the deep distinct select (trid_index_group_best_f32, trid_topk_rows_deep_pairs_f32 and their composition,
GalleryIndex.shortlist_pids): numpy on the host, checked against a dict-based brute force in test_gallery_deep_distinct_cpu.py.
Both steps move values and never compute one, so everything here compares bit patterns (topk_deep_ref.same)."""

import numpy as np

ABSENT = 0x7FFFFFFF  # the row of a group without an allowed row, the column of an absent pair


def table(groups):
    """groups int [G] (equal = one group) -> (order int32 [G], starts int32 [n_groups + 1], n_groups): the rows sorted by group -
    groups numbered by ascending value -, ascending row inside a group"""
    g = np.asarray(groups).reshape(-1).astype(np.int64)
    order = np.argsort(g, kind="stable")
    s = g[order]
    first = np.ones(g.size, dtype=bool)
    first[1:] = s[1:] != s[:-1]
    starts = np.concatenate([np.nonzero(first)[0], [g.size]]) if g.size else np.zeros(1)
    return order.astype(np.int32), starts.astype(np.int32), int(first.sum())


def group_best(sim, order, starts, n_groups, n_slots, allowed=None):
    """sim [Q, G] float32 -> (values [Q, n_slots] float32, rows [Q, n_slots] int32): per (query, group) the group's first allowed row
    in the order value descending by float comparison (+0 == -0), then row ascending - a real -inf is an ordinary value -;
    (-inf, ABSENT) for a group without an allowed row and for the slots n_groups .. n_slots - 1.  An order entry outside [0, G) is
    skipped; a starts pair is clamped to [0, G]."""
    sim = np.ascontiguousarray(np.asarray(sim, dtype=np.float32))
    Q, G = sim.shape
    vals = np.full((Q, n_slots), -np.inf, dtype=np.float32)
    rows = np.full((Q, n_slots), ABSENT, dtype=np.int32)
    ok = np.ones(G, dtype=bool) if allowed is None else np.asarray(allowed).reshape(-1) != 0
    for s in range(n_groups):
        lo, hi = (min(max(int(x), 0), G) for x in (starts[s], starts[s + 1]))
        members = np.asarray(order[lo:hi], dtype=np.int64)
        members = members[(members >= 0) & (members < G)]
        members = np.sort(members[ok[members]])
        if members.size == 0:
            continue
        sub = sim[:, members] + np.float32(0.0)  # (x + 0.0 turns -0 into +0: the two tie, by row)
        at = np.argmax(sub, axis=1)                # (the first maximum: the lowest row)
        rows[:, s] = members[at]
        vals[:, s] = sim[np.arange(Q), members[at]]
    return vals, rows


def pairs_topk(val, col, k, offset=0):
    """val [Q, S] float32, col [Q, S] int32 -> (values [Q, k] float32, columns [Q, k] int64): the k best pairs of every row, value
    descending by float comparison then the GIVEN column ascending; a column of ABSENT is absent whatever its value; columns come
    back + offset; slots beyond the present pairs are (-inf, -1)"""
    val = np.ascontiguousarray(np.asarray(val, dtype=np.float32))
    col = np.asarray(col).astype(np.int64)
    Q = val.shape[0]
    vals = np.full((Q, k), -np.inf, dtype=np.float32)
    idx = np.full((Q, k), -1, dtype=np.int64)
    for q in range(Q):
        here = np.nonzero(col[q] != ABSENT)[0]
        here = here[np.argsort(col[q, here], kind="stable")]             # column ascending ...
        here = here[np.argsort(-(val[q, here] + np.float32(0.0)), kind="stable")][:k]  # ... kept inside equal values
        vals[q, : here.size] = val[q, here]
        idx[q, : here.size] = col[q, here] + offset
    return vals, idx


def distinct_topk(sim, groups, k, allowed=None):
    """the composition: the k best distinct groups of every row of sim, each by its first allowed row -> (values [Q, k] float32,
    rows [Q, k] int64), (-inf, -1) behind the allowed groups"""
    order, starts, n_groups = table(groups)
    n_slots = max(n_groups, k)
    return pairs_topk(*group_best(sim, order, starts, n_groups, n_slots, allowed), k)
