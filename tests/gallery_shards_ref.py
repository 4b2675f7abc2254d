"""CPU restatement of the list merge (trid_index_merge_lists_f32), written as its definition: collect the present candidates, sort
them by (value descending, global row ascending), walk the order and drop later entries of a pid already seen.  numpy on the host,
checked against a per-candidate insertion loop in test_gallery_shards_cpu.py.  The merge moves values and never computes one, so
everything here compares bit patterns."""

import numpy as np


def merge(val, row, k, list_base=None, pid=None):
    """val float32, row int64, pid int64 or None: [Q, n_lists, k_in]; list_base int64 [n_lists] or None (zeros).  row < 0 = absent
    whatever the value.  -> (values [Q, k] float32, global rows [Q, k] int64[, pids [Q, k] int64]); short queries end in
    (-inf, -1[, -1])."""
    val = np.ascontiguousarray(np.asarray(val, dtype=np.float32))
    row = np.asarray(row, dtype=np.int64)
    Q, S, kin = val.shape
    base = np.zeros(S, dtype=np.int64) if list_base is None else np.asarray(list_base, dtype=np.int64)
    grow = (row + base[None, :, None]).reshape(Q, -1)
    here = (row >= 0).reshape(Q, -1)
    flat = val.reshape(Q, -1)
    pids = None if pid is None else np.asarray(pid, dtype=np.int64).reshape(Q, -1)
    out_v = np.full((Q, k), -np.inf, dtype=np.float32)
    out_r = np.full((Q, k), -1, dtype=np.int64)
    out_p = np.full((Q, k), -1, dtype=np.int64)
    for q in range(Q):
        cand = np.nonzero(here[q])[0]
        # lexsort: the last key is the primary one; x + 0.0 turns -0 into +0 (the two tie, by row)
        order = cand[np.lexsort((grow[q, cand], -(flat[q, cand] + np.float32(0.0))))]
        seen, t = set(), 0
        for c in order:
            if t == k:
                break
            if pids is not None:
                if int(pids[q, c]) in seen:
                    continue
                seen.add(int(pids[q, c]))
                out_p[q, t] = pids[q, c]
            out_v[q, t] = flat[q, c]
            out_r[q, t] = grow[q, c]
            t += 1
    return (out_v, out_r) if pid is None else (out_v, out_r, out_p)


def bits(x):
    """float32 array -> its bit patterns as int64 (so that +0 / -0 differ)"""
    return np.ascontiguousarray(np.asarray(x, dtype=np.float32)).view(np.uint32).astype(np.int64)


def same(got, want):
    """(values, rows[, pids]) tuples equal: the values bit for bit"""
    return len(got) == len(want) and np.array_equal(bits(got[0]), bits(want[0])) and all(
        np.array_equal(np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)) for a, b in zip(got[1:], want[1:]))


def special_inputs(Q, n_lists, k_in, seed, levels=4, absent=0.2, n_pids=None, sort_lists=False):
    """(val, row, list_base, pid) with heavy exact ties, +0 / -0, a real -inf on present rows, absent slots (their values are junk:
    +inf), one all-absent list when there are several, and a pid that sits in EVERY list with equal values.  The local rows
    of one query are distinct over ALL its lists and the bases are wider apart than any local row, so the global rows are distinct
    with the bases and without them."""
    rng = np.random.RandomState(seed)
    pool = np.concatenate([np.linspace(-1.0, 1.0, levels), [0.0, -0.0, -np.inf]]).astype(np.float32)
    val = pool[rng.randint(0, pool.size, size=(Q, n_lists, k_in))]
    span = n_lists * (4 * k_in + 8)
    row = np.stack([rng.permutation(span)[: n_lists * k_in].reshape(n_lists, k_in) for _ in range(Q)]).astype(np.int64)
    base = (rng.permutation(n_lists).astype(np.int64) * span * 3) + (1 << 33)  # (not ascending; past 2^32)
    n_pids = n_pids or max(2, (n_lists * k_in) // 3)
    pid = rng.randint(0, n_pids, size=(Q, n_lists, k_in)).astype(np.int64) * (1 << 35) - (1 << 36)
    pid[:, :, 0] = 77  # one pid in every list ...
    val[:, :, 0] = np.float32(0.5)  # ... with equal values: the lowest global row wins
    if sort_lists:
        for q in range(Q):
            for s in range(n_lists):
                o = np.lexsort((row[q, s], -(val[q, s] + np.float32(0.0))))
                val[q, s], row[q, s], pid[q, s] = val[q, s, o], row[q, s, o], pid[q, s, o]
    gone = rng.rand(Q, n_lists, k_in) < absent
    if n_lists > 1:
        gone[:, n_lists // 2, :] = True
    row[gone] = -1 - rng.randint(0, 5, size=int(gone.sum()))
    val[gone] = np.inf
    return val, row, base, pid
