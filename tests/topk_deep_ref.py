"""CPU restatement of the deep top-k (trid_topk_rows_deep_f32): numpy on the host, checked against a brute-force loop in
test_topk_deep_cpu.py.  The select moves values and never computes one, so everything here compares bit patterns."""

import numpy as np


def topk(sim, k, allowed=None, offset=0):
    """sim [Q, G] float32, allowed bool [G] or None -> (values [Q, k] float32, columns [Q, k] int64): the k best ALLOWED columns of
    every row, value descending by float comparison (+0 == -0, a real -inf is an ordinary value) then column ascending; the values
    carry the input's bit patterns; columns are + offset; slots beyond the allowed count are (-inf, -1)"""
    sim = np.ascontiguousarray(np.asarray(sim, dtype=np.float32))
    Q, G = sim.shape
    cols = np.arange(G, dtype=np.int64) if allowed is None else np.nonzero(np.asarray(allowed).reshape(-1) != 0)[0].astype(np.int64)
    vals = np.full((Q, k), -np.inf, dtype=np.float32)
    idx = np.full((Q, k), -1, dtype=np.int64)
    m = min(k, cols.size)
    for q in range(Q):
        row = sim[q, cols]
        order = np.argsort(-(row + np.float32(0.0)), kind="stable")[:m]  # (x + 0.0 turns -0 into +0: the two tie, by column)
        vals[q, :m] = row[order]
        idx[q, :m] = cols[order] + offset
    return vals, idx


def bits(x):
    """float32 array -> its bit patterns as int64 (so that +0 / -0 differ and NaN-free comparisons are exact)"""
    return np.ascontiguousarray(np.asarray(x, dtype=np.float32)).view(np.uint32).astype(np.int64)


def same(got, want):
    """(values, columns) pairs equal bit for bit"""
    return np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(np.asarray(got[1], dtype=np.int64), np.asarray(want[1], dtype=np.int64))
