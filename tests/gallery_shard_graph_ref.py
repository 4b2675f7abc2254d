"""CPU restatement of the neighbour graph over gallery shards (GalleryShards.build_neighbours / refresh_neighbours,
trid_index_nn_merge_sharded_f32): numpy on the host.  The definition is written by brute force over the CONCATENATED gallery and
mapped to global row ids; the merge step of the kernel is a per-row insertion loop in plain Python.  Nothing computes a value: every
comparison downstream is of bit patterns and exact ids.  sim[i, g] is the similarity of row i AS THE QUERY to gallery row g."""

import numpy as np

import topk_deep_ref as TR

SHARD_BITS = 21
SHARD_STRIDE = 1 << SHARD_BITS
LOCAL_MASK = SHARD_STRIDE - 1


def offsets(sizes):
    """the row of the concatenated gallery at which every part starts, and the total"""
    return np.concatenate([[0], np.cumsum(np.asarray(sizes, dtype=np.int64))])


def to_global(rows, sizes):
    """rows of the concatenated gallery -> global ids shard * 2**21 + local (the inverse of locate through the parts' offsets);
    negative rows stay as they are"""
    rows = np.asarray(rows, dtype=np.int64)
    off = offsets(sizes)
    shard = np.searchsorted(off[1:], np.maximum(rows, 0), side="right")
    shard = np.minimum(shard, len(sizes) - 1)
    return np.where(rows < 0, rows, shard * SHARD_STRIDE + (np.maximum(rows, 0) - off[shard]))


def to_concat(ids, sizes):
    """global ids -> rows of the concatenated gallery; negative ids stay as they are"""
    ids = np.asarray(ids, dtype=np.int64)
    off = offsets(sizes)
    safe = np.maximum(ids, 0)
    return np.where(ids < 0, ids, off[np.minimum(safe >> SHARD_BITS, len(sizes) - 1)] + (safe & LOCAL_MASK))


def graph(sim, n, sizes, live=None):
    """THE DEFINITION: (lists int32 [G, n] of global ids, values float32 [G, n]) of the concatenated gallery sim [G, G] split into
    parts of ``sizes`` rows: every live row's n best live rows, value descending then row ascending; (-1, -inf) in every slot of a
    removed row"""
    vals, rows = TR.topk(sim, n, live)
    nn = to_global(rows, sizes).astype(np.int32)
    if live is not None:
        dead = np.asarray(live).reshape(-1) == 0
        nn[dead], vals[dead] = -1, -np.inf
    return nn, vals


def split(a, sizes):
    off = offsets(sizes)
    return [a[off[s] : off[s + 1]] for s in range(len(sizes))]


def is_live(e, lives):
    """the liveness rule of the kernel for an id e >= 0: removed when the shard or the local row is out of range, or the byte is 0"""
    s, l = int(e) >> SHARD_BITS, int(e) & LOCAL_MASK
    return s < len(lives) and l < len(lives[s]) and bool(lives[s][l])


def merge(cand, m, cand_first, rows, lives, self_shard, nn, nn_val):
    """the kernel on copies -> (nn, nn_val, redo): a per-row insertion loop.  cand [m, >= rows] float32 (None with m == 0):
    cand[j, i] = similarity of row i of shard ``self_shard`` to candidate j = id cand_first + j; lives: one 0 / 1 array per shard;
    nn int32 [>= rows, n] of global ids, nn_val float32 the same shape"""
    nn, nn_val = np.array(nn, dtype=np.int32), np.array(nn_val, dtype=np.float32)
    n = nn.shape[1]
    redo = np.zeros(rows, dtype=np.uint8)
    for i in range(rows):
        if not is_live(self_shard * SHARD_STRIDE + i, lives):
            nn[i], nn_val[i] = -1, -np.inf
            continue
        if nn[i, 0] < 0 or any(e >= 0 and not is_live(e, lives) for e in nn[i]):
            redo[i] = 1
            continue
        ids, vals = nn[i].tolist(), [nn_val[i, u] for u in range(n)]  # (numpy float32 scalars: they keep their bits)
        for j in range(m):
            r = cand_first + j
            if not is_live(r, lives):
                continue
            c = np.float32(cand[j][i])
            at = n
            for u in range(n):
                if ids[u] < 0 or c > vals[u] or (c == vals[u] and r < ids[u]):
                    at = u
                    break
            if at < n:
                ids = ids[:at] + [r] + ids[at : n - 1]
                vals = vals[:at] + [c] + vals[at : n - 1]
        nn[i] = ids
        nn_val[i] = np.array(vals, dtype=np.float32)
    return nn, nn_val, redo


def refresh(sim, live, old_sizes, sizes, nn, nn_val, group=32):
    """GalleryShards.refresh_neighbours on the reference -> (nn int32 [G, n], nn_val, new_rows, redone_rows), all in the row order
    of the concatenated gallery as it stands.  sim [G, G], live [G] and ``sizes`` describe the gallery now; ``old_sizes`` the rows of
    every part the graph covered (shorter than sizes when parts were opened since); nn / nn_val: one array per OLD part, the graph
    as it was last current.  Old rows take the new rows in through merge(), group by group; the new rows' lists and the flagged
    rows' lists come from the definition."""
    sim = np.asarray(sim, dtype=np.float32)
    live = np.asarray(live).reshape(-1) != 0
    S = len(sizes)
    old = list(old_sizes) + [0] * (S - len(old_sizes))
    off = offsets(sizes)
    lives = split(live, sizes)
    n = nn[0].shape[1]
    out = np.full((sim.shape[0], n), -1, dtype=np.int32)
    val = np.full((sim.shape[0], n), -np.inf, dtype=np.float32)
    groups = [(t, at, min(group, sizes[t] - at)) for t in range(S) for at in range(old[t], sizes[t], group)]
    flagged = np.zeros(sim.shape[0], dtype=bool)
    for s in range(S):
        n0 = old[s]
        if n0 == 0:
            continue
        a, b = np.array(nn[s][:n0]), np.array(nn_val[s][:n0])
        redo = np.zeros(n0, dtype=np.uint8)
        if not groups:
            a, b, redo = merge(None, 0, 0, n0, lives, s, a, b)
        for t, at, m in groups:
            cand = np.ascontiguousarray(sim[off[s] : off[s] + n0, off[t] + at : off[t] + at + m].T)  # cand[j, i] = s(query i, gallery j)
            a, b, r = merge(cand, m, t * SHARD_STRIDE + at, n0, lives, s, a, b)
            redo |= r
        out[off[s] : off[s] + n0], val[off[s] : off[s] + n0] = a, b
        flagged[off[s] : off[s] + n0] = redo != 0
    scratch_nn, scratch_val = graph(sim, n, sizes, live)
    new = np.zeros(sim.shape[0], dtype=bool)
    for t in range(S):
        new[off[t] + old[t] : off[t + 1]] = True
    again = flagged | new
    out[again], val[again] = scratch_nn[again], scratch_val[again]
    return out, val, int((new & live).sum()), int(flagged.sum())
