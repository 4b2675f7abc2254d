"""CPU restatement of the incremental neighbour-graph refresh of GalleryIndex (trid_index_nn_merge_f32, refresh_neighbours): numpy on
the host.  The merge moves values and never computes one and every select goes through topk_deep_ref.topk, so everything downstream
compares bit patterns.  sim[i, g] is the similarity of row i AS THE QUERY to gallery row g - the direction of the definition; the
matrices the tests use are not symmetric."""

import numpy as np

import topk_deep_ref as TR


def merge(cand, m, cand_first, rows, live, nn, nn_val):
    """the merge kernel on copies -> (nn, nn_val, redo).  cand [m, >= rows] float32 (None with m == 0): cand[j, i] = similarity of old
    row i to candidate j = row cand_first + j; live: [cand_first + m]; nn int32 [>= rows, n], nn_val float32 the same shape"""
    nn, nn_val = np.array(nn, dtype=np.int32), np.array(nn_val, dtype=np.float32)
    live = np.asarray(live).reshape(-1) != 0
    n = nn.shape[1]
    assert rows <= cand_first and live.size == cand_first + m
    e, v = nn[:rows], nn_val[:rows]  # (views: written in place below)
    alive = live[:rows]
    known = (e >= 0) & (e < live.size)
    dead_entry = ((e >= 0) & ~known) | (known & ~live[np.where(known, e, 0)])
    redo = (alive & ((e[:, 0] < 0) | dead_entry.any(axis=1))).astype(np.uint8)
    e[~alive], v[~alive] = -1, -np.inf
    go = np.nonzero(alive & (redo == 0))[0]
    le, lv = e[go], v[go]
    for j in range(m):
        if not live[cand_first + j]:
            continue
        c = np.asarray(cand[j], dtype=np.float32)[go]
        before = c[:, None] > lv  # float comparison: +0 == -0, an equal value stays behind
        at = np.where(before.any(axis=1), before.argmax(axis=1), n)  # the first entry the candidate comes strictly before
        for u in range(n - 1, -1, -1):  # slots from the last one up: slot u - 1 still holds its old entry
            shifted = at < u
            here = at == u
            lv[:, u] = np.where(shifted, lv[:, u - 1] if u else lv[:, 0], np.where(here, c, lv[:, u]))
            le[:, u] = np.where(shifted, le[:, u - 1] if u else le[:, 0], np.where(here, cand_first + j, le[:, u]))
    e[go], v[go] = le, lv
    return nn, nn_val, redo


def built(sim, n, live=None):
    """(lists int32 [G, n], values float32 [G, n]) of build_neighbours on sim [G, G]: gallery_rerank_ref.graph with the values kept,
    (-1, -inf) in every slot of a dead row"""
    vals, rows = TR.topk(sim, n, live)
    nn = rows.astype(np.int32)
    if live is not None:
        dead = np.asarray(live).reshape(-1) == 0
        nn[dead], vals[dead] = -1, -np.inf
    return nn, vals


def refresh(sim, live, nn, nn_val, n0, group=32):
    """refresh_neighbours -> (nn int32 [n1, n], nn_val, new_rows, redone_rows).  sim [n1, n1] float32 of the gallery as it stands, live
    [n1] as it stands, nn / nn_val [n0, n] the graph as it was last current (it covered n0 rows).  Old rows against the new rows in
    groups of ``group`` through merge(); the new rows' lists and the flagged rows' lists from scratch."""
    sim = np.asarray(sim, dtype=np.float32)
    live = np.asarray(live).reshape(-1) != 0
    n1, n = sim.shape[0], nn.shape[1]
    out = np.full((n1, n), -1, dtype=np.int32)
    val = np.full((n1, n), -np.inf, dtype=np.float32)
    out[:n0], val[:n0] = nn[:n0], nn_val[:n0]
    redo = np.zeros(n0, dtype=np.uint8)
    if n1 == n0:
        out[:n0], val[:n0], redo = merge(None, 0, n0, n0, live, out[:n0], val[:n0])
    for at in range(n0, n1, group):
        m = min(group, n1 - at)
        cand = np.ascontiguousarray(sim[:n0, at : at + m].T)  # cand[j, i] = s(query i, gallery at + j)
        a, b, r = merge(cand, m, at, n0, live[: at + m], out[:n0], val[:n0])
        out[:n0], val[:n0] = a, b
        redo |= r  # (every launch flags the same rows: a flagged list is not written)
    scratch_nn, scratch_val = built(sim, n, live)
    again = np.nonzero(redo)[0]
    out[again], val[again] = scratch_nn[again], scratch_val[again]
    out[n0:], val[n0:] = scratch_nn[n0:], scratch_val[n0:]
    return out, val, int(live[n0:].sum()), int(again.size)
