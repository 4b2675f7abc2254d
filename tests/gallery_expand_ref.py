"""CPU restatement of the blend of query expansion and database-side augmentation (trid_index_blend_rows_f32) and of what
GalleryIndex.expand_queries / search_expanded / augmented build on it: numpy on the host, every step rounded in np.float32 on its
own and taken in list order, so the device's bits can be compared as bit patterns.  Checked against planted cases in
test_gallery_expand_cpu.py."""

import numpy as np

import gallery_deep_distinct_ref as DD
import topk_deep_ref as TR

DIM = 256


def weight(v, power):
    """np.float32 value -> np.float32 weight: t = max(v, 0); power 0: 1; else t multiplied by itself power - 1 times, every product
    rounded to float32 (NOT np.power: the two differ in the last bit for some t)"""
    t = np.maximum(np.float32(v), np.float32(0.0))
    if power == 0:
        return np.float32(1.0)
    w = t
    for _ in range(power - 1):
        w = np.float32(w * t)
    return np.float32(w)


def blend(parts, ids, vals, m, power, base=None, shift=None):
    """parts: a list of float32 [len_s, 256] arrays (one array: the one-part case); ids int [M, >= m], vals float32 [M, >= m]; base
    float32 [M, 256] or None -> float32 [M, 256].  An id is row ``id & ((1 << shift) - 1)`` of part ``id >> shift``; shift 0 (the
    default with one part): id = local row of part 0; the default with several parts is 21.  For every output row, in list order:
    an id < 0 or outside the parts' extents is skipped; acc = acc + (w * row), one float32 multiply and one float32 add per column,
    always both."""
    if isinstance(parts, np.ndarray):
        parts = [parts]
    parts = [np.ascontiguousarray(np.asarray(p, dtype=np.float32)) for p in parts]
    if shift is None:
        shift = 0 if len(parts) == 1 else 21
    assert shift != 0 or len(parts) == 1
    assert 0 <= power <= 4 and 1 <= m <= 32
    ids = np.asarray(ids).astype(np.int64)
    vals = np.asarray(vals, dtype=np.float32)
    M = ids.shape[0]
    out = np.zeros((M, DIM), dtype=np.float32) if base is None else np.array(base, dtype=np.float32, copy=True)
    assert out.shape == (M, DIM)
    lens = np.array([p.shape[0] for p in parts], dtype=np.int64)
    for j in range(m):  # list order; the output rows are independent of each other, so one step runs over all of them at once
        e = ids[:, j]
        part = np.zeros_like(e) if shift == 0 else e >> shift
        row = e if shift == 0 else e & ((1 << shift) - 1)
        ok = (e >= 0) & (part < len(parts))
        ok[ok] = row[ok] < lens[part[ok]]
        if not ok.any():
            continue
        t = np.maximum(vals[:, j], np.float32(0.0))
        w = np.ones(M, dtype=np.float32) if power == 0 else t.copy()
        for _ in range(power - 1):
            w = (w * t).astype(np.float32)
        at = np.nonzero(ok)[0]
        got = np.empty((at.size, DIM), dtype=np.float32)
        for p in np.unique(part[at]):
            here = part[at] == p
            got[here] = parts[int(p)][row[at][here]]
        prod = (w[at, None] * got).astype(np.float32)   # one float32 multiply ...
        out[at] = (out[at] + prod).astype(np.float32)   # ... one float32 add
    return out


def expand(rows, q_unit, sim, m, power, allowed=None):
    """the blend of expand_queries BEFORE its normalisation: rows float32 [G, 256] the stored unit rows, q_unit float32 [Q, 256] the
    unit queries, sim float32 [Q, G] their similarities (the dense product) -> (blend float32 [Q, 256], values [Q, m], rows [Q, m]):
    phase 1 = topk_deep_ref.topk(sim, m, allowed), absent slots (-inf, -1) skipped by the blend"""
    v, r = TR.topk(sim, m, allowed)
    return blend(rows, r, v, m, power, base=q_unit), v, r


def expanded_topk(sim_expanded, k, allowed=None, groups=None):
    """the second pass: sim_expanded float32 [Q, G] = the similarities of the EXPANDED queries -> (values [Q, k], rows [Q, k]), the
    k best allowed rows (topk_deep_ref.topk), or with ``groups`` the k best distinct groups (gallery_deep_distinct_ref)"""
    if groups is None:
        return TR.topk(sim_expanded, k, allowed)
    return DD.distinct_topk(sim_expanded, groups, k, allowed)


def augment(rows, nn, nn_val, m, power):
    """the blend of augmented BEFORE its normalisation: every row's first m list entries (nn int [G, n], nn_val float32 [G, n]), no
    base; a removed row's list is all -1: zeros"""
    return blend(rows, nn, nn_val, m, power)
