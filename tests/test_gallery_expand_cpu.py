"""Query expansion and database-side augmentation without a device: the numpy reference (gallery_expand_ref) against planted cases
where a looser restatement would give other bits, the C ABI of trid_index_blend_rows_f32 (declared, exported, every argument error
reported before anything is dereferenced or launched) and the host rules of GalleryIndex.expand_queries / search_expanded /
augmented and of GalleryShards."""

import re

import numpy as np
import pytest
import torch

import gallery_expand_ref as XR
import topk_deep_ref as TR
from textreid_amd import GalleryIndex, GalleryShards
from textreid_amd import index as IX
from textreid_amd import lib as L


def const_rows(*values):
    """one row per value, every column that value"""
    return np.repeat(np.asarray(values, dtype=np.float32)[:, None], 256, axis=1)


def loop_blend(parts, ids, vals, m, power, base, shift):
    """the definition as the plainest loop: one output row, one list entry, one column at a time"""
    M = len(ids)
    out = np.zeros((M, 256), dtype=np.float32)
    for i in range(M):
        for c in range(256):
            acc = np.float32(0.0) if base is None else np.float32(base[i][c])
            for j in range(m):
                e = int(ids[i][j])
                if e < 0:
                    continue
                part, row = (0, e) if shift == 0 else (e >> shift, e & ((1 << shift) - 1))
                if part >= len(parts) or row >= len(parts[part]):
                    continue
                acc = np.float32(acc + np.float32(XR.weight(vals[i][j], power) * np.float32(parts[part][row][c])))
            out[i, c] = acc
    return out


# ------------------------------------------------------------------ the reference
def test_the_sum_is_taken_in_list_order():
    # 1 + 2^-24 is a tie that rounds back to 1, twice; 2^-24 + 2^-24 = 2^-23 and 1 + 2^-23 is a float32
    tiny = np.float32(2.0 ** -24)
    rows = const_rows(1.0, tiny, tiny)
    vals = np.ones((2, 3), dtype=np.float32)
    out = XR.blend(rows, np.array([[0, 1, 2], [1, 2, 0]]), vals, 3, 0)
    assert (TR.bits(out[0]) == TR.bits(np.float32(1.0))).all()
    assert (TR.bits(out[1]) == TR.bits(np.float32(1.0) + np.float32(2.0 ** -23))).all()
    assert TR.bits(out[0, 0]) != TR.bits(out[1, 0])
    # the base comes first: base 1, then the two tiny rows - not the rows summed and added to the base
    out = XR.blend(rows, np.array([[1, 2]]), vals[:1], 2, 0, base=const_rows(1.0))
    assert (TR.bits(out) == TR.bits(np.float32(1.0))).all()


def test_the_power_is_repeated_multiplication_not_pow():
    t = np.float32(0.59248704)
    rep = np.float32(np.float32(t * t) * t)
    exact = np.float32(np.float64(t) ** 3)
    assert TR.bits(rep) != TR.bits(exact) and TR.bits(np.power(t, np.float32(3))) == TR.bits(exact)  # (the planted value: the two differ)
    assert TR.bits(XR.weight(t, 3)) == TR.bits(rep)
    out = XR.blend(const_rows(1.0), np.array([[0]]), np.array([[t]], dtype=np.float32), 1, 3)
    assert (TR.bits(out) == TR.bits(rep)).all()
    assert TR.bits(XR.weight(t, 1)) == TR.bits(t) and TR.bits(XR.weight(t, 0)) == TR.bits(np.float32(1.0))
    assert TR.bits(XR.weight(t, 4)) == TR.bits(np.float32(rep * t)) and TR.bits(XR.weight(t, 2)) == TR.bits(np.float32(t * t))


def test_multiply_and_add_are_two_roundings():
    # w * x = (1 + 2^-12)^2 = 1 + 2^-11 + 2^-24 rounds to 1 + 2^-11; a fused multiply-add onto -(1 + 2^-11) would keep the 2^-24
    a = np.float32(1.0 + 2.0 ** -12)
    out = XR.blend(const_rows(a), np.array([[0]]), np.array([[a]], dtype=np.float32), 1, 1, base=const_rows(-(1.0 + 2.0 ** -11)))
    assert (TR.bits(out) == TR.bits(np.float32(0.0))).all()


def test_absent_out_of_extent_and_duplicate_entries():
    rows = const_rows(1.0, 2.0, 4.0)
    ones = np.ones((1, 5), dtype=np.float32)
    base = const_rows(0.5)
    for ids, want in (([-1, 0, -1, 2, -1], 5.5), ([-1] * 5, 0.5), ([3, 2 ** 31 - 1, 1, -7, 2 ** 40], 2.5), ([1, 1, 0, 1, -1], 7.5)):
        out = XR.blend(rows, np.array([ids]), ones, 5, 0, base=base)
        assert (TR.bits(out) == TR.bits(np.float32(want))).all(), ids
    assert (TR.bits(XR.blend(rows, np.array([[-1] * 5]), ones, 5, 0)) == 0).all()  # (no base: +0.0)
    # m cuts the list: the entries behind it are not read
    assert (TR.bits(XR.blend(rows, np.array([[0, 1, 2, 2, 2]]), ones, 2, 0)) == TR.bits(np.float32(3.0))).all()
    # several parts: id = part << 21 | row; a part beyond the table and a row at the part's length are skipped
    parts = [const_rows(1.0), const_rows(2.0, 4.0), const_rows(8.0)]
    S = 1 << 21
    ids = np.array([[0, S + 1, 2 * S, 3 * S, S + 2, 1, 2 * S + 1, S]])
    out = XR.blend(parts, ids, np.ones((1, 8), dtype=np.float32), 8, 0)
    assert (TR.bits(out) == TR.bits(np.float32(1.0 + 4.0 + 8.0 + 2.0))).all()


def test_values_that_give_weight_zero_or_one():
    rows = const_rows(3.0)
    vals = np.array([[-0.25, 0.0, -np.inf, -0.0]], dtype=np.float32)
    ids = np.zeros((1, 4), dtype=np.int64)
    for power in (1, 2, 3, 4):
        out = XR.blend(rows, ids, vals, 4, power, base=const_rows(0.5))
        assert (TR.bits(out) == TR.bits(np.float32(0.5))).all(), power
        assert TR.bits(XR.weight(np.float32(-np.inf), power)) == 0
    assert (TR.bits(XR.blend(rows, ids, vals, 4, 0, base=const_rows(0.5))) == TR.bits(np.float32(12.5))).all()
    # the add happens also with w == 0: -0.0 + (0 * 3) = +0.0
    assert (TR.bits(XR.blend(rows, ids[:, :1], vals[:, :1], 1, 1, base=const_rows(-0.0))) == 0).all()
    assert (TR.bits(XR.blend(rows, np.array([[-1]]), vals[:, :1], 1, 1, base=const_rows(-0.0))) == TR.bits(np.float32(-0.0))).all()


def test_the_vectorised_reference_equals_the_plain_loop():
    rng = np.random.RandomState(11)
    S = 1 << 21
    parts = [rng.standard_normal((n, 256)).astype(np.float32) for n in (3, 1, 5)]
    M, m = 6, 7
    ids = rng.randint(0, 3, size=(M, m)) * S + rng.randint(0, 6, size=(M, m))
    ids[0, 0], ids[1, 3], ids[2] = -1, 5 * S, -1
    vals = rng.standard_normal((M, m)).astype(np.float32)
    base = rng.standard_normal((M, 256)).astype(np.float32)
    for power in (0, 1, 3):
        for b in (None, base):
            assert np.array_equal(TR.bits(XR.blend(parts, ids, vals, m, power, base=b)), TR.bits(loop_blend(parts, ids, vals, m, power, b, 21)))
    one = parts[2]
    ids1 = rng.randint(-1, 7, size=(M, m))
    assert np.array_equal(TR.bits(XR.blend(one, ids1, vals, m, 2, base=base)), TR.bits(loop_blend([one], ids1, vals, m, 2, base, 0)))


def test_expand_takes_the_m_best_allowed_rows_and_skips_absent_slots():
    rng = np.random.RandomState(5)
    rows = rng.standard_normal((9, 256)).astype(np.float32)
    q = rng.standard_normal((2, 256)).astype(np.float32)
    sim = (q @ rows.T).astype(np.float32)
    allow = np.zeros(9, dtype=bool)
    allow[[2, 7]] = True
    got, v, r = XR.expand(rows, q, sim, 4, 1, allow)
    assert (r[:, 2:] == -1).all() and np.isneginf(v[:, 2:]).all() and set(r[0, :2].tolist()) == {2, 7}
    assert np.array_equal(TR.bits(got), TR.bits(loop_blend([rows], r, v, 4, 1, q, 0)))
    vals, idx = XR.expanded_topk(sim, 3, allow)
    assert (idx[:, 2] == -1).all() and TR.same((vals, idx), TR.topk(sim, 3, allow))
    vals, idx = XR.expanded_topk(sim, 2, None, groups=np.array([0, 0, 0, 1, 1, 1, 2, 2, 2]))
    assert all(len({int(i) // 3 for i in row}) == 2 for row in idx)


# ------------------------------------------------------------------ the C ABI
def test_the_symbol_is_declared_and_exported():
    lib = L.load()
    assert "trid_index_blend_rows_f32" in L.EXPORTS and hasattr(lib, "trid_index_blend_rows_f32")
    assert L.DECLS["trid_index_blend_rows_f32"] == ("int", "ppiipipliiiplpp")


FAKE = 0x10000  # a 16-byte aligned non-null address: every limit is checked before anything is dereferenced or launched


def _blend(table=FAKE, lens=FAKE, n_parts=1, shift=0, ids=FAKE, id_bytes=8, vals=FAKE, ld_list=5, M=4, m=5, power=1, base=FAKE, ld_base=256,
           out=FAKE):
    L.call("trid_index_blend_rows_f32", table, lens, n_parts, shift, ids, id_bytes, vals, ld_list, M, m, power, base, ld_base, out, None)


@pytest.mark.parametrize("kw,word", [
    (dict(table=None), "null"),
    (dict(lens=None), "null"),
    (dict(ids=None), "null"),
    (dict(vals=None), "null"),
    (dict(out=None), "null"),
    (dict(m=0, ld_list=5), "m must be"),
    (dict(m=33, ld_list=40), "m must be"),
    (dict(power=-1), "power must be"),
    (dict(power=5), "power must be"),
    (dict(ld_list=4), "ld_list"),
    (dict(id_bytes=2), "id_bytes"),
    (dict(id_bytes=16), "id_bytes"),
    (dict(M=0), "M must be"),
    (dict(M=-3), "M must be"),
    (dict(shift=-1), "shift"),
    (dict(shift=31), "shift"),
    (dict(n_parts=0), "n_parts"),
    (dict(n_parts=3, shift=0), "n_parts"),
    (dict(base=FAKE + 4), "aligned"),
    (dict(out=FAKE + 8), "aligned"),
    (dict(ld_base=258), "aligned"),
    (dict(ld_base=252), "aligned"),
    (dict(ids=FAKE + 4), "aligned"),
    (dict(ids=FAKE + 2, id_bytes=4), "aligned"),
    (dict(vals=FAKE + 2), "aligned"),
    (dict(table=FAKE + 4), "aligned"),
])
def test_bad_arguments_are_errors_that_name_the_function(kw, word):
    with pytest.raises(RuntimeError, match="trid_index_blend_rows_f32") as e:
        _blend(**kw)
    assert re.search(word, str(e.value)), str(e.value)
    assert L.last_error().startswith("trid_index_blend_rows_f32:")
    # the process survives and the library still answers
    assert L.load().trid_topk_rows_deep_ws_bytes(4, 100, 10, 0) > 0


# ------------------------------------------------------------------ host rules
@pytest.mark.parametrize("name", ["expand_queries", "search_expanded", "search_expanded_pids"])
def test_expanded_search_argument_rules(name):
    assert IX.MAX_EXPAND == 32 and IX.MAX_EXPAND_POWER == 4
    q = torch.zeros(1, 256)
    idx = GalleryIndex()
    idx._has_pids = True
    with pytest.raises(ValueError, match="%s: the index is empty" % name):
        getattr(idx, name)(q)
    idx._n = 5000  # (rows held: the rules are checked before anything touches the storage)
    for m in (0, -1, 33, 2.0):
        with pytest.raises(ValueError, match="%s: m must be in \\[1, 32\\]" % name):
            getattr(idx, name)(q, m=m)
    for power in (-1, 5, 1.5):
        with pytest.raises(ValueError, match="%s: power must be an integer in \\[0, 4\\]" % name):
            getattr(idx, name)(q, power=power)
    idx._dead = 4997
    with pytest.raises(ValueError, match="%s: m must be <= live_count = 3" % name):
        getattr(idx, name)(q, m=5)
    with pytest.raises(ValueError, match="%s: mask must have shape" % name):  # (with a mask m is not held against live_count)
        getattr(idx, name)(q, m=5, mask=torch.ones(7, dtype=torch.bool))
    idx._dead = 0
    with pytest.raises(ValueError, match="%s: expected" % name):
        getattr(idx, name)(torch.zeros(1, 128))
    if name != "expand_queries":
        for k in (0, 1025):
            with pytest.raises(ValueError, match="%s: k must be" % name):
                getattr(idx, name)(q, k=k)
    with pytest.raises(RuntimeError, match="%s runs on the HIP kernel library only.*no CPU fallback" % name):
        getattr(idx, name)(q)
    small = GalleryIndex()
    small._n = 4
    with pytest.raises(ValueError, match="%s: m must be in \\[1, 32\\] and <= len\\(index\\) = 4" % name):
        getattr(small, name)(q, m=5)
    if name == "search_expanded_pids":
        small._has_pids = False
        with pytest.raises(ValueError, match="search_expanded_pids: the index holds no pids"):
            small.search_expanded_pids(q, k=2, m=2)


def test_augmented_needs_a_current_graph_with_values():
    idx = GalleryIndex()
    with pytest.raises(RuntimeError, match="augmented: the neighbour graph is absent.*build_neighbours.*refresh_neighbours"):
        idx.augmented()
    idx._n = 100
    idx._nn, idx._nn_ok = torch.zeros(100, 5, dtype=torch.int32), False
    with pytest.raises(RuntimeError, match="augmented: the neighbour graph is stale.*build_neighbours"):
        idx.augmented()
    idx._nn_ok = True
    with pytest.raises(RuntimeError, match="augmented: the neighbour graph is held without its values.*build_neighbours"):
        idx.augmented()
    idx._nn_val = torch.zeros(100, 5)
    for m in (0, 6, 2.0):
        with pytest.raises(ValueError, match="augmented: m must be in \\[1, n = 5\\]"):
            idx.augmented(m=m)
    for power in (-1, 5):
        with pytest.raises(ValueError, match="augmented: power must be an integer in \\[0, 4\\]"):
            idx.augmented(power=power)


@pytest.mark.parametrize("name", ["expand_queries", "search_expanded", "search_expanded_pids"])
def test_shards_rules_and_the_by_rank_form(name):
    q = torch.zeros(1, 256)
    with pytest.raises(RuntimeError, match="%s: query expansion is not built for the by-rank form" % name):
        getattr(GalleryShards(collective=True), name)(q)
    sh = GalleryShards(shard_rows=7)
    for m in (0, 33):
        with pytest.raises(ValueError, match="GalleryShards.%s: m must be in \\[1, 32\\]" % name):
            getattr(sh, name)(q, m=m)
    with pytest.raises(ValueError, match="GalleryShards.%s: power must be" % name):
        getattr(sh, name)(q, power=7)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        getattr(sh, name)(q)
    assert not hasattr(sh, "augmented")
