"""Incremental neighbour-graph refresh without a device: the numpy reference (gallery_nn_update_ref) against a loop that inserts one
candidate at a time and against the from-scratch graph of the final matrix (gallery_rerank_ref.graph), the C ABI of
trid_index_nn_merge_f32 (declared, exported, every argument error reported before anything is dereferenced or launched) and the host
rules of GalleryIndex.refresh_neighbours / neighbour_values / state_dict."""

import re

import numpy as np
import pytest
import torch

import gallery_nn_update_ref as NU
import gallery_rerank_ref as RR
import topk_deep_ref as TR
from textreid_amd import GalleryIndex
from textreid_amd import lib as L


# ------------------------------------------------------------------ the reference
def asymmetric(rng, G, grid):
    """[G, G] float32, sim[i, g] != sim[g, i]: a symmetric part plus a direction-dependent term in the last bits (grid=False), or
    rounded to multiples of 1/64 (grid=True: many exact ties, asymmetric where the rounding falls differently)"""
    x = rng.standard_normal((G, 16)).astype(np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    sim = (x @ x.T).astype(np.float32)
    if grid:
        sim = (np.rint((sim + rng.uniform(-0.02, 0.02, size=(G, G)).astype(np.float32)) * 64) / 64).astype(np.float32)
    else:
        sim = (sim * (1 + rng.randint(-3, 4, size=(G, G)).astype(np.float32) * np.float32(2.0 ** -23))).astype(np.float32)
    assert (sim != sim.T).any()
    return sim


def test_merge_equals_inserting_one_candidate_at_a_time():
    rng = np.random.RandomState(2)
    rows, m, n, first = 70, 9, 5, 80
    live = rng.randint(0, 5, size=first + m) != 0
    live[:4] = [True, False, True, True]
    vals = np.sort((rng.randint(-8, 9, size=(rows, n)) / 8).astype(np.float32), axis=1)[:, ::-1].copy()
    nn = np.stack([np.sort(rng.permutation(first)[:n]) for _ in range(rows)]).astype(np.int32)
    nn[2] = -1  # a live row no graph has covered
    nn[3], live[[5, 6]], live[first] = [0, 2, 3, 5, 6], True, True
    vals[3] = [0.5, 0.0, -0.0, -0.5, -1.0]
    cand = (rng.randint(-8, 9, size=(m, rows + 3)) / 8).astype(np.float32)
    cand[:, 3] = -2.0
    cand[0, 3] = -0.0  # +0 == -0: the candidate stays behind both zeros and keeps its sign bit
    got_nn, got_val, redo = NU.merge(cand, m, first, rows, live, nn, vals)
    for i in range(rows):
        if not live[i]:
            assert (got_nn[i] == -1).all() and np.isneginf(got_val[i]).all() and redo[i] == 0
            continue
        if nn[i, 0] < 0 or not live[nn[i]].all():
            assert redo[i] == 1 and np.array_equal(got_nn[i], nn[i]) and np.array_equal(TR.bits(got_val[i]), TR.bits(vals[i]))
            continue
        pairs = list(zip(vals[i].tolist(), nn[i].tolist(), TR.bits(vals[i]).tolist()))
        for j in range(m):
            if live[first + j]:
                c = cand[j, i]
                at = next((u for u in range(n) if c > pairs[u][0]), n)
                pairs = (pairs[:at] + [(float(c), first + j, int(TR.bits(c).reshape(-1)[0]))] + pairs[at:])[:n]
        assert redo[i] == 0 and got_nn[i].tolist() == [p[1] for p in pairs] and TR.bits(got_val[i]).tolist() == [p[2] for p in pairs], i
    assert redo.sum() >= 2 and (redo[live[:rows]] == 0).sum() >= 10
    assert got_nn[3].tolist() == [0, 2, 3, first, 5] and TR.bits(got_val[3]).tolist() == TR.bits(np.float32([0.5, 0.0, -0.0, -0.0, -0.5])).tolist()
    # the pure-removal pass
    a, b, r = NU.merge(None, 0, first, rows, live[:first], nn, vals)
    assert np.array_equal(r, redo) and np.array_equal(a[live[:rows] & (r == 0)], nn[live[:rows] & (r == 0)])


@pytest.mark.parametrize("grid", [False, True])
@pytest.mark.parametrize("n", [1, 5, 8])
@pytest.mark.parametrize("n0,added", [(64, 32), (65, 1), (300, 45), (20, 100)])
def test_reference_refresh_equals_the_graph_of_the_final_matrix(n0, added, n, grid):
    rng = np.random.RandomState(1000 * n0 + 10 * added + n + (5 if grid else 0))
    n1 = n0 + added
    sim = asymmetric(rng, n1, grid)
    # tombstones at build time
    live0 = np.ones(n0, dtype=bool)
    live0[rng.permutation(n0)[: n0 // 8]] = False
    nn, val = NU.built(sim[:n0, :n0], n, live0)
    assert np.array_equal(nn, RR.graph(sim[:n0, :n0], n, live0))
    # add, then remove old rows and just-added rows
    live = np.concatenate([live0, np.ones(added, dtype=bool)])
    live[rng.permutation(n0)[: n0 // 6]] = False
    if added > 1:
        live[n0 + rng.permutation(added)[: (added + 3) // 4]] = False
    assert live.sum() >= n
    got_nn, got_val, new_rows, redone = NU.refresh(sim, live, nn, val, n0)
    want = RR.graph(sim, n, live)
    assert np.array_equal(got_nn, want), (n0, added, n, grid)
    want_val = np.where(want >= 0, np.take_along_axis(sim, np.maximum(want, 0).astype(np.int64), axis=1), -np.inf).astype(np.float32)
    assert np.array_equal(TR.bits(got_val), TR.bits(want_val))
    assert new_rows == int(live[n0:].sum())
    held_dead = np.array([live[i] and live0[i] and not live[nn[i][nn[i] >= 0]].all() for i in range(n0)])
    assert redone == int(held_dead.sum()) and (redone > 0 or n < 5 or n0 < 64)
    # adds alone, and removals alone
    only_add = np.concatenate([live0, np.ones(added, dtype=bool)])
    a, b, nr, rd = NU.refresh(sim, only_add, nn, val, n0)
    assert np.array_equal(a, RR.graph(sim, n, only_add)) and (nr, rd) == (added, 0)
    only_rm = live[:n0]
    if only_rm.sum() >= n:
        a, b, nr, rd = NU.refresh(sim[:n0, :n0], only_rm, nn, val, n0)
        assert np.array_equal(a, RR.graph(sim[:n0, :n0], n, only_rm)) and nr == 0


# ------------------------------------------------------------------ the C ABI
def test_the_symbol_is_declared_and_exported():
    lib = L.load()
    assert "trid_index_nn_merge_f32" in L.EXPORTS and hasattr(lib, "trid_index_nn_merge_f32")
    assert L.DECLS["trid_index_nn_merge_f32"] == ("int", "pliiipppipp")


FAKE = 0x10000  # a 16-byte aligned non-null address: every limit is checked before anything is dereferenced or launched


def _merge(cand=FAKE, ld_cand=100, m=4, cand_first=100, rows=100, live=FAKE, nn=FAKE, nn_val=FAKE, n=5, redo=FAKE):
    L.call("trid_index_nn_merge_f32", cand, ld_cand, m, cand_first, rows, live, nn, nn_val, n, redo, None)


@pytest.mark.parametrize("kw,word", [
    (dict(live=None), "null"),
    (dict(nn=None), "null"),
    (dict(nn_val=None), "null"),
    (dict(redo=None), "null"),
    (dict(cand=None), "null"),
    (dict(n=0), "n must be"),
    (dict(n=9), "n must be"),
    (dict(m=-1), "m must be"),
    (dict(rows=0), "rows must be"),
    (dict(rows=-3), "rows must be"),
    (dict(rows=101), "rows must be"),
    (dict(rows=100, cand_first=99), "rows must be"),
    (dict(ld_cand=99), "ld_cand"),
    (dict(ld_cand=0), "ld_cand"),
    (dict(cand_first=2 ** 31 - 2, m=4), "int32"),
    (dict(cand=FAKE + 2), "aligned"),
    (dict(nn=FAKE + 1), "aligned"),
    (dict(nn_val=FAKE + 2), "aligned"),
])
def test_bad_arguments_are_errors_that_name_the_function(kw, word):
    with pytest.raises(RuntimeError, match="trid_index_nn_merge_f32") as e:
        _merge(**kw)
    assert re.search(word, str(e.value)), str(e.value)
    assert L.last_error().startswith("trid_index_nn_merge_f32:")
    # the process survives and the library still answers
    assert L.load().trid_topk_rows_deep_ws_bytes(4, 100, 10, 0) > 0


# ------------------------------------------------------------------ host rules of the index
def test_refresh_without_a_graph_names_build_neighbours():
    idx = GalleryIndex()
    assert idx.neighbour_values is None and not idx.neighbours_refreshable
    with pytest.raises(RuntimeError, match="refresh_neighbours: .*build_neighbours"):
        idx.refresh_neighbours()
    idx._n = 40  # (rows held: the rules are checked before anything touches the storage)
    with pytest.raises(RuntimeError, match="refresh_neighbours: .*build_neighbours"):
        idx.refresh_neighbours()
    # lists without values: current, not refreshable
    idx._nn, idx._nn_ok = torch.zeros(40, 5, dtype=torch.int32), True
    assert idx.neighbours_current and not idx.neighbours_refreshable and idx.neighbour_values is None
    with pytest.raises(RuntimeError, match="refresh_neighbours: .*without its values.*build_neighbours"):
        idx.refresh_neighbours()
    # values of another n do not count
    idx._nn_val = torch.zeros(40, 4)
    assert not idx.neighbours_refreshable
    # refreshable: n beyond live_count is build_neighbours' error, raised before anything is modified; a current graph is (0, 0)
    idx._nn_val = torch.zeros(40, 5)
    assert idx.neighbours_refreshable and tuple(idx.neighbour_values.shape) == (40, 5)
    assert idx.refresh_neighbours() == (0, 0)
    idx._dead, idx._nn_ok = 36, False
    with pytest.raises(ValueError, match="build_neighbours: n must be <= live_count = 4"):
        idx.refresh_neighbours()
    assert not idx.neighbours_current and bool((idx._nn == 0).all())


def test_state_dict_keys_of_an_empty_index():
    sd = GalleryIndex().state_dict()
    assert "neighbour_values" in sd and sd["neighbour_values"] is None and sd["neighbours"] is None


@pytest.mark.parametrize("val,word", [
    (torch.zeros(6, 5), "float32 \\[7, 5\\]"),
    (torch.zeros(7, 4), "float32 \\[7, 5\\]"),
    (torch.zeros(35), "float32 \\[7, 5\\]"),
    (torch.zeros(7, 5, dtype=torch.float64), "float32"),
    (torch.zeros(7, 5, dtype=torch.int32), "float32"),
    ([[0.0] * 5] * 7, "float32"),
])
def test_load_state_dict_refuses_bad_values(val, word):
    idx = GalleryIndex()
    nn = torch.full((7, 5), -1, dtype=torch.int32)
    with pytest.raises(ValueError, match="load_state_dict: neighbour_values must") as e:
        idx.load_state_dict({"rows": torch.zeros(7, 256), "pids": None, "neighbours": nn, "neighbour_values": val})
    assert re.search(word, str(e.value)), str(e.value)
    assert len(idx) == 0 and idx.neighbours is None and idx.neighbour_values is None
    with pytest.raises(ValueError, match="load_state_dict: neighbour_values without neighbours"):
        idx.load_state_dict({"rows": torch.zeros(7, 256), "pids": None, "neighbours": None, "neighbour_values": torch.zeros(7, 5)})
    # a dict with no "neighbours" key at all loads with no graph, as it always did: the next rule is the device's
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        idx.load_state_dict({"rows": torch.zeros(7, 256), "pids": None, "neighbour_values": torch.zeros(7, 5)})
    # well-formed values pass the rules: the next rule is the device's
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        idx.load_state_dict({"rows": torch.zeros(7, 256), "pids": None, "neighbours": nn, "neighbour_values": torch.zeros(7, 5)})
