"""CPU: the sharded matrix-free rank metrics (evaluation.*_sharded; csrc/rank_stream.hip): the new entry point in the header and
the library, the rewritten `offset` contract, the refusals of the Python surface and the pure-torch list helpers against a
brute-force restatement."""

import subprocess

import pytest
import torch


def test_shard_fix_declared_and_exported():
    import textreid_amd.lib as L

    assert "trid_rank_rerank_fix_shard" in L.EXPORTS
    # trid_rank_rerank_fix's arguments with the row offset (long long) before the stream
    assert L.DECLS["trid_rank_rerank_fix"] == ("int", "pppppppppifilp")
    assert L.DECLS["trid_rank_rerank_fix_shard"] == ("int", "pppppppppifillp")
    out = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True).stdout
    syms = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert "trid_rank_rerank_fix_shard" in syms and "trid_rank_rerank_fix" in syms


def test_header_states_the_offset_contract():
    import textreid_amd.lib as L

    text = open(L.HEADER_PATH).read()
    a = text.index("/* Matrix-free rank metrics")
    block = text[a:text.index("trid_rank_finalize(", a)]
    assert "CURRENTLY UNUSED" not in block
    assert "offset:" in block and "GLOBAL rows" in block and "offset + i < j" in block and "clamp(j - offset, -1, G)" in block


def test_refusals():
    import textreid_amd.evaluation as E

    q, g = torch.randn(4, 8), torch.randn(6, 8)
    qp, gp = torch.arange(4), torch.arange(6)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        E.positive_ranks_sharded(q, g, qp, gp)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        E.rank_from_embeddings_sharded(q, g, qp, gp)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        E.tables_sharded(g, gp, q, qp, (1, 5), rerank=False)


# 5 queries over a gallery of 12 rows cut 5 | 0 | 7 (an empty shard); query 2 has no positive, query 4 has one in each
# non-empty shard and both rows next to the cut (4 | 5)
SIZES = [5, 0, 7]
LISTS = [[0, 6, 11], [3], [], [5, 7, 8, 9], [4, 5]]


def _toy():
    ptr = torch.tensor([0] + [sum(len(r) for r in LISTS[:i + 1]) for i in range(5)])
    idx = torch.tensor([j for r in LISTS for j in r])
    return ptr, idx


def test_owner_split_against_brute_force():
    from textreid_amd.evaluation import _owner_split

    ptr, idx = _toy()
    seen = torch.zeros(idx.numel(), dtype=torch.int64)
    for w, n in enumerate(SIZES):
        off = sum(SIZES[:w])
        own_ptr, own_idx, own_pos = _owner_split(ptr, idx, off, n)
        want_ptr, want_idx, want_pos, e = [0], [], [], 0
        for rows in LISTS:
            for j in rows:
                if off <= j < off + n:
                    want_idx.append(j - off)
                    want_pos.append(e)
                e += 1
            want_ptr.append(len(want_idx))
        assert own_ptr.tolist() == want_ptr and own_idx.tolist() == want_idx and own_pos.tolist() == want_pos, w
        assert own_ptr.dtype == torch.int64 and own_idx.dtype == torch.int64
        seen[own_pos] += 1
    assert seen.tolist() == [1] * idx.numel()  # one owner per entry: the SUM over the ranks is exact
    assert _owner_split(ptr, idx, 5, 0)[2].numel() == 0 and _owner_split(ptr, idx, 5, 0)[0].tolist() == [0] * 6


def test_local_neighbour_list_against_brute_force():
    """the pairs (q, LOCAL row i) of one shard whose rows of GLOBAL neighbour indices intersect"""
    from textreid_amd.evaluation import _neighbour_list

    gen = torch.Generator().manual_seed(4)
    n, G = 3, sum(SIZES)
    qnn = torch.stack([torch.randperm(G, generator=gen)[:n] for _ in range(5)])
    gnn = torch.stack([torch.randperm(G, generator=gen)[:n] for _ in range(G)])
    total = 0
    for w, m in enumerate(SIZES):
        if m == 0:
            continue  # (an empty shard builds no list)
        off = sum(SIZES[:w])
        loc = gnn[off:off + m]
        ptr, idx = _neighbour_list(qnn, loc)
        want = [[i for i in range(m) if set(qnn[q].tolist()) & set(loc[i].tolist())] for q in range(5)]
        assert ptr.tolist() == [0] + [sum(len(r) for r in want[:q + 1]) for q in range(5)], w
        assert idx.tolist() == [i for r in want for i in r], w
        total += idx.numel()
    p_all, i_all = _neighbour_list(qnn, gnn)
    assert total == i_all.numel()
