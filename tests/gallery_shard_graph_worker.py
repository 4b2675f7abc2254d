"""One rank of tests/test_gallery_shard_graph_gpu.py::test_two_ranks: GalleryShards(collective=True) over gloo, both ranks sharing the
one GPU - build_neighbours, search_reranked and search_reranked_pids against ONE GalleryIndex over the whole gallery, whose graph and
results are computed before init_process_group.  Every rank checks its own lists and results against the same expectation (so the
results are identical on every rank); rank 0 prints one tag per case."""

import os
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from gallery_shards_worker import G, Q, bits, inputs  # noqa: E402

N = 5
CASES = (("search_reranked", 10), ("search_reranked", 100), ("search_reranked", 301), ("search_reranked_pids", 10), ("search_reranked_pids", 100))


def main():
    r, W = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    assert W == 2
    dev = torch.device("cuda", r % torch.cuda.device_count())
    torch.cuda.set_device(dev)
    from textreid_amd import GalleryIndex, GalleryShards
    from textreid_amd.index_shards import SHARD_STRIDE

    q, g, pids = (t.to(dev) for t in inputs())
    gone = torch.tensor([7, 150, 199, 200, 263])  # removed rows on both sides of the cut at 200
    one = GalleryIndex()
    one.add(g, pids, normalize=False)
    one.remove(rows=gone)
    one.build_neighbours(N)
    nn, nn_val = one.neighbours.long().cpu(), one.neighbour_values.cpu()
    want = {(name, k): [t.cpu() for t in getattr(one, name)(q, k=min(k, one.live_count), alpha=0.2, normalize=False)] for name, k in CASES}
    torch.cuda.synchronize()

    dist.init_process_group(os.environ.get("TRID_DIST_BACKEND", "gloo"), init_method="env://")
    assert dist.get_world_size() == 2 and dist.get_rank() == r

    def to_global(rows, cut):
        return torch.where(rows < 0, rows, torch.where(rows < cut, rows, rows - cut + SHARD_STRIDE))

    def check(cut, what):
        """rank 0 holds rows [0, cut), rank 1 the rest"""
        sh = GalleryShards(collective=True)
        lo, hi = (0, cut) if r == 0 else (cut, G)
        sh.add(g[lo:hi], pids[lo:hi], normalize=False)
        sh.remove(rows=to_global(gone, cut))  # (every rank passes the same rows: those of the other rank are skipped)
        assert sh.neighbours is None and not sh.neighbours_current
        sh.build_neighbours(N)
        assert sh.neighbours_current and len(sh.neighbours) == 1 and tuple(sh.neighbours[0].shape) == (hi - lo, N)
        assert torch.equal(sh.neighbours[0].long().cpu(), to_global(nn[lo:hi], cut)), (what, "lists")
        assert np.array_equal(bits(sh.neighbour_values[0]), bits(nn_val[lo:hi])), (what, "values")
        try:
            sh.refresh_neighbours()
            raise AssertionError("the by-rank refresh must be refused")
        except RuntimeError as e:
            assert "build_neighbours" in str(e)
        for name, k in CASES:
            got = [t.cpu() for t in getattr(sh, name)(q, k=k, alpha=0.2, normalize=False)]
            exp = want[(name, k)]
            kk = exp[0].shape[1]
            assert all(tuple(t.shape) == (Q, k) for t in got), (what, name, k)
            assert np.array_equal(bits(got[0][:, :kk]), bits(exp[0])), (what, name, k, "values")
            assert torch.equal(got[1][:, :kk], to_global(exp[1], cut)), (what, name, k, "rows")
            if len(exp) == 3:
                assert torch.equal(got[2][:, :kk], exp[2]), (what, name, k, "pids")
            assert bool(torch.isneginf(got[0][:, kk:]).all()) and all(bool((t[:, kk:] == -1).all()) for t in got[1:]), (what, name, k, "tail")
        if r == 0:
            print(what, flush=True)

    check(200, "SHARD_GRAPH_UNEVEN_OK")
    check(G, "SHARD_GRAPH_EMPTY_OK")  # (rank 1 holds nothing and joins with all-absent lists)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
