"""One rank of tests/test_gallery_shards_gpu.py::test_two_ranks: GalleryShards(collective=True) over gloo, both ranks sharing the
one GPU, against the results of ONE GalleryIndex over the whole gallery, which are computed before init_process_group.  Every rank
checks its own results against the same expectation (so they are identical on every rank); rank 0 prints one tag per case."""

import os
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

G, Q = 300, 33
CASES = (("search", 10), ("search", 16), ("search_pids", 10), ("shortlist", 100), ("shortlist", 301), ("shortlist_pids", 100), ("shortlist_pids", 17))


def inputs():
    """the exact-arithmetic levels of _tie_inputs (tests/test_rank_shard_gpu.py), a few base rows repeated: exact ties straddle the cut"""
    gen = torch.Generator().manual_seed(23)
    lv = torch.tensor([-1.0, -0.5, 0.0, 0.5, 1.0]) / 8
    q = lv[torch.randint(0, 5, (Q, 256), generator=gen)]
    base = lv[torch.randint(0, 5, (12, 256), generator=gen)]
    g = base[torch.randint(0, 12, (G,), generator=gen)]
    pids = torch.randint(0, 40, (G,), generator=gen)
    return q, g, pids


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32).numpy()


def main():
    r, W = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    assert W == 2
    dev = torch.device("cuda", r % torch.cuda.device_count())
    torch.cuda.set_device(dev)
    from textreid_amd import GalleryIndex, GalleryShards
    from textreid_amd.index_shards import SHARD_STRIDE

    q, g, pids = (t.to(dev) for t in inputs())
    one = GalleryIndex()
    one.add(g, pids, normalize=False)
    # Q = 33: the plain index's shortlist / shortlist_pids are the panelled comparators (bit-identical to search at k <= 16)
    want = {}
    for name, k in CASES:
        fn = getattr(one, "shortlist_pids" if name.endswith("pids") else "shortlist")
        got = fn(q, k=min(k, G), normalize=False)
        want[(name, k)] = [t.cpu() for t in got]
    torch.cuda.synchronize()

    dist.init_process_group(os.environ.get("TRID_DIST_BACKEND", "gloo"), init_method="env://")
    assert dist.get_world_size() == 2 and dist.get_rank() == r

    def check(cut, what):
        """rank 0 holds rows [0, cut), rank 1 the rest"""
        sh = GalleryShards(collective=True)
        lo, hi = (0, cut) if r == 0 else (cut, G)
        first = sh.add(g[lo:hi], pids[lo:hi], normalize=False)
        assert first == r * SHARD_STRIDE and len(sh) == hi - lo and sh.n_shards == 2 and sh.shard == r
        for name, k in CASES:
            got = [t.cpu() for t in getattr(sh, name)(q, k=k, normalize=False)]
            exp = want[(name, k)]
            kk = exp[0].shape[1]
            assert all(tuple(t.shape) == (Q, k) for t in got), (what, name, k)
            assert np.array_equal(bits(got[0][:, :kk]), bits(exp[0])), (what, name, k, "values")
            rows = torch.where(exp[1] < cut, exp[1], exp[1] - cut + SHARD_STRIDE)
            rows = torch.where(exp[1] < 0, exp[1], rows)
            assert torch.equal(got[1][:, :kk], rows), (what, name, k, "rows")
            if len(exp) == 3:
                assert torch.equal(got[2][:, :kk], exp[2]), (what, name, k, "pids")
            assert bool(torch.isneginf(got[0][:, kk:]).all()) and all(bool((t[:, kk:] == -1).all()) for t in got[1:]), (what, name, k, "tail")
        if r == 0:
            print(what, flush=True)

    check(200, "SHARDS_UNEVEN_OK")
    check(G, "SHARDS_EMPTY_OK")  # (rank 1 holds nothing and joins with all-absent lists)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
