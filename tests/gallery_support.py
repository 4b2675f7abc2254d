"""What the GalleryIndex / GalleryShards GPU tests share, written once: the `gpu` fixture, the dense comparator that defines "exact" for
every search test, the direct call of the C search entries, the host-packed allow words, the seeded inputs with their caches, the two
result comparators, and the GalleryIndex / GalleryShards pair.  A plain module imported by name, like the *_ref.py modules; a test file
imports `gpu` by name and pytest registers it there.  Nothing here is a test, and no test module is imported from here or from another
test module."""

import numpy as np
import pytest
import torch

import oracle.fill as OF
import topk_deep_ref as TR


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda")


# ------------------------------------------------------------------------------------------------------------------ the dense comparator
def unit_rows(x):
    from textreid_amd import ops

    return ops.l2norm_rows(x.contiguous())[0]


def query_panel(idx, q_unit, rows=32):
    """the zero-padded P16 query panel, packed with the index's unit scalar as the searches pack it"""
    from textreid_amd import ops

    panel = torch.zeros(rows, 256, device=q_unit.device)
    panel[: q_unit.shape[0]] = ops.p16_pack(q_unit.contiguous(), amax_=idx.unit_amax).data
    return panel


def dense_product(idx, q_unit):
    """-> fp32 [Q, len] on the host: trid_gemm_p16 with the index's own P16 gallery (removed rows included) as A and zero-padded panels
    of 32 queries as B.  These are the similarities every search must reproduce bit for bit: same arithmetic, same product order."""
    from textreid_amd import ops

    G = len(idx)
    A = ops.P16(idx.rows_p16, idx.unit_amax)
    out = []
    for at in range(0, q_unit.shape[0], 32):
        part = q_unit[at : at + 32]
        sim = None
        for cols in (32, 64):  # (a 64-row panel if the tile kernel declines 32 columns)
            B = ops.P16(query_panel(idx, part, cols), idx.unit_amax)
            C = torch.empty(G, cols, device=q_unit.device)
            try:
                ops.gemm_p16(A, B, C, G, cols, 256, cols)
            except RuntimeError:
                continue
            sim = C[:, : part.shape[0]].t().contiguous().cpu()
            break
        assert sim is not None
        out.append(sim)
    return torch.cat(out, dim=0)


# ------------------------------------------------------------------------------------------------------------------ the C entries
def words_tensor(allow, device, extra=0, garbage=False, seed=None):
    """bool [n] (tensor or array) -> the packed allow words, made on the host and NOT by the pack kernel, as the int32 device buffer the
    C entries read.  garbage: the bits of rows >= n in the last word are set, which a reader must ignore - all of them, or with a seed
    random ones with bit n itself set.  extra: that many words of all ones behind the (n + 31) // 32 the contract names."""
    allow = np.asarray(allow.cpu() if torch.is_tensor(allow) else allow).reshape(-1) != 0
    n = allow.size
    nw = (n + 31) // 32
    bits = np.zeros(nw * 32, dtype=np.uint64)
    bits[:n] = allow
    if garbage and nw * 32 > n:
        bits[n:] = 1 if seed is None else np.random.RandomState(seed).randint(0, 2, size=nw * 32 - n)
        bits[n] = 1
    w = (bits.reshape(nw, 32) << np.arange(32, dtype=np.uint64)[None, :]).sum(axis=1).astype(np.uint32)
    w = np.concatenate([w, np.full(extra, 0xFFFFFFFF, dtype=np.uint32)])
    return torch.from_numpy(w.view(np.int32).copy()).to(device)


def c_search(idx, q_unit, k, workgroups, allow=None, gid=None):
    """trid_index_search_p16 itself with a forced number of workers; with allow trid_index_search_masked_p16; with gid (any int32
    labels, one per row) trid_index_search_distinct_p16, its mask_words NULL unless allow is given.  The outputs start as garbage."""
    from textreid_amd import lib as L
    from textreid_amd.ops import _p, stream

    Q, G = q_unit.shape[0], len(idx)
    dev = q_unit.device
    q16 = query_panel(idx, q_unit)
    nws = L.load().trid_index_search_ws_bytes(G, Q, k, workgroups)
    assert nws > 0
    ws = torch.empty(nws, dtype=torch.uint8, device=dev)
    vals = torch.full((Q, k), float("nan"), device=dev)
    rows = torch.full((Q, k), -7, dtype=torch.int64, device=dev)
    words = None
    if allow is not None:
        words = words_tensor(allow, dev)
        assert words.numel() == (G + 31) // 32  # exactly the words the contract names: nothing beyond them may be read
    if gid is not None:
        ids = gid.to(torch.int32).to(dev)
        assert ids.numel() == G
        L.call("trid_index_search_distinct_p16", _p(q16), _p(idx.rows_p16), _p(idx.unit_amax), _p(ids), _p(words), Q, G, k, 0, _p(vals), _p(rows),
               _p(ws), workgroups, stream())
    elif allow is not None:
        L.call("trid_index_search_masked_p16", _p(q16), _p(idx.rows_p16), _p(idx.unit_amax), _p(words), Q, G, k, 0, _p(vals), _p(rows), _p(ws),
               workgroups, stream())
    else:
        L.call("trid_index_search_p16", _p(q16), _p(idx.rows_p16), _p(idx.unit_amax), Q, G, k, 0, _p(vals), _p(rows), _p(ws), workgroups, stream())
    return vals.cpu(), rows.cpu()


# ------------------------------------------------------------------------------------------------------------------ the two comparators
def same_bits(got, want, what=""):
    """(values, rows) equal as bit patterns and exactly (topk_deep_ref.same): +0.0 and -0.0 differ"""
    assert TR.same((got[0].cpu().numpy(), got[1].cpu().numpy()), (np.asarray(want[0]), np.asarray(want[1]))), what


def same_values(got, ref, what, pids=None):
    """(values, rows) equal under torch.equal, rows first; pids: the third output of search_pids is the pids of the rows, -1 in the
    short slots"""
    gv, gr = got[0].cpu(), got[1].cpu()
    assert torch.equal(gr, ref[1]), (what, "rows", gr, ref[1])
    assert torch.equal(gv, ref[0]), (what, "values", gv, ref[0])
    if pids is not None:
        want = torch.where(ref[1] >= 0, pids[ref[1].clamp(min=0)], torch.full_like(ref[1], -1))
        assert got[2].dtype == torch.int64 and torch.equal(got[2].cpu(), want), (what, "pids", got[2], want)


# ------------------------------------------------------------------------------------------------------------------ seeded inputs
def fresh_index(gpu, rows, pids=None, n=None, **kw):
    """a new GalleryIndex over the rows, with a neighbour graph of list length n if one is named"""
    from textreid_amd import GalleryIndex

    idx = GalleryIndex()
    assert idx.add(rows.to(gpu), pids=pids, **kw) == 0 and len(idx) == rows.shape[0]
    if n is not None:
        idx.build_neighbours(n)
    return idx


_built, _galleries, _indexes, _products = {}, {}, {}, {}  # keyed by tag and seed as well as shape: see Inputs


class Inputs:
    """The seeded inputs of one test file and what is built from them once.  Every oracle.fill name is the file's tag followed by the
    name the file always used, so every tensor is the one it always was.  raw_tag: the tag of the raw queries and galleries where it
    differs from the tag of the coins; graph_n: the list length of the graph a shared index carries unless the call names one (None:
    no graph).  The caches are keyed by the tags and the seed, so two files share an entry exactly where they name the same inputs.
    A shared index and a cached product are NEVER modified by a test: a test that adds, removes or compacts builds its own with
    fresh_index."""

    def __init__(self, tag, seed, raw_tag=None, graph_n=None):
        self.tag, self.seed, self.raw_tag, self.graph_n = tag, seed, raw_tag or tag, graph_n

    def raw(self, Q, G):
        return OF.randn("%sq%d" % (self.raw_tag, Q), (Q, 256), self.seed), OF.randn("%sg%d" % (self.raw_tag, G), (G, 256), self.seed)

    def coin_keep(self, name, n, keep_of=2):
        """bool [n], true with probability 1 / keep_of (2: about half), drawn from the name"""
        return OF.randint(self.tag + name, 0, keep_of, (n,), self.seed) == 0

    def coin_one_in(self, name, n, one_in=2):
        """bool [n]: with one_in = 2 true where the draw is NOT zero, otherwise true where it is zero (probability 1 / one_in)"""
        draw = OF.randint(self.tag + name, 0, one_in, (n,), self.seed)
        return draw != 0 if one_in == 2 else draw == 0

    def gallery(self, G):
        key = (self.tag, self.seed, G)
        if key not in _galleries:
            _galleries[key] = OF.randn("%sg%d" % (self.tag, G), (G, 256), self.seed)
        return _galleries[key]

    def queries(self, gpu, Q, tag="q"):
        return unit_rows(OF.randn("%s%s%d" % (self.tag, tag, Q), (Q, 256), self.seed).to(gpu))

    def built(self, gpu, Q, G):
        """-> (index over the raw gallery of G rows, the raw queries, the raw gallery, the unit queries, their dense product)"""
        key = (self.tag, self.raw_tag, self.seed, Q, G)
        if key not in _built:
            te, ie = self.raw(Q, G)
            idx = fresh_index(gpu, ie)
            qu = unit_rows(te.to(gpu))
            _built[key] = (idx, te, ie, qu, dense_product(idx, qu))
        return _built[key]

    def shared_index(self, gpu, G, n=None):
        """one index over gallery(G) per (length, list length)"""
        n = self.graph_n if n is None else n
        key = (self.tag, self.seed, G, n)
        if key not in _indexes:
            _indexes[key] = fresh_index(gpu, self.gallery(G), n=n)
        return _indexes[key]

    def product_of(self, idx, key):
        """the [len, len] dense product of an index's rows against themselves (numpy), once per key: it depends on the rows alone"""
        key = (self.tag, self.seed, key)
        if key not in _products:
            _products[key] = dense_product(idx, idx.rows).numpy()
        return _products[key]

    def self_product(self, gpu, G):
        return self.product_of(self.shared_index(gpu, G), G)


# ------------------------------------------------------------------------------------------------------------------ index and shards
def shard_inputs(kind, gen_seed, n_queries, G, pid_range):
    """-> (queries, G gallery rows, pids, normalize): exact-level rows (12 base rows repeated: every product and sum exact, exact ties
    across every cut) or unit random rows, drawn from one torch.Generator in this order"""
    gen = torch.Generator().manual_seed(gen_seed)
    pids = torch.randint(0, pid_range, (G,), generator=gen)
    if kind == "ties":
        lv = torch.tensor([-1.0, -0.5, 0.0, 0.5, 1.0]) / 8
        q = lv[torch.randint(0, 5, (n_queries, 256), generator=gen)]
        base = lv[torch.randint(0, 5, (12, 256), generator=gen)]
        return q, base[torch.randint(0, 12, (G,), generator=gen)], pids, False
    q = torch.nn.functional.normalize(torch.randn(n_queries, 256, generator=gen), dim=1)
    return q, torch.nn.functional.normalize(torch.randn(G, 256, generator=gen), dim=1), pids, True


class ShardPair:
    """ONE GalleryIndex and one GalleryShards for the same rows, both empty here (a subclass adds the rows to both in its own order),
    and what every comparison between them needs"""

    def __init__(self, gpu, inputs, shard_rows):
        from textreid_amd import GalleryIndex, GalleryShards

        q, g, pids, self.normalize = inputs
        self.q, self.g, self.pids = q.to(gpu), g.to(gpu), pids.to(gpu)
        self.one, self.sh, self.shard_rows = GalleryIndex(), GalleryShards(shard_rows=shard_rows), shard_rows

    def to_global(self, rows):
        """rows of the one index -> the shards' global ids; absent slots stay -1"""
        from textreid_amd.index_shards import SHARD_STRIDE

        rows = rows.long()
        return torch.where(rows < 0, rows, (rows // self.shard_rows) * SHARD_STRIDE + rows % self.shard_rows)

    def split(self, mask):
        return [mask[at : at + self.shard_rows] for at in range(0, len(self.one), self.shard_rows)]

    def compare(self, got, want, kk, what):
        """the shards' [Q, k] results against the one index's [Q, kk] (None: nothing it could give): values bit for bit, rows after
        mapping, pids, and (-inf, -1) in every slot from kk on"""
        if want is not None:
            assert torch.equal(got[0][:, :kk].view(torch.int32), want[0].view(torch.int32)), what + ("values",)
            assert torch.equal(got[1][:, :kk], self.to_global(want[1])), what + ("rows",)
            if len(got) == 3:
                assert torch.equal(got[2][:, :kk], want[2]), what + ("pids",)
        assert bool(torch.isneginf(got[0][:, kk:]).all()) and all(bool((t[:, kk:] == -1).all()) for t in got[1:]), what + ("tail",)
