"""GalleryShards: exact search over a gallery that is held as several ``GalleryIndex`` parts - in one process (more rows than the
``MAX_ROWS`` = 2**21 - 1 of one index: the 31-bit byte offsets of the P16 retrieval kernels) or one part per rank of the default
process group.  DESIGN.md section 7l.

It composes plain ``GalleryIndex`` parts and adds ONE step, the merge of the parts' lists (``trid_index_merge_lists_f32``,
csrc/index_merge.hip).  An index normalises and packs every row alone with the fixed unit scale, and its one-pass kernels and
``trid_gemm_p16`` give a (query, row) similarity the same bits whatever the partition or the tile position - so the definition is:

    the results equal those of ONE GalleryIndex holding the parts' rows concatenated in shard order: the values bit for bit, the
    rows after mapping through ``locate`` and the parts' offsets, the pids equal.

Row ids: ``row = shard * SHARD_STRIDE + local`` (int64, ``SHARD_STRIDE`` = 2**21 > MAX_ROWS), stable across ``add`` and ``remove``.
The order rule of the index - value descending, then row ascending - ties by this global row: shard ascending, then local row
ascending, which is the insertion order of the concatenated gallery.  ``locate(rows) -> (shard, local)``; negative rows (the -1 of
a short list) stay negative in both.

``GalleryShards(shard_rows=MAX_ROWS)`` - the in-process form: an ordered list of parts on one device.  ``add`` fills the last part
up to ``shard_rows`` rows and opens the next; one call may span parts, so the global order is the insertion order.  (``shard_rows``
exists so that tests reach many shards with few rows.)
``GalleryShards(collective=True)`` - the by-rank form: ONE part per rank, shard number = rank.  ``add`` and ``remove`` are local to
the rank (no collective; every rank may hold a different number of rows, none included); the four search methods are COLLECTIVE:
every rank calls them with the same queries and k and gets identical results.  The per-rank lists are gathered with
``parallel.all_gather_rows`` (as ``evaluation._merge_shard_lists`` does), then merged on every rank; a rank with an empty part joins
with an all-absent list.  Without a process group it is the one-shard case and joins no collective.

The search methods return the tuples of their ``GalleryIndex`` namesakes: ``search`` / ``search_pids`` (k <= 16) through every part's
one-pass kernel, ``shortlist`` / ``shortlist_pids`` (k <= 1024) through its dense product and deep select - always in panels of at
most 32 queries, never the large-batch streaming route of ``GalleryIndex.search``, whose values agree with the dense product only
to the last bits.  A part is asked for ``min(k, part.live_count)`` when no mask is given (``min(k, len(part))`` with one); a part
with no live row contributes an absent list.  With one shard in the in-process form the part's answer is the answer: no merge.
  * The k rule: k is NOT checked against a total row count (the by-rank form cannot know it without a collective): a query with
    fewer than k allowed rows (or pids) overall ends in ``(-inf, -1[, -1])`` slots, in both forms.
  * ``mask=``: in-process, a sequence with one bool / uint8 tensor (or None) per part; by-rank, this rank's own tensor.  The allow
    set is ``live & mask`` per part, as in the index.
  * Distinct pids: merging the parts' distinct top-k lists is exact - a pid in the global top-k has fewer than k pids ahead of it
    in every shard, so the shard that holds its best row lists it with that row (section 7l).
  * More than ``trid_index_merge_max_candidates()`` = 8192 candidates per query (many shards at deep k) are merged in rounds:
    groups of lists first, then the groups' results - exact for both forms (section 7l).

``remove(rows=global rows | pids=...)``: each part applies what it owns; in the by-rank form every rank may pass the same arguments
and rows of other ranks are skipped.  ``state_dict()`` / ``load_state_dict()``: the parts' own dicts plus ``shard_rows``.

Capture: in the in-process form, after one eager call a search reads nothing on the host and - while the candidates fit one merge
launch - allocates nothing but its outputs: it can be recorded with ``torch.cuda.graph`` and replays against the current contents
of the queries and masks (record again after ``add`` / ``remove``, as for the index).  ONE eager call before a capture is needed in
any case: the first merge on a device raises the dynamic-LDS limit of the kernel.  The by-rank form is NOT capturable: its searches
are collectives.

Not built: ``compact`` (it would renumber rows inside a part), the neighbour graph and the re-ranked search over shards,
rebalancing rows between ranks, shards on several devices of one process.
"""

import torch

from . import ops, parallel
from .index import DIM, MAX_K, MAX_ROWS, MAX_SHORTLIST_K, SMALL_Q, GalleryIndex
from .ops import _p, call, stream

SHARD_BITS = 21
SHARD_STRIDE = 1 << SHARD_BITS  # global row = shard * SHARD_STRIDE + local row; MAX_ROWS = SHARD_STRIDE - 1


def _need_cuda(name, t):
    if not t.is_cuda:
        raise RuntimeError("textreid_amd.index_shards.GalleryShards.%s runs on the HIP kernel library only (CUDA tensors); no CPU fallback" % name)


def max_merge_candidates():
    """candidates per query one launch of trid_index_merge_lists_f32 takes (8192)"""
    return int(ops.L.load().trid_index_merge_max_candidates())


def merge_lists(val, row, k, list_base=None, pid=None):
    """trid_index_merge_lists_f32 on device tensors: val fp32, row int64, pid int64 or None, all [Q, n_lists, k_in]; list_base int64
    [n_lists] or None -> (values [Q, k], global rows [Q, k][, pids [Q, k]]).  One launch: n_lists * k_in <= 8192, k <= n_lists * k_in."""
    for t in (val, row):
        _need_cuda("merge_lists", t)
    if val.dim() != 3 or val.dtype != torch.float32 or row.dtype != torch.int64 or row.shape != val.shape or (
            pid is not None and (pid.dtype != torch.int64 or pid.shape != val.shape)) or (
            list_base is not None and (list_base.dtype != torch.int64 or list_base.numel() != val.shape[1])):
        raise ValueError("GalleryShards.merge_lists: expected val fp32, row / pid int64 [Q, n_lists, k_in] and list_base int64 [n_lists]")
    val, row = val.contiguous(), row.contiguous()
    pid = None if pid is None else pid.contiguous()
    base = None if list_base is None else list_base.contiguous()
    Q, S, kin = val.shape
    out_val = torch.empty(Q, k, dtype=torch.float32, device=val.device)
    out_row = torch.empty(Q, k, dtype=torch.int64, device=val.device)
    out_pid = None if pid is None else torch.empty(Q, k, dtype=torch.int64, device=val.device)
    call("trid_index_merge_lists_f32", _p(val), _p(row), _p(base), _p(pid), Q, S, kin, k, _p(out_val), _p(out_row), _p(out_pid), stream())
    return (out_val, out_row) if pid is None else (out_val, out_row, out_pid)


class GalleryShards:
    """``g = GalleryShards(); g.add(image_embed, pids); vals, rows = g.search(text_embed, k=10); shard, local = g.locate(rows)``.
    See the module docstring for the two forms, the row ids, the k rule and what is out of scope."""

    def __init__(self, shard_rows=MAX_ROWS, collective=False):
        if not isinstance(shard_rows, int) or shard_rows < 1 or shard_rows > MAX_ROWS:
            raise ValueError("GalleryShards: shard_rows must be in [1, %d]; got %r" % (MAX_ROWS, shard_rows))
        self.shard_rows = shard_rows
        self.collective = bool(collective)
        self._parts = [GalleryIndex()]
        self._has_pids = None
        self._ws = {}  # the cached staging buffers of the merge and the shard bases

    # ------------------------------------------------------------------ storage
    @property
    def parts(self):
        """the GalleryIndex parts held by THIS process, in shard order (by-rank form: the one part of this rank)"""
        return tuple(self._parts)

    @property
    def n_shards(self):
        """shards of the whole gallery: the parts (in-process form), the ranks of the default process group (by-rank form)"""
        return parallel.world_size() if self.collective else len(self._parts)

    @property
    def shard(self):
        """the shard number of this process's first part: the rank in the by-rank form, 0 otherwise"""
        return parallel.rank() if self.collective else 0

    def __len__(self):
        """rows held by this process, removed rows included (by-rank form: this rank's rows)"""
        return sum(len(p) for p in self._parts)

    @property
    def live_count(self):
        """rows held by this process and not removed (a host int)"""
        return sum(p.live_count for p in self._parts)

    @staticmethod
    def locate(rows):
        """global rows (an int64 tensor or a list) -> (shard, local), int64 tensors of the same shape; a negative row stays itself in both"""
        r = torch.as_tensor(rows, dtype=torch.int64)
        neg = r < 0
        return torch.where(neg, r, r >> SHARD_BITS), torch.where(neg, r, r & (SHARD_STRIDE - 1))

    def add(self, embeddings, pids=None, normalize=True):
        """Append rows; -> the global row of the first appended row.  In-process form: the last part is filled up to shard_rows, then
        the next is opened (one call may span parts).  By-rank form: local to the rank, at most MAX_ROWS rows in all.  pids,
        normalize: as GalleryIndex.add (normalize=False: one host read per part touched)."""
        if not torch.is_tensor(embeddings) or embeddings.dim() != 2 or embeddings.shape[1] != DIM:
            raise ValueError("GalleryShards.add: expected a [n, %d] tensor" % DIM)
        n = embeddings.shape[0]
        has = pids is not None
        if self._has_pids is not None and has != self._has_pids:
            raise ValueError("GalleryShards.add: pids must be given on every add or on none")
        if has:
            pids = torch.as_tensor(pids).reshape(-1)
            if pids.numel() != n:
                raise ValueError("GalleryShards.add: %d pids for %d rows" % (pids.numel(), n))
        _need_cuda("add", embeddings)
        limit = MAX_ROWS if self.collective else self.shard_rows
        if self.collective and len(self._parts[0]) + n > limit:
            raise ValueError("GalleryShards.add: a rank holds at most %d rows; %d + %d asked" % (limit, len(self._parts[0]), n))
        if len(self._parts[-1]) >= limit and n:
            self._parts.append(GalleryIndex())
        first = (self.shard + len(self._parts) - 1) * SHARD_STRIDE + len(self._parts[-1])
        at = 0
        while at < n:
            part = self._parts[-1]
            take = min(n - at, limit - len(part))
            part.add(embeddings[at : at + take], None if not has else pids[at : at + take], normalize=normalize)
            at += take
            if at < n:
                self._parts.append(GalleryIndex())
        if n:
            self._has_pids = has
        return first

    def remove(self, rows=None, pids=None):
        """Mark rows as removed; -> how many were newly removed in THIS process.  Exactly one of ``rows`` (GLOBAL rows, a list or an
        int64 tensor; duplicates and rows already removed are ignored) and ``pids``.  Each part applies what it owns.  In-process
        form: a row no part holds is a ValueError.  By-rank form: every rank may pass the same arguments; rows of other shards are
        skipped, a row of this shard outside [0, len) is a ValueError."""
        if (rows is None) == (pids is None):
            raise ValueError("GalleryShards.remove: give exactly one of rows and pids")
        if pids is not None:
            if not self._has_pids and not self.collective:
                raise ValueError("GalleryShards.remove(pids=...): the shards hold no pids")
            return sum(p.remove(pids=pids) for p in self._parts if len(p) and p.pids is not None)
        if torch.is_tensor(rows) and rows.dtype != torch.int64:
            raise ValueError("GalleryShards.remove(rows=...): a list or an int64 tensor; got %s" % rows.dtype)
        r = torch.as_tensor(rows, dtype=torch.int64).reshape(-1).cpu()
        if r.numel() == 0:
            return 0
        if int(r.min()) < 0:
            raise ValueError("GalleryShards.remove(rows=...): rows must be >= 0; got %d" % int(r.min()))
        shard, local = self.locate(r)
        shard = shard - self.shard
        if not self.collective and int(shard.max()) >= len(self._parts):
            raise ValueError("GalleryShards.remove(rows=...): row %d lies in shard %d of %d" % (
                int(r[shard.argmax()]), int(shard.max()), len(self._parts)))
        newly = 0
        for s, part in enumerate(self._parts):
            own = local[shard == s]
            if own.numel():
                if int(own.max()) >= len(part):
                    raise ValueError("GalleryShards.remove(rows=...): shard %d holds %d rows; got local row %d" % (s + self.shard, len(part), int(own.max())))
                newly += part.remove(rows=own)
        return newly

    # ------------------------------------------------------------------ search
    def _masks(self, name, mask):
        """-> one mask (or None) per part of this process, checked against the parts"""
        parts = self._parts
        if self.collective:
            masks = [mask]
        elif mask is None:
            masks = [None] * len(parts)
        else:
            if torch.is_tensor(mask) or not isinstance(mask, (list, tuple)) or len(mask) != len(parts):
                raise ValueError("GalleryShards.%s: mask must be a sequence of n_shards = %d tensors (or None), one per part; got %s" % (
                    name, len(parts), "%d" % len(mask) if isinstance(mask, (list, tuple)) else type(mask)))
            masks = list(mask)
        for s, (m, part) in enumerate(zip(masks, parts)):
            if m is None:
                continue
            if not torch.is_tensor(m) or m.dtype not in (torch.bool, torch.uint8):
                raise ValueError("GalleryShards.%s: the mask of shard %d must be a bool or uint8 tensor; got %s" % (
                    name, s + self.shard, m.dtype if torch.is_tensor(m) else type(m)))
            if m.dim() != 1 or m.shape[0] != len(part):
                raise ValueError("GalleryShards.%s: the mask of shard %d must have shape [%d]; got %s" % (name, s + self.shard, len(part), tuple(m.shape)))
        return masks

    def _check(self, name, queries, k, mask, max_k, distinct):
        """the argument rules of the four searches, in the order of the index -> (queries fp32 contiguous, one mask per part)"""
        if not torch.is_tensor(queries) or queries.dim() != 2 or queries.shape[1] != DIM:
            raise ValueError("GalleryShards.%s: expected a [Q, %d] tensor" % (name, DIM))
        if distinct and self._has_pids is False:
            raise ValueError("GalleryShards.%s: the shards hold no pids" % name)
        if not isinstance(k, int) or k < 1 or k > max_k:
            raise ValueError("GalleryShards.%s: k must be in [1, %d]; got %r" % (name, max_k, k))
        masks = self._masks(name, mask)
        if queries.shape[0] == 0:
            raise ValueError("GalleryShards.%s: no queries" % name)
        _need_cuda(name, queries)
        return queries.contiguous().float(), masks

    def _ask(self, part, name, x, k, normalize, mask):
        """one part's answer -> None (no live row: an absent list) or the tuple of its namesake method at k' = min(k, what it holds)"""
        if len(part) == 0 or part.live_count == 0:
            return None
        kk = min(k, len(part) if mask is not None else part.live_count)
        if name != "search" or x.shape[0] <= SMALL_Q:
            return getattr(part, name)(x, k=kk, normalize=normalize, mask=mask)
        # search with more than 32 queries: panels through the one-pass kernel, never the streaming route of GalleryIndex.search
        outs = [part.search(x[at : at + SMALL_Q], k=kk, normalize=normalize, mask=mask) for at in range(0, x.shape[0], SMALL_Q)]
        return torch.cat([o[0] for o in outs]), torch.cat([o[1] for o in outs])

    def _staging(self, Q, S, kin, distinct, device):
        """the cached [Q, S, kin] candidate buffers of the merge (values, local rows, pids) and the shard bases"""
        key = (Q, S, kin, distinct)
        buf = self._ws.get(key)
        if buf is None or buf[0].device != device:  # (kept per shape and never dropped: a recorded search writes into them at every replay)
            buf = (torch.empty(Q, S, kin, dtype=torch.float32, device=device), torch.full((Q, S, kin), -1, dtype=torch.int64, device=device),
                   torch.zeros(Q, S, kin, dtype=torch.int64, device=device) if distinct else None)
            self._ws[key] = buf
        base = self._ws.get("base")
        if base is None or base.numel() < S or base.device != device:
            base = torch.arange(max(S, 8), dtype=torch.int64, device=device) * SHARD_STRIDE
            self._ws["base"] = base
        return buf, base[:S]

    def _merge(self, val, row, pid, base, k):
        """[Q, S, kin] candidates -> the first k in the order, padded to k: one launch, or rounds (groups of lists, then the groups'
        results) when S * kin exceeds what one launch takes"""
        Q, S, kin = val.shape
        cap = max_merge_candidates()
        if S * kin <= cap:
            kk = min(k, S * kin)
            out = merge_lists(val, row, kk, base, pid)
            if kk == k:
                return out
            fills = (float("-inf"), -1, -1)
            return tuple(torch.cat([o, torch.full((Q, k - kk), f, dtype=o.dtype, device=o.device)], dim=1) for o, f in zip(out, fills))
        g = cap // kin
        k2 = min(k, g * kin)
        outs = [self._merge(val[:, at : at + g].contiguous(), row[:, at : at + g].contiguous(), None if pid is None else pid[:, at : at + g].contiguous(),
                            None if base is None else base[at : at + g], k2) for at in range(0, S, g)]
        nxt = [torch.stack([o[i] for o in outs], dim=1) for i in range(len(outs[0]))]  # (global rows now: no bases)
        return self._merge(nxt[0], nxt[1], nxt[2] if pid is not None else None, None, k)

    def _search(self, name, queries, k, normalize, mask, max_k, distinct):
        x, masks = self._check(name, queries, k, mask, max_k, distinct)
        Q, dev = x.shape[0], x.device
        lists = [self._ask(part, name, x, k, normalize, m) for part, m in zip(self._parts, masks)]
        W = parallel.world_size() if self.collective else 1
        if not self.collective and len(lists) == 1 or self.collective and W == 1:
            # one shard: the part's answer is the answer (global row = local row + this shard's base), padded to k
            got, off = lists[0], self.shard * SHARD_STRIDE
            fills = (float("-inf"), -1, -1)[: 3 if distinct else 2]
            dts = (torch.float32, torch.int64, torch.int64)
            if got is None:
                return tuple(torch.full((Q, k), f, dtype=d, device=dev) for f, d in zip(fills, dts))
            if off:
                got = (got[0], torch.where(got[1] < 0, got[1], got[1] + off)) + tuple(got[2:])
            if got[0].shape[1] == k:
                return tuple(got)
            return tuple(torch.cat([o, torch.full((Q, k - o.shape[1]), f, dtype=o.dtype, device=dev)], dim=1) for o, f in zip(got, fills))
        if self.collective:
            # this rank's list padded to k with absent slots, gathered rank-major, [W * Q, k] -> [Q, W, k]
            mine = [torch.full((Q, k), f, dtype=d, device=dev) for f, d in zip((float("-inf"), -1, -1), (torch.float32, torch.int64, torch.int64))]
            if lists[0] is not None:
                for dst, src in zip(mine, lists[0]):
                    dst[:, : src.shape[1]].copy_(src)
            cand = [parallel.all_gather_rows(t).view(W, Q, k).permute(1, 0, 2).contiguous() for t in mine[: 3 if distinct else 2]]
            base = torch.arange(W, dtype=torch.int64, device=dev) * SHARD_STRIDE
            return self._merge(cand[0], cand[1], cand[2] if distinct else None, base, k)
        S = len(lists)
        widest = max([0] + [got[0].shape[1] for got in lists if got is not None])
        kin = max(widest, -(-k // S))  # (S * kin >= k: the merge's own k rule)
        (val, row, pid), base = self._staging(Q, S, kin, distinct, dev)
        for s, got in enumerate(lists):
            kk = 0 if got is None else got[0].shape[1]
            if kk:
                val[:, s, :kk].copy_(got[0])
                row[:, s, :kk].copy_(got[1])
                if distinct:
                    pid[:, s, :kk].copy_(got[2])
            if kk < kin:
                row[:, s, kk:].fill_(-1)
        return self._merge(val, row, pid, base, k)

    def search(self, queries, k=10, normalize=True, mask=None):
        """-> (values [Q,k] f32, rows [Q,k] i64 GLOBAL): GalleryIndex.search over the shards, k <= 16; every part through its one-pass
        kernel in panels of at most 32 queries.  By-rank form: collective."""
        return self._search("search", queries, k, normalize, mask, MAX_K, False)

    def search_pids(self, queries, k=10, normalize=True, mask=None):
        """-> (values, rows GLOBAL, pids), each [Q,k]: GalleryIndex.search_pids over the shards, k <= 16.  By-rank form: collective."""
        return self._search("search_pids", queries, k, normalize, mask, MAX_K, True)

    def shortlist(self, queries, k=100, normalize=True, mask=None):
        """-> (values [Q,k] f32, rows [Q,k] i64 GLOBAL): GalleryIndex.shortlist over the shards, k <= 1024.  By-rank form: collective."""
        return self._search("shortlist", queries, k, normalize, mask, MAX_SHORTLIST_K, False)

    def shortlist_pids(self, queries, k=100, normalize=True, mask=None):
        """-> (values, rows GLOBAL, pids), each [Q,k]: GalleryIndex.shortlist_pids over the shards, k <= 1024.  By-rank form: collective."""
        return self._search("shortlist_pids", queries, k, normalize, mask, MAX_SHORTLIST_K, True)

    # ------------------------------------------------------------------ persistence
    def state_dict(self):
        """{"shard_rows", "collective", "parts": the parts' own state dicts in shard order} (by-rank form: this rank's one part)"""
        return {"shard_rows": self.shard_rows, "collective": self.collective, "parts": [p.state_dict() for p in self._parts]}

    def load_state_dict(self, sd):
        """Replace the contents with the parts of ``sd`` (each loaded by GalleryIndex.load_state_dict; the row ids are those of the
        saved shards).  shard_rows is taken from the dict; the form (collective or not) stays that of this object, and the by-rank
        form takes exactly one part."""
        parts = list(sd["parts"])
        shard_rows = int(sd["shard_rows"])
        if shard_rows < 1 or shard_rows > MAX_ROWS:
            raise ValueError("GalleryShards.load_state_dict: shard_rows must be in [1, %d]; got %d" % (MAX_ROWS, shard_rows))
        if self.collective and len(parts) != 1:
            raise ValueError("GalleryShards.load_state_dict: the by-rank form holds one part per rank; got %d" % len(parts))
        if not parts:
            parts = [GalleryIndex().state_dict()]
        loaded = []
        for one in parts:
            part = GalleryIndex()
            part.load_state_dict(one)
            loaded.append(part)
        self.shard_rows, self._parts, self._ws = shard_rows, loaded, {}
        held = [p._has_pids for p in loaded if len(p)]
        self._has_pids = held[0] if held else None
