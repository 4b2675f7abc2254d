"""GalleryShards: exact search over a gallery that is held as several ``GalleryIndex`` parts - in one process (more rows than the
``MAX_ROWS`` = 2**21 - 1 of one index: the 31-bit byte offsets of the P16 retrieval kernels) or one part per rank of the default
process group.  DESIGN.md sections 7l (the searches) and 7m (the neighbour graph and the re-ranked search).

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
and rows of other ranks are skipped.  ``state_dict()`` / ``load_state_dict()``: the parts' own dicts plus ``shard_rows``, and the
lists and values of a CURRENT neighbour graph (a dict written before the graph existed loads with no graph).

The neighbour graph and the re-ranked search (section 7m).  A part's own ``GalleryIndex.build_neighbours`` keeps its local meaning and
is not used here: a row's n nearest rows may lie in another part, and the k-reciprocal bonus compares lists of row ids that must mean
the same thing everywhere.  The graph over ALL shards lives on this object: per part int32 ``[capacity_s, n]`` lists of GLOBAL row
ids (they fit int32 up to ``MAX_GRAPH_SHARDS`` = 1023 shards; more is a ValueError of ``build_neighbours``) and their fp32 values;
``neighbours`` / ``neighbour_values`` (one ``[len_s, n]`` tensor per part), ``neighbours_current`` (false after any ``add`` / ``remove``,
told by the parts' row and removal counts), ``neighbours_refreshable``.  The definition is the same sentence: ONE GalleryIndex over the
concatenated rows has these lists (ids after the mapping), these values bit for bit, and these re-ranked results.
  * ``build_neighbours(n=5)``: for every panel of 32 consecutive rows of a part (in place in its P16 storage; a ragged panel through a
    cached zero-padded one) one one-pass search per part at ``k = min(n, live rows of that part)`` (the masked form once it has
    removed rows), the candidates staged ``[32, n_shards, n]``, ONE merge launch with the parts' bases, narrowed to int32.  No host
    read.  By rank: collective - in round i every rank contributes the panel of its rows ``[32 i, 32 i + 32)``, searches its part with
    every rank's panel, the lists are gathered, and a rank merges and keeps the lists of its own rows.
  * ``search_reranked`` / ``search_reranked_pids`` (signatures and tuples of the index), per panel of 32 queries.  Phase 1 in every
    part: the dense product into the part's cached score buffer and a deep select with k = n over the allowed rows; the parts' lists
    merged into the query's own GLOBAL list.  Phase 2 in every part: ``trid_index_rerank_add_f32`` in place with that list and the
    part's global-id lists, then the final deep select (or the two distinct-pid steps); the lists merged as ``shortlist`` /
    ``shortlist_pids`` merge theirs.  Both run the private steps of ``GalleryIndex._reranked``.  ``alpha == 0.0`` is ``shortlist`` /
    ``shortlist_pids``.  A part with fewer rows than n (a freshly opened last part) is walked as n rows whose extra rows are masked
    off: the bonus kernel's and the select's ``n <= G`` rule stays as it is, the allow words are zero behind ``len`` and the stored
    lists there are -1 (an index's buffers always hold at least 64 rows, so nothing has to grow).  In-process, after one eager call
    a search allocates nothing but its outputs, the queries' lists and the parts' select outputs: it can be recorded.  By rank: a
    gather and a merge after each phase; not capturable.
  * ``refresh_neighbours()`` -> ``(new_rows, redone_rows)``, in-process only (by rank: RuntimeError naming ``build_neighbours``): per
    part and per group of at most 32 new rows one ``trid_gemm_p16`` product (tile kernel, the group as A, the part's old rows as B)
    and one ``trid_index_nn_merge_sharded_f32`` (csrc/index_nn_update.hip, the kernel of the index's merge with the sharded policy: liveness by global id, order by value then global id -
    the new rows of a middle part are numbered BELOW the stored rows of later parts); removals only: one launch per part with
    m = 0; the new rows' lists from the build's panel step; the flags of all parts read once on the host, flagged rows gathered
    32 at a time, recomputed by the panel step and scattered back.  Lists and values equal a fresh build bit for bit.

Query expansion: ``expand_queries`` / ``search_expanded`` / ``search_expanded_pids`` with the signatures of the
index and global row ids, in-process form only.  Phase 1 is the sharded ``shortlist`` with k = m; the blend is ONE launch of
``trid_index_blend_rows_f32`` over the parts' fp32 row storages, through a device table of their addresses and lengths and
``shift = 21`` (a global row decodes to its part and local row); ``trid_l2norm_rows_f32``; phase 2 is the sharded ``shortlist`` /
``shortlist_pids`` with the same masks.  Equal to one index over the concatenated rows bit for bit.  By rank (``collective=True``) they
raise a RuntimeError: the blend gathers rows by address and the rows of another rank are not addressable.  ``augmented()`` over
shards is not built.

Capture: in the in-process form, after one eager call a search reads nothing on the host and - while the candidates fit one merge
launch - allocates nothing but its outputs: it can be recorded with ``torch.cuda.graph`` and replays against the current contents
of the queries and masks (record again after ``add`` / ``remove``, as for the index).  ONE eager call before a capture is needed in
any case: the first merge on a device raises the dynamic-LDS limit of the kernel.  The by-rank form is NOT capturable: its searches
are collectives.

Not built: ``compact`` (it would renumber rows inside a part), the by-rank ``refresh_neighbours`` (the merge kernel's order rule is
general, so it can be added), rebalancing rows between ranks, shards on several devices of one process.
"""

from functools import partial

import torch

from . import index, ops, parallel
from .index import DIM, MAX_EXPAND, MAX_EXPAND_POWER, MAX_K, MAX_NEIGHBOURS, MAX_ROWS, MAX_SHORTLIST_K, SMALL_Q, GalleryIndex, _blank_dead, _fill_panel, _graph_pair
from .ops import _p, call, stream

SHARD_BITS = 21
SHARD_STRIDE = 1 << SHARD_BITS  # global row = shard * SHARD_STRIDE + local row; MAX_ROWS = SHARD_STRIDE - 1
MAX_GRAPH_SHARDS = 1023  # the neighbour graph holds global rows as int32: shard * SHARD_STRIDE + local < 2**31


_need_cuda = partial(index._need_cuda, owner="index_shards.GalleryShards")
_ABSENT = ((float("-inf"), torch.float32), (-1, torch.int64), (-1, torch.int64))  # what a slot without a result holds: value, row, pid


def _pad_lists(lists, n_out, Q, k, device):
    """a tuple of [Q, k'] tensors (values, rows[, pids]; k' <= k), or None for no list at all -> ``n_out`` tensors [Q, k] that end in
    absent slots (-inf, -1[, -1])"""
    if lists is None:
        return tuple(torch.full((Q, k), f, dtype=d, device=device) for f, d in _ABSENT[:n_out])
    if lists[0].shape[1] == k:
        return tuple(lists[:n_out])
    return tuple(torch.cat([o, torch.full((Q, k - o.shape[1]), f, dtype=d, device=device)], dim=1) for o, (f, d) in zip(lists[:n_out], _ABSENT))


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
        self._g_nn = None   # the neighbour graph over the shards: per part int32 [>= capacity_s, n] of GLOBAL rows (build_neighbours)
        self._g_val = None  # per part fp32 [>= capacity_s, n]: the similarity of every entry (refresh_neighbours merges by them)
        self._g_sig = None  # (len, removed rows) of every part when the graph was last current

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

    def _check(self, name, queries, k, mask, max_k, distinct, need_graph=False):
        """the argument rules of the searches, in the order of the index -> (queries fp32 contiguous, one mask per part).  need_graph:
        a current neighbour graph, asked for after the argument rules and before the device's"""
        if not torch.is_tensor(queries) or queries.dim() != 2 or queries.shape[1] != DIM:
            raise ValueError("GalleryShards.%s: expected a [Q, %d] tensor" % (name, DIM))
        if distinct and self._has_pids is False:
            raise ValueError("GalleryShards.%s: the shards hold no pids" % name)
        if not isinstance(k, int) or k < 1 or k > max_k:
            raise ValueError("GalleryShards.%s: k must be in [1, %d]; got %r" % (name, max_k, k))
        masks = self._masks(name, mask)
        if queries.shape[0] == 0:
            raise ValueError("GalleryShards.%s: no queries" % name)
        if need_graph and not self.neighbours_current:
            raise RuntimeError("GalleryShards.%s: the neighbour graph is %s; call build_neighbours() first" % (
                name, "absent" if self._g_nn is None else "stale (add / remove since it was built)"))
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

    @staticmethod
    def _stage(bufs, s, got, Q=None):
        """one part's lists ``got`` - (values, rows[, pids]) of [Q, kk] each, or None: no list - into list s of the staging buffers
        ``bufs`` (their first Q rows; default: all); the slots behind kk are marked absent (row -1)"""
        kk = 0 if got is None else got[0].shape[1]
        for dst, src in zip(bufs, got or ()):
            if dst is not None:
                dst[:Q, s, :kk].copy_(src)
        if kk < bufs[1].shape[2]:
            bufs[1][:Q, s, kk:].fill_(-1)

    def _merge(self, val, row, pid, base, k):
        """[Q, S, kin] candidates -> the first k in the order, padded to k: one launch, or rounds (groups of lists, then the groups'
        results) when S * kin exceeds what one launch takes"""
        Q, S, kin = val.shape
        cap = max_merge_candidates()
        if S * kin <= cap:
            out = merge_lists(val, row, min(k, S * kin), base, pid)
            return _pad_lists(out, len(out), Q, k, val.device)
        g = cap // kin
        k2 = min(k, g * kin)
        outs = [self._merge(val[:, at : at + g].contiguous(), row[:, at : at + g].contiguous(), None if pid is None else pid[:, at : at + g].contiguous(),
                            None if base is None else base[at : at + g], k2) for at in range(0, S, g)]
        nxt = [torch.stack([o[i] for o in outs], dim=1) for i in range(len(outs[0]))]  # (global rows now: no bases)
        return self._merge(nxt[0], nxt[1], nxt[2] if pid is not None else None, None, k)

    def _search(self, name, queries, k, normalize, mask, max_k, distinct):
        x, masks = self._check(name, queries, k, mask, max_k, distinct)
        Q, dev, n_out = x.shape[0], x.device, 3 if distinct else 2
        lists = [self._ask(part, name, x, k, normalize, m) for part, m in zip(self._parts, masks)]
        W = parallel.world_size() if self.collective else 1
        if not self.collective and len(lists) == 1 or self.collective and W == 1:
            # one shard: the part's answer is the answer (global row = local row + this shard's base), padded to k
            got, off = lists[0], self.shard * SHARD_STRIDE
            if got is not None and off:
                got = (got[0], torch.where(got[1] < 0, got[1], got[1] + off)) + tuple(got[2:])
            return _pad_lists(got, n_out, Q, k, dev)
        if self.collective:
            # this rank's list padded to k with absent slots, gathered rank-major, [W * Q, k] -> [Q, W, k]
            cand = [parallel.all_gather_rows(t).view(W, Q, k).permute(1, 0, 2).contiguous() for t in _pad_lists(lists[0], n_out, Q, k, dev)]
            base = torch.arange(W, dtype=torch.int64, device=dev) * SHARD_STRIDE
            return self._merge(cand[0], cand[1], cand[2] if distinct else None, base, k)
        S = len(lists)
        widest = max([0] + [got[0].shape[1] for got in lists if got is not None])
        kin = max(widest, -(-k // S))  # (S * kin >= k: the merge's own k rule)
        (val, row, pid), base = self._staging(Q, S, kin, distinct, dev)
        for s, got in enumerate(lists):
            self._stage((val, row, pid), s, got)
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

    # ------------------------------------------------------------------ query expansion
    def _blend_tables(self, dev):
        """-> (part addresses int64 [S], part lengths int64 [S]) on the device: the parts' fp32 row storages as the address table of
        trid_index_blend_rows_f32 (shift = SHARD_BITS: a global row decodes to its part and local row).  Cached; rebuilt - one small
        upload, outside any capture - when a part's storage or length changed.  A part without storage has length 0."""
        key = tuple((0, 0) if p.rows is None else (p.rows.data_ptr(), len(p)) for p in self._parts)
        if self._ws.get("blend_key") != key:
            self._ws["blend_tab"] = torch.tensor([[a for a, _ in key], [n for _, n in key]], dtype=torch.int64, device=dev)
            self._ws["blend_key"] = key
        tab = self._ws["blend_tab"]
        return tab[0], tab[1]

    def _expanded(self, name, queries, k, m, power, normalize, mask, distinct=False):
        """expand_queries (k None) and the expanded searches, in-process form: phase 1 the sharded shortlist with k = m (global rows),
        ONE blend launch over the parts' row storages with the unit queries as base, trid_l2norm_rows_f32, phase 2 the sharded
        shortlist / shortlist_pids with the same masks"""
        if self.collective:
            raise RuntimeError("GalleryShards.%s: query expansion is not built for the by-rank form (collective=True): the blend gathers "
                               "stored rows by address and the rows of another rank are not addressable" % name)
        if not isinstance(m, int) or m < 1 or m > MAX_EXPAND:
            raise ValueError("GalleryShards.%s: m must be in [1, %d]; got %r" % (name, MAX_EXPAND, m))
        if not isinstance(power, int) or power < 0 or power > MAX_EXPAND_POWER:
            raise ValueError("GalleryShards.%s: power must be an integer in [0, %d]; got %r" % (name, MAX_EXPAND_POWER, power))
        x, _ = self._check(name, queries, 1 if k is None else k, mask, MAX_SHORTLIST_K, distinct)
        if len(self) == 0:
            raise ValueError("GalleryShards.%s: the shards are empty" % name)
        Q = x.shape[0]
        unit = ops.l2norm_rows(x)[0] if normalize else (x if x.data_ptr() % 16 == 0 else x.clone())
        qv, qr = self._search("shortlist", unit, m, False, mask, MAX_SHORTLIST_K, False)
        tab, lens = self._blend_tables(x.device)
        blend = torch.empty(Q, DIM, dtype=torch.float32, device=x.device)
        call("trid_index_blend_rows_f32", _p(tab), _p(lens), len(self._parts), SHARD_BITS, _p(qr), 8, _p(qv), m, Q, m, power, _p(unit), DIM,
             _p(blend), stream())
        new = ops.l2norm_rows(blend)[0]
        if k is None:
            return new
        return self._search("shortlist_pids" if distinct else "shortlist", new, k, False, mask, MAX_SHORTLIST_K, distinct)

    def expand_queries(self, queries, m=5, power=1, normalize=True, mask=None):
        """-> unit fp32 [Q, 256]: GalleryIndex.expand_queries over the shards - every query replaced by the normalised weighted sum of
        itself and its m best allowed rows of the WHOLE gallery (1 <= m <= 32, 0 <= power <= 4), bit for bit what one index over the
        concatenated rows gives.  Like k, m is not checked against a row count: a query with fewer than m allowed rows blends what
        it has.  In-process form only (by rank: RuntimeError)."""
        return self._expanded("expand_queries", queries, None, m, power, normalize, mask)

    def search_expanded(self, queries, k=10, m=5, power=1, normalize=True, mask=None):
        """-> (values [Q,k] f32, rows [Q,k] i64 GLOBAL): GalleryIndex.search_expanded over the shards = shortlist(expand_queries(...), k,
        normalize=False, mask=mask).  In-process form only (by rank: RuntimeError)."""
        return self._expanded("search_expanded", queries, k, m, power, normalize, mask)

    def search_expanded_pids(self, queries, k=10, m=5, power=1, normalize=True, mask=None):
        """-> (values, rows GLOBAL, pids), each [Q,k]: GalleryIndex.search_expanded_pids over the shards.  In-process form only."""
        return self._expanded("search_expanded_pids", queries, k, m, power, normalize, mask, distinct=True)

    # ------------------------------------------------------------------ neighbour graph over the shards
    def _sig(self):
        """(len, removed rows) of every part: what a graph is current FOR (add and remove change it, wherever they were called)"""
        return [(len(p), len(p) - p.live_count) for p in self._parts]

    @property
    def neighbours(self):
        """one int32 [len_s, n] tensor per part of this process: the neighbour lists as GLOBAL row ids, as build_neighbours /
        refresh_neighbours (or load_state_dict) left them, -1 in every slot of a row that was removed then or appended since (views of
        the storage: read-only); None when no graph is held"""
        if self._g_nn is None:
            return None
        self._grow_graph()
        return tuple(t[: len(p)] for t, p in zip(self._g_nn, self._parts))

    @property
    def neighbour_values(self):
        """one fp32 [len_s, n] tensor per part: the similarity of every entry of ``neighbours`` (-inf in the slots that hold -1); None
        when no values are held (no graph, or lists loaded without them)"""
        if self._g_nn is None or self._g_val is None:
            return None
        self._grow_graph()
        return tuple(t[: len(p)] for t, p in zip(self._g_val, self._parts))

    @property
    def neighbours_current(self):
        """the lists describe the shards as they stand (no add / remove since): search_reranked takes them"""
        return self._g_nn is not None and self._g_sig == self._sig()

    @property
    def neighbours_refreshable(self):
        """lists and their values are both held: the in-process form's refresh_neighbours can bring the graph up to date"""
        return self._g_nn is not None and self._g_val is not None

    def _grow_graph(self):
        """the graph storage follows the parts: one pair of [>= capacity_s, n] buffers per part, (-1, -inf) in every row no build or
        refresh has written (parts opened and rows appended since)"""
        n = self._g_nn[0].shape[1]
        dev = next((p.device for p in self._parts if p.device is not None), self._g_nn[0].device)
        for s, part in enumerate(self._parts):
            want = max(part.capacity, MAX_NEIGHBOURS)
            if s == len(self._g_nn):  # (a part opened since)
                nn, val = _graph_pair(want, n, dev, values=self._g_val is not None)
                self._g_nn.append(nn)
                if val is not None:
                    self._g_val.append(val)
            elif self._g_nn[s].shape[0] < want:
                old = (self._g_nn[s], None if self._g_val is None else self._g_val[s])
                nn, val = _graph_pair(want, n, dev, old=old, rows=old[0].shape[0])
                self._g_nn[s] = nn
                if val is not None:
                    self._g_val[s] = val

    def _fill_panel(self, src, Q, dev):
        """Q < 32 P16 rows into the shards' own cached zero-padded [32, 256] panel (a part's cached panel carries that part's state)"""
        q16 = self._ws.get("panel")
        if q16 is None or q16.device != dev:
            q16 = torch.zeros(SMALL_Q, DIM, dtype=torch.float32, device=dev)
            self._ws["panel"], self._ws["panel_rows"] = q16, 0
        self._ws["panel_rows"] = _fill_panel(q16, src, Q, self._ws["panel_rows"])
        return q16

    def _panel_tmp(self, n, dev):
        """the cached contiguous outputs of one one-pass search at k <= n: fp32 and int64, 32 * n elements each"""
        tmp = self._ws.get(("tmp", n))
        if tmp is None or tmp[0].device != dev:
            tmp = (torch.empty(SMALL_Q * n, dtype=torch.float32, device=dev), torch.empty(SMALL_Q * n, dtype=torch.int64, device=dev))
            self._ws[("tmp", n)] = tmp
        return tmp

    @staticmethod
    def _one_pass(part, panel, Q, kk, vals, rows):
        """one one-pass search of ``part`` with the Q rows of ``panel`` as the queries, k = kk <= part.live_count -> vals / rows [Q, kk]
        (local rows): the masked form once the part has removed rows"""
        _, lists, words = part._neighbour_workspace(kk)
        part._one_pass(panel, Q, kk, vals, rows, lists, words)

    def _graph_panel(self, panel, Q, n):
        """the panel step of the build: the Q <= 32 P16 rows of ``panel`` as the queries of one one-pass search per part at k = min(n,
        live rows of the part), the candidates staged as [Q, n_shards, n] and merged in one launch with the parts' bases -> (values
        fp32 [Q, n], GLOBAL rows int64 [Q, n]).  No host read."""
        parts = self._parts
        dev = panel.device
        (val, row, _), base = self._staging(SMALL_Q, len(parts), n, False, dev)
        tv, tr = self._panel_tmp(n, dev)
        for t, other in enumerate(parts):
            kk = min(n, other.live_count) if len(other) else 0
            got = None
            if kk:
                got = tv[: Q * kk].view(Q, kk), tr[: Q * kk].view(Q, kk)
                self._one_pass(other, panel, Q, kk, *got)
            self._stage((val, row), t, got, Q)
        return merge_lists(val[:Q], row[:Q], n, base)

    def _graph_rows(self, s, first, last, n):
        """the lists of the rows [first, last) of part s from scratch, into the graph storage: panels of 32 consecutive rows - in place
        in the P16 storage, a ragged one through the cached zero-padded panel - through the panel step; (-1, -inf) for removed rows"""
        part = self._parts[s]
        nn, val = self._g_nn[s], self._g_val[s]
        for at in range(first, last, SMALL_Q):
            Q = min(SMALL_Q, last - at)
            panel = part.rows_p16[at : at + SMALL_Q] if Q == SMALL_Q else self._fill_panel(part.rows_p16[at : at + Q], Q, part.device)
            v, r = self._graph_panel(panel, Q, n)
            nn[at : at + Q].copy_(r)  # (narrowed: global ids of at most 1023 shards fit int32)
            val[at : at + Q].copy_(v)
        if part.live_count < len(part):
            _blank_dead(nn[first:last], val[first:last], part.live[first:last])

    def _check_build(self, name, n):
        if not isinstance(n, int) or n < 1 or n > MAX_NEIGHBOURS:
            raise ValueError("GalleryShards.%s: n must be in [1, %d]; got %r" % (name, MAX_NEIGHBOURS, n))
        if self.n_shards > MAX_GRAPH_SHARDS:
            raise ValueError("GalleryShards.%s: the lists hold global rows as int32, which reach %d shards; the gallery has %d" % (
                name, MAX_GRAPH_SHARDS, self.n_shards))

    def build_neighbours(self, n=5):
        """Build the neighbour graph over ALL shards: for every live row, the n best live rows of the whole gallery for the row's own
        embedding as the query, as GLOBAL row ids (value descending, then global row ascending), with their values; (-1, -inf) in every
        slot of a removed row.  Equal to GalleryIndex.build_neighbours of the concatenated gallery, values bit for bit, ids after the
        mapping.  1 <= n <= 8, n <= the live rows of all shards, at most 1023 shards.  Per panel of 32 rows one
        one-pass search per part and one merge launch; quadratic in the rows, no host read.  By-rank form: COLLECTIVE - every rank's
        panels go to every rank (parallel.all_gather_rows), every rank searches its part, the lists are gathered and merged, every
        rank keeps the lists of its own rows (the row counts are gathered and read once)."""
        self._check_build("build_neighbours", n)
        if self.collective and parallel.world_size() > 1:
            return self._build_by_rank(n)
        if len(self) == 0:
            raise ValueError("GalleryShards.build_neighbours: the shards are empty")
        if n > self.live_count:
            raise ValueError("GalleryShards.build_neighbours: n must be <= live_count = %d; got %d" % (self.live_count, n))
        dev = next(p.device for p in self._parts if len(p))
        self._g_nn, self._g_val = map(list, zip(*[_graph_pair(max(p.capacity, MAX_NEIGHBOURS), n, dev) for p in self._parts]))
        self._g_sig = None
        for s, part in enumerate(self._parts):
            if len(part):
                self._graph_rows(s, 0, len(part), n)
        self._g_sig = self._sig()

    def _build_by_rank(self, n):
        """the collective build: in round i every rank contributes the panel of its rows [32 i, 32 i + 32) (zeros once it has none),
        searches its part with every rank's panel, and the [W, 32, n] lists are gathered; a rank merges the W lists of its own panel"""
        W, r = parallel.world_size(), parallel.rank()
        part = self._parts[0]
        dev = part.device if part.device is not None else torch.device("cuda", torch.cuda.current_device())
        counts = parallel.all_gather_rows(torch.tensor([[len(part), part.live_count]], dtype=torch.int64, device=dev)).cpu()
        if int(counts[:, 0].sum()) == 0:
            raise ValueError("GalleryShards.build_neighbours: the shards are empty")
        if n > int(counts[:, 1].sum()):
            raise ValueError("GalleryShards.build_neighbours: n must be <= live_count = %d; got %d" % (int(counts[:, 1].sum()), n))
        G = len(part)
        kk = min(n, part.live_count) if G else 0
        nn, val = _graph_pair(max(part.capacity, MAX_NEIGHBOURS), n, dev)
        zero = torch.zeros(SMALL_Q, DIM, dtype=torch.float32, device=dev)
        cv = torch.empty(W * SMALL_Q, n, dtype=torch.float32, device=dev)
        cr = torch.empty(W * SMALL_Q, n, dtype=torch.int64, device=dev)
        tv, tr = self._panel_tmp(n, dev)
        base = torch.arange(W, dtype=torch.int64, device=dev) * SHARD_STRIDE
        for at in range(0, int(counts[:, 0].max()), SMALL_Q):
            Q = max(0, min(SMALL_Q, G - at))
            mine = zero if Q == 0 else part.rows_p16[at : at + SMALL_Q] if Q == SMALL_Q else self._fill_panel(part.rows_p16[at : at + Q], Q, dev)
            panels = parallel.all_gather_rows(mine.view(torch.int32)).view(torch.float32)  # [W * 32, 256]: bit copies of P16 rows
            cr.fill_(-1)
            for w in range(W):
                Qw = max(0, min(SMALL_Q, int(counts[w, 0]) - at))
                if Qw and kk:
                    ov, orow = tv[: Qw * kk].view(Qw, kk), tr[: Qw * kk].view(Qw, kk)
                    self._one_pass(part, panels[w * SMALL_Q : (w + 1) * SMALL_Q], Qw, kk, ov, orow)
                    cv[w * SMALL_Q : w * SMALL_Q + Qw, :kk].copy_(ov)
                    cr[w * SMALL_Q : w * SMALL_Q + Qw, :kk].copy_(orow)
            # [source rank, panel owner, 32, n] -> this rank's panel: [32, source rank, n]
            gv = parallel.all_gather_rows(cv).view(W, W, SMALL_Q, n)[:, r].permute(1, 0, 2).contiguous()
            gr = parallel.all_gather_rows(cr).view(W, W, SMALL_Q, n)[:, r].permute(1, 0, 2).contiguous()
            if Q:
                v, rows = merge_lists(gv[:Q], gr[:Q], n, base)
                nn[at : at + Q].copy_(rows)
                val[at : at + Q].copy_(v)
        if G and part.live_count < G:
            _blank_dead(nn[:G], val[:G], part.live)
        self._g_nn, self._g_val, self._g_sig = [nn], [val], self._sig()

    def refresh_neighbours(self):
        """Bring a stale graph up to date EXACTLY -> (new_rows, redone_rows): the live rows appended since the graph was last current,
        and the older rows whose lists were recomputed because they held a row removed since.  Lists and values afterwards equal those
        of a fresh build_neighbours(n) bit for bit.  In-process form only: the by-rank form raises a
        RuntimeError (call build_neighbours again).  Needs ``neighbours_refreshable`` (RuntimeError naming build_neighbours) and
        n <= live_count (the ValueError of build_neighbours); a current graph returns (0, 0) without a launch.  With the rows covered
        so far as "old":
          * per part s and per group of at most 32 new rows: the trid_gemm_p16 product (tile kernel) of the group's P16 rows as A with
            part s's old P16 rows as B - the direction of the definition, old row as the query - into part s's cached score buffer,
            then ONE trid_index_nn_merge_sharded_f32 launch; removals only: one launch per part with m = 0;
          * the lists of the new rows from the build's panel step over their range;
          * the flags of all parts are read once on the host; flagged rows are gathered 32 at a time into the cached panel, put
            through the build's panel step and scattered back."""
        if self.collective:
            raise RuntimeError("GalleryShards.refresh_neighbours: the by-rank form has no refresh; call build_neighbours() again")
        if not self.neighbours_refreshable:
            raise RuntimeError("GalleryShards.refresh_neighbours: %s; call build_neighbours() first" % (
                "there is no neighbour graph" if self._g_nn is None else "the neighbour graph was loaded without its values"))
        n = self._g_nn[0].shape[1]
        if n > self.live_count:
            raise ValueError("GalleryShards.build_neighbours: n must be <= live_count = %d; got %d" % (self.live_count, n))
        if self.neighbours_current:
            return 0, 0
        self._check_build("refresh_neighbours", n)
        self._grow_graph()
        parts, S = self._parts, len(self._parts)
        lens = [len(p) for p in parts]
        old = [min(c, g) for (c, _), g in zip(self._g_sig or [], lens)] + [0] * (S - len(self._g_sig or []))
        dev = next(p.device for p in parts if len(p))
        live_all = torch.cat([p.live.view(torch.uint8) for p, g in zip(parts, lens) if g])  # (bool storage: one byte per row, 0 / 1)
        offs = [sum(lens[:s]) for s in range(S)]
        live_off = torch.tensor(offs, dtype=torch.int64, device=dev)
        live_len = torch.tensor(lens, dtype=torch.int32, device=dev)
        groups = [(t, at, min(SMALL_Q, lens[t] - at)) for t in range(S) for at in range(old[t], lens[t], SMALL_Q)]
        starts = [sum(old[:s]) for s in range(S + 1)]
        redo = torch.zeros(max(starts[S], 1), dtype=torch.uint8, device=dev)
        for s, part in enumerate(parts):
            n0 = old[s]
            if n0 == 0:
                continue

            def merge(cand, m, first):
                call("trid_index_nn_merge_sharded_f32", _p(cand), n0, m, first, n0, _p(live_all), _p(live_off), _p(live_len), live_all.numel(), S, s,
                     _p(self._g_nn[s]), _p(self._g_val[s]), n, _p(redo[starts[s] :]), stream())

            if not groups:
                merge(None, 0, 0)
            for t, at, m in groups:
                merge(part._candidate_scores(at, m, n0, src=parts[t]), m, t * SHARD_STRIDE + at)  # (the A panel comes from part t)
        for t in range(S):
            if lens[t] > old[t]:
                self._graph_rows(t, old[t], lens[t], n)
        again = torch.nonzero(redo[: starts[S]]).reshape(-1).cpu()  # (the one host read: how many rows, and which)
        for s, part in enumerate(parts):
            own = (again[(again >= starts[s]) & (again < starts[s + 1])] - starts[s]).to(dev)
            for at in range(0, own.numel(), SMALL_Q):
                rows = own[at : at + SMALL_Q]
                Q = rows.numel()
                v, r = self._graph_panel(self._fill_panel(part.rows_p16.view(torch.int32)[rows], Q, dev), Q, n)
                self._g_nn[s][rows] = r.int()
                self._g_val[s][rows] = v
        new_rows = sum(int(parts[t].live[old[t] :].sum()) for t in range(S) if lens[t] > old[t])
        self._g_sig = self._sig()
        return new_rows, int(again.numel())

    # ------------------------------------------------------------------ re-ranked search
    def _combine(self, val, row, pid, base, k):
        """the candidates of this process's parts, [Q, parts, kin] with LOCAL rows, -> the first k over all shards: one merge with the
        parts' bases, or - by rank - a gather of every rank's [Q, kin] list first"""
        if self.collective and parallel.world_size() > 1:
            W = parallel.world_size()
            Q, _, kin = val.shape
            cand = [parallel.all_gather_rows(t.reshape(Q, kin)).view(W, Q, kin).permute(1, 0, 2).contiguous() for t in (val, row) + (() if pid is None else (pid,))]
            base = torch.arange(W, dtype=torch.int64, device=val.device) * SHARD_STRIDE
            return self._merge(cand[0], cand[1], None if pid is None else cand[2], base, k)
        return self._merge(val, row, pid, base, k)

    def _reranked(self, name, queries, k, alpha, normalize, mask, distinct):
        """search_reranked (distinct=False) and search_reranked_pids (True): per panel of 32 queries, phase 1 in every part (the dense
        product into the part's score buffer, the deep select with k = n, the lists merged into the query's own GLOBAL list), phase 2
        in every part (the bonus pass in place with that list and the part's global-id lists, the final select, the lists merged) -
        the private steps of GalleryIndex._reranked"""
        x, masks = self._check(name, queries, k, mask, MAX_SHORTLIST_K, distinct, need_graph=True)
        alpha = float(alpha)
        if alpha == 0.0:  # (no bonus, and no select that only feeds it: the shortlist itself)
            return self._search("shortlist_pids" if distinct else "shortlist", queries, k, normalize, mask, MAX_SHORTLIST_K, distinct)
        self._grow_graph()
        parts, S = self._parts, len(self._parts)
        Q, dev, n = x.shape[0], x.device, self._g_nn[0].shape[1]
        # a part is asked for min(k, what it holds), as in the other searches; one with no live row contributes absent lists.  A part
        # with fewer rows than n is walked as n rows, the extra ones masked off (GalleryIndex._search_plan)
        ks = [0 if len(p) == 0 or p.live_count == 0 else min(k, len(p) if m is not None else p.live_count) for p, m in zip(parts, masks)]
        plans = [p._search_plan(kk, m, distinct, also=(n,), extent=n) if kk else None for p, m, kk in zip(parts, masks, ks)]
        kin = k if self.collective else max(max(ks), -(-k // S))
        outs = [torch.empty(Q, k, dtype=d, device=dev) for d in (torch.float32, torch.int64, torch.int64)[: 3 if distinct else 2]]
        own = [(torch.empty(SMALL_Q, n, dtype=torch.float32, device=dev), torch.empty(SMALL_Q, n, dtype=torch.int64, device=dev)) if kk else None for kk in ks]
        tmp = [(torch.empty(SMALL_Q * kk, dtype=torch.float32, device=dev), torch.empty(SMALL_Q * kk, dtype=torch.int64, device=dev)) if kk else None for kk in ks]
        scores = [None] * S
        for at in range(0, Q, SMALL_Q):
            xp = x[at : at + SMALL_Q]
            Qp = xp.shape[0]
            (sv, sr, _), base = self._staging(Qp, S, n, False, dev)
            for s, part in enumerate(parts):
                got = None
                if ks[s]:
                    scores[s] = part._panel_scores(xp, normalize)
                    got = own[s][0][:Qp], own[s][1][:Qp]
                    part._rerank_own_lists(plans[s], scores[s], Qp, n, *got)
                self._stage((sv, sr), s, got)
            qnn = self._combine(sv, sr, None, base, n)[1]  # the queries' own lists, GLOBAL rows, int64 [Qp, n]
            (fv, fr, fp), base = self._staging(Qp, S, kin, distinct, dev)
            for s, part in enumerate(parts):
                kk, got = ks[s], None
                if kk:
                    part._rerank_bonus(plans[s], scores[s], Qp, qnn, self._g_nn[s], n, alpha)
                    got = tmp[s][0][: Qp * kk].view(Qp, kk), tmp[s][1][: Qp * kk].view(Qp, kk)
                    part._rerank_select(plans[s], scores[s], Qp, kk, *got)
                    if distinct:
                        got += (part._pids_of(got[1]),)
                self._stage((fv, fr, fp), s, got)
            for dst, src in zip(outs, self._combine(fv, fr, fp, base, k)):
                dst[at : at + Qp].copy_(src)
        return tuple(outs)

    def search_reranked(self, queries, k=10, alpha=0.05, normalize=True, mask=None):
        """-> (values [Q,k] f32, rows [Q,k] i64 GLOBAL): GalleryIndex.search_reranked over the shards - the exact k best allowed rows by
        similarity + k-reciprocal bonus against the graph of build_neighbours, k <= 1024; a query with fewer than k allowed rows ends in
        (-inf, -1) slots; alpha == 0.0 equals shortlist bit for bit.  Needs a current graph (RuntimeError naming build_neighbours).
        In-process: capturable after one eager call.  By-rank form: collective."""
        return self._reranked("search_reranked", queries, k, alpha, normalize, mask, False)

    def search_reranked_pids(self, queries, k=10, alpha=0.05, normalize=True, mask=None):
        """-> (values, rows GLOBAL, pids), each [Q,k]: GalleryIndex.search_reranked_pids over the shards - the k best distinct pids, each
        by its best re-ranked allowed row; alpha == 0.0 equals shortlist_pids bit for bit.  By-rank form: collective."""
        return self._reranked("search_reranked_pids", queries, k, alpha, normalize, mask, True)

    # ------------------------------------------------------------------ persistence
    def state_dict(self):
        """{"shard_rows", "collective", "parts": the parts' own state dicts in shard order (by-rank form: this rank's one part),
        "neighbours" / "neighbour_values": one int32 / fp32 [len_s, n] tensor per part when the graph over the shards is current (the
        values when they are held), None otherwise}"""
        current = self.neighbours_current and len(self) != 0
        nn, val = (self.neighbours, self.neighbour_values) if current else (None, None)
        return {"shard_rows": self.shard_rows, "collective": self.collective, "parts": [p.state_dict() for p in self._parts],
                "neighbours": None if nn is None else [t.clone() for t in nn], "neighbour_values": None if val is None else [t.clone() for t in val]}

    @staticmethod
    def _load_graph(parts, nn, val):
        """the lists (and values) of a state dict, checked against the loaded parts -> the graph storage (lists, values or None)"""
        ok = isinstance(nn, (list, tuple)) and len(nn) == len(parts) and all(
            torch.is_tensor(t) and t.dtype == torch.int32 and t.dim() == 2 and t.shape[0] == len(p) and 1 <= t.shape[1] <= MAX_NEIGHBOURS and
            t.shape[1] == nn[0].shape[1] for t, p in zip(nn, parts))
        if not ok:
            raise ValueError("GalleryShards.load_state_dict: neighbours must be one int32 [len, n] tensor per part with 1 <= n <= %d" % MAX_NEIGHBOURS)
        if val is not None and not (isinstance(val, (list, tuple)) and len(val) == len(nn) and all(
                torch.is_tensor(v) and v.dtype == torch.float32 and tuple(v.shape) == tuple(t.shape) for v, t in zip(val, nn))):
            raise ValueError("GalleryShards.load_state_dict: neighbour_values must be one float32 tensor per part, shaped like neighbours")
        if len(parts) > MAX_GRAPH_SHARDS:
            raise ValueError("GalleryShards.load_state_dict: the lists hold global rows as int32, which reach %d shards; got %d" % (MAX_GRAPH_SHARDS, len(parts)))
        dev = next((p.device for p in parts if p.device is not None), nn[0].device)
        n = nn[0].shape[1]
        g_nn, g_val = [], None if val is None else []
        for s, part in enumerate(parts):
            a, b = _graph_pair(max(part.capacity, MAX_NEIGHBOURS), n, dev, values=val is not None)
            a[: len(part)].copy_(nn[s].to(dev))
            g_nn.append(a)
            if val is not None:
                b[: len(part)].copy_(val[s].to(dev))
                g_val.append(b)
        return g_nn, g_val

    def load_state_dict(self, sd):
        """Replace the contents with the parts of ``sd`` (each loaded by GalleryIndex.load_state_dict; the row ids are those of the
        saved shards).  "neighbours" present and not None: adopted as the current graph over the shards, refreshable when
        "neighbour_values" came with them (both are checked before anything is replaced); a dict without the key (as written before
        the graph existed) loads with no graph.  shard_rows is taken from the dict; the form (collective or not) stays that of this
        object, and the by-rank form takes exactly one part."""
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
        graph = (None, None) if sd.get("neighbours") is None else self._load_graph(loaded, sd["neighbours"], sd.get("neighbour_values"))
        self.shard_rows, self._parts, self._ws = shard_rows, loaded, {}
        held = [p._has_pids for p in loaded if len(p)]
        self._has_pids = held[0] if held else None
        self._g_nn, self._g_val = graph
        self._g_sig = None if graph[0] is None else self._sig()
