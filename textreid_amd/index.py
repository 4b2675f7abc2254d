"""GalleryIndex: the deployed form of the retrieval match - a gallery held on the device that grows as images arrive, small
query batches answered against it.

``evaluation.similarity_topk`` normalises, measures and packs the whole gallery on every call and then runs a match built for
Q = 1e4 queries.  The index pays those costs once per appended row: it keeps the L2-normalised fp32 rows and the same rows
pre-split (P16, include/textreid_hip.h "P16").  Unit rows satisfy ``|x| <= 1``, so the P16 scale is the analytic one for
``amax = 1.0`` - one constant device scalar that is never recomputed: appending never re-packs earlier rows.  ``search`` with
at most 32 queries is ONE pass over the P16 gallery (csrc/gallery_index.hip, ``trid_index_search_p16``): no host read, no
allocation but the outputs and a workspace cached on the index, so it can be recorded with ``torch.cuda.graph`` and replayed.
Larger batches run the launch sequence of ``similarity_topk`` (``evaluation._Operands.topk``) with the index's own pre-split rows
and unit scale handed in: nothing of the gallery is measured or packed.

Order of the results: value descending, then row number ascending (row number = insertion order).

Removal and filtered search are ONE mechanism: a per-row allow bit that the one-pass kernel honours in its selection step, before
the running threshold sees a value (``trid_index_search_masked_p16``) - a row that may not be returned is never a candidate and
never tightens the threshold, so the answer is the exact top-k of the allowed rows.
  * ``remove(rows=... | pids=...)`` marks rows as removed (tombstones) in a device liveness array, the single source of truth; the
    packed mask words (one uint32 per 32 rows) are derived from it by ``trid_index_pack_mask_u32`` and cached until the next
    ``add`` / ``remove`` / growth.  Row numbers never change: insertion order, stable across ``add`` and ``remove``; ``len``,
    ``rows``, ``rows_p16``, ``pids`` and ``capacity`` include removed rows, ``live`` / ``live_count`` tell them apart.
  * ``search(..., mask=m)``: ``m`` is a bool / uint8 tensor of length ``len`` on the index's device, true = the row may be returned;
    the effective allow set is ``live & m``.  The mask's CONTENTS are an input like the queries: it is packed on the device on
    every call (no host read), and a recorded search replays against whatever the tensor holds at replay time.
  * k: with tombstones only, ``k <= live_count`` (the host knows the count; ValueError otherwise).  With a ``mask`` nothing is read
    back: a query with fewer than k allowed rows gets its real results first, then ``(-inf, -1)`` slots.
  * More than 32 queries with tombstones or a mask run in panels of 32 through the masked one-pass kernel, one gallery pass per
    panel, written into slices of the outputs: exact, but one pass per 32 queries is slower per query than the unmasked large-batch
    route (G = 1e6, Q = 256: 2.45 against 0.52 ms) - bulk callers ``compact()`` first.
  * ``compact()`` drops the removed rows (stable order, P16 rows copied: they carry the fixed unit scale) and returns the old-row
    -> new-row map; afterwards there are no tombstones and searches run the unmasked path again.
An index that never saw ``remove`` and is searched without ``mask`` runs exactly the unmasked path (``trid_index_search_p16``).

``search_pids`` answers "which k PEOPLE are best" where ``search`` answers "which k rows": a gallery holds several images per person
and in a list of rows a person with many good images crowds every other identity out.  The representative of a pid for a query is
its first allowed row in the order above; the result is the first k representatives in that order - at most one row per pid, ties
to the lower row inside a pid and between pids.  It is exact and still ONE pass (``trid_index_search_distinct_p16``, DESIGN.md section
7g): every list of the kernel holds at most one entry per person.  The kernel compares int32 group ids (``group_ids(pids)``: equal
pids = equal ids), derived state like the mask words: a cached buffer, rebuilt by the first ``search_pids`` after ``add`` /
``compact`` / ``load_state_dict`` / growth (``remove`` leaves it valid).  The allow set composes as in ``search``: a removed or
masked row is never a representative, a pid without allowed rows is absent.  The number of distinct pids is never read back: a
query with fewer than k of them ends in ``(-inf, -1, -1)`` slots.  More than 32 queries run in panels of 32.

``shortlist`` is the deep counterpart of ``search``: the exact top-k of the allowed rows for k up to ``MAX_SHORTLIST_K`` = 1024 (a results
page, 100-1000 candidates for a second-stage matcher), any number of queries in panels of 32.  ``search`` and ``search_pids`` stay at
k <= 16, the length of the one-pass kernel's per-lane lists, which do not stretch: a 1024-deep list does not fit in registers.
``shortlist`` selects from the DENSE product instead - ``trid_gemm_p16`` of the index's own operands (P16 gallery as A, the zero-padded
query panel as B, unit scale), to which the one-pass kernel's similarities are bit-identical, so ``shortlist(k <= 16)`` equals ``search``
bit for bit - followed by ``trid_topk_rows_deep_f32`` (csrc/topk_deep.hip) with the same allow words.  Memory: a
score buffer of ``len * cols * 4`` bytes cached on the index and grown with it (cols = 32, or 64 if the tile kernel declines 32 columns:
128 MB at 1e6 rows) plus the select workspace (``trid_topk_rows_deep_ws_bytes``: 3 MB at k = 100, 192 MB at k = 1024 for 1e6 rows).

``shortlist_pids`` is the deep counterpart of ``search_pids``: the exact k best DISTINCT pids, k up to 1024, by the same definition (so
``shortlist_pids(k <= 16)`` equals ``search_pids`` bit for bit, and with all pids different it equals ``shortlist``).  Over-fetching rows
from ``shortlist`` and de-duplicating is not this: a person with many good images eats the list.  Two device steps after the dense
product: ``trid_index_group_best_f32`` (csrc/index_group.hip) walks the cached group table (``group_table(pids)``:
the rows sorted by pid and the start of every pid; derived state like the group ids, one host read of the group count when it is
rebuilt after ``add`` / ``compact`` / ``load_state_dict``; ``remove`` leaves it valid) and leaves every pid's first allowed row per
query, or the sentinel ``(-inf, INT_MAX)``, in a ``[n_slots, 32]`` pair of buffers; ``trid_topk_rows_deep_pairs_f32`` selects over
those pairs, ties to the lower REPRESENTATIVE row.  ``n_slots = max(pids, k)``; a query with fewer than k allowed pids ends in
``(-inf, -1, -1)`` slots and nothing is read back.  ``search_reranked_pids`` runs the same two steps on the bonus-modified buffer of
``search_reranked``: a person's score is their best re-ranked row.  One wave walks a pid: a pid that holds most of the gallery is
serial - the known limit.

``search_reranked`` is the second stage on the index itself: the exact top-k (k <= 1024) by the RE-RANKED score the evaluation's
``rerank=True`` tables measure, ``similarity + alpha * Jaccard(N(query), N(row))`` over neighbour lists of n rows (DESIGN.md section
7i).  It needs the neighbour graph, derived state like the mask words and the group ids but built on request:
  * ``build_neighbours(n=5)``: ``N(j)`` of a live row j = the n best live rows for row j's own embedding as the query, in the order
    above - so j itself normally comes first, an exact duplicate with a lower row number before it.  1 <= n <= 8, n <= live_count.
    The similarities are those of the dense ``trid_gemm_p16`` product: panels of 32 consecutive gallery rows run as the query panel of
    the one-pass kernel (k = n), full panels in place in the P16 storage, the ragged last one through the cached zero-padded panel;
    with tombstones the masked form.  ``ceil(len / 32)`` gallery passes: quadratic in ``len`` (n = 5 on one MI355X: 0.29 s at 1e5
    rows, 7.7 s at 1e6).  Stored as int32 ``[capacity, n]``,
    -1 in every slot of a removed row; read-only face ``neighbours`` (int32 [len, n]; None when no lists are held: never built, or
    dropped by a ``compact`` that renumbered the rows) and ``neighbours_current``.
  * ``add``, ``remove`` (when it removed something), ``compact`` (when it dropped something) and ``load_state_dict`` without a graph
    make the graph stale; ``search_reranked`` then raises and names ``build_neighbours``.  A ``mask=`` never makes it stale: the lists
    are a property of the stored gallery, the mask of one question.  ``state_dict()["neighbours"]`` carries a current graph.
  * ``refresh_neighbours()`` brings a stale graph up to date EXACTLY - lists and values bit-identical to a rebuild - at the cost of
    the change, not of the gallery squared.  The build keeps the VALUE of every list entry (fp32
    ``[capacity, n]``, -inf in every slot of a removed row; ``neighbour_values``, ``state_dict()["neighbour_values"]``) and the graph
    remembers how many rows it covered.  Old rows against new rows is a second query direction whose values must be those of the
    definition (old row i as the B panel, new row g as A: ``s(i, g)`` and ``s(g, i)`` differ in the last bits): per group of 32 new
    rows one ``trid_gemm_p16`` product with the group as A and ALL old P16 rows as B - bit-identical to the narrow products of the
    build, because an element's accumulation order in the tile kernel depends on neither tile shape nor position - and one
    ``trid_index_nn_merge_f32`` (csrc/index_nn_update.hip: one old row per lane, branch-free insert into the register-held list).
    The new rows' own lists come from the build's panel loop over their range; old rows whose list held a removed row are flagged
    by the merge, read once on the host and recomputed in panels of 32.  ``neighbours_refreshable``: lists and values are both
    held (not after a ``compact`` that dropped them, not after loading lists without values).  ``compact(keep_neighbours=True)``
    gathers a current graph to the new row numbers instead of dropping it.
  * per panel of 32 queries: the dense product of ``shortlist``; a deep select with k = n and the allow words of ``live & mask``
    gives the query's own list (its n best ALLOWED rows; fewer allowed rows leave -1 slots and nq < n);
    ``trid_index_rerank_add_f32`` (csrc/index_rerank.hip) adds ``(alpha * c) / (nq + n - c)`` in place where the lists share c > 0
    rows; a second deep select with k over every allowed row of the modified buffer - exact by construction.  ``alpha = 0.0``
    skips the pass and equals ``shortlist`` bit for bit.  G = 1e6, k = 100: 0.50 / 0.80 / 1.29 ms at Q = 1 / 8 / 32 against
    ``shortlist``'s 0.44 / 0.60 / 0.97 ms; the extra select is the cost, the bonus pass takes 0.01-0.05 ms.

``expand_queries`` / ``search_expanded`` / ``search_expanded_pids`` and ``augmented`` are the other two post-processing steps of
re-identification retrieval, query expansion (AQE; weighted: alpha-QE) and database-side augmentation (DBA), on the index itself
(DESIGN.md section 7n).  Both are ONE kernel, ``trid_index_blend_rows_f32`` (csrc/index_blend.hip): a weighted gather-sum of stored
unit fp32 rows, ``out[i] = base[i] + sum_j max(v_ij, 0) ** power * rows[id_ij]`` in list order, every multiply and add rounded to fp32
on its own and the integer power (0 .. 4; 0 = plain averaging) formed by repeated multiplication - so a numpy float32 loop gives the
same bits and the results are exact against a host restatement, like everything above.
  * ``expand_queries(queries, m=5, power=1)``: per panel of 32 queries the two steps of ``shortlist`` with k = m (the m best ALLOWED
    rows and their values), the blend with the unit query as base, ``trid_l2norm_rows_f32`` on the blend.  1 <= m <= ``MAX_EXPAND`` =
    32; no mask: m <= live_count; with a mask nothing is read back and a query with fewer than m allowed rows blends what it has.
  * ``search_expanded(queries, k, m, power)`` = ``shortlist(expand_queries(...), k, normalize=False, mask=mask)`` bit for bit (the same
    allow set in both phases), without leaving the device or the cached buffers: no host read, capturable after one eager call.
    ``search_expanded_pids`` selects through the two steps of ``shortlist_pids`` on the second pass.
  * ``augmented(m=None, power=1)`` -> a NEW index whose every live row is the normalised blend of the first m entries of its own
    neighbour list (weights from ``neighbour_values``; no base: the row leads its list), put through the ordinary ``add``; same
    length, row numbers, pids and tombstones, no graph.  It needs a current graph with its values and leaves this index untouched.

An index is used from ONE stream: ``add``, ``remove`` and ``search`` run on torch's current stream and share the cached workspace.
A recorded search answers against the gallery as it stood at the capture (row count, storage, tombstones and neighbour graph are
part of the recording): record again after ``add`` / ``remove`` / ``compact`` / ``build_neighbours`` / ``refresh_neighbours``.

More than ``MAX_ROWS`` rows, or one part per rank: ``GalleryShards`` (textreid_amd/index_shards.py) composes
plain indexes and merges their lists exactly; its neighbour graph over all shards and its re-ranked searches (section 7m) run the
private steps of this module.  The whole set it touches: the module helpers ``_need_cuda``, ``_graph_pair``, ``_blank_dead`` and
``_fill_panel``; of a part, the steps of the deep panel loop (``_search_plan``, ``_panel_scores``, ``_rerank_own_lists``,
``_rerank_bonus``, ``_rerank_select``), the one-pass dispatcher and its workspace (``_one_pass``, ``_neighbour_workspace``),
``_candidate_scores``, ``_pids_of`` and the field ``_has_pids``.  Everything else goes through the public faces.

Inside the class every step is written once: ``_allow_words`` (the allow words of a call), ``_pids_of``, ``_outputs``, ``_one_pass`` (the
only caller of the three one-pass entry points), ``_search_plan`` (what the panels of a deep search share) and ``_deep_panels`` (the
one panel loop of ``shortlist``, ``shortlist_pids``, the re-ranked and the expanded searches: product, optional middle step, select).
Not built: widths other than 256, in-place re-embedding of a row, an
image-encoder convenience wrapper (``add`` takes embeddings, e.g. the image half of ``inference`` output); a refresh that ``add``
or ``remove`` runs by itself (they make the graph stale; the caller decides when ``refresh_neighbours`` is worth its gallery
pass); a graph build on the streaming filter kernel (its values only agree with the dense product to the last bits); a
non-integer expansion power (``powf`` has no exact host restatement); ``augmented`` over ``GalleryShards`` and the expanded searches
of its by-rank form (the rows of another rank are not addressable); an augmentation that keeps or rebuilds the graph (the new rows
have other neighbours: ``build_neighbours`` on the result).
"""

import torch

from . import ops
from .evaluation import MAX_DEEP_TOPK, MAX_P16_ROWS, _deep_topk, _Operands
from .ops import _p, call, stream

DIM = 256
MAX_ROWS = MAX_P16_ROWS   # the 31-bit byte offsets of the P16 retrieval kernels: rows * 1024 < 2^31 (2**21 - 1)
SMALL_Q = 32              # the panel width of trid_index_search_p16
MAX_K = 16                # search / search_pids: the per-lane lists of the one-pass kernel
MAX_SHORTLIST_K = MAX_DEEP_TOPK  # shortlist / search_reranked: the deep select over the dense score buffer (1024)
MAX_NEIGHBOURS = 8        # build_neighbours: the list length of trid_index_rerank_add_f32 (and of trid_jaccard_add_f32)
MAX_EXPAND = 32           # expand_queries / search_expanded: the list length of trid_index_blend_rows_f32
MAX_EXPAND_POWER = 4      # ... and its largest integer power


def _need_cuda(name, t, owner="index.GalleryIndex"):
    if not t.is_cuda:
        raise RuntimeError("textreid_amd.%s.%s runs on the HIP kernel library only (CUDA tensors); no CPU fallback" % (owner, name))


def _graph_pair(cap, n, device, values=True, old=None, rows=0):
    """-> (lists int32 [cap, n] filled with -1, values fp32 [cap, n] filled with -inf, or None without ``values``): the storage of a
    neighbour graph.  ``old`` = (lists, values or None): its first ``rows`` rows are carried over, and values are held iff it held them."""
    if old is not None:
        values = old[1] is not None
    nn = torch.full((cap, n), -1, dtype=torch.int32, device=device)
    val = torch.full((cap, n), float("-inf"), dtype=torch.float32, device=device) if values else None
    if old is not None and rows:
        nn[:rows].copy_(old[0][:rows])
        if values:
            val[:rows].copy_(old[1][:rows])
    return nn, val


def _blank_dead(nn, val, live):
    """(-1, -inf) into every slot of the rows that are not live: lists, values (or None) and liveness of the SAME row range"""
    dead = ~live[:, None]
    nn.masked_fill_(dead, -1)
    if val is not None:
        val.masked_fill_(dead, float("-inf"))


def _fill_panel(q16, src, Q, held):
    """the Q P16 rows ``src`` into a zero-padded [32, 256] panel whose first ``held`` rows were written before (bit copies: the rows
    carry the fixed unit scale) -> the rows it holds now, Q"""
    q16.view(torch.int32)[:Q].copy_(src.view(torch.int32))
    if Q < held:
        q16[Q:held].zero_()
    return Q


def _panel_of(at, Q, *tensors):
    """the rows [at, at + 32) of tensors that hold Q rows (None stays None) - the tensors themselves when they are ONE panel: the
    latency path makes no views"""
    return tensors if Q <= SMALL_Q else tuple(None if t is None else t[at : at + SMALL_Q] for t in tensors)


def group_ids(pids):
    """int32 [n] on the device of ``pids``: equal pids <=> equal ids (the rank of the pid among the distinct pids, so < n whatever
    the int64 values are).  No host read: stable sort, boundaries, running count, scattered back through the permutation."""
    p = torch.as_tensor(pids).reshape(-1).long()
    n = p.numel()
    out = torch.empty(n, dtype=torch.int32, device=p.device)
    if n == 0:
        return out
    ordered, perm = torch.sort(p, stable=True)
    step = torch.zeros(n, dtype=torch.int32, device=p.device)
    step[1:] = ordered[1:] != ordered[:-1]
    out[perm] = torch.cumsum(step, 0, dtype=torch.int32)
    return out


def group_table(pids):
    """-> (order int32 [n], starts int32 [n_groups + 1], n_groups): the groups of ``group_ids(pids)`` as a table - group s holds the
    rows ``order[starts[s] : starts[s + 1]]``, ascending (the same stable sort, the same numbering).  One host read, the group
    count: like add, not the latency path."""
    p = torch.as_tensor(pids).reshape(-1).long()
    n = p.numel()
    if n == 0:
        return torch.empty(0, dtype=torch.int32, device=p.device), torch.zeros(1, dtype=torch.int32, device=p.device), 0
    ordered, perm = torch.sort(p, stable=True)
    step = torch.zeros(n, dtype=torch.int32, device=p.device)
    step[1:] = ordered[1:] != ordered[:-1]
    gid = torch.cumsum(step, 0, dtype=torch.int32)  # (of the sorted rows: ascending)
    n_groups = int(gid[-1]) + 1
    starts = torch.searchsorted(gid, torch.arange(n_groups + 1, dtype=torch.int32, device=p.device)).int()
    return perm.int(), starts, n_groups


class GalleryIndex:
    """``idx = GalleryIndex(); idx.add(image_embed, pids); vals, rows = idx.search(text_embed, k=10)``.  See the module docstring
    for the storage, the order rule, the one-stream rule and what is out of scope."""

    def __init__(self, dim=DIM, capacity=0):
        if dim != DIM:
            raise ValueError("GalleryIndex: dim must be %d (every config has FEATURE_SIZE 256 and the P16 retrieval kernels are K = 256); got %d" % (DIM, dim))
        if capacity < 0 or capacity > MAX_ROWS:
            raise ValueError("GalleryIndex: capacity must be in [0, %d]; got %d" % (MAX_ROWS, capacity))
        self.dim = dim
        self._want = int(capacity)  # rows the first allocation holds at least
        self._n = 0
        self._rows = None   # fp32 [capacity, 256], L2-normalised
        self._p16 = None    # the same rows, P16
        self._pids = None   # int64 [capacity] once pids were given
        self._live = None   # bool [capacity]: False = removed (the single source of truth for tombstones)
        self._dead = 0      # removed rows among the first len (host count)
        self._words_ok = False  # the cached mask words of the tombstones are current
        self._gids_ok = False   # the cached group ids of the pids are current
        self._gtab_ok = False   # the cached group table of the pids (order, starts, count) is current
        self._nn = None     # int32 [capacity, n]: the neighbour graph (build_neighbours), -1 in every slot of a removed row
        self._nn_ok = False     # the graph is current: no add / remove / compact since it was built or loaded
        self._nn_val = None  # fp32 [capacity, n]: the similarity of every list entry (refresh_neighbours merges by them), -inf in every slot of a removed row
        self._nn_rows = 0    # rows the graph covered when it was last current: refresh_neighbours treats [_nn_rows, len) as new
        self._has_pids = None
        self._unit = None   # device scalar 1.0: the amax every row and every query is packed with
        self._ws = {}       # the cached workspace of the small-batch search
        self._panel_rows = 0  # rows of the cached query panel the last search wrote

    # ------------------------------------------------------------------ storage
    def __len__(self):
        return self._n

    @property
    def capacity(self):
        return 0 if self._rows is None else self._rows.shape[0]

    @property
    def device(self):
        return None if self._rows is None else self._rows.device

    @property
    def rows(self):
        """the normalised fp32 rows held, [len, 256] (a view of the storage)"""
        return None if self._rows is None else self._rows[: self._n]

    @property
    def rows_p16(self):
        """the same rows pre-split, [len, 256] (a view of the storage)"""
        return None if self._p16 is None else self._p16[: self._n]

    @property
    def unit_amax(self):
        return self._unit

    @property
    def pids(self):
        return None if not self._has_pids or self._pids is None else self._pids[: self._n]

    @property
    def live(self):
        """bool [len]: False where the row was removed (a view of the storage)"""
        return None if self._live is None else self._live[: self._n]

    @property
    def live_count(self):
        """rows not removed (a host int)"""
        return self._n - self._dead

    @property
    def neighbours(self):
        """int32 [len, n]: the neighbour lists as build_neighbours (or load_state_dict) left them, -1 in every slot of a row that was
        removed then or appended since (a view of the storage: read-only); None when no lists are held"""
        return None if self._nn is None else self._nn[: self._n]

    @property
    def neighbours_current(self):
        """the lists describe the gallery as it stands: search_reranked takes them"""
        return self._nn is not None and self._nn_ok

    @property
    def neighbour_values(self):
        """fp32 [len, n]: the similarity of every entry of ``neighbours`` (the dense product's own bits), -inf in every slot of a
        row that was removed then or appended since (a view of the storage: read-only); None when no values are held (no lists, or
        lists loaded from a state dict without them)"""
        return None if self._nn is None or self._nn_val is None else self._nn_val[: self._n]

    @property
    def neighbours_refreshable(self):
        """lists and their values are both held, with the same n: refresh_neighbours can bring the graph up to date"""
        return self._nn is not None and self._nn_val is not None and self._nn_val.shape[1] == self._nn.shape[1]

    def _reserve(self, total, device):
        if self._rows is not None and self._rows.device != device:
            raise ValueError("GalleryIndex: the index lives on %s; got a tensor on %s" % (self._rows.device, device))
        cap = self.capacity
        if self._rows is not None and total <= cap:
            return
        new_cap = min(MAX_ROWS, max(total, self._want, 2 * cap, 64))
        rows = torch.empty(new_cap, self.dim, dtype=torch.float32, device=device)
        p16 = torch.empty(new_cap, self.dim, dtype=torch.float32, device=device)
        pids = torch.empty(new_cap, dtype=torch.int64, device=device)
        live = torch.ones(new_cap, dtype=torch.bool, device=device)
        if self._n:
            rows[: self._n].copy_(self._rows[: self._n])
            p16[: self._n].copy_(self._p16[: self._n])
            pids[: self._n].copy_(self._pids[: self._n])
            live[: self._n].copy_(self._live[: self._n])
        self._rows, self._p16, self._pids, self._live = rows, p16, pids, live
        self._words_ok = self._gids_ok = self._gtab_ok = False
        if self._nn is not None:  # (the lists grow with the storage like the other workspaces; growth alone changes nothing in them)
            self._nn, self._nn_val = _graph_pair(new_cap, self._nn.shape[1], device, old=(self._nn, self._nn_val), rows=self._n)
        if self._unit is None:
            self._unit = torch.ones(1, dtype=torch.float32, device=device)

    def _check_rows(self, name, x):
        if not torch.is_tensor(x) or x.dim() != 2 or x.shape[1] != self.dim:
            raise ValueError("GalleryIndex.%s: expected a [n, %d] tensor; got %s" % (name, self.dim, tuple(x.shape) if torch.is_tensor(x) else type(x)))
        _need_cuda(name, x)
        return x.contiguous().float()

    def _pack_into(self, first, n):
        dst = self._p16[first : first + n]
        call("trid_p16_pack_f32", _p(self._rows[first:]), n, self.dim, self.dim, _p(self._unit), _p(dst), 1, stream())

    def add(self, embeddings, pids=None, normalize=True):
        """Append rows; -> row number of the first appended row.  normalize=False takes the rows as they are and checks
        max|x| <= 1 (one host read; add is not the latency path)."""
        if not torch.is_tensor(embeddings) or embeddings.dim() != 2 or embeddings.shape[1] != self.dim:
            raise ValueError("GalleryIndex.add: expected a [n, %d] tensor" % self.dim)
        n = embeddings.shape[0]
        has = pids is not None
        if self._has_pids is not None and has != self._has_pids:
            raise ValueError("GalleryIndex.add: pids must be given on every add or on none")
        if has:
            pids = torch.as_tensor(pids)
            if pids.numel() != n:
                raise ValueError("GalleryIndex.add: %d pids for %d rows" % (pids.numel(), n))
        first = self._n
        if first + n > MAX_ROWS:
            raise ValueError("GalleryIndex.add: at most %d rows (2**21 - 1: the 31-bit offsets of the P16 retrieval kernels); %d + %d asked" % (MAX_ROWS, first, n))
        x = self._check_rows("add", embeddings)
        if n == 0:
            return first
        if not normalize:
            biggest = float(ops.amax(x).item())
            if not biggest <= 1.0:
                raise ValueError("GalleryIndex.add(normalize=False): rows must satisfy max|x| <= 1 (the fixed unit scale); got %g" % biggest)
        self._reserve(first + n, x.device)
        dst = self._rows[first : first + n]
        if normalize:
            inv = ops.empty((n,), x)
            call("trid_l2norm_rows_f32", _p(x), _p(dst), _p(inv), n, self.dim, 1e-12, stream())
        else:
            dst.copy_(x)
        self._pack_into(first, n)
        if has:
            self._pids[first : first + n].copy_(pids.to(x.device).long().reshape(-1))
        self._has_pids = has
        self._live[first : first + n] = True
        self._n = first + n
        self._words_ok = self._gids_ok = self._gtab_ok = False
        if self._nn is not None:  # (no list knows the new rows and they have none: the graph is stale until the next build or refresh)
            self._nn[first : first + n] = -1
            if self._nn_val is not None:
                self._nn_val[first : first + n] = float("-inf")
        self._nn_ok = False
        return first

    # ------------------------------------------------------------------ removal
    def remove(self, rows=None, pids=None):
        """Mark rows as removed; -> how many were newly removed.  Exactly one of ``rows`` (a list or an int64 tensor on any device;
        a row outside [0, len) is a ValueError; duplicates and rows already removed are ignored) and ``pids`` (every row whose pid is
        in the set).  Row numbers do not change.  One host read (the count): like add, not the latency path."""
        if (rows is None) == (pids is None):
            raise ValueError("GalleryIndex.remove: give exactly one of rows and pids")
        n = self._n
        if pids is not None:
            if not self._has_pids:
                raise ValueError("GalleryIndex.remove(pids=...): the index holds no pids")
            want = torch.as_tensor(pids).to(self._rows.device).long().reshape(-1)
            sel = torch.isin(self._pids[:n], want)
        else:
            if torch.is_tensor(rows) and rows.dtype != torch.int64:
                raise ValueError("GalleryIndex.remove(rows=...): a list or an int64 tensor; got %s" % rows.dtype)
            r = torch.as_tensor(rows, dtype=torch.int64).reshape(-1)
            if r.numel() == 0:
                return 0
            lo, hi = int(r.min()), int(r.max())
            if lo < 0 or hi >= n:
                raise ValueError("GalleryIndex.remove(rows=...): rows must be in [0, len(index) = %d); got %d" % (n, lo if lo < 0 else hi))
            sel = torch.zeros(n, dtype=torch.bool, device=self._rows.device)
            sel[r.to(self._rows.device)] = True
        live = self._live[:n]
        newly = int((sel & live).sum())
        if newly:
            live &= ~sel
            self._dead += newly
            self._words_ok = False
            self._nn_ok = False  # (lists that held a removed row are one live neighbour short)
        return newly

    def compact(self, keep_neighbours=False):
        """Drop the removed rows, order kept; -> int64 [old len] on the device, old row -> new row, -1 for a removed row.  Out of
        place: rows, rows_p16 (copied, not re-packed: the fixed unit scale) and pids are gathered into new storage.  Afterwards
        there are no tombstones and searches run the unmasked path; recorded searches must be recorded again.
        keep_neighbours=True with a CURRENT graph: the lists (and their values, when held) of the kept rows are gathered to the new
        row numbers - a current graph holds live rows only, so every entry has one - and the graph stays current (and refreshable).
        The default, and a stale graph, drop the lists."""
        n = self._n
        if self._rows is None:
            return torch.empty(0, dtype=torch.int64)
        dev = self._rows.device
        if not self._dead:
            return torch.arange(n, dtype=torch.int64, device=dev)
        keep = torch.nonzero(self._live[:n]).reshape(-1)
        m = keep.numel()
        new_of = torch.full((n,), -1, dtype=torch.int64, device=dev)
        new_of[keep] = torch.arange(m, dtype=torch.int64, device=dev)
        cap = max(m, 64)
        rows = torch.empty(cap, self.dim, dtype=torch.float32, device=dev)
        p16 = torch.empty(cap, self.dim, dtype=torch.float32, device=dev)
        pids = torch.empty(cap, dtype=torch.int64, device=dev)
        rows[:m] = self._rows[keep]
        p16.view(torch.int32)[:m] = self._p16.view(torch.int32)[keep]
        pids[:m] = self._pids[keep]
        self._rows, self._p16, self._pids = rows, p16, pids
        self._live = torch.ones(cap, dtype=torch.bool, device=dev)
        self._n, self._dead, self._words_ok, self._gids_ok, self._gtab_ok = m, 0, False, False, False
        if keep_neighbours and self.neighbours_current and m:
            nn, val = _graph_pair(cap, self._nn.shape[1], dev, values=self._nn_val is not None)
            nn[:m] = new_of[self._nn[keep].long()].int()
            if val is not None:
                val[:m] = self._nn_val[keep]
            self._nn, self._nn_val, self._nn_rows = nn, val, m
        else:
            self._nn, self._nn_val, self._nn_ok, self._nn_rows = None, None, False, 0  # (the lists hold the old row numbers: dropped, not kept as a trap)
        if m == 0:
            self._has_pids = None
        return new_of

    # ------------------------------------------------------------------ search
    def _workspace(self, nbytes):
        """ONE cached buffer: the query panel (P16 [32, 256]), the normalised queries ([32, 256] fp32), their inverse norms and
        the workers' lists - allocated on first use (and after a growth), zero-filled so that the panel's padding rows are zero"""
        head = 2 * SMALL_Q * self.dim * 4 + 256
        ws = self._ws.get("small")
        if ws is None or ws.numel() < head + nbytes:
            ws = torch.zeros(head + max(nbytes, 16), dtype=torch.uint8, device=self._rows.device)
            self._ws["small"] = ws
            self._panel_rows = 0
        pb = SMALL_Q * self.dim * 4
        q16 = ws[:pb].view(torch.float32).view(SMALL_Q, self.dim)
        qn = ws[pb : 2 * pb].view(torch.float32).view(SMALL_Q, self.dim)
        inv = ws[2 * pb : 2 * pb + SMALL_Q * 4].view(torch.float32)
        return q16, qn, inv, ws[head:]

    def _word_buffer(self, name):
        """a cached uint32 buffer of one mask word per 32 rows of the CAPACITY: part of the index workspace, allocated on first use
        and after a growth (outside any capture, as the workspace above)"""
        nw = (self.capacity + 31) // 32
        buf = self._ws.get(name)
        if buf is None or buf.numel() < nw:
            buf = torch.zeros(nw, dtype=torch.int32, device=self._rows.device)
            self._ws[name] = buf
            if name == "words_live":
                self._words_ok = False
        return buf

    def _mask_words(self, mask):
        """-> the packed allow words of ``live & mask`` (mask None: the tombstones alone, cached until add / remove / growth).  A
        mask is packed on every call: its contents are an input."""
        n = self._n
        if mask is None:
            if self._words_ok:  # (the latency path: nothing to derive, nothing to launch)
                return self._ws["words_live"]
            words = self._word_buffer("words_live")
            if not self._words_ok:
                call("trid_index_pack_mask_u32", _p(self._live), None, n, _p(words), words.numel(), stream())
                self._words_ok = True
            return words
        words = self._word_buffer("words_mask")
        call("trid_index_pack_mask_u32", _p(self._live) if self._dead else None, _p(mask), n, _p(words), words.numel(), stream())
        return words

    def _group_ids(self):
        """-> the cached int32 group ids of the pids, one per row of the CAPACITY (the first len are meaningful): rebuilt after add /
        compact / load_state_dict / growth, outside any capture like the workspace.  remove leaves them valid."""
        buf = self._ws.get("gids")
        if buf is None or buf.numel() < self.capacity:
            buf = torch.zeros(self.capacity, dtype=torch.int32, device=self._rows.device)
            self._ws["gids"] = buf
            self._gids_ok = False
        if not self._gids_ok:
            buf[: self._n].copy_(group_ids(self._pids[: self._n]))
            self._gids_ok = True
        return buf

    def _query_panel(self, x, normalize, need):
        """Q <= 32 queries -> (the cached zero-padded P16 panel [32, 256] holding them, packed with the unit scalar; the rest of the
        cached workspace, >= need bytes)"""
        Q = x.shape[0]
        q16, qn, inv, lists = self._workspace(need)
        if normalize:
            call("trid_l2norm_rows_f32", _p(x), _p(qn), _p(inv), Q, self.dim, 1e-12, stream())
            x = qn
        if Q < self._panel_rows:  # (rows a larger earlier batch left: the panel stays zero-padded)
            q16[Q : self._panel_rows].zero_()
        self._panel_rows = Q
        call("trid_p16_pack_f32", _p(x), Q, self.dim, self.dim, _p(self._unit), _p(q16), 1, stream())
        return q16, lists

    def _one_pass(self, panel, Q, k, vals, rows, lists, words=None, gids=None, workgroups=0):
        """THE dispatcher of the one-pass kernel: the Q <= 32 rows of the P16 panel at ``panel`` as the queries against the whole P16
        gallery -> vals fp32 / rows int64 [Q, k].  lists: the kernel's list workspace (_query_panel, _neighbour_workspace).  words:
        the packed allow bits (the masked kernel); None: every row may be returned.  gids: the rows' group ids (the distinct kernel:
        at most one row per group)."""
        G = self._n
        if gids is not None:
            call("trid_index_search_distinct_p16", _p(panel), _p(self._p16), _p(self._unit), _p(gids), None if words is None else _p(words), Q, G, k, 0,
                 _p(vals), _p(rows), _p(lists), workgroups, stream())
        elif words is None:
            call("trid_index_search_p16", _p(panel), _p(self._p16), _p(self._unit), Q, G, k, 0, _p(vals), _p(rows), _p(lists), workgroups, stream())
        else:
            call("trid_index_search_masked_p16", _p(panel), _p(self._p16), _p(self._unit), _p(words), Q, G, k, 0, _p(vals), _p(rows), _p(lists), workgroups, stream())

    def _search_small(self, x, k, normalize, vals, rows, workgroups=0, words=None, gids=None):
        """Q <= 32: normalise into the cached buffer, pack with the unit scalar, ONE pass over the P16 gallery (_one_pass).  No host read."""
        Q, G = x.shape[0], self._n
        L = ops.L.load()
        need = max(L.trid_index_search_ws_bytes(G, SMALL_Q, MAX_K, 0), L.trid_index_search_ws_bytes(G, Q, k, workgroups))
        q16, lists = self._query_panel(x, normalize, need)
        self._one_pass(q16, Q, k, vals, rows, lists, words, gids, workgroups)

    def _allow_words(self, mask, extent=0):
        """the allow words of one call: those of ``live & mask`` (_mask_words), or None when every row is allowed - no mask, no
        tombstones, and no ``extent`` beyond len (rows the caller walks behind len: their bits are zero)"""
        if mask is None and not self._dead and extent <= self._n:
            return None
        return self._mask_words(None if mask is None else mask.contiguous())

    def _pids_of(self, rows):
        """rows int64 (local, -1 in short slots) -> their pids, -1 in short slots (a -1 indexes the last row: in range, then overwritten)"""
        return self._pids[: self._n][rows].masked_fill_(rows < 0, -1)

    @staticmethod
    def _outputs(Q, k, device):
        """-> (values fp32 [Q, k], rows int64 [Q, k]): the only allocation of a search in steady state"""
        return torch.empty(Q, k, dtype=torch.float32, device=device), torch.empty(Q, k, dtype=torch.int64, device=device)

    def _check_search(self, name, queries, k, mask, need_pids=False, max_k=MAX_K, need_graph=False):
        """the argument rules search, search_pids, shortlist, shortlist_pids and the re-ranked searches share, in the order the messages are promised -> the
        queries, fp32 contiguous.  need_graph: a current neighbour graph, asked for after the argument rules and before the device's"""
        if not torch.is_tensor(queries) or queries.dim() != 2 or queries.shape[1] != self.dim:
            raise ValueError("GalleryIndex.%s: expected a [Q, %d] tensor" % (name, self.dim))
        if need_pids and not self._has_pids:
            raise ValueError("GalleryIndex.%s: the index holds no pids" % name)
        G = self._n
        if G == 0:
            raise ValueError("GalleryIndex.%s: the index is empty" % name)
        if k < 1 or k > max_k or k > G:
            raise ValueError("GalleryIndex.%s: k must be in [1, %d] and <= len(index) = %d; got %d" % (name, max_k, G, k))
        if mask is not None:
            if not torch.is_tensor(mask) or mask.dtype not in (torch.bool, torch.uint8):
                raise ValueError("GalleryIndex.%s: mask must be a bool or uint8 tensor; got %s" % (name, mask.dtype if torch.is_tensor(mask) else type(mask)))
            if mask.dim() != 1 or mask.shape[0] != G:
                raise ValueError("GalleryIndex.%s: mask must have shape [len(index) = %d]; got %s" % (name, G, tuple(mask.shape)))
        elif k > self.live_count:
            raise ValueError("GalleryIndex.%s: k must be <= live_count = %d (%d of %d rows were removed); got %d" % (name, self.live_count, self._dead, G, k))
        if queries.shape[0] == 0:
            raise ValueError("GalleryIndex.%s: no queries" % name)
        if need_graph and not self.neighbours_current:
            raise RuntimeError("GalleryIndex.%s: the neighbour graph is %s; call build_neighbours() first" % (
                name, "absent" if self._nn is None else "stale (add / remove / compact / load_state_dict since it was built)"))
        _need_cuda(name, queries)
        x = queries.contiguous().float()
        if x.device != self._rows.device:
            raise ValueError("GalleryIndex.%s: the index lives on %s; got queries on %s" % (name, self._rows.device, x.device))
        if mask is not None and mask.device != self._rows.device:
            raise ValueError("GalleryIndex.%s: the index lives on %s; got a mask on %s" % (name, self._rows.device, mask.device))
        return x

    def search(self, queries, k=10, normalize=True, mask=None):
        """-> (values [Q,k] f32, rows [Q,k] i64), value descending then row ascending.  Q <= 32: one pass of
        trid_index_search_p16 (no host read, capturable with torch.cuda.graph); larger batches: the launch sequence of
        similarity_topk on the index's own gallery operands.  normalize=False: the queries are unit rows already.
        mask: bool / uint8 [len] on the index's device, true = the row may be returned; the allow set is ``live & mask``.  With
        removed rows or a mask the search runs trid_index_search_masked_p16 (still no host read, still capturable: the mask's
        contents are read at replay time; the tombstones are part of the recording - record again after add / remove / compact),
        in panels of 32 queries when Q > 32 (one gallery pass per panel: compact() before bulk queries).  Removed rows only:
        k <= live_count.  With a mask: a query with fewer than k allowed rows ends in (-inf, -1) slots."""
        x = self._check_search("search", queries, k, mask)
        Q, G = x.shape[0], self._n
        vals, rows = self._outputs(Q, k, x.device)
        words = self._allow_words(mask)
        if words is not None or Q <= SMALL_Q:
            for at in range(0, Q, SMALL_Q):  # panels of 32 queries, one gallery pass each, into slices of the outputs
                part, pv, pr = _panel_of(at, Q, x, vals, rows)
                self._search_small(part, k, normalize, pv, pr, words=words)
            return vals, rows
        q = ops.l2norm_rows(x)[0] if normalize else x
        return _Operands(q, self._rows[:G], ga=self._unit, g16=self._p16[:G]).topk(k, out=(vals, rows))

    def search_pids(self, queries, k=10, normalize=True, mask=None):
        """-> (values [Q,k] f32, rows [Q,k] i64, pids [Q,k] i64): the k best DISTINCT pids of every query, each by its best allowed
        row (value descending, then row ascending, inside a pid and between pids); pids = self.pids[rows].  One pass of
        trid_index_search_distinct_p16 per 32 queries, no host read; capturable with torch.cuda.graph after one eager call (which
        builds the cached group ids and workspaces): a replay reads the queries' and the mask's contents at replay time; record
        again after add / remove / compact.  queries, k, normalize, mask: as search (no mask: k <= live_count).  The index must
        hold pids.  A query with fewer than k distinct allowed pids ends in (-inf, -1, -1) slots."""
        x = self._check_search("search_pids", queries, k, mask, need_pids=True)
        Q = x.shape[0]
        vals, rows = self._outputs(Q, k, x.device)
        words = self._allow_words(mask)
        gids = self._group_ids()
        for at in range(0, Q, SMALL_Q):  # panels of 32 queries, one gallery pass each, into slices of the outputs
            part, pv, pr = _panel_of(at, Q, x, vals, rows)
            self._search_small(part, k, normalize, pv, pr, words=words, gids=gids)
        return vals, rows, self._pids_of(rows)

    # ------------------------------------------------------------------ shortlist
    def _score_buffer(self, cols):
        """the dense product's output, fp32 [capacity, cols]: cached on the index and grown with it"""
        buf = self._ws.get("scores")
        if buf is None or buf.shape[0] < self._n or buf.shape[1] != cols:
            buf = torch.empty(self.capacity, cols, dtype=torch.float32, device=self._rows.device)
            self._ws["scores"] = buf
        return buf

    def _dense_scores(self, q16):
        """-> scores [capacity, cols], rows < len written: trid_gemm_p16 with the P16 gallery as A and the zero-padded query panel as
        B, both at the unit scale.  cols is 32, the width of the search panel - or 64 once the tile kernel has declined 32 columns
        (the first call finds out, outside any capture; the 32 panel rows are then copied into a zero-padded panel of 64)."""
        G = self._n
        gallery = ops.P16(self._p16[:G], self._unit)
        if self._ws.get("cols", SMALL_Q) == SMALL_Q:
            scores = self._score_buffer(SMALL_Q)
            try:
                ops.gemm_p16(gallery, ops.P16(q16, self._unit), scores, G, SMALL_Q, self.dim, SMALL_Q)
                return scores
            except RuntimeError:
                self._ws["cols"] = 2 * SMALL_Q
        cols = 2 * SMALL_Q
        wide = self._ws.get("panel_wide")
        if wide is None:
            wide = torch.zeros(cols, self.dim, dtype=torch.float32, device=self._rows.device)
            self._ws["panel_wide"] = wide
        wide[:SMALL_Q].copy_(q16)
        scores = self._score_buffer(cols)
        ops.gemm_p16(gallery, ops.P16(wide, self._unit), scores, G, cols, self.dim, cols)
        return scores

    def _deep_workspace(self, *ks, slots=None, rows=None):
        """the cached workspace of the deep select, large enough for a panel of 32 queries at every k given over the rows (``rows``:
        another extent than len) - and, with ``slots`` = (n_slots, k), for the pairs select of k over n_slots group slots as well"""
        L = ops.L.load()
        G = self._n if rows is None else rows
        nws = max([L.trid_topk_rows_deep_ws_bytes(SMALL_Q, G, k, 0) for k in ks] +
                  ([L.trid_topk_rows_deep_ws_bytes(SMALL_Q, slots[0], slots[1], 0)] if slots else []))
        ws = self._ws.get("deep")
        if ws is None or ws.numel() < nws:
            ws = torch.empty(nws, dtype=torch.uint8, device=self._rows.device)
            self._ws["deep"] = ws
        return ws

    def shortlist(self, queries, k=100, normalize=True, mask=None):
        """-> (values [Q,k] f32, rows [Q,k] i64): the exact k best allowed rows of every query for 1 <= k <= MAX_SHORTLIST_K = 1024,
        value descending then row ascending - the deep counterpart of search (a results page, candidates for a second stage).
        Per panel of 32 queries: the dense trid_gemm_p16 product of the index's own operands (P16 gallery as A, the zero-padded
        query panel as B, unit scale) into the cached score buffer, then trid_topk_rows_deep_f32 over it with the allow words of
        ``live & mask``.  The one-pass kernel's similarities are bit-identical to that product, so shortlist(k <= 16) equals search
        bit for bit.  queries, normalize, mask: as search (no mask: k <= live_count; with a mask nothing is read back and a query
        with fewer than k allowed rows ends in (-inf, -1) slots).  No host read; after one eager call (which builds the score
        buffer and the workspaces) nothing is allocated but the outputs, so it can be captured with torch.cuda.graph: a replay
        reads the queries' and the mask's contents at replay time; record again after add / remove / compact."""
        return self._reranked("shortlist", queries, k, None, normalize, mask, distinct=False)

    # ------------------------------------------------------------------ deep distinct search
    def _group_table(self):
        """-> (order int32 [len], starts int32 [n_groups + 1], n_groups): the cached group table of the pids (``group_table``), derived
        state like the group ids: rebuilt - one host read, the group count - on the first use after add / compact / load_state_dict
        / growth, outside any capture like the workspace.  remove leaves it valid: a pid with no live row yields the sentinel."""
        if not self._gtab_ok or "gtable" not in self._ws:
            self._ws["gtable"] = group_table(self._pids[: self._n])
            self._gtab_ok = True
        return self._ws["gtable"]

    def _group_best_buffers(self, n_slots):
        """the cached best-pair buffers of one query panel, fp32 and int32 [n_slots, 32]: held for max(n_groups, MAX_SHORTLIST_K)
        slots, so that a recording with another k than the eager call before it allocates nothing"""
        held = max(n_slots, MAX_SHORTLIST_K)
        val = self._ws.get("gbest_val")
        if val is None or val.shape[0] < held:
            val = torch.empty(held, SMALL_Q, dtype=torch.float32, device=self._rows.device)
            self._ws["gbest_val"] = val
            self._ws["gbest_row"] = torch.empty(held, SMALL_Q, dtype=torch.int32, device=self._rows.device)
        return val, self._ws["gbest_row"]

    def _distinct_setup(self, k):
        """-> (table, n_slots, (best values, best rows)) of a distinct select of k: n_slots = max(n_groups, k), so that the select's
        k <= n_slots holds without reading the number of allowed pids"""
        table = self._group_table()
        n_slots = max(table[2], k)
        return table, n_slots, self._group_best_buffers(n_slots)

    def _distinct_select(self, scores, Q, k, words, table, n_slots, best, ws, vals, rows):
        """steps 1 and 2 on the score buffer of one panel: trid_index_group_best_f32 with the allow words into the best-pair buffers,
        then trid_topk_rows_deep_pairs_f32 over the n_slots pairs of every query (ld_q = 1)"""
        order, starts, n_groups = table
        bv, br = best
        call("trid_index_group_best_f32", _p(scores), 1, scores.shape[1], Q, self._n, _p(order), _p(starts), n_groups, n_slots, _p(words),
             _p(bv), _p(br), 1, SMALL_Q, stream())
        call("trid_topk_rows_deep_pairs_f32", _p(bv), _p(br), 1, SMALL_Q, Q, n_slots, k, 0, _p(vals), _p(rows), _p(ws), ws.numel(), 0, stream())

    def shortlist_pids(self, queries, k=100, normalize=True, mask=None):
        """-> (values [Q,k] f32, rows [Q,k] i64, pids [Q,k] i64): the exact k best DISTINCT pids of every query for 1 <= k <=
        MAX_SHORTLIST_K = 1024, each by its best allowed row - the definition of search_pids (value descending, then row ascending,
        inside a pid and between pids; pids = self.pids[rows]) at the depth of shortlist.  Per panel of 32 queries: the dense product
        of shortlist into the cached score buffer; trid_index_group_best_f32 (csrc/index_group.hip) over the cached group table with
        the allow words of ``live & mask`` - every pid's first allowed row, (-inf, INT_MAX) for a pid without one - into the cached
        [n_slots, 32] best-pair buffers; trid_topk_rows_deep_pairs_f32 over those pairs, ordered by value and then by the
        REPRESENTATIVE row.  n_slots = max(number of pids, k): the number of allowed pids is never read back, and a query with fewer
        than k of them ends in (-inf, -1, -1) slots.  shortlist_pids(k <= 16) equals search_pids bit for bit.  queries, normalize,
        mask: as search (no mask: k <= live_count).  The index must hold pids.  No host read; after one eager call (which builds the
        group table - one read of the group count - the buffers and the workspaces) nothing is allocated but the outputs, so it can
        be captured with torch.cuda.graph: a replay reads the queries' and the mask's contents at replay time; record again after
        add / remove / compact.  One wave walks a pid's rows: a pid holding most of the gallery is serial."""
        vals, rows = self._reranked("shortlist_pids", queries, k, None, normalize, mask, distinct=True)
        return vals, rows, self._pids_of(rows)

    # ------------------------------------------------------------------ neighbour graph and re-ranked search
    def build_neighbours(self, n=5):
        """Build the neighbour graph search_reranked needs: for every live row j, N(j) = the n best live rows for row j's own
        embedding as the query (value descending, then row ascending: j itself first unless an exact duplicate has a lower row
        number); -1 in every slot of a removed row.  1 <= n <= 8, n <= live_count.  ceil(len / 32) passes of the one-pass kernel
        (the masked form with the cached tombstone words once rows were removed), panels of 32 consecutive gallery rows as the
        query panel - in place in the P16 storage, the ragged last one through the cached zero-padded panel - so the similarities
        are bit-identical to the dense trid_gemm_p16 product of the index's own operands.  The kernel's values are kept beside the
        lists (``neighbour_values``, -inf in every slot of a removed row): refresh_neighbours merges by them.  Quadratic in len; no
        host read."""
        if n < 1 or n > MAX_NEIGHBOURS:
            raise ValueError("GalleryIndex.build_neighbours: n must be in [1, %d]; got %d" % (MAX_NEIGHBOURS, n))
        G = self._n
        if G == 0:
            raise ValueError("GalleryIndex.build_neighbours: the index is empty")
        if n > self.live_count:
            raise ValueError("GalleryIndex.build_neighbours: n must be <= live_count = %d; got %d" % (self.live_count, n))
        found, vals = self._neighbour_panels(0, G, n)
        self._nn, self._nn_val = _graph_pair(self.capacity, n, self._rows.device)
        self._nn[:G].copy_(found)
        self._nn_val[:G].copy_(vals)
        if self._dead:
            _blank_dead(self._nn[:G], self._nn_val[:G], self._live[:G])
        self._nn_ok, self._nn_rows = True, G

    def _neighbour_workspace(self, n):
        """-> (the cached zero-padded panel, the kernel's list workspace, the tombstone words or None) for neighbour searches at k = n
        with any number of panel rows"""
        L = ops.L.load()
        need = max(L.trid_index_search_ws_bytes(self._n, SMALL_Q, MAX_K, 0), L.trid_index_search_ws_bytes(self._n, SMALL_Q, n, 0))
        q16, _, _, lists = self._workspace(need)  # (workers x Q x k x 8 bytes: the full panel covers every smaller one)
        return q16, lists, (self._mask_words(None) if self._dead else None)

    def _neighbour_panels(self, first, last, n):
        """the panel loop of build_neighbours over the rows [first, last) -> (found int64 [last - first, n], vals fp32 [same]): panels
        of 32 consecutive gallery rows as the query panel of the one-pass kernel with k = n against the WHOLE gallery (the masked form
        once rows were removed) - full panels in place in the P16 storage, the ragged last one through the cached zero-padded panel.
        Rows and values of removed rows are whatever the search gives: the caller overwrites them."""
        q16, lists, words = self._neighbour_workspace(n)
        dev = self._rows.device
        vals = torch.empty(last - first, n, dtype=torch.float32, device=dev)
        found = torch.empty(last - first, n, dtype=torch.int64, device=dev)
        for at in range(first, last, SMALL_Q):
            Q = min(SMALL_Q, last - at)
            if Q == SMALL_Q:  # (the stored rows ARE a panel: packed with the unit scalar, 1024 bytes per row, 16-byte aligned)
                panel = self._p16[at : at + SMALL_Q]
            else:
                self._panel_rows = _fill_panel(q16, self._p16[at : at + Q], Q, self._panel_rows)
                panel = q16
            self._one_pass(panel, Q, n, vals[at - first :], found[at - first :], lists, words)
        return found, vals

    def _candidate_scores(self, at, m, n0, src=None):
        """-> the cached score buffer holding, as a row-major [m, n0] matrix at its start, the similarity of every old row i < n0 AS THE
        QUERY to the m <= 32 rows from ``at`` of ``src`` (another index: a part of GalleryShards; default: this one): trid_gemm_p16
        with the m P16 rows as A (gallery role) and the P16 rows [0, n0) as B
        (query role), both at the unit scale - the operand roles of the build's products, so the same fp32 numbers (DESIGN.md section
        7j).  Always the tile kernel: the streaming short-K kernel ops.gemm_p16 would pick for n0 % 32 == 0 sums in another order."""
        src = self if src is None else src
        cand = self._score_buffer(self._ws.get("cols", SMALL_Q))  # (capacity * cols >= 32 * n0 floats)
        ops.gemm_p16(ops.P16(src._p16[at : at + m], src._unit), ops.P16(self._p16[:n0], self._unit), cand, m, n0, self.dim, n0, tile_only=True)
        return cand

    def refresh_neighbours(self):
        """Bring a stale neighbour graph up to date EXACTLY, without the quadratic rebuild -> (new_rows, redone_rows): the live rows
        appended since the graph was last current, and the older rows whose lists had to be recomputed because they held a row that
        was removed since.  Lists and values afterwards equal those of build_neighbours(n) on the same contents bit for bit.
        Needs ``neighbours_refreshable`` (RuntimeError naming build_neighbours otherwise: never built, dropped by compact, loaded
        without values) and n <= live_count (the ValueError of build_neighbours); both are checked before anything is modified.  A
        current graph returns (0, 0) without a launch.  With n0 rows covered and len rows now:
          * per group of at most 32 new rows at ``at``: the product of the group's P16 rows (A, gallery role) with the P16 rows
            [0, n0) (B, query role) at the unit scale on the tile kernel trid_gemm_p16 - the definition's direction: old row i as the
            B panel - into the cached score buffer, then ONE trid_index_nn_merge_f32 with cand_first = at, rows = n0; removals
            only: one merge launch with m = 0;
          * the lists of the new rows [n0, len) from build_neighbours' own panel loop over that range;
          * the merge flags every old live row whose list holds a removed row: the flags are read once on the host (refresh is not
            the latency path, like add and remove), the flagged rows' P16 rows are gathered 32 at a time into the cached panel,
            searched with k = n and scattered back.
        Exact: a live old row whose list holds no removed row keeps it as its top n over the still-live old rows (removing
        non-members cannot change a top n), and merging the live new rows into it gives the top n over all live rows; every other row
        is recomputed from scratch.  A recorded search must be recorded again afterwards, as after a build."""
        if not self.neighbours_refreshable:
            raise RuntimeError("GalleryIndex.refresh_neighbours: %s; call build_neighbours() first" % (
                "there is no neighbour graph" if self._nn is None else "the neighbour graph was loaded without its values"))
        n = self._nn.shape[1]
        if n > self.live_count:
            raise ValueError("GalleryIndex.build_neighbours: n must be <= live_count = %d; got %d" % (self.live_count, n))
        if self._nn_ok:
            return 0, 0
        n0, n1 = self._nn_rows, self._n
        dev = self._rows.device
        redo = torch.zeros(n0, dtype=torch.uint8, device=dev)
        live = self._live  # (bool storage: one byte per row, 0 / 1)

        def merge(cand, m, at):
            call("trid_index_nn_merge_f32", _p(cand), n0, m, at, n0, _p(live), _p(self._nn), _p(self._nn_val), n, _p(redo), stream())

        if n1 == n0:
            merge(None, 0, n0)
        else:
            for at in range(n0, n1, SMALL_Q):
                m = min(SMALL_Q, n1 - at)
                merge(self._candidate_scores(at, m, n0), m, at)
            found, vals = self._neighbour_panels(n0, n1, n)
            self._nn[n0:n1].copy_(found)
            self._nn_val[n0:n1].copy_(vals)
            _blank_dead(self._nn[n0:n1], self._nn_val[n0:n1], self._live[n0:n1])
        again = torch.nonzero(redo).reshape(-1)  # (the one host read: how many rows, and which)
        if again.numel():
            q16, lists, words = self._neighbour_workspace(n)
            vals = torch.empty(SMALL_Q, n, dtype=torch.float32, device=dev)
            found = torch.empty(SMALL_Q, n, dtype=torch.int64, device=dev)
            for at in range(0, again.numel(), SMALL_Q):
                rows = again[at : at + SMALL_Q]
                Q = rows.numel()
                self._panel_rows = _fill_panel(q16, self._p16.view(torch.int32)[rows], Q, self._panel_rows)
                self._one_pass(q16, Q, n, vals, found, lists, words)
                self._nn[rows] = found[:Q].int()
                self._nn_val[rows] = vals[:Q]
        new_rows = int(self._live[n0:n1].sum()) if n1 > n0 else 0
        self._nn_ok, self._nn_rows = True, n1
        return new_rows, int(again.numel())

    def search_reranked(self, queries, k=10, alpha=0.05, normalize=True, mask=None):
        """-> (values [Q,k] f32, rows [Q,k] i64): the exact k best allowed rows of every query by RE-RANKED score, similarity +
        (alpha * c) / (nq + n - c) with c = rows the query's own neighbour list and the row's stored list share, n = the graph's
        list length, nq = the query's list length (n unless fewer rows are allowed) - for nq == n alpha times the Jaccard index of
        the two lists, the term of evaluation.k_reciprocal.  1 <= k <= MAX_SHORTLIST_K = 1024, value descending then row ascending.
        Needs a current graph (build_neighbours; RuntimeError otherwise).  Per panel of 32 queries: the dense product of shortlist
        into the cached score buffer; a deep select with k = n over the allowed rows (``live & mask``) = the query's own list;
        trid_index_rerank_add_f32 in place on the buffer; a deep select with k over every allowed row of the modified buffer - so
        the result is exact, not a re-ordered shortlist.  alpha == 0.0 skips the bonus (and the select that only feeds it) and equals shortlist bit for bit.  queries,
        normalize, mask: as shortlist.  No host read; after one eager call nothing is allocated but the outputs and the queries'
        lists, so it can be captured with torch.cuda.graph; record again after add / remove / compact / build_neighbours."""
        return self._reranked("search_reranked", queries, k, alpha, normalize, mask, distinct=False)

    def _reranked(self, name, queries, k, alpha, normalize, mask, distinct):
        """the shortlists (alpha None: no graph is asked for) and the re-ranked searches, over rows (distinct=False) or distinct pids
        (True) -> (values, rows): the panel loop with, for alpha != 0, the query's own list and the bonus pass as its middle step"""
        graph = alpha is not None
        x = self._check_search(name, queries, k, mask, need_pids=distinct, max_k=MAX_SHORTLIST_K, need_graph=graph)
        alpha = float(alpha) if graph else 0.0
        plan = self._search_plan(k, mask, distinct, also=(self._nn.shape[1],) if graph else ())
        if alpha == 0.0:  # (no bonus, and no select that only feeds it)
            return self._deep_panels(x, k, normalize, plan)
        n, Qp = self._nn.shape[1], min(x.shape[0], SMALL_Q)
        qnn = torch.empty(Qp, n, dtype=torch.int64, device=x.device)
        qval = torch.empty(Qp, n, dtype=torch.float32, device=x.device)

        def bonus(at, part, scores):
            self._rerank_own_lists(plan, scores, part.shape[0], n, qval, qnn)
            self._rerank_bonus(plan, scores, part.shape[0], qnn, self._nn, n, alpha)
            return scores

        return self._deep_panels(x, k, normalize, plan, bonus)

    # the private steps of a deep search: _deep_panels runs them on one index, GalleryShards (index_shards.py) runs them in two phases
    # over its parts with the merge of the parts' lists between them.
    def _search_plan(self, k, mask, distinct=False, also=(), extent=0):
        """what every panel of one deep search shares -> (G, words, ws, distinct state or None).  G = the rows the selects and the
        bonus pass walk: len, or ``extent`` when that is more (GalleryShards: a part with fewer rows than the graph's n is walked as
        ``extent`` = n rows, the extra ones masked off - the allow words are then always given, and they are zero behind len).
        words: the allow words of the call (_allow_words); ws: the deep select's workspace over G rows for the final select - k
        (None: no final select), or the pairs select of the distinct form - and for every other k in ``also`` (the graph's n, the
        expansion's m)."""
        G = max(self._n, extent)
        words = self._allow_words(mask, extent)
        if distinct:
            table, n_slots, best = self._distinct_setup(k)
            return G, words, self._deep_workspace(*also, slots=(n_slots, k), rows=G), (table, n_slots, best)
        return G, words, self._deep_workspace(*([] if k is None else [k]), *also, rows=G), None

    def _deep_panels(self, x, k, normalize, plan, middle=None):
        """THE panel loop of the deep searches -> (values [Q, k], rows [Q, k]): per panel of 32 queries the dense product into the one
        score buffer (_panel_scores), the optional ``middle(at, part, scores)`` -> the buffer to select from (None: this panel is
        done), the final select (_rerank_select) into slices of the outputs.  k None: no outputs, the middle step keeps what it makes."""
        Q = x.shape[0]
        vals, rows = self._outputs(Q, k, x.device) if k is not None else (None, None)
        for at in range(0, Q, SMALL_Q):
            part, pv, pr = _panel_of(at, Q, x, vals, rows)
            scores = self._panel_scores(part, normalize)
            if middle is not None:
                scores = middle(at, part, scores)
            if scores is not None:
                self._rerank_select(plan, scores, part.shape[0], k, pv, pr)
        return vals, rows

    def _panel_scores(self, part, normalize):
        """at most 32 queries -> the cached score buffer holding their dense product with the gallery (shortlist's first step)"""
        q16, _ = self._query_panel(part, normalize, ops.L.load().trid_index_search_ws_bytes(self._n, SMALL_Q, MAX_K, 0))
        return self._dense_scores(q16)

    def _rerank_own_lists(self, plan, scores, Q, n, qval, qnn):
        """the queries' own neighbour lists: a deep select with k = n over the allowed rows of the score buffer -> qval fp32, qnn int64 [Q, n]"""
        G, words, ws, _ = plan
        _deep_topk(_p(scores), 1, scores.shape[1], Q, G, n, words, qval, qnn, ws=ws)

    def _rerank_bonus(self, plan, scores, Q, qnn, gnn, n, alpha):
        """trid_index_rerank_add_f32 in place on the score buffer: qnn int64 [Q, n] the queries' lists, gnn int32 [>= G, n] the rows' lists
        (the same id space: local rows here, global ids over shards)"""
        G, words, _, _ = plan
        call("trid_index_rerank_add_f32", _p(scores), 1, scores.shape[1], Q, G, _p(qnn), _p(gnn), n, alpha, _p(words), stream())

    def _rerank_select(self, plan, scores, Q, k, vals, rows):
        """the final select over the (modified) score buffer: the deep row select, or the two distinct-pid steps"""
        G, words, ws, distinct = plan
        if distinct is not None:
            table, n_slots, best = distinct
            self._distinct_select(scores, Q, k, words, table, n_slots, best, ws, vals, rows)
        else:
            _deep_topk(_p(scores), 1, scores.shape[1], Q, G, k, words, vals, rows, ws=ws)

    def search_reranked_pids(self, queries, k=10, alpha=0.05, normalize=True, mask=None):
        """-> (values [Q,k] f32, rows [Q,k] i64, pids [Q,k] i64): search_reranked over DISTINCT pids - a person's score is their best
        re-ranked allowed row, the result the k best persons (1 <= k <= MAX_SHORTLIST_K = 1024; value descending, then row ascending,
        inside a pid and between pids; fewer allowed pids than k end in (-inf, -1, -1) slots).  It is search_reranked with the final row
        select replaced by the two steps of shortlist_pids (trid_index_group_best_f32, trid_topk_rows_deep_pairs_f32) on the
        bonus-modified buffer: exact by construction.  alpha == 0.0 equals shortlist_pids bit for bit.  Needs pids and a current graph;
        queries, normalize, mask and the capture rule: as search_reranked and shortlist_pids."""
        vals, rows = self._reranked("search_reranked_pids", queries, k, alpha, normalize, mask, distinct=True)
        return vals, rows, self._pids_of(rows)

    # ------------------------------------------------------------------ query expansion and database-side augmentation
    def _blend_tables(self):
        """-> (part addresses int64 [1], part lengths int64 [1]) on the device: this index as the ONE part of
        trid_index_blend_rows_f32 (shift 0: id = local row).  Derived state like the mask words: rebuilt - one small upload, outside
        any capture - when the storage or the length changed."""
        key = (self._rows.data_ptr(), self._n)
        if self._ws.get("blend_key") != key:
            self._ws["blend_tab"] = torch.tensor(key, dtype=torch.int64, device=self._rows.device)
            self._ws["blend_key"] = key
        tab = self._ws["blend_tab"]
        return tab[:1], tab[1:]

    def _expand_buffers(self):
        """the cached buffers of one expanded panel: the queries' own lists (fp32 values and int64 rows, 32 * MAX_EXPAND each), the
        blend and the unit queries / the expanded queries ([32, 256] fp32 each) - allocated on first use, outside any capture"""
        buf = self._ws.get("expand")
        if buf is None:
            dev = self._rows.device
            buf = (torch.empty(SMALL_Q * MAX_EXPAND, dtype=torch.float32, device=dev), torch.empty(SMALL_Q * MAX_EXPAND, dtype=torch.int64, device=dev),
                   torch.empty(SMALL_Q, self.dim, dtype=torch.float32, device=dev), torch.empty(SMALL_Q, self.dim, dtype=torch.float32, device=dev))
            self._ws["expand"] = buf
        return buf

    def _check_expand(self, name, queries, k, m, power, mask, need_pids=False):
        """the argument rules of expand_queries (k None) and the expanded searches: m and power (an empty index is told by the
        shared rules), then those of shortlist -> the queries, fp32 contiguous"""
        G = self._n
        if G and (not isinstance(m, int) or m < 1 or m > MAX_EXPAND or m > G):
            raise ValueError("GalleryIndex.%s: m must be in [1, %d] and <= len(index) = %d; got %r" % (name, MAX_EXPAND, G, m))
        if G and mask is None and m > self.live_count:
            raise ValueError("GalleryIndex.%s: m must be <= live_count = %d (%d of %d rows were removed); got %d" % (name, self.live_count, self._dead, G, m))
        if not isinstance(power, int) or power < 0 or power > MAX_EXPAND_POWER:
            raise ValueError("GalleryIndex.%s: power must be an integer in [0, %d]; got %r" % (name, MAX_EXPAND_POWER, power))
        return self._check_search(name, queries, 1 if k is None else k, mask, need_pids=need_pids, max_k=MAX_SHORTLIST_K)

    def _expanded(self, name, queries, k, m, power, normalize, mask, distinct=False):
        """expand_queries (k None -> the expanded queries), search_expanded and search_expanded_pids (-> values, rows): the panel
        loop with the expansion as its middle step.  Per panel of 32 queries: the dense product and the deep select with k = m over
        the allowed rows (shortlist's two steps) = the queries' m best rows and their values; trid_index_blend_rows_f32 with the
        unit queries as base; trid_l2norm_rows_f32 on the blend; then, for the searches, the product again with the expanded
        queries and the final select with the SAME allow words."""
        x = self._check_expand(name, queries, k, m, power, mask, need_pids=distinct)
        plan = self._search_plan(k, mask, distinct, also=(m,))
        qval, qrow, blend, unit = self._expand_buffers()
        tab, lens = self._blend_tables()
        out = torch.empty(x.shape[0], self.dim, dtype=torch.float32, device=x.device) if k is None else None

        def expand(at, part, scores):
            Qp = part.shape[0]
            if normalize:
                base = self._workspace(0)[1]  # (the normalised queries the panel was packed from)
            else:
                base = part if part.data_ptr() % 16 == 0 else unit[:Qp].copy_(part)  # (the blend reads 16 bytes per lane)
            qv, qr = qval[: Qp * m].view(Qp, m), qrow[: Qp * m].view(Qp, m)
            self._rerank_own_lists(plan, scores, Qp, m, qv, qr)
            call("trid_index_blend_rows_f32", _p(tab), _p(lens), 1, 0, _p(qr), 8, _p(qv), m, Qp, m, power, _p(base), self.dim, _p(blend), stream())
            new = out[at : at + Qp] if k is None else unit[:Qp]
            call("trid_l2norm_rows_f32", _p(blend), _p(new), None, Qp, self.dim, 1e-12, stream())
            return None if k is None else self._panel_scores(new, False)

        found = self._deep_panels(x, k, normalize, plan, expand)
        return out if k is None else found

    def expand_queries(self, queries, m=5, power=1, normalize=True, mask=None):
        """-> unit fp32 [Q, 256]: query expansion (AQE for power = 0, its weighted form alpha-QE for power >= 1).  Every query is
        replaced by the normalised weighted sum of itself and its m best allowed rows: with (v_j, r_j) the values and rows of
        shortlist(queries, k=m, mask=mask), expanded = l2norm(unit query + sum_j max(v_j, 0) ** power * rows[r_j]), the sum taken in list order and
        every multiply and add rounded to fp32 on its own (trid_index_blend_rows_f32, csrc/index_blend.hip; the power by repeated
        multiplication), the norm by trid_l2norm_rows_f32 (eps 1e-12).  1 <= m <= MAX_EXPAND = 32, m <= len; without a mask
        m <= live_count (ValueError); with a mask nothing is read back and a query with fewer than m allowed rows blends what it
        has (-1 slots are skipped).  0 <= power <= 4.  queries, normalize, mask and the capture rule: as shortlist."""
        return self._expanded("expand_queries", queries, None, m, power, normalize, mask)

    def search_expanded(self, queries, k=10, m=5, power=1, normalize=True, mask=None):
        """-> (values [Q,k] f32, rows [Q,k] i64): the exact k best allowed rows (1 <= k <= MAX_SHORTLIST_K = 1024) for the EXPANDED
        queries - shortlist(expand_queries(queries, m, power, normalize, mask), k, normalize=False, mask=mask) bit for bit, the same
        allow set in both phases - in panels of 32 queries through the cached score buffer and workspaces.  No host read; after one
        eager call nothing is allocated but the outputs, so it can be captured with torch.cuda.graph: a replay reads the queries'
        and the mask's contents at replay time; record again after add / remove / compact."""
        return self._expanded("search_expanded", queries, k, m, power, normalize, mask)

    def search_expanded_pids(self, queries, k=10, m=5, power=1, normalize=True, mask=None):
        """-> (values [Q,k] f32, rows [Q,k] i64, pids [Q,k] i64): search_expanded over DISTINCT pids - the first phase is the same
        (the m best allowed ROWS), the second pass selects through the two steps of shortlist_pids; it equals
        shortlist_pids(expand_queries(...), k, normalize=False, mask=mask) bit for bit.  The index must hold pids."""
        vals, rows = self._expanded("search_expanded_pids", queries, k, m, power, normalize, mask, distinct=True)
        return vals, rows, self._pids_of(rows)

    def augmented(self, m=None, power=1):
        """-> a NEW GalleryIndex, database-side augmentation (DBA): every live row's embedding becomes the normalised weighted sum of
        the first m entries of its own neighbour list - the row itself leads its list, so there is no base - with the weights
        max(neighbour_values, 0) ** power (power 0: the plain mean direction): ONE trid_index_blend_rows_f32 launch over the lists
        and their values, then the ordinary add (normalise, pack at the unit scale).  Same length, row numbers and pids; the same
        rows are removed (their lists are all -1: a zero blend, and they are tombstones anyway); no graph.  This index is not
        touched.  Needs a current graph whose values are held (RuntimeError naming build_neighbours / refresh_neighbours).  m
        defaults to the graph's n; 1 <= m <= n; 0 <= power <= 4."""
        if not self.neighbours_current or not self.neighbours_refreshable or self._n == 0:
            raise RuntimeError("GalleryIndex.augmented: the neighbour graph is %s; call build_neighbours() (or refresh_neighbours()) first" % (
                "absent" if self._nn is None else "held without its values" if self.neighbours_current else
                "stale (add / remove / compact / load_state_dict since it was built)"))
        n = self._nn.shape[1]
        m = n if m is None else m
        if not isinstance(m, int) or m < 1 or m > n:
            raise ValueError("GalleryIndex.augmented: m must be in [1, n = %d] (the graph's list length); got %r" % (n, m))
        if not isinstance(power, int) or power < 0 or power > MAX_EXPAND_POWER:
            raise ValueError("GalleryIndex.augmented: power must be an integer in [0, %d]; got %r" % (MAX_EXPAND_POWER, power))
        G = self._n
        tab, lens = self._blend_tables()
        blend = torch.empty(G, self.dim, dtype=torch.float32, device=self._rows.device)
        call("trid_index_blend_rows_f32", _p(tab), _p(lens), 1, 0, _p(self._nn), 4, _p(self._nn_val), n, G, m, power, None, 0, _p(blend), stream())
        new = GalleryIndex(capacity=G)
        new.add(blend, self.pids)
        if self._dead:
            new.remove(rows=torch.nonzero(~self._live[:G]).reshape(-1))
        return new

    # ------------------------------------------------------------------ persistence
    def state_dict(self):
        """the normalised fp32 rows, the pids (None without) and the liveness (bool [len]; None when nothing was removed); P16 is
        re-derived on load; "neighbours": the int32 [len, n] lists of a CURRENT neighbour graph, None otherwise; "neighbour_values":
        their fp32 [len, n] values when the graph is current and holds them, None otherwise"""
        current = self.neighbours_current and self._n != 0
        return {"rows": None if self._rows is None else self._rows[: self._n].clone(),
                "pids": None if not self._has_pids else self._pids[: self._n].clone(),
                "live": None if not self._dead else self._live[: self._n].clone(),
                "neighbours": self._nn[: self._n].clone() if current else None,
                "neighbour_values": self._nn_val[: self._n].clone() if current and self.neighbours_refreshable else None}

    @staticmethod
    def _check_neighbours(nn, rows):
        """the lists of a state dict: int32 [rows, n], 1 <= n <= 8, values in [-1, rows) (one host read: load is not the latency path)"""
        if not torch.is_tensor(nn) or nn.dtype != torch.int32 or nn.dim() != 2 or nn.shape[0] != rows or not 1 <= nn.shape[1] <= MAX_NEIGHBOURS:
            raise ValueError("GalleryIndex.load_state_dict: neighbours must be an int32 [%d, n] tensor with 1 <= n <= %d; got %s" % (
                rows, MAX_NEIGHBOURS, "%s %s" % (nn.dtype, tuple(nn.shape)) if torch.is_tensor(nn) else type(nn)))
        lo, hi = int(nn.min()), int(nn.max())
        if lo < -1 or hi >= rows:
            raise ValueError("GalleryIndex.load_state_dict: neighbours must hold rows in [-1, %d); got %d" % (rows, lo if lo < -1 else hi))

    def load_state_dict(self, sd):
        """Replace the contents.  The rows are taken as they are (already normalised: no second normalisation) and re-packed.  A
        state dict without "live" (as written before removal existed) loads as all-live.  "neighbours" present and not None: the
        lists are adopted as the current neighbour graph; a dict without them loads with no graph.  "neighbour_values" (fp32, shaped
        like the lists; ValueError otherwise, and when "neighbours" is None) is adopted with them: the graph is then refreshable; lists
        without values load as a current graph that refresh_neighbours refuses.  A dict with no "neighbours" key at all loads with
        no graph whatever else it holds, as it always did."""
        rows = sd["rows"]
        if rows is None or rows.shape[0] == 0:
            self._n, self._has_pids, self._dead, self._words_ok, self._gids_ok, self._gtab_ok = 0, None, 0, False, False, False
            self._nn, self._nn_val, self._nn_ok, self._nn_rows = None, None, False, 0
            return
        if rows.shape[0] > MAX_ROWS:
            raise ValueError("GalleryIndex.load_state_dict: at most %d rows; got %d" % (MAX_ROWS, rows.shape[0]))
        nn = sd.get("neighbours")
        if nn is not None:
            self._check_neighbours(nn, rows.shape[0])
        val = sd.get("neighbour_values") if "neighbours" in sd else None  # (no "neighbours" key at all: no graph, as before the values existed)
        if val is not None:
            if nn is None:
                raise ValueError("GalleryIndex.load_state_dict: neighbour_values without neighbours")
            if not torch.is_tensor(val) or val.dtype != torch.float32 or tuple(val.shape) != tuple(nn.shape):
                raise ValueError("GalleryIndex.load_state_dict: neighbour_values must be a float32 %s tensor like neighbours; got %s" % (
                    list(nn.shape), "%s %s" % (val.dtype, list(val.shape)) if torch.is_tensor(val) else type(val)))
        x = self._check_rows("load_state_dict", rows)
        n = x.shape[0]
        live = sd.get("live")
        if live is not None and (not torch.is_tensor(live) or live.numel() != n):
            raise ValueError("GalleryIndex.load_state_dict: live must hold one entry per row (%d)" % n)
        self._n, self._has_pids, self._dead, self._words_ok, self._gids_ok, self._gtab_ok = 0, None, 0, False, False, False
        self._nn, self._nn_val, self._nn_ok, self._nn_rows = None, None, False, 0
        self._reserve(n, x.device)
        self._rows[:n].copy_(x)
        self._pack_into(0, n)
        pids = sd.get("pids")
        self._has_pids = pids is not None
        if pids is not None:
            self._pids[:n].copy_(torch.as_tensor(pids).to(x.device).long().reshape(-1))
        self._live[:n] = True
        if live is not None:
            self._live[:n].copy_(live.to(x.device).reshape(-1) != 0)
            self._dead = n - int(self._live[:n].sum())
        self._n = n
        if nn is not None:
            self._nn, self._nn_val = _graph_pair(self.capacity, nn.shape[1], x.device, values=val is not None)
            self._nn[:n].copy_(nn.to(x.device))
            self._nn_ok, self._nn_rows = True, n
            if val is not None:
                self._nn_val[:n].copy_(val.to(x.device))
