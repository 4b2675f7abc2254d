"""Retrieval match + rank metric on the HIP library.

Surface of the reference ``lib/data/metrics/evaluation.py``: ``rank(similarity,
q_pids, g_pids, topk, get_mAP)`` (:11-37) and ``evaluation(dataset, predictions,
output_folder, topk, save_data, rerank)`` (:76-173) incl. the k-reciprocal / Jaccard re-rank
(:40-65, row f3).  ``similarity_topk`` is the
fused form for large galleries (config 5): the [Q,G] matrix is never kept, only
per-query top-k (value, index) pairs; with ``world_size > 1`` the gallery is
sharded by rows and the per-shard top-k lists are merged after one all-gather.
``positive_ranks`` / ``rank_from_embeddings`` / ``evaluation(matrix_free=True)`` give
CMC at any k and mAP without the [Q,G] matrix on one rank; the ``*_sharded`` functions
are their explicitly collective forms over a gallery sharded the same way.

One host path: ``_Operands`` describes query rows against a gallery or a shard of one (fp32 rows, pre-split rows, scales,
arithmetic, path, global offset) and holds THE top-k launch sequence (``topk``) and the rank passes (``run``);
``_merge_shard_lists`` is THE merge of per-shard top-k lists; ``_Shards`` lays a gallery out over the ranks - one rank holding the
whole gallery is its one-shard case - and ``_positive_counts`` is THE count pass over it.  ``index.GalleryIndex`` hands its own
pre-split rows and unit scale to the same ``_Operands``.
"""

import logging
import os

import numpy as np
import torch

from . import ops
from .ops import _p, call, stream


def l2_normalize_rows(x):
    y, _ = ops.l2norm_rows(x.contiguous())
    return y


def similarity(text_embed, image_embed):
    """normalise + text @ image.T (evaluation.py:117-120)."""
    return ops.linear(l2_normalize_rows(text_embed), l2_normalize_rows(image_embed))


MAX_TOPK = 16        # trid_topk_rows_f32 and every one-pass top-k (csrc/topk_wave.h TOPK_MAX)
MAX_DEEP_TOPK = 1024  # trid_topk_rows_deep_f32 (csrc/topk_deep.hip TOPK_DEEP_MAX)


def _deep_topk(sim_ptr, ld_q, ld_g, Q, G, k, words, vals, cols, ws=None):
    """THE launch of trid_topk_rows_deep_f32 on torch's current stream.  ws: a uint8 workspace the caller keeps between calls
    (GalleryIndex.shortlist); None: allocated for this call, as rank does for its sort."""
    if ws is None:
        nws = ops.L.load().trid_topk_rows_deep_ws_bytes(Q, G, k, 0)
        if nws <= 0:
            raise RuntimeError("trid_topk_rows_deep_f32: Q = %d, G = %d, k = %d out of range (k must be in [1,%d] and <= G)" % (Q, G, k, MAX_DEEP_TOPK))
        ws = torch.empty(nws, dtype=torch.uint8, device=vals.device)
    call("trid_topk_rows_deep_f32", sim_ptr, ld_q, ld_g, Q, G, k, _p(words), 0, _p(vals), _p(cols), _p(ws), ws.numel(), 0, stream())


def topk_rows(sim, k, mask=None):
    """-> (values [Q,k] f32, columns [Q,k] i64): the exact k best columns of every row of a CUDA fp32 [Q, G] matrix, 1 <= k <= 1024,
    k <= G, value descending then column ascending (trid_topk_rows_deep_f32; the values are the input's bit patterns).  The rows
    need not be contiguous (a view such as ``sim[:, ::2]`` is read in place).  mask: bool / uint8 [G] on the same device, true = the
    column may be returned; a row with fewer than k allowed columns ends in (-inf, -1) slots.  No host read."""
    if not torch.is_tensor(sim) or sim.dim() != 2:
        raise ValueError("textreid_amd.evaluation.topk_rows: expected a [Q, G] tensor")
    if not sim.is_cuda:
        raise RuntimeError("textreid_amd.evaluation.topk_rows runs on the HIP kernel library only (CUDA tensors); no CPU fallback")
    Q, G = sim.shape
    if Q < 1 or k < 1 or k > MAX_DEEP_TOPK or k > G:
        raise ValueError("textreid_amd.evaluation.topk_rows: k must be in [1, %d] and <= G = %d, Q >= 1; got k = %d, Q = %d" % (MAX_DEEP_TOPK, G, k, Q))
    if sim.dtype != torch.float32:
        sim = sim.float()
    ld_q, ld_g = (1 if Q == 1 else sim.stride(0)), (1 if G == 1 else sim.stride(1))
    if not (ld_q >= 1 and ld_g >= 1 and (ld_q >= (G - 1) * ld_g + 1 or ld_g >= (Q - 1) * ld_q + 1)):
        sim = sim.contiguous()  # (an expanded view: its elements alias)
        ld_q, ld_g = G, 1
    dev = sim.device
    words = None
    if mask is not None:
        if not torch.is_tensor(mask) or mask.dtype not in (torch.bool, torch.uint8) or mask.dim() != 1 or mask.shape[0] != G:
            raise ValueError("textreid_amd.evaluation.topk_rows: mask must be a bool or uint8 tensor of shape [G = %d]" % G)
        if mask.device != dev:
            raise ValueError("textreid_amd.evaluation.topk_rows: sim is on %s; got a mask on %s" % (dev, mask.device))
        m = mask.contiguous()
        words = torch.empty((G + 31) // 32, dtype=torch.int32, device=dev)
        call("trid_index_pack_mask_u32", None, _p(m), G, _p(words), words.numel(), stream())
    vals = torch.empty(Q, k, dtype=torch.float32, device=dev)
    cols = torch.empty(Q, k, dtype=torch.int64, device=dev)
    _deep_topk(_p(sim), ld_q, ld_g, Q, G, k, words, vals, cols)
    return vals, cols


def topk_distinct_rows(sim, groups, k, mask=None):
    """-> (values [Q,k] f32, rows [Q,k] i64): the k best DISTINCT groups of every row of a CUDA fp32 [Q, G] matrix, each by its first
    allowed column in the library's order (value descending, then column ascending), 1 <= k <= 1024 - the definition of
    GalleryIndex.search_pids on a given matrix.  groups: an integer tensor [G] (equal = one group).  trid_index_group_best_f32 over
    the table of ``index.group_table(groups)`` (one host read: the group count), then trid_topk_rows_deep_pairs_f32 over max(groups,
    k) slots; a row with fewer than k allowed groups ends in (-inf, -1) slots.  The values are the input's bit patterns; the rows
    need not be contiguous.  mask: bool / uint8 [G] on the same device, true = the column may be returned.  The table, the pair
    buffers and the workspace are allocated per call, as topk_rows does."""
    from .index import group_table

    if not torch.is_tensor(sim) or sim.dim() != 2:
        raise ValueError("textreid_amd.evaluation.topk_distinct_rows: expected a [Q, G] tensor")
    if not sim.is_cuda:
        raise RuntimeError("textreid_amd.evaluation.topk_distinct_rows runs on the HIP kernel library only (CUDA tensors); no CPU fallback")
    Q, G = sim.shape
    if Q < 1 or G < 1 or k < 1 or k > MAX_DEEP_TOPK:
        raise ValueError("textreid_amd.evaluation.topk_distinct_rows: k must be in [1, %d], Q >= 1, G >= 1; got k = %d, Q = %d, G = %d" % (MAX_DEEP_TOPK, k, Q, G))
    groups = torch.as_tensor(groups)
    if groups.dim() != 1 or groups.shape[0] != G or groups.is_floating_point():
        raise ValueError("textreid_amd.evaluation.topk_distinct_rows: groups must be an integer tensor of shape [G = %d]" % G)
    if sim.dtype != torch.float32:
        sim = sim.float()
    ld_q, ld_g = (1 if Q == 1 else sim.stride(0)), (1 if G == 1 else sim.stride(1))
    if not (ld_q >= 1 and ld_g >= 1 and (ld_q >= (G - 1) * ld_g + 1 or ld_g >= (Q - 1) * ld_q + 1)):
        sim = sim.contiguous()  # (an expanded view: its elements alias)
        ld_q, ld_g = G, 1
    dev = sim.device
    words = None
    if mask is not None:
        if not torch.is_tensor(mask) or mask.dtype not in (torch.bool, torch.uint8) or mask.dim() != 1 or mask.shape[0] != G:
            raise ValueError("textreid_amd.evaluation.topk_distinct_rows: mask must be a bool or uint8 tensor of shape [G = %d]" % G)
        if mask.device != dev:
            raise ValueError("textreid_amd.evaluation.topk_distinct_rows: sim is on %s; got a mask on %s" % (dev, mask.device))
        m = mask.contiguous()
        words = torch.empty((G + 31) // 32, dtype=torch.int32, device=dev)
        call("trid_index_pack_mask_u32", None, _p(m), G, _p(words), words.numel(), stream())
    order, starts, n_groups = group_table(groups.to(dev))
    n_slots = max(n_groups, k)
    best_val = torch.empty(Q, n_slots, dtype=torch.float32, device=dev)
    best_row = torch.empty(Q, n_slots, dtype=torch.int32, device=dev)
    call("trid_index_group_best_f32", _p(sim), ld_q, ld_g, Q, G, _p(order), _p(starts), n_groups, n_slots, _p(words), _p(best_val), _p(best_row),
         n_slots, 1, stream())
    nws = ops.L.load().trid_topk_rows_deep_ws_bytes(Q, n_slots, k, 0)
    if nws <= 0:
        raise RuntimeError("trid_topk_rows_deep_pairs_f32: Q = %d, n_slots = %d, k = %d out of range" % (Q, n_slots, k))
    ws = torch.empty(nws, dtype=torch.uint8, device=dev)
    vals = torch.empty(Q, k, dtype=torch.float32, device=dev)
    rows = torch.empty(Q, k, dtype=torch.int64, device=dev)
    call("trid_topk_rows_deep_pairs_f32", _p(best_val), _p(best_row), n_slots, 1, Q, n_slots, k, 0, _p(vals), _p(rows), _p(ws), nws, 0, stream())
    return vals, rows


def rank(similarity, q_pids, g_pids, topk=(1, 5, 10), get_mAP=True):
    """CMC (and mAP) of a given [Q, G] similarity matrix (evaluation.py:11-37).  get_mAP=False keeps max(topk) columns per query:
    up to 16 by trid_topk_rows_f32, up to 1024 by trid_topk_rows_deep_f32, beyond that a slice of the full argsort - one order
    (value descending, then column ascending) on every route."""
    if not similarity.is_cuda:
        raise RuntimeError("textreid_amd.evaluation.rank runs on the HIP kernel library only (CUDA tensors); no CPU fallback")
    dev = similarity.device
    topk_t = torch.as_tensor(topk, dtype=torch.int64, device=dev)
    max_rank = int(max(topk)) if not torch.is_tensor(topk) else int(topk.max())
    sim = similarity.contiguous().float()
    Q, G = sim.shape
    full_sort = get_mAP or max_rank > MAX_DEEP_TOPK
    if full_sort:
        indices = torch.empty(Q, G, dtype=torch.int64, device=dev)
        # rows beyond the in-LDS sort (G > 16384, e.g. ICFG-PEDES i2t) go through a segmented radix sort in a workspace;
        # row batches keep Q*G below the sort's 2^31-item limit
        rows_per = Q if G <= 16384 else max(1, min(Q, ((1 << 31) - 1) // G))
        for q0 in range(0, Q, rows_per):
            nq = min(rows_per, Q - q0)
            nws = ops.L.load().trid_argsort_ws_bytes(nq, G)
            ws = torch.empty(nws, dtype=torch.uint8, device=dev) if nws > 0 else None
            call("trid_argsort_rows_desc_f32", _p(sim[q0:]), G, nq, G, _p(indices[q0:]), _p(ws), nws, stream())
        if not get_mAP:  # (max(topk) beyond the deep select: the first max_rank columns of the same order)
            indices = indices[:, :max_rank].contiguous()
    else:
        vals = torch.empty(Q, max_rank, dtype=torch.float32, device=dev)
        indices = torch.empty(Q, max_rank, dtype=torch.int64, device=dev)
        if max_rank <= MAX_TOPK:
            call("trid_topk_rows_f32", _p(sim), G, Q, G, max_rank, _p(vals), _p(indices), stream())
        else:
            _deep_topk(_p(sim), G, 1, Q, G, max_rank, None, vals, indices)
    return _metrics(indices, q_pids, g_pids, topk_t, get_mAP)


def _rank_outputs(Q, topk_t):
    """(first hit [Q] int32, AP [Q], cmc [len(topk)]) of the rank metric kernels"""
    dev = topk_t.device
    return (torch.empty(Q, dtype=torch.int32, device=dev), torch.empty(Q, dtype=torch.float32, device=dev),
            torch.empty(topk_t.numel(), dtype=torch.float32, device=dev))


def _mean_ap(ap):
    mAP = torch.empty(1, dtype=torch.float32, device=ap.device)
    ops.sum_to(ap, mAP, 100.0 / ap.numel())
    return mAP[0]


def _metrics(indices, q_pids, g_pids, topk_t, get_mAP):
    dev = indices.device
    Q, R = indices.shape
    first, ap, cmc = _rank_outputs(Q, topk_t)
    # (locals: a temporary passed straight into _p() is freed before the next argument is built, and the caching
    # allocator may hand its block to that next temporary - the kernel would then read the wrong ids)
    qp = q_pids.to(dev).long().contiguous()
    gp = g_pids.to(dev).long().contiguous()
    call("trid_rank_metrics", _p(indices), _p(qp), _p(gp),
         Q, R, _p(first), _p(ap), _p(topk_t), topk_t.numel(), _p(cmc), stream())
    if not get_mAP:
        return cmc, indices
    return cmc, _mean_ap(ap), indices


USE_SIM_P16 = os.environ.get("TRID_SIM_P16", "1") != "0"  # retrieval match on pre-split operands (0: the on-the-fly split GEMM, A/B runs)
DEVICE_GATED_FALLBACK = False  # True: the capture-safe form (fall-back passes gated on the device) outside a capture too (tests)
PAIR_CHUNK = 1 << 18  # listed pairs per pair-value launch of the streaming kernel (256 MB of gathered gallery rows)
MAX_P16_ROWS = ((1 << 31) - 1) // 1024  # pre-split rows of 256 (1024 bytes each) the 31-bit byte offsets of the streaming kernels reach


def _sim_precision():
    """Arithmetic of the similarity GEMM: the fp16 two-plane split (half the MFMA work of the bf16 one, same fp32-class
    accuracy) while the library-wide mode is the fp32-class default; it needs the operands' largest magnitudes as
    device scalars (one streaming pass each - the gallery pass is ~1 % of the scoring time)."""
    return 16 if ops.GEMM_PRECISION == 6 and ops.CONV_PRECISION == 16 else ops.GEMM_PRECISION


def _p16_path(prec, C, G):
    """the case the streaming P16 kernels take: fp16-split default arithmetic, C == 256, more rows than the first panel, 31-bit
    offsets"""
    return USE_SIM_P16 and prec == 16 and C == 256 and 8192 < G <= MAX_P16_ROWS


class _Operands:
    """Query rows q and a gallery (or a shard of one) g as the top-k and the rank passes take them.  On the streaming path
    (p16: C == 256 in the fp32-class default arithmetic, see _p16_path) both are split into their fp16 planes ONCE (p16_pack:
    the gallery is written once and scored against every query panel, the queries stay resident in registers); else the fp32
    rows and, for the rank passes, ONE [Q, 8192] panel (ws).  The path and the gallery's scale are decided here from the local
    rows unless the caller imposes them: ga (the scalar the gallery is packed with: the GLOBAL amax of a sharded gallery, the
    unit scale of index.GalleryIndex), g16 (the gallery already packed with ga), p16 (the one path of all shards) and offset
    (the global row of g's row 0)."""

    def __init__(self, q, g, ga=None, p16=None, offset=0, g16=None):
        self.g, self.offset = g, offset
        self.G, self.C = g.shape
        self.prec = _sim_precision()
        self.ga = None if self.prec != 16 else (ops.amax(g) if ga is None else ga)
        self.p16 = _p16_path(self.prec, self.C, self.G) if p16 is None else p16
        self.g16 = self._pack(g, self.ga, torch.empty_like(g)) if self.p16 and g16 is None else g16
        self.q, self.qa, self.q16 = self.queries(q)
        self.Q = q.shape[0]
        self.ws = None

    @staticmethod
    def _pack(x, amax, out):
        n, C = x.shape
        call("trid_p16_pack_f32", _p(x), n, C, C, _p(amax), _p(out), 1, stream())
        return out

    def queries(self, q, qa=None):
        """(rows, their scale, the rows pre-split in zero-padded panels of 32) of query rows in this gallery's arithmetic"""
        if qa is None and self.prec == 16:
            qa = ops.amax(q)
        q16 = self._pack(q, qa, torch.zeros((q.shape[0] + 31) // 32 * 32, self.C, dtype=torch.float32, device=q.device)) if self.p16 else None
        return q, qa, q16

    def topk(self, k, rows=None, out=None):
        """THE fused similarity + top-k launch sequence: (values, GLOBAL rows) [Q, k] of the k largest q @ g.T per query, no
        [Q,G] kept.  rows: (query rows, their scale) other than self.q; out: (values, rows) to write."""
        q, qa, q16 = (self.q, self.qa, self.q16) if rows is None else self.queries(*rows)
        Q, G, dev = q.shape[0], self.G, q.device
        vals, idx = out or (torch.empty(Q, k, dtype=torch.float32, device=dev), torch.empty(Q, k, dtype=torch.int64, device=dev))
        ws = ops.empty((ops.L.load().trid_topk_ws_floats(Q, G, k),), q)
        if not self.p16:
            call("trid_sim_topk_f32", _p(q), _p(self.g), _p(vals), _p(idx), Q, G, self.C, k, self.offset, self.prec, _p(qa), _p(self.ga), _p(ws), stream())
            return vals, idx
        args = (_p(q), _p(self.g), _p(q16), _p(self.g16), _p(vals), _p(idx), Q, G, k, self.offset, _p(qa), _p(self.ga), _p(ws))
        if DEVICE_GATED_FALLBACK or torch.cuda.is_current_stream_capturing():  # (no host read inside a capture: the device-gated fall-back passes)
            call("trid_sim_topk_p16", *args, 0, stream())
            return vals, idx
        call("trid_sim_topk_p16", *args, 1, stream())
        # a candidate list overflowed (adversarially ordered gallery)?  One 4-byte read; the dense passes only then
        flag = ws[ops.L.load().trid_topk_ws_flag_offset(Q, G):][:1].view(torch.int32)
        if int(flag.item()) != 0:
            call("trid_sim_topk_p16", *args, 2, stream())
        return vals, idx

    def run(self, ptr, idx, val, counts, max_list, mode, local=False):
        """One rank pass over a CSR list.  idx: GLOBAL rows in mode 1 (count); mode 0 (pair values) takes rows of THIS g
        (local=True when g is a shard: the pairs it owns, its neighbour list)"""
        NP = idx.numel()
        if NP == 0:
            return
        offset = 0 if local else self.offset
        if self.p16 and mode == 0:
            # pair values: the listed rows are gathered and stream through the counting tile code, PAIR_CHUNK entries at a time
            # (the gathered copy stays small; the kernel's 31-bit offsets allow 2^21 rows): entries a .. b - 1 with the CSR
            # ranges cut to them
            for a in range(0, NP, PAIR_CHUNK):
                b = min(a + PAIR_CHUNK, NP)
                cptr = (ptr.clamp(a, b) - a).contiguous()
                cidx, cval, a16 = idx[a:b], val[a:b], self.g16[idx[a:b]]
                call("trid_rank_stream_p16", _p(self.q16), _p(a16), _p(self.qa), _p(self.ga), _p(cptr), _p(cidx), _p(cval), None, self.Q,
                     b - a, b - a, 0, 0, 0, stream())
        elif self.p16:
            call("trid_rank_stream_p16", _p(self.q16), _p(self.g16), _p(self.qa), _p(self.ga), _p(ptr), _p(idx), _p(val), _p(counts), self.Q,
                 self.G, NP, max_list, offset, 1, stream())
        else:
            if self.ws is None:
                self.ws = ops.empty((ops.L.load().trid_rank_ws_floats(self.Q, self.G),), self.q)
            call("trid_rank_stream_f32", _p(self.q), _p(self.g), _p(ptr), _p(idx), _p(val), _p(counts), self.Q, self.G, self.C, NP, max_list,
                 offset, self.prec, _p(self.qa), _p(self.ga), _p(self.ws), mode, stream())


def _merge_shard_lists(vals, idx):
    """THE shard merge: every rank's top-k lists [Q, k] all-gathered (rank-major), then one row top-k over the W * k candidates
    of a query (ties: the lower candidate, i.e. the lower global row, first) -> (vals, rows), identical on every rank"""
    from .parallel import all_gather_rows

    Q, k = vals.shape
    cand = [all_gather_rows(x).view(-1, Q, k).permute(1, 0, 2).reshape(Q, -1).contiguous() for x in (vals, idx)]
    n = cand[0].shape[1]
    sel = torch.empty(Q, k, dtype=torch.int64, device=vals.device)
    call("trid_topk_rows_f32", _p(cand[0]), n, Q, n, k, _p(vals), _p(sel), stream())
    return vals, torch.gather(cand[1], 1, sel)


def similarity_topk(text_embed, image_embed, k=10, normalize=True):
    """Per-query top-k of text @ image.T without materialising [Q,G]; gallery rows
    sharded across ranks when torch.distributed is initialised (each rank passes
    its OWN shard of image_embed and decides scale and path from it; returned indices are global, rank-major)."""
    from .parallel import all_gather_rows, dp_active, rank as dist_rank

    q = l2_normalize_rows(text_embed) if normalize else text_embed.contiguous()
    g = l2_normalize_rows(image_embed) if normalize else image_embed.contiguous()
    if not dp_active():  # (active: more than one rank, or a forced one-rank group: the RCCL transport test)
        return _Operands(q, g).topk(k)
    sizes = all_gather_rows(torch.tensor([g.shape[0]], dtype=torch.int64, device=q.device))
    return _merge_shard_lists(*_Operands(q, g, offset=int(sizes[: dist_rank()].sum())).topk(k))


def _topk_neighbours(q, g, k):
    """indices [Q,k] of the k largest q @ g.T per row (fused similarity + top-k, no [Q,G] kept)."""
    return _Operands(q, g).topk(k)[1]


def k_reciprocal(q_feats, g_feats, neighbor_num=5, alpha=0.05, base=None):
    """alpha * Jaccard(top-k neighbours of query i, top-k neighbours of gallery j) (+ base):
    the reference's k_reciprocal/jaccard_mat (evaluation.py:40-65; there an O(Q*G) pure-Python
    double loop) as two fused top-k launches and one set-intersection kernel."""
    q, g = q_feats.contiguous(), g_feats.contiguous()
    qnn = _topk_neighbours(q, g, neighbor_num)
    gnn = _topk_neighbours(g, g, neighbor_num)
    Q, G = q.shape[0], g.shape[0]
    out = torch.empty(Q, G, dtype=torch.float32, device=q.device)
    b = base.contiguous() if base is not None else None
    call("trid_jaccard_add_f32", _p(qnn), _p(gnn), _p(b), G, _p(out), Q, G, neighbor_num, float(alpha), stream())
    return out


def _refuse(name, *tensors):
    """what no rank entry point takes: CPU tensors, a capturing stream and - the unsharded ones, which are not collective
    (engine.inference calls evaluation on rank 0 alone) - a process group"""
    from .parallel import dp_active

    for t in tensors:
        if not t.is_cuda:
            raise RuntimeError("textreid_amd.evaluation.%s runs on the HIP kernel library only (CUDA tensors); no CPU fallback" % name)
    if not name.endswith("_sharded") and dp_active():
        raise NotImplementedError("textreid_amd.evaluation.%s is not collective: under a process group call the sharded form "
                                  "%s_sharded on every rank, or run it on one rank" % (name, name))
    if torch.cuda.is_current_stream_capturing():
        # the CSR lists' lengths and the longest list are host values (one pass of the gallery per RANK_PC entries of it)
        raise RuntimeError("textreid_amd.evaluation.%s reads list lengths back to the host and cannot run inside a stream capture" % name)


def _expand_ranges(lo, cnt):
    """entries lo[r] .. lo[r] + cnt[r] - 1 of every range r, concatenated: (range id, entry) - device bookkeeping, no host loop"""
    rid = torch.repeat_interleave(torch.arange(cnt.numel(), device=cnt.device), cnt)
    first = torch.cumsum(cnt, 0) - cnt
    return rid, lo[rid] + (torch.arange(rid.numel(), device=cnt.device) - first[rid])


def _csr(qid, idx, Q, G):
    """unique (query, row) pairs in (query, row) order -> (ptr [Q+1], idx) int64"""
    key = torch.unique(qid * G + idx)  # sorted
    ptr = torch.searchsorted(key, torch.arange(Q + 1, device=key.device) * G)
    return ptr.contiguous(), (key % G).contiguous()


def _positive_list(q_pids, g_pids):
    """CSR list of the gallery rows that carry each query's pid, rows ascending"""
    dev = g_pids.device
    gp, order = torch.sort(g_pids.long())
    qp = q_pids.to(dev).long()
    lo = torch.searchsorted(gp, qp)
    rid, ent = _expand_ranges(lo, torch.searchsorted(gp, qp, right=True) - lo)
    return _csr(rid, order[ent], qp.numel(), gp.numel())


def _neighbour_list(qnn, gnn):
    """CSR list of ALL pairs (q, i) whose neighbour rows share an index: the only ones the Jaccard term moves"""
    Q, n = qnn.shape
    G = gnn.shape[0]
    vals, order = torch.sort(gnn.reshape(-1))
    flat = qnn.reshape(-1)
    lo = torch.searchsorted(vals, flat)
    rid, ent = _expand_ranges(lo, torch.searchsorted(vals, flat, right=True) - lo)
    return _csr(rid // n, order[ent] // n, Q, G)


# ---- the rank passes run over a gallery split by rows into shards (rank-major global order, as similarity_topk takes it), the
# queries replicated; ONE rank holding the whole gallery is the one-shard case.  The *_sharded entry points are explicitly
# collective: EVERY rank calls them (the unsharded ones refuse under a process group).  DESIGN.md section 7e.

GNN_ROWS = 8192  # gallery rows (all ranks together) scored per step of the gallery x gallery neighbour match


def _owner_split(ptr, idx, offset, G_local):
    """the entries of a CSR list of GLOBAL rows that lie in the shard [offset, offset + G_local): (ptr of the sub-list [Q+1], their
    LOCAL rows, their positions in the full list) - device bookkeeping, no host loop"""
    own = (idx >= offset) & (idx < offset + G_local)
    before = torch.cat([own.new_zeros(1, dtype=torch.int64), torch.cumsum(own.long(), 0)])  # owned entries before entry e
    pos = own.nonzero().reshape(-1)
    return before[ptr].contiguous(), (idx[pos] - offset).contiguous(), pos


class _Shards:
    """The layout of the gallery and this rank's share of it.  Collective form: what every rank decides alike before the first
    pass - the shard sizes, this shard's offset, the GLOBAL gallery amax and the path - then this rank's operands (None for an
    empty shard: it joins the collectives and launches no rank kernel).  collective=False: the ONE shard of a rank that holds the
    whole gallery, laid out from host shapes alone (no collective, no host read; the operands decide scale and path from the
    rows).  With one shard (W == 1) no pass joins a collective."""

    def __init__(self, q, g, collective=True):
        from .parallel import group_gather_rows, rank as dist_rank

        self.q, self.g = q, g
        self.Q, self.C = q.shape
        self.G_local = g.shape[0]
        dev = q.device
        self.sizes, ga, p16 = [self.G_local], None, None
        if collective:
            self.sizes = [int(v) for v in group_gather_rows(torch.tensor([self.G_local], dtype=torch.int64, device=dev)).tolist()]
            # ONE scale for every shard: each product then has the bits it has in the one-rank run
            if _sim_precision() == 16:
                mine = ops.amax(g) if self.G_local else torch.zeros(1, dtype=torch.float32, device=dev)
                ga = group_gather_rows(mine.reshape(1)).max().reshape(1)
            # ONE path: the streaming kernel only if every non-empty shard qualifies (two arithmetics would break "a row
            # compares equal to its own duplicate" across a cut)
            p16 = bool(all(_p16_path(_sim_precision(), self.C, n) for n in self.sizes if n))
        self.W, self.r = len(self.sizes), (dist_rank() if len(self.sizes) > 1 else 0)
        self.offset, self.G = sum(self.sizes[: self.r]), sum(self.sizes)
        self.opnd = _Operands(q, g, ga, p16, self.offset) if self.G_local else None
        self.ga, self.p16 = (ga, bool(p16)) if self.opnd is None else (self.opnd.ga, self.opnd.p16)

    def gather_gallery(self, x):
        from .parallel import group_gather_varrows

        return x.contiguous() if self.W == 1 else group_gather_varrows(x, self.sizes)

    def reduce_sum_(self, x):
        from .parallel import group_reduce_sum_

        return x if self.W == 1 else group_reduce_sum_(x)

    def topk(self, qrows, qa, k):
        """global top-k rows [Qn, k] of replicated query rows (qa: their scale, the same on every rank) against the sharded
        gallery: this shard's list (offset -> global rows; fewer than k rows: the rest stays -inf), the lists of all shards
        merged (ties: lower global row first)"""
        Qn, dev = qrows.shape[0], qrows.device
        vals = torch.full((Qn, k), float("-inf"), dtype=torch.float32, device=dev)
        idx = torch.zeros(Qn, k, dtype=torch.int64, device=dev)
        o = self.opnd
        if o is not None:
            kk = min(k, o.G)
            out = (vals, idx) if kk == k else (torch.empty(Qn, kk, dtype=torch.float32, device=dev), torch.empty(Qn, kk, dtype=torch.int64, device=dev))
            o.topk(kk, (qrows, qa), out)
            if kk != k:
                vals[:, :kk], idx[:, :kk] = out
        return idx if self.W == 1 else _merge_shard_lists(vals, idx)[1]

    def neighbours(self, n):
        """(qnn [Q, n], gnn_local [G_local, n]), GLOBAL rows: the queries' and this shard's rows' nearest gallery rows.  The
        gallery x gallery match goes GNN_ROWS rows at a time (every rank's next rows, all-gathered): nothing grows with
        G_total x 8192"""
        from .parallel import group_gather_rows

        if self.G < n:
            raise ValueError("the re-rank needs at least neighbor_num gallery rows")
        dev = self.q.device
        qnn = self.topk(self.q, self.opnd.qa if self.opnd is not None else None, n)
        gnn = torch.empty(self.G_local, n, dtype=torch.int64, device=dev)
        ch = max(256, GNN_ROWS // self.W)
        for c0 in range(0, max(self.sizes), ch):
            m = min(max(self.G_local - c0, 0), ch)
            rows = torch.zeros(ch, self.C, dtype=torch.float32, device=dev)
            rows[:m] = self.g[c0:c0 + m]
            idx = self.topk(group_gather_rows(rows), self.ga, n)  # (gallery rows as queries: the gallery's scale)
            gnn[c0:c0 + m] = idx[self.r * ch:self.r * ch + m]
        return qnn, gnn


def _positive_counts(sh, q_pids, g_pids_local, qnn, gnn_local, alpha):
    """THE count pass -> (pos_ptr, pos_idx GLOBAL rows, counts [NP] int32: the rows that precede each positive), identical on
    every rank.  With one shard the shard owns every listed row: the pair values go straight into thr and nothing is reduced."""
    dev = sh.q.device
    Q, one = sh.Q, sh.W == 1
    # the global list, identical on every rank
    ptr, idx = _positive_list(q_pids, sh.gather_gallery(g_pids_local.to(dev).long()))
    NP = idx.numel()
    counts = torch.zeros(max(NP, 1), dtype=torch.int32, device=dev)
    thr = (torch.empty if one else torch.zeros)(max(NP, 1), dtype=torch.float32, device=dev)
    if NP == 0:
        return ptr, idx, counts[:0]
    max_list = int((ptr[1:] - ptr[:-1]).max())
    o = sh.opnd
    if qnn is not None:
        n = qnn.shape[1]
        qnn = qnn.long().contiguous()
        gnn_local = gnn_local.long().contiguous()
    # pair values: the owner of a row computes its entries (with the re-rank: plus their Jaccard term, from its own gnn rows);
    # the others leave +0.0 there, so the SUM is exact
    if o is not None:
        if one:
            own_ptr, own_idx, own_val = ptr, idx, thr
        else:
            own_ptr, own_idx, own_pos = _owner_split(ptr, idx, sh.offset, sh.G_local)
            own_val = torch.empty(own_pos.numel(), dtype=torch.float32, device=dev)
        if own_idx.numel():
            o.run(own_ptr, own_idx, own_val, None, 0, 0, local=True)
            if qnn is not None:
                call("trid_rank_pairs_jaccard_f32", _p(own_ptr), _p(own_idx), _p(own_val), _p(qnn), _p(gnn_local), n, float(alpha), Q,
                     own_idx.numel(), stream())
            if not one:
                thr[own_pos] = own_val
    sh.reduce_sum_(thr)
    # this shard's share of every count: the global list, the reduced thresholds, the tie rule on offset + i
    if o is not None:
        o.run(ptr, idx, thr, counts, max_list, 1)
        if qnn is not None:
            nb_ptr, nb_idx = _neighbour_list(qnn, gnn_local)  # (pairs (q, LOCAL row i))
            NB = nb_idx.numel()
            if NB:
                nb_val = torch.empty(NB, dtype=torch.float32, device=dev)
                o.run(nb_ptr, nb_idx, nb_val, None, 0, 0, local=True)
                call("trid_rank_rerank_fix_shard", _p(ptr), _p(idx), _p(thr), _p(counts), _p(nb_ptr), _p(nb_idx), _p(nb_val), _p(qnn),
                     _p(gnn_local), n, float(alpha), Q, NB, sh.offset, stream())
    sh.reduce_sum_(counts)
    return ptr, idx, counts


def _rows(x, normalize):
    if normalize and x.shape[0]:
        return l2_normalize_rows(x)
    return x.contiguous().float()


def _positive_ranks(name, collective, q, g, q_pids, g_pids, qnn, gnn, alpha, normalize):
    _refuse(name, q, g)
    if (qnn is None) != (gnn is None):
        raise ValueError("%s: qnn and %s go together" % (name, "gnn_local" if collective else "gnn"))
    ptr, idx, counts = _positive_counts(_Shards(_rows(q, normalize), _rows(g, normalize), collective), q_pids, g_pids, qnn, gnn, alpha)
    return ptr, idx, counts.long() + 1


def _rank_from_embeddings(name, collective, text_embed, image_embed, q_pids, g_pids, topk, get_mAP, normalize, rerank, neighbor_num, alpha):
    _refuse(name, text_embed, image_embed)
    q, g = _rows(text_embed, normalize), _rows(image_embed, normalize)
    qnn = gnn = None
    if rerank and not collective:  # (the whole gallery on this rank: one gallery x gallery launch, done before the rank operands exist)
        qnn, gnn = _topk_neighbours(q, g, neighbor_num), _topk_neighbours(g, g, neighbor_num)
    sh = _Shards(q, g, collective)
    if rerank and collective:
        qnn, gnn = sh.neighbours(neighbor_num)
    ptr, idx, counts = _positive_counts(sh, q_pids, g_pids, qnn, gnn, alpha)
    topk_t = torch.as_tensor(topk, dtype=torch.int64, device=text_embed.device)
    first, ap, cmc = _rank_outputs(sh.Q, topk_t)
    call("trid_rank_finalize", _p(counts), _p(ptr), sh.Q, _p(first), _p(ap), _p(topk_t), topk_t.numel(), _p(cmc), stream())
    return (cmc, _mean_ap(ap)) if get_mAP else (cmc,)


def positive_ranks(q, g, q_pids, g_pids, qnn=None, gnn=None, alpha=0.05, normalize=False):
    """Overall rank (1-based, int64, CSR order) of every relevant gallery row of every query under s'(q,i) = q_i . g_i +
    alpha * Jaccard(qnn[q], gnn[i]) (no neighbours: the plain similarity), descending, ties lower index first - what a full
    argsort of the [Q,G] matrix would give (evaluation.py:14), without the matrix.  -> (pos_ptr [Q+1], pos_idx [NP], ranks [NP])"""
    return _positive_ranks("positive_ranks", False, q, g, q_pids, g_pids, qnn, gnn, alpha, normalize)


def positive_ranks_sharded(q, g_local, q_pids, g_pids_local, qnn=None, gnn_local=None, alpha=0.05, normalize=False):
    """positive_ranks over a gallery sharded by rows: COLLECTIVE over the default process group (every rank calls it; one rank:
    the unsharded result).  q, q_pids (and qnn) are replicated; g_local, g_pids_local (and gnn_local, rows of GLOBAL neighbour
    indices) are this rank's rows, rank-major global order; shard sizes may differ and may be 0.
    -> (pos_ptr [Q+1], pos_idx [NP] GLOBAL rows, ranks [NP]), identical on every rank"""
    return _positive_ranks("positive_ranks_sharded", True, q, g_local, q_pids, g_pids_local, qnn, gnn_local, alpha, normalize)


def rank_from_embeddings(text_embed, image_embed, q_pids, g_pids, topk=(1, 5, 10), get_mAP=True, normalize=True, rerank=False,
                         neighbor_num=5, alpha=0.05):
    """rank() (evaluation.py:11-37) from the embeddings: CMC at any k and mAP from the ranks of the relevant rows; with rerank the
    k-reciprocal term (evaluation.py:40-65) is part of the compared value.  No [Q,G] tensor.  -> (cmc, mAP) or (cmc,)"""
    return _rank_from_embeddings("rank_from_embeddings", False, text_embed, image_embed, q_pids, g_pids, topk, get_mAP, normalize, rerank,
                                 neighbor_num, alpha)


def rank_from_embeddings_sharded(text_embed, image_embed_local, q_pids, g_pids_local, topk=(1, 5, 10), get_mAP=True, normalize=True,
                                 rerank=False, neighbor_num=5, alpha=0.05):
    """rank_from_embeddings over a gallery sharded by rows (layout and collectivity as positive_ranks_sharded); the neighbour
    lists of the re-rank come from the sharded top-k.  -> (cmc, mAP) or (cmc,), identical on every rank"""
    return _rank_from_embeddings("rank_from_embeddings_sharded", True, text_embed, image_embed_local, q_pids, g_pids_local, topk, get_mAP,
                                 normalize, rerank, neighbor_num, alpha)


def _four_tables(table, rerank):
    """{"i2t", "t2i"[, "re-i2t", "re-t2i"]: table(direction, re) -> (cmc, mAP or None)} in the order evaluation logs them"""
    todo = [("i2t", False), ("t2i", False), ("i2t", True), ("t2i", True)] if rerank else [("t2i", False), ("i2t", False)]
    return {("re-" if re else "") + d: table(d, re) for d, re in todo}


def _embedding_tables(rank_fn, sides, topk, rerank):
    """the tables from rank_from_embeddings[_sharded]; sides: {direction: (queries, gallery, q_pids, g_pids)}, rows normalised"""

    def table(d, re):
        r = rank_fn(*sides[d], topk, get_mAP=rerank, normalize=False, rerank=re)
        return (r[0], r[1] if rerank else None)

    return _four_tables(table, rerank)


def tables_sharded(image_local, image_pid_local, text_local, text_pid_local, topk=(1, 5, 10), rerank=True):
    """The tables evaluation(matrix_free=True) leaves in evaluation.last_results, from L2-normalised image and text rows that
    are BOTH sharded over the ranks (collective): per direction the query side is all-gathered and replicated, the gallery side
    stays sharded.  -> {"t2i", "i2t"[, "re-t2i", "re-i2t"]: (cmc, mAP or None)}"""
    from .parallel import group_gather_rows, group_gather_varrows

    _refuse("tables_sharded", image_local, text_local)
    dev = image_local.device

    def whole(x):
        sizes = [int(v) for v in group_gather_rows(torch.tensor([x.shape[0]], dtype=torch.int64, device=dev)).tolist()]
        return group_gather_varrows(x.contiguous(), sizes)

    image_local, text_local = image_local.contiguous().float(), text_local.contiguous().float()
    image_pid_local, text_pid_local = image_pid_local.to(dev).long(), text_pid_local.to(dev).long()
    image_all, image_pid_all = whole(image_local), whole(image_pid_local)
    text_all, text_pid_all = whole(text_local), whole(text_pid_local)
    sides = {"i2t": (image_all, text_local, image_pid_all, text_pid_local), "t2i": (text_all, image_local, text_pid_all, image_pid_local)}
    return _embedding_tables(rank_from_embeddings_sharded, sides, topk, rerank)


def get_unique(image_ids):
    keep = {}
    for i, image_id in enumerate(image_ids):
        keep.setdefault(image_id, i)
    return torch.tensor(list(keep.values()))


def _gather_predictions(dataset, predictions):
    """-> (image rows [unique images, C], their pids, text rows [captions, C], their pids), rows L2-normalised (evaluation.py:98-120)"""
    image_ids, pids, image_global, text_global = [], [], [], []
    for idx, prediction in predictions.items():
        image_id, pid = dataset.get_id_info(idx)
        image_ids.append(image_id)
        pids.append(pid)
        image_global.append(prediction[0])
        text_global.append(prediction[1])
    dev = image_global[0].device
    text_pid = torch.tensor(pids, device=dev)
    keep = get_unique(image_ids).to(dev)
    image_global = l2_normalize_rows(torch.stack(image_global, dim=0)[keep])
    return image_global, text_pid[keep], l2_normalize_rows(torch.stack(text_global, dim=0)), text_pid


def _tables_matrix_free(dataset, predictions, output_folder, topk, save_data, rerank, logger):
    embed_dir = os.path.join(output_folder, "inference_embed.npz") if output_folder else None
    if predictions is None:
        data = np.load(embed_dir)
        logger.info("Load inference embeddings from %s", embed_dir)
        dev = torch.device("cuda")
        image_pid = torch.as_tensor(data["image_pid"]).to(dev)
        text_pid = torch.as_tensor(data["text_pid"]).to(dev)
        image_global = torch.as_tensor(data["image_embed"]).float().to(dev).contiguous()
        text_global = torch.as_tensor(data["text_embed"]).float().to(dev).contiguous()
    else:
        image_global, image_pid, text_global, text_pid = _gather_predictions(dataset, predictions)
        if save_data and embed_dir:
            np.savez(embed_dir, image_pid=image_pid.cpu().numpy(), text_pid=text_pid.cpu().numpy(),
                     image_embed=image_global.cpu().numpy(), text_embed=text_global.cpu().numpy())
    sides = {"i2t": (image_global, text_global, image_pid, text_pid), "t2i": (text_global, image_global, text_pid, image_pid)}
    return _embedding_tables(rank_from_embeddings, sides, topk, rerank)


def _tables_matrix(dataset, predictions, output_folder, topk, save_data, rerank, logger):
    data_dir = os.path.join(output_folder, "inference_data.npz") if output_folder else None
    dev = torch.device("cuda")
    rtn = rvn = None
    if predictions is None:
        # `test_net.py --load-result`: metrics from the arrays a previous run saved (evaluation.py:87-96)
        data = np.load(data_dir)
        logger.info("Load inference data from %s", data_dir)
        image_pid = torch.as_tensor(data["image_pid"]).to(dev)
        text_pid = torch.as_tensor(data["text_pid"]).to(dev)
        sim = torch.as_tensor(data["similarity"]).float().to(dev).contiguous()
        if rerank:
            rvn = torch.as_tensor(data["rvn_mat"]).float().to(dev)
            rtn = torch.as_tensor(data["rtn_mat"]).float().to(dev)
    else:
        image_global, image_pid, text_global, text_pid = _gather_predictions(dataset, predictions)
        sim = ops.linear(text_global, image_global)  # [texts, images]
        if rerank:
            rtn = k_reciprocal(image_global, text_global)  # [images, texts] (evaluation.py:122-124)
            rvn = k_reciprocal(text_global, image_global)  # [texts, images]
        if save_data and data_dir:
            arrays = dict(image_pid=image_pid.cpu().numpy(), text_pid=text_pid.cpu().numpy(), similarity=sim.cpu().numpy())
            if rerank:
                arrays.update(rvn_mat=rvn.cpu().numpy(), rtn_mat=rtn.cpu().numpy())
            np.savez(data_dir, **arrays)
    mats = {("t2i", False): sim, ("i2t", False): sim.t().contiguous()}
    if rerank:
        ones = torch.ones(3, device=sim.device)
        rtn, rvn = rtn.contiguous(), rvn.contiguous()
        for d, nn in (("i2t", rtn), ("t2i", rvn)):  # rtn_mat + similarity.t(), rvn_mat + similarity
            mats[d, True] = torch.empty_like(nn)
            call("trid_axpby3_f32", _p(mats[d, True]), _p(nn), _p(mats[d, False]), None, _p(ones), nn.numel(), stream())
    pids = {"i2t": (image_pid, text_pid), "t2i": (text_pid, image_pid)}

    def table(d, re):
        r = rank(mats[d, re], *pids[d], topk, get_mAP=rerank)
        return (r[0], r[1] if rerank else None)

    return _four_tables(table, rerank)


def evaluation(dataset, predictions, output_folder, topk, save_data=True, rerank=True, matrix_free=False):
    """matrix_free: the four tables from rank_from_embeddings - no [Q,G] tensor is made; save_data then keeps the normalised
    embeddings and pids (inference_embed.npz), which predictions=None reads back."""
    logger = logging.getLogger("PersonSearch.inference")
    tables = _tables_matrix_free if matrix_free else _tables_matrix
    results = tables(dataset, predictions, output_folder, topk, save_data, rerank, logger)
    if rerank:
        for k, (cmc, mAP) in results.items():
            logger.info("%-7s topk %s cmc %s mAP %.3f", k, list(topk), [round(float(c), 3) for c in cmc], float(mAP))
    else:
        logger.info("topk %s  t2i %s  i2t %s", list(topk), results["t2i"][0].tolist(), results["i2t"][0].tolist())
    evaluation.last_results = results
    return results["t2i"][0][0]
