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


def rank(similarity, q_pids, g_pids, topk=(1, 5, 10), get_mAP=True):
    if not similarity.is_cuda:
        raise RuntimeError("textreid_amd.evaluation.rank runs on the HIP kernel library only (CUDA tensors); no CPU fallback")
    dev = similarity.device
    topk_t = torch.as_tensor(topk, dtype=torch.int64, device=dev)
    max_rank = int(max(topk)) if not torch.is_tensor(topk) else int(topk.max())
    sim = similarity.contiguous().float()
    Q, G = sim.shape
    if get_mAP:
        indices = torch.empty(Q, G, dtype=torch.int64, device=dev)
        # rows beyond the in-LDS sort (G > 16384, e.g. ICFG-PEDES i2t) go through a segmented radix sort in a workspace;
        # row batches keep Q*G below the sort's 2^31-item limit
        rows_per = Q if G <= 16384 else max(1, min(Q, ((1 << 31) - 1) // G))
        for q0 in range(0, Q, rows_per):
            nq = min(rows_per, Q - q0)
            nws = ops.L.load().trid_argsort_ws_bytes(nq, G)
            ws = torch.empty(nws, dtype=torch.uint8, device=dev) if nws > 0 else None
            call("trid_argsort_rows_desc_f32", _p(sim[q0:]), G, nq, G, _p(indices[q0:]), _p(ws), nws, stream())
    else:
        vals = torch.empty(Q, max_rank, dtype=torch.float32, device=dev)
        indices = torch.empty(Q, max_rank, dtype=torch.int64, device=dev)
        call("trid_topk_rows_f32", _p(sim), G, Q, G, max_rank, _p(vals), _p(indices), stream())
    return _metrics(indices, q_pids, g_pids, topk_t, get_mAP)


def _metrics(indices, q_pids, g_pids, topk_t, get_mAP):
    dev = indices.device
    Q, R = indices.shape
    first = torch.empty(Q, dtype=torch.int32, device=dev)
    ap = torch.empty(Q, dtype=torch.float32, device=dev)
    cmc = torch.empty(topk_t.numel(), dtype=torch.float32, device=dev)
    # (locals: a temporary passed straight into _p() is freed before the next argument is built, and the caching
    # allocator may hand its block to that next temporary - the kernel would then read the wrong ids)
    qp = q_pids.to(dev).long().contiguous()
    gp = g_pids.to(dev).long().contiguous()
    call("trid_rank_metrics", _p(indices), _p(qp), _p(gp),
         Q, R, _p(first), _p(ap), _p(topk_t), topk_t.numel(), _p(cmc), stream())
    if not get_mAP:
        return cmc, indices
    mAP = torch.empty(1, dtype=torch.float32, device=dev)
    ops.sum_to(ap, mAP, 100.0 / Q)
    return cmc, mAP[0], indices


def _sim_precision(q, g, ga=None):
    """Arithmetic of the similarity GEMM: the fp16 two-plane split (half the MFMA work of the bf16 one, same fp32-class
    accuracy) while the library-wide mode is the fp32-class default; it needs the operands' largest magnitudes as
    device scalars (one streaming pass each - the gallery pass is ~1 % of the scoring time; ga: the gallery's scalar, already known)."""
    if ops.GEMM_PRECISION != 6 or ops.CONV_PRECISION != 16:
        return ops.GEMM_PRECISION, None, None
    return 16, ops.amax(q), (ops.amax(g) if ga is None else ga)


USE_SIM_P16 = os.environ.get("TRID_SIM_P16", "1") != "0"  # retrieval match on pre-split operands (0: the on-the-fly split GEMM, A/B runs)
DEVICE_GATED_FALLBACK = False  # True: the capture-safe form (fall-back passes gated on the device) outside a capture too (tests)


def _sim_topk_call(q, g, vals, idx, k, offset, ws, g16=None, ga=None):
    """The fused similarity + top-k launch sequence.  g16 / ga: the gallery already pre-split and the scalar it was packed with
    (index.GalleryIndex holds both); by default the gallery is measured and packed here.  C == 256 embeddings in the fp32-class default arithmetic: the gallery (written
    once, scored against every query panel) and the queries are split into their fp16 planes ONCE (p16_pack) and the
    admission-filter pass runs on the streaming kernel with the queries resident in registers (trid_sim_topk_p16)."""
    Q, C = q.shape
    G = g.shape[0]
    if (g16 is None) != (ga is None):
        raise ValueError("_sim_topk_call: g16 and ga go together")
    prec, qa, ga = _sim_precision(q, g, ga)
    if USE_SIM_P16 and prec == 16 and C == 256 and G > 8192 and G * 1024 < (1 << 31):
        q16 = torch.zeros((Q + 31) // 32 * 32, C, dtype=torch.float32, device=q.device)
        call("trid_p16_pack_f32", _p(q), Q, C, C, _p(qa), _p(q16), 1, stream())
        if g16 is None:
            g16 = torch.empty_like(g)
            call("trid_p16_pack_f32", _p(g), G, C, C, _p(ga), _p(g16), 1, stream())
        if DEVICE_GATED_FALLBACK or torch.cuda.is_current_stream_capturing():  # (no host read inside a capture: the device-gated fall-back passes)
            call("trid_sim_topk_p16", _p(q), _p(g), _p(q16), _p(g16), _p(vals), _p(idx), Q, G, k, offset, _p(qa), _p(ga), _p(ws), 0, stream())
            return
        call("trid_sim_topk_p16", _p(q), _p(g), _p(q16), _p(g16), _p(vals), _p(idx), Q, G, k, offset, _p(qa), _p(ga), _p(ws), 1, stream())
        # a candidate list overflowed (adversarially ordered gallery)?  One 4-byte read; the dense passes only then
        flag = ws[ops.L.load().trid_topk_ws_flag_offset(Q, G):][:1].view(torch.int32)
        if int(flag.item()) != 0:
            call("trid_sim_topk_p16", _p(q), _p(g), _p(q16), _p(g16), _p(vals), _p(idx), Q, G, k, offset, _p(qa), _p(ga), _p(ws), 2, stream())
        return
    call("trid_sim_topk_f32", _p(q), _p(g), _p(vals), _p(idx), Q, G, C, k, offset, prec, _p(qa), _p(ga), _p(ws), stream())


def similarity_topk(text_embed, image_embed, k=10, normalize=True):
    """Per-query top-k of text @ image.T without materialising [Q,G]; gallery rows
    sharded across ranks when torch.distributed is initialised (each rank passes
    its OWN shard of image_embed; returned indices are global, rank-major)."""
    from .parallel import rank as dist_rank, world_size

    q = l2_normalize_rows(text_embed) if normalize else text_embed.contiguous()
    g = l2_normalize_rows(image_embed) if normalize else image_embed.contiguous()
    Q, C = q.shape
    G = g.shape[0]
    W = world_size()
    vals = torch.empty(Q, k, dtype=torch.float32, device=q.device)
    idx = torch.empty(Q, k, dtype=torch.int64, device=q.device)
    ws = ops.empty((ops.L.load().trid_topk_ws_floats(Q, G, k),), q)
    offset = 0
    from .parallel import dp_active

    dp = dp_active()  # more than one rank (or a forced one-rank group: the RCCL transport test)
    if dp:
        from .parallel import all_gather_rows

        sizes = all_gather_rows(torch.tensor([G], dtype=torch.int64, device=q.device))
        offset = int(sizes[: dist_rank()].sum())
    _sim_topk_call(q, g, vals, idx, k, offset, ws)
    if not dp:
        return vals, idx
    # per-shard lists -> every rank: [W*Q, k] rank-major, then one row top-k over the W*k candidates
    av = all_gather_rows(vals).view(W, Q, k)
    ai = all_gather_rows(idx).view(W, Q, k)
    cand_v = av.permute(1, 0, 2).reshape(Q, W * k).contiguous()
    cand_i = ai.permute(1, 0, 2).reshape(Q, W * k).contiguous()
    sel = torch.empty(Q, k, dtype=torch.int64, device=q.device)
    call("trid_topk_rows_f32", _p(cand_v), W * k, Q, W * k, k, _p(vals), _p(sel), stream())
    return vals, torch.gather(cand_i, 1, sel)


def _topk_neighbours(q, g, k):
    """indices [Q,k] of the k largest q @ g.T per row (fused similarity + top-k, no [Q,G] kept)."""
    Q, C = q.shape
    G = g.shape[0]
    vals = torch.empty(Q, k, dtype=torch.float32, device=q.device)
    idx = torch.empty(Q, k, dtype=torch.int64, device=q.device)
    ws = ops.empty((ops.L.load().trid_topk_ws_floats(Q, G, k),), q)
    _sim_topk_call(q, g, vals, idx, k, 0, ws)
    return idx


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
    from .parallel import dp_active

    for t in tensors:
        if not t.is_cuda:
            raise RuntimeError("textreid_amd.evaluation.%s runs on the HIP kernel library only (CUDA tensors); no CPU fallback" % name)
    if dp_active():
        raise NotImplementedError("textreid_amd.evaluation.%s: the sharded form (all-gather of the thresholds, SUM-reduce of the "
                                  "counts over the gallery shards) is not built; run it on one rank" % name)
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


def _p16_path(prec, C, G):
    """the case the streaming P16 kernels take (as _sim_topk_call): fp16-split default arithmetic, C == 256, more rows than the
    first panel, 31-bit offsets"""
    return USE_SIM_P16 and prec == 16 and C == 256 and G > 8192 and G * 1024 < (1 << 31)


PAIR_CHUNK = 1 << 18  # listed pairs per pair-value launch of the streaming kernel (256 MB of gathered gallery rows)


class _RankOperands:
    """q and g as the rank passes take them: pre-split once for the streaming kernel (the case _sim_topk_call runs on it), else
    the fp32 rows and ONE [Q, 8192] panel.  The sharded form hands in what it decided over ALL shards: ga (the GLOBAL gallery
    amax the local rows are packed with), p16 (the path) and offset (the global index of g's row 0)."""

    def __init__(self, q, g, ga=None, p16=None, offset=0):
        self.q, self.g = q, g
        self.Q, self.C = q.shape
        self.G = g.shape[0]
        self.offset = offset
        self.prec, self.qa, self.ga = _sim_precision(q, g, ga)
        self.p16 = _p16_path(self.prec, self.C, self.G) if p16 is None else p16
        if self.p16:
            self.q16 = torch.zeros((self.Q + 31) // 32 * 32, self.C, dtype=torch.float32, device=q.device)
            call("trid_p16_pack_f32", _p(q), self.Q, self.C, self.C, _p(self.qa), _p(self.q16), 1, stream())
            self.g16 = torch.empty_like(g)
            call("trid_p16_pack_f32", _p(g), self.G, self.C, self.C, _p(self.ga), _p(self.g16), 1, stream())
        else:
            self.ws = ops.empty((ops.L.load().trid_rank_ws_floats(self.Q, self.G),), q)

    def run(self, ptr, idx, val, counts, max_list, mode, local=False):
        """idx: GLOBAL rows in mode 1; mode 0 takes rows of THIS g (local=True when g is a shard: the pairs it owns, its
        neighbour list)"""
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
            call("trid_rank_stream_f32", _p(self.q), _p(self.g), _p(ptr), _p(idx), _p(val), _p(counts), self.Q, self.G, self.C, NP, max_list,
                 offset, self.prec, _p(self.qa), _p(self.ga), _p(self.ws), mode, stream())


def _positive_counts(q, g, q_pids, g_pids, qnn, gnn, alpha):
    dev = q.device
    Q, G = q.shape[0], g.shape[0]
    ptr, idx = _positive_list(q_pids, g_pids.to(dev))
    NP = idx.numel()
    counts = torch.zeros(max(NP, 1), dtype=torch.int32, device=dev)
    thr = torch.empty(max(NP, 1), dtype=torch.float32, device=dev)
    if NP == 0:
        return ptr, idx, counts[:0], thr[:0]
    opnd = _RankOperands(q, g)
    max_list = int((ptr[1:] - ptr[:-1]).max())
    opnd.run(ptr, idx, thr, None, 0, 0)
    if qnn is not None:
        n = qnn.shape[1]
        qnn, gnn = qnn.long().contiguous(), gnn.long().contiguous()
        call("trid_rank_pairs_jaccard_f32", _p(ptr), _p(idx), _p(thr), _p(qnn), _p(gnn), n, float(alpha), Q, NP, stream())
    opnd.run(ptr, idx, thr, counts, max_list, 1)
    if qnn is not None:
        nb_ptr, nb_idx = _neighbour_list(qnn, gnn)
        NB = nb_idx.numel()
        if NB:
            nb_val = torch.empty(NB, dtype=torch.float32, device=dev)
            opnd.run(nb_ptr, nb_idx, nb_val, None, 0, 0)
            call("trid_rank_rerank_fix", _p(ptr), _p(idx), _p(thr), _p(counts), _p(nb_ptr), _p(nb_idx), _p(nb_val), _p(qnn), _p(gnn), n,
                 float(alpha), Q, NB, stream())
    return ptr, idx, counts, thr


def positive_ranks(q, g, q_pids, g_pids, qnn=None, gnn=None, alpha=0.05, normalize=False):
    """Overall rank (1-based, int64, CSR order) of every relevant gallery row of every query under s'(q,i) = q_i . g_i +
    alpha * Jaccard(qnn[q], gnn[i]) (no neighbours: the plain similarity), descending, ties lower index first - what a full
    argsort of the [Q,G] matrix would give (evaluation.py:14), without the matrix.  -> (pos_ptr [Q+1], pos_idx [NP], ranks [NP])"""
    _refuse("positive_ranks", q, g)
    if (qnn is None) != (gnn is None):
        raise ValueError("positive_ranks: qnn and gnn go together")
    q = l2_normalize_rows(q) if normalize else q.contiguous().float()
    g = l2_normalize_rows(g) if normalize else g.contiguous().float()
    ptr, idx, counts, _ = _positive_counts(q, g, q_pids, g_pids, qnn, gnn, alpha)
    return ptr, idx, counts.long() + 1


def rank_from_embeddings(text_embed, image_embed, q_pids, g_pids, topk=(1, 5, 10), get_mAP=True, normalize=True, rerank=False,
                         neighbor_num=5, alpha=0.05):
    """rank() (evaluation.py:11-37) from the embeddings: CMC at any k and mAP from the ranks of the relevant rows; with rerank the
    k-reciprocal term (evaluation.py:40-65) is part of the compared value.  No [Q,G] tensor.  -> (cmc, mAP) or (cmc,)"""
    _refuse("rank_from_embeddings", text_embed, image_embed)
    dev = text_embed.device
    q = l2_normalize_rows(text_embed) if normalize else text_embed.contiguous().float()
    g = l2_normalize_rows(image_embed) if normalize else image_embed.contiguous().float()
    qnn = gnn = None
    if rerank:
        qnn = _topk_neighbours(q, g, neighbor_num)
        gnn = _topk_neighbours(g, g, neighbor_num)
    ptr, idx, counts, _ = _positive_counts(q, g, q_pids, g_pids, qnn, gnn, alpha)
    Q = q.shape[0]
    topk_t = torch.as_tensor(topk, dtype=torch.int64, device=dev)
    first = torch.empty(Q, dtype=torch.int32, device=dev)
    ap = torch.empty(Q, dtype=torch.float32, device=dev)
    cmc = torch.empty(topk_t.numel(), dtype=torch.float32, device=dev)
    call("trid_rank_finalize", _p(counts), _p(ptr), Q, _p(first), _p(ap), _p(topk_t), topk_t.numel(), _p(cmc), stream())
    if not get_mAP:
        return (cmc,)
    mAP = torch.empty(1, dtype=torch.float32, device=dev)
    ops.sum_to(ap, mAP, 100.0 / Q)
    return cmc, mAP[0]


# ---- the sharded form: the gallery split by rows over the ranks (rank-major global order, as similarity_topk takes it), the
# queries replicated.  Explicitly collective: EVERY rank calls these (the unsharded entry points above keep refusing under a
# process group - engine.inference calls evaluation on rank 0 alone).  DESIGN.md section 7e.

GNN_ROWS = 8192  # gallery rows (all ranks together) scored per step of the gallery x gallery neighbour match


def _refuse_sharded(name, *tensors):
    for t in tensors:
        if not t.is_cuda:
            raise RuntimeError("textreid_amd.evaluation.%s runs on the HIP kernel library only (CUDA tensors); no CPU fallback" % name)
    if torch.cuda.is_current_stream_capturing():
        raise RuntimeError("textreid_amd.evaluation.%s reads list lengths back to the host and cannot run inside a stream capture" % name)


def _owner_split(ptr, idx, offset, G_local):
    """the entries of a CSR list of GLOBAL rows that lie in the shard [offset, offset + G_local): (ptr of the sub-list [Q+1], their
    LOCAL rows, their positions in the full list) - device bookkeeping, no host loop"""
    own = (idx >= offset) & (idx < offset + G_local)
    before = torch.cat([own.new_zeros(1, dtype=torch.int64), torch.cumsum(own.long(), 0)])  # owned entries before entry e
    pos = own.nonzero().reshape(-1)
    return before[ptr].contiguous(), (idx[pos] - offset).contiguous(), pos


class _Shards:
    """What every rank decides alike before the first pass: the shard sizes, this shard's offset, the GLOBAL gallery amax and
    the path; then this rank's operands (None for an empty shard: it joins the collectives and launches no rank kernel)."""

    def __init__(self, q, g):
        from .parallel import group_gather_rows, rank as dist_rank

        self.q, self.g = q, g
        self.Q, self.C = q.shape
        self.G_local = g.shape[0]
        dev = q.device
        self.sizes = [int(v) for v in group_gather_rows(torch.tensor([self.G_local], dtype=torch.int64, device=dev)).tolist()]
        self.W, self.r = len(self.sizes), (dist_rank() if len(self.sizes) > 1 else 0)
        self.offset, self.G = sum(self.sizes[: self.r]), sum(self.sizes)
        # ONE scale for every shard: each product then has the bits it has in the one-rank run
        ga = None
        if ops.GEMM_PRECISION == 6 and ops.CONV_PRECISION == 16:  # (the fp16-split default of _sim_precision: it takes the scalars)
            mine = ops.amax(g) if self.G_local else torch.zeros(1, dtype=torch.float32, device=dev)
            ga = group_gather_rows(mine.reshape(1)).max().reshape(1)
        # ONE path: the streaming kernel only if every non-empty shard qualifies (two arithmetics would break "a row compares
        # equal to its own duplicate" across a cut)
        self.p16 = ga is not None and all(_p16_path(16, self.C, n) for n in self.sizes if n)
        self.opnd = _RankOperands(q, g, ga, self.p16, self.offset) if self.G_local else None
        self.ga = ga

    def gather_gallery(self, x):
        from .parallel import group_gather_varrows

        return group_gather_varrows(x, self.sizes)

    def topk(self, qrows, qa, k):
        """global top-k rows [Qn, k] of replicated query rows against the sharded gallery: this shard's list with the operands
        packed once (offset -> global rows), the lists of all shards merged (ties: lower global row first).  The launch sequence
        of _sim_topk_call with what that decides per call - the path from the local G, the query scale from the rows passed -
        fixed by the caller for all shards"""
        from .parallel import group_gather_rows

        Qn, dev = qrows.shape[0], qrows.device
        vals = torch.full((Qn, k), float("-inf"), dtype=torch.float32, device=dev)
        idx = torch.zeros(Qn, k, dtype=torch.int64, device=dev)
        o = self.opnd
        if o is not None:
            kk = min(k, o.G)
            v, i = (vals, idx) if kk == k else (torch.empty(Qn, kk, dtype=torch.float32, device=dev), torch.empty(Qn, kk, dtype=torch.int64, device=dev))
            ws = ops.empty((ops.L.load().trid_topk_ws_floats(Qn, o.G, kk),), qrows)
            if self.p16:
                q16 = torch.zeros((Qn + 31) // 32 * 32, self.C, dtype=torch.float32, device=dev)
                call("trid_p16_pack_f32", _p(qrows), Qn, self.C, self.C, _p(qa), _p(q16), 1, stream())
                args = (_p(qrows), _p(o.g), _p(q16), _p(o.g16), _p(v), _p(i), Qn, o.G, kk, self.offset, _p(qa), _p(o.ga), _p(ws))
                call("trid_sim_topk_p16", *args, 1, stream())
                flag = ws[ops.L.load().trid_topk_ws_flag_offset(Qn, o.G):][:1].view(torch.int32)
                if int(flag.item()) != 0:  # (a candidate list overflowed: the dense passes, as _sim_topk_call)
                    call("trid_sim_topk_p16", *args, 2, stream())
            else:
                call("trid_sim_topk_f32", _p(qrows), _p(o.g), _p(v), _p(i), Qn, o.G, self.C, kk, self.offset, o.prec, _p(qa), _p(o.ga), _p(ws), stream())
            if kk != k:
                vals[:, :kk], idx[:, :kk] = v, i
        if self.W == 1:
            return idx
        W = self.W
        cand_v = group_gather_rows(vals).view(W, Qn, k).permute(1, 0, 2).reshape(Qn, W * k).contiguous()
        cand_i = group_gather_rows(idx).view(W, Qn, k).permute(1, 0, 2).reshape(Qn, W * k).contiguous()
        sel = torch.empty(Qn, k, dtype=torch.int64, device=dev)
        call("trid_topk_rows_f32", _p(cand_v), W * k, Qn, W * k, k, _p(vals), _p(sel), stream())
        return torch.gather(cand_i, 1, sel)

    def neighbours(self, n):
        """(qnn [Q, n], gnn_local [G_local, n]), GLOBAL rows: the queries' and this shard's rows' nearest gallery rows.  The
        gallery x gallery match goes GNN_ROWS rows at a time (every rank's next rows, all-gathered): nothing grows with
        G_total x 8192"""
        from .parallel import group_gather_rows

        if self.G < n:
            raise ValueError("the re-rank needs at least neighbor_num gallery rows")
        dev = self.q.device
        qa = self.opnd.qa if self.opnd is not None else (ops.amax(self.q) if self.ga is not None else None)
        qnn = self.topk(self.q, qa, n)
        gnn = torch.empty(self.G_local, n, dtype=torch.int64, device=dev)
        ch = max(256, GNN_ROWS // self.W)
        for c0 in range(0, max(self.sizes), ch):
            m = min(max(self.G_local - c0, 0), ch)
            rows = torch.zeros(ch, self.C, dtype=torch.float32, device=dev)
            rows[:m] = self.g[c0:c0 + m]
            idx = self.topk(group_gather_rows(rows), self.ga, n)  # (gallery rows as queries: the gallery's scale)
            gnn[c0:c0 + m] = idx[self.r * ch:self.r * ch + m]
        return qnn, gnn


def _positive_counts_sharded(sh, q_pids, g_pids_local, qnn, gnn_local, alpha):
    from .parallel import group_reduce_sum_

    dev = sh.q.device
    Q = sh.Q
    # the global list, identical on every rank
    ptr, idx = _positive_list(q_pids, sh.gather_gallery(g_pids_local.to(dev).long()))
    NP = idx.numel()
    counts = torch.zeros(max(NP, 1), dtype=torch.int32, device=dev)
    thr = torch.zeros(max(NP, 1), dtype=torch.float32, device=dev)
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
        own_ptr, own_idx, own_pos = _owner_split(ptr, idx, sh.offset, sh.G_local)
        if own_pos.numel():
            own_val = torch.empty(own_pos.numel(), dtype=torch.float32, device=dev)
            o.run(own_ptr, own_idx, own_val, None, 0, 0, local=True)
            if qnn is not None:
                call("trid_rank_pairs_jaccard_f32", _p(own_ptr), _p(own_idx), _p(own_val), _p(qnn), _p(gnn_local), n, float(alpha), Q,
                     own_pos.numel(), stream())
            thr[own_pos] = own_val
    group_reduce_sum_(thr)
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
    group_reduce_sum_(counts)
    return ptr, idx, counts


def _sharded_rows(x, normalize):
    if normalize and x.shape[0]:
        return l2_normalize_rows(x)
    return x.contiguous().float()


def positive_ranks_sharded(q, g_local, q_pids, g_pids_local, qnn=None, gnn_local=None, alpha=0.05, normalize=False):
    """positive_ranks over a gallery sharded by rows: COLLECTIVE over the default process group (every rank calls it; one rank:
    the unsharded result).  q, q_pids (and qnn) are replicated; g_local, g_pids_local (and gnn_local, rows of GLOBAL neighbour
    indices) are this rank's rows, rank-major global order; shard sizes may differ and may be 0.
    -> (pos_ptr [Q+1], pos_idx [NP] GLOBAL rows, ranks [NP]), identical on every rank"""
    _refuse_sharded("positive_ranks_sharded", q, g_local)
    if (qnn is None) != (gnn_local is None):
        raise ValueError("positive_ranks_sharded: qnn and gnn_local go together")
    sh = _Shards(_sharded_rows(q, normalize), _sharded_rows(g_local, normalize))
    ptr, idx, counts = _positive_counts_sharded(sh, q_pids, g_pids_local, qnn, gnn_local, alpha)
    return ptr, idx, counts.long() + 1


def rank_from_embeddings_sharded(text_embed, image_embed_local, q_pids, g_pids_local, topk=(1, 5, 10), get_mAP=True, normalize=True,
                                 rerank=False, neighbor_num=5, alpha=0.05):
    """rank_from_embeddings over a gallery sharded by rows (layout and collectivity as positive_ranks_sharded); the neighbour
    lists of the re-rank come from the sharded top-k.  -> (cmc, mAP) or (cmc,), identical on every rank"""
    _refuse_sharded("rank_from_embeddings_sharded", text_embed, image_embed_local)
    dev = text_embed.device
    sh = _Shards(_sharded_rows(text_embed, normalize), _sharded_rows(image_embed_local, normalize))
    qnn, gnn = sh.neighbours(neighbor_num) if rerank else (None, None)
    ptr, idx, counts = _positive_counts_sharded(sh, q_pids, g_pids_local, qnn, gnn, alpha)
    Q = sh.Q
    topk_t = torch.as_tensor(topk, dtype=torch.int64, device=dev)
    first = torch.empty(Q, dtype=torch.int32, device=dev)
    ap = torch.empty(Q, dtype=torch.float32, device=dev)
    cmc = torch.empty(topk_t.numel(), dtype=torch.float32, device=dev)
    call("trid_rank_finalize", _p(counts), _p(ptr), Q, _p(first), _p(ap), _p(topk_t), topk_t.numel(), _p(cmc), stream())
    if not get_mAP:
        return (cmc,)
    mAP = torch.empty(1, dtype=torch.float32, device=dev)
    ops.sum_to(ap, mAP, 100.0 / Q)
    return cmc, mAP[0]


def tables_sharded(image_local, image_pid_local, text_local, text_pid_local, topk=(1, 5, 10), rerank=True):
    """The tables evaluation(matrix_free=True) leaves in evaluation.last_results, from L2-normalised image and text rows that
    are BOTH sharded over the ranks (collective): per direction the query side is all-gathered and replicated, the gallery side
    stays sharded.  -> {"t2i", "i2t"[, "re-t2i", "re-i2t"]: (cmc, mAP or None)}"""
    from .parallel import group_gather_rows, group_gather_varrows

    _refuse_sharded("tables_sharded", image_local, text_local)
    dev = image_local.device

    def whole(x):
        sizes = [int(v) for v in group_gather_rows(torch.tensor([x.shape[0]], dtype=torch.int64, device=dev)).tolist()]
        return group_gather_varrows(x.contiguous(), sizes)

    image_local, text_local = image_local.contiguous().float(), text_local.contiguous().float()
    image_pid_local, text_pid_local = image_pid_local.to(dev).long(), text_pid_local.to(dev).long()
    image_all, image_pid_all = whole(image_local), whole(image_pid_local)
    text_all, text_pid_all = whole(text_local), whole(text_pid_local)

    def table(q, g, qp, gp, re):
        r = rank_from_embeddings_sharded(q, g, qp, gp, topk, get_mAP=rerank, normalize=False, rerank=re)
        return (r[0], r[1] if rerank else None)

    results = {}
    for re in ((False, True) if rerank else (False,)):
        pre = "re-" if re else ""
        results[pre + "i2t"] = table(image_all, text_local, image_pid_all, text_pid_local, re)
        results[pre + "t2i"] = table(text_all, image_local, text_pid_all, image_pid_local, re)
    return results


def _evaluation_matrix_free(dataset, predictions, output_folder, topk, save_data, rerank, logger):
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
        image_ids, pids, image_global, text_global = [], [], [], []
        for idx, prediction in predictions.items():
            image_id, pid = dataset.get_id_info(idx)
            image_ids.append(image_id)
            pids.append(pid)
            image_global.append(prediction[0])
            text_global.append(prediction[1])
        dev = image_global[0].device
        image_pid = torch.tensor(pids, device=dev)
        text_pid = torch.tensor(pids, device=dev)
        keep = get_unique(image_ids).to(dev)
        image_global = l2_normalize_rows(torch.stack(image_global, dim=0)[keep])
        image_pid = image_pid[keep]
        text_global = l2_normalize_rows(torch.stack(text_global, dim=0))
        if save_data and embed_dir:
            np.savez(embed_dir, image_pid=image_pid.cpu().numpy(), text_pid=text_pid.cpu().numpy(),
                     image_embed=image_global.cpu().numpy(), text_embed=text_global.cpu().numpy())
    results = {}

    def table(q, g, qp, gp, re):
        r = rank_from_embeddings(q, g, qp, gp, topk, get_mAP=rerank, normalize=False, rerank=re)
        return (r[0], r[1] if rerank else None)

    if rerank:
        results["i2t"] = table(image_global, text_global, image_pid, text_pid, False)
        results["t2i"] = table(text_global, image_global, text_pid, image_pid, False)
        results["re-i2t"] = table(image_global, text_global, image_pid, text_pid, True)
        results["re-t2i"] = table(text_global, image_global, text_pid, image_pid, True)
        for k, (cmc, mAP) in results.items():
            logger.info("%-7s topk %s cmc %s mAP %.3f", k, list(topk), [round(float(c), 3) for c in cmc], float(mAP))
    else:
        results["t2i"] = table(text_global, image_global, text_pid, image_pid, False)
        results["i2t"] = table(image_global, text_global, image_pid, text_pid, False)
        logger.info("topk %s  t2i %s  i2t %s", list(topk), results["t2i"][0].tolist(), results["i2t"][0].tolist())
    evaluation.last_results = results
    return results["t2i"][0][0]


def get_unique(image_ids):
    keep = {}
    for i, image_id in enumerate(image_ids):
        keep.setdefault(image_id, i)
    return torch.tensor(list(keep.values()))


def evaluation(dataset, predictions, output_folder, topk, save_data=True, rerank=True, matrix_free=False):
    """matrix_free: the four tables from rank_from_embeddings - no [Q,G] tensor is made; save_data then keeps the normalised
    embeddings and pids (inference_embed.npz), which predictions=None reads back."""
    logger = logging.getLogger("PersonSearch.inference")
    if matrix_free:
        return _evaluation_matrix_free(dataset, predictions, output_folder, topk, save_data, rerank, logger)
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
        image_ids, pids, image_global, text_global = [], [], [], []
        for idx, prediction in predictions.items():
            image_id, pid = dataset.get_id_info(idx)
            image_ids.append(image_id)
            pids.append(pid)
            image_global.append(prediction[0])
            text_global.append(prediction[1])
        dev = image_global[0].device
        image_pid = torch.tensor(pids, device=dev)
        text_pid = torch.tensor(pids, device=dev)
        image_global = torch.stack(image_global, dim=0)
        text_global = torch.stack(text_global, dim=0)
        keep = get_unique(image_ids).to(dev)
        image_global = l2_normalize_rows(image_global[keep])
        image_pid = image_pid[keep]
        text_global = l2_normalize_rows(text_global)
        sim = ops.linear(text_global, image_global)  # [texts, images]
        if rerank:
            rtn = k_reciprocal(image_global, text_global)  # [images, texts] (evaluation.py:122-124)
            rvn = k_reciprocal(text_global, image_global)  # [texts, images]
        if save_data and data_dir:
            arrays = dict(image_pid=image_pid.cpu().numpy(), text_pid=text_pid.cpu().numpy(), similarity=sim.cpu().numpy())
            if rerank:
                arrays.update(rvn_mat=rvn.cpu().numpy(), rtn_mat=rtn.cpu().numpy())
            np.savez(data_dir, **arrays)
    sim_t = sim.t().contiguous()
    results = {}
    if rerank:
        ones = torch.ones(3, device=dev)
        re_i2t, re_t2i = torch.empty_like(rtn), torch.empty_like(rvn)
        rtn, rvn = rtn.contiguous(), rvn.contiguous()
        call("trid_axpby3_f32", _p(re_i2t), _p(rtn), _p(sim_t), None, _p(ones), rtn.numel(), stream())  # rtn_mat + similarity.t()
        call("trid_axpby3_f32", _p(re_t2i), _p(rvn), _p(sim), None, _p(ones), rvn.numel(), stream())    # rvn_mat + similarity
        results["i2t"] = rank(sim_t, image_pid, text_pid, topk, get_mAP=True)[:2]
        results["t2i"] = rank(sim, text_pid, image_pid, topk, get_mAP=True)[:2]
        results["re-i2t"] = rank(re_i2t, image_pid, text_pid, topk, get_mAP=True)[:2]
        results["re-t2i"] = rank(re_t2i, text_pid, image_pid, topk, get_mAP=True)[:2]
        for k, (cmc, mAP) in results.items():
            logger.info("%-7s topk %s cmc %s mAP %.3f", k, list(topk), [round(float(c), 3) for c in cmc], float(mAP))
    else:
        results["t2i"] = (rank(sim, text_pid, image_pid, topk, get_mAP=False)[0], None)
        results["i2t"] = (rank(sim_t, image_pid, text_pid, topk, get_mAP=False)[0], None)
        logger.info("topk %s  t2i %s  i2t %s", list(topk), results["t2i"][0].tolist(), results["i2t"][0].tolist())
    evaluation.last_results = results
    return results["t2i"][0][0]
