"""Token-embedding + bias-free (stacked) BiGRU + max-over-time text encoder on the HIP library.

Operator surface of the reference ``lib/models/backbones/gru.py`` (``GRU``
:8-88, ``build_gru`` :91-117): ``forward(list[Caption]) -> [B, 2*hidden]``,
``out_channels``, parameters ``gru.weight_{ih,hh}_l0[_reverse]`` (the nn.GRU is
a parameter holder; its forward is never called), frozen ``vocab_dict`` table as
a plain attribute.  Instead of sort/pack/pad (gru.py:66-82, one host sync), the
recurrence runs as a masked time loop: per step one batched fp32 MFMA GEMM
(h @ W_hh^T, both directions) and one fused gate/state/max kernel; the
zero-pad-enters-the-max behaviour of gru.py:63 is reproduced by the max init.

``MODEL.GRU.NUM_LAYER > 1`` (gru.py:36-43): parameters ``gru.weight_{ih,hh}_l{k}[_reverse]`` as nn.GRU names them; every
layer below the last emits its output sequence ``yseq [B*L, 2H]`` (the next layer's input, zero at t >= length), only
the last layer feeds the max; in training mode nn.GRU's dropout sits between the layers (csrc/dropout_seq.hip).
One autograd Function (``_BiGRUFn``) serves every depth: one layer is the stack of depth one.
"""

import os

import numpy as np
import torch
from torch import nn

from .. import ops
from ..caption import CaptionBatch


def load_vocab_dict(root, use_onehot):
    names = {"bert_c4": "bert_vocab_c4.npy", "bert_l2": "bert_vocab_l2.npy", "clip_vit": "clip_vocab_vit.npy",
             "clip_rn50x4": "clip_vocab_rn50x4.npy"}
    if use_onehot not in names:
        raise NotImplementedError(use_onehot)
    return np.load(os.path.join(root, "./datasets/cuhkpedes", names[use_onehot]))


FUSED_GRU_STEP = os.environ.get("TRID_FUSED_GRU", "1") != "0"  # A/B switch: 0 = one GEMM + one cell kernel per step


def _step_ptrs(t, n, stride):
    """Addresses of the `n` per-step slices of fp32 `t`, `stride` elements apart, computed once per layer (the time loops
    are host-bound); `n` Nones for a tensor that is not kept."""
    return [None] * n if t is None else [t.data_ptr() + 4 * stride * s for s in range(n)]


def _input_rows(mod, tokens, emb_w, emb_b, B, L, P, st):
    """The rows the first layer reads -> (x [B*L, E], x0, vocab, a_x).  The three input forms of gru.py:22-31,55-60:
    0 = rows of the frozen table (every MoCo config); 1 = a TRAINABLE nn.Embedding (`use_onehot == "yes"`); 2 = rows of the
    frozen table (kept as x0 for the backward pass) through nn.Linear(vocab_size, embed_size)."""
    mode = mod.embed_mode
    table = emb_w.detach() if mode == 1 else mod.vocab_dict
    x = ops.empty((B * L, table.shape[1]), table)
    ops.call("trid_embedding_gather_f32", ops._p(table), ops._p(tokens), ops._p(x), B, L, tokens.stride(0), table.shape[1],
             table.shape[0], st)
    x0 = x if mode == 2 else None
    if mode == 2:
        x = ops.linear(x0, emb_w.detach(), emb_b.detach())  # [B*L, E]
    # operand bound of the fp16-split projection GEMMs: every gathered row is a row of the frozen table, so
    # max|x| <= max|table| (computed once per table)
    a_x = None
    if P and mode != 0:
        a_x = ops.amax(x)  # (a trained table / the Linear's output: no bound carries over from step to step)
    elif P:
        if getattr(mod, "_table_amax", None) is None or mod._table_amax[0] is not table:
            mod._table_amax = (table, ops.amax(table))
        a_x = mod._table_amax[1]
    return x, x0, table.shape[0], a_x


def _layer_forward(x, a_x, P, w_ih_f, w_hh_f, w_ih_r, w_hh_r, lengths, lmax_dev, B, L, last, save, img_bytes, st):
    """One layer: input projections, W_hh image pack, time loop -> (maxv [B, 2H] on the last layer / yseq [B*L, 2H] below it,
    argt, the layer's record for the backward pass).  The zero-pad quirk of gru.py:63 is the last layer's alone."""
    H, E = w_hh_f.shape[1], w_ih_f.shape[1]
    dev = x.device
    gi = ops.empty((B * L, 6 * H), x)
    # fp16-split arithmetic for the big text GEMMs while that is the library's conv mode
    for w, c_off in ((w_ih_f, 0), (w_ih_r, 3 * H)):
        ops.gemm(x, w, gi, B * L, 3 * H, E, E, E, 6 * H, c_off=c_off, precision=P, a_amax=a_x, b_amax=ops.amax(w) if P else None)
    whh = torch.stack([w_hh_f.detach(), w_hh_r.detach()])  # [2,3H,H] (plumbing copy)
    h = torch.zeros(2, B, H, device=dev)
    if last:
        out = ops.empty((B, 2 * H), x)
        argt = torch.empty(B, 2 * H, dtype=torch.int32, device=dev)
        ops.call("trid_gru_max_init_f32", ops._p(out), ops._p(argt), ops._p(lengths), L, ops._p(lmax_dev), B, H, st)
        form, outs = "", (ops._p(out), ops._p(argt))
    else:
        out, argt = ops.empty((B * L, 2 * H), x), None  # every row is written by the steps (zero at t >= length)
        form, outs = "_seq", (ops._p(out),)
    gates = ops.empty((2, L, B, 4 * H), x) if save else None
    hprev = ops.empty((2, L, B, H), x) if save else None
    p_gates, p_hprev = _step_ptrs(gates, L, B * 4 * H), _step_ptrs(hprev, L, B * H)
    p_h, p_gi, p_len = ops._p(h), ops._p(gi), ops._p(lengths)
    fused = None
    if img_bytes > 0:
        # ONE launch per step (gru_step.hip): W_hh split once into MFMA fragment images, the state carried as
        # packed fp16 planes between the steps
        wamax = ops.amax(whh)
        img_f = torch.empty(img_bytes, dtype=torch.uint8, device=dev)
        img_b = torch.empty(img_bytes, dtype=torch.uint8, device=dev)
        ops.call("trid_gru_pack_whh_f16", ops._p(whh), ops._p(wamax), ops._p(img_f), ops._p(img_b), H, st)
        Bp = (B + 15) // 16 * 16
        hp = torch.zeros(2, 2, Bp, H, dtype=torch.int32, device=dev)
        name, p_img, p_wamax, p_hp = "trid_gru_step%s_fwd_f32" % form, ops._p(img_f), ops._p(wamax), (ops._p(hp[0]), ops._p(hp[1]))
        tail = (L, L, B, Bp, H, L * B * 4 * H, L * B * H, st)
        for s in range(L):
            ops.call(name, p_img, p_wamax, p_hp[s & 1], p_hp[(s + 1) & 1], p_h, p_gi, p_len, p_gates[s], p_hprev[s], *outs, s, *tail)
        fused = (img_b, wamax)
    else:
        gh = ops.empty((2, B, 3 * H), x)
        name, p_gh = "trid_gru_cell%s_fwd_f32" % form, ops._p(gh)
        tail = (L, L, B, H, L * B * 4 * H, L * B * H, st)
        for s in range(L):
            ops.gemm(h, whh, gh, B, 3 * H, H, H, H, 3 * H, batch=2, strideA=B * H, strideB=3 * H * H, strideC=B * 3 * H)
            ops.call(name, p_gi, p_gh, p_h, p_len, p_gates[s], p_hprev[s], *outs, s, *tail)
    return out, argt, (x, whh, gates, hprev, fused, a_x)


def _layer_backward_steps(layer, dy, argt, lengths, B, L, st):
    """One layer's backward time loop -> (dGi [B*L, 6H], dgh [2, L, B, 3H], the per-workgroup max|dgh| the fused steps
    published or None).  `dy`: dout [B, 2H] with `argt` on the last layer, dyseq [B*L, 2H] (argt None) below it."""
    x, whh, gates, hprev, fused, a_x = layer
    H = whh.shape[2]
    dh = torch.zeros(2, B, H, device=dy.device)
    dGi = ops.empty((B * L, 6 * H), dy)
    dgh = ops.empty((2, L, B, 3 * H), dy)
    p_gates, p_hprev, p_dgh = _step_ptrs(gates, L, B * 4 * H), _step_ptrs(hprev, L, B * H), _step_ptrs(dgh, L, B * 3 * H)
    form, ins = ("_seq", (ops._p(dy),)) if argt is None else ("", (ops._p(dy), ops._p(argt)))
    mid = (ops._p(lengths), ops._p(dh), ops._p(dGi))
    tail = (L, L, B, H, L * B * 4 * H, L * B * H, L * B * 3 * H, st)
    amax = None
    if fused is not None:
        img_b, wamax = fused
        nwg = ops.L.load().trid_gru_step_workgroups(B, H)
        amax = ops.empty((L + 1, nwg), dy)  # per-workgroup max|dgh| published by each step
        name, p_img, p_wamax, p_amax = "trid_gru_step%s_bwd_f32" % form, ops._p(img_b), ops._p(wamax), _step_ptrs(amax, L, nwg)
        for s in range(L - 1, -1, -1):
            more = s + 1 < L
            ops.call(name, p_img, p_wamax, p_dgh[s + 1] if more else None, p_amax[s + 1] if more else None, p_amax[s], *ins,
                     p_gates[s], p_hprev[s], *mid, p_dgh[s], s, *tail)
    else:
        name = "trid_gru_cell%s_bwd_f32" % form
        for s in range(L - 1, -1, -1):
            ops.call(name, *ins, p_gates[s], p_hprev[s], *mid, p_dgh[s], s, *tail)
            # dh[d] += dgh[d,s] @ W_hh[d]
            ops.gemm(dgh, whh, dh, B, H, 3 * H, 3 * H, H, H, b_mode=ops.B_NC, batch=2, strideA=L * B * 3 * H,
                     strideB=3 * H * H, strideC=B * H, accumulate=True, a_off=s * B * 3 * H)
    return dGi, dgh, amax


def _weight_grads(mod, layer, dGi, dgh, amax, B, L, st):
    """dW_hh[d] = sum_{s,b} dgh[d,s,b,:]^T hprev[d,s,b,:] and dW_ih[d] = sum dGi[:, d]^T x -> (dwih [2,3H,E], dwhh [2,3H,H]);
    for a layer above the first the saved x is the dropped-out sequence itself."""
    x, whh, gates, hprev, fused, a_x = layer
    H, E = whh.shape[2], x.shape[1]
    KK = L * B
    splits = max(1, min(8, KK // 512))
    dwhh = ops.empty((2, 3 * H, H), dGi)
    dwih = ops.empty((2, 3 * H, E), dGi)
    # operand magnitudes of the fp16-split form: |hprev| < 1 by construction; max|dgh| is the maximum the backward
    # steps published (dGi's r / z rows equal dgh's, its n row is dgh's divided by a gate <= 1: one streaming pass)
    kw_hh = kw_ih = {}
    if a_x is not None and fused is not None:
        kw_hh = dict(precision=16, a_amax=torch.amax(amax[:L]).reshape(1), b_amax=mod._seq_bound(0.0, dGi.device))
        kw_ih = dict(precision=16, a_amax=ops.amax(dGi), b_amax=a_x)
    slab = ops.empty((splits, 2, 3 * H, max(H, E)), dGi) if splits > 1 else None
    for A, Bm, dw, N, lda, strideA, strideB, kw in ((dgh, hprev, dwhh, H, 3 * H, KK * 3 * H, KK * H, kw_hh),
                                                    (dGi, x, dwih, E, 6 * H, 3 * H, 0, kw_ih)):
        n = 2 * 3 * H * N
        kw = dict(kw, a_mode=ops.A_MC, b_mode=ops.B_NC, batch=2, strideA=strideA, strideB=strideB, strideC=3 * H * N)
        if splits == 1:
            ops.gemm(A, Bm, dw, 3 * H, N, KK, lda, N, N, **kw)
        else:
            ops.gemm(A, Bm, slab, 3 * H, N, KK, lda, N, N, splits=splits, strideSplit=n, **kw)
            ops.call("trid_slab_reduce_f32", ops._p(slab), ops._p(dw), n, splits, n, 0, st)
    return dwih, dwhh


def _embedding_grad(mode, dX, tokens, x0, vocab, B, L, st):
    """-> (d_emb_w, d_emb_b) of the input form's own parameters, from the gradient dX [B*L, E] of the first layer's rows"""
    if mode == 1:  # nn.Embedding(padding_idx=0): rows summed per token, deterministic (csrc/attn_text.hip)
        d_emb_w = ops.empty((vocab, dX.shape[1]), dX)
        ops.call("trid_embedding_bwd_f32", ops._p(dX), ops._p(tokens), B, L, tokens.stride(0), dX.shape[1], ops._p(d_emb_w), vocab, 0, st)
        return d_emb_w, None
    return ops.matmul_tn(dX, x0), ops.colsum(dX)  # nn.Linear on the frozen rows: dW = dX^T x0, db = column sums


class _BiGRUFn(torch.autograd.Function):
    """Any depth (gru.py:36-43,77).  Layer l >= 1 reads [h_fwd_t, h_bwd_t] of layer l - 1 (K = 2H), with nn.GRU's dropout
    in between while training; only the last layer feeds the max over time."""

    @staticmethod
    def forward(ctx, mod, tokens, lengths, L, lmax_dev, save, p_drop, *params):
        # L: the time-loop length; `save` comes from the caller: ctx.needs_input_grad ignores torch.no_grad()
        nl = mod.gru.num_layers
        ws, (emb_w, emb_b) = params[: 4 * nl], params[4 * nl :]
        B, H = tokens.shape[0], ws[1].shape[1]
        st = ops.stream()
        dev = tokens.device
        P = 16 if ops.conv_precision() == 16 else None
        x, x0, vocab, a_x = _input_rows(mod, tokens, emb_w, emb_b, B, L, P, st)
        img_bytes = ops.L.load().trid_gru_whh_image_bytes(H) if FUSED_GRU_STEP else 0
        layers, masks = [], []
        for l in range(nl):
            last = l == nl - 1
            x, argt, layer = _layer_forward(x, a_x, P, *ws[4 * l : 4 * l + 4], lengths, lmax_dev, B, L, last, save, img_bytes, st)
            layers.append(layer)
            if not last:
                if p_drop > 0:
                    keep = torch.empty(B * L, 2 * H, dtype=torch.uint8, device=dev)
                    ops.call("trid_dropout_seq_fwd_f32", ops._p(x), ops._p(x), ops._p(keep), x.numel(), p_drop,
                             ops._p(mod.dropout_state(dev)), l, st)
                    masks.append(keep)
                # |h| < 1 by construction, so the next projection's operand bound needs no pass: max|x| <= 1 / (1 - p)
                a_x = mod._seq_bound(p_drop, dev) if P else None
        if masks:
            ops.call("trid_dropout_advance", ops._p(mod.dropout_state(dev)), len(masks), st)  # a replay draws the next masks
        mod.last_dropout_masks = [k.view(B, L, 2 * H) for k in masks] if masks else None
        mod.last_layer_inputs = [lay[0].view(B, L, -1) for lay in layers[1:]]  # (the tests look at the padding rows)
        if save:
            ctx.saved = (mod, layers, masks, argt, lengths, B, L, p_drop)
            ctx.embed = (mod.embed_mode, tokens, x0, vocab, [w.detach() for w in ws])
        return x

    @staticmethod
    def backward(ctx, dout):
        mod, layers, masks, argt, lengths, B, L, p_drop = ctx.saved
        mode, tokens, x0, vocab, ws = ctx.embed
        ctx.saved = ctx.embed = None
        st = ops.stream()
        nl = len(layers)
        grads = [None] * (4 * nl)
        dy = dout.contiguous()
        for l in range(nl - 1, -1, -1):
            dGi, dgh, amax = _layer_backward_steps(layers[l], dy, argt if l == nl - 1 else None, lengths, B, L, st)
            dwih, dwhh = _weight_grads(mod, layers[l], dGi, dgh, amax, B, L, st)
            grads[4 * l : 4 * l + 4] = [dwih[0], dwhh[0], dwih[1], dwhh[1]]
            if l > 0 or mode != 0:
                # the layer's input is itself a function of parameters: dX = dGi_fwd W_ih + dGi_rev W_ih_reverse (zero at
                # t >= length: the steps zero those dGi rows)
                H = dGi.shape[1] // 6
                dy = ops.matmul_nn(dGi[:, : 3 * H], ws[4 * l])
                ops.matmul_nn(dGi[:, 3 * H :], ws[4 * l + 2], out=dy, accumulate=True)
            if l > 0 and masks:
                ops.call("trid_dropout_seq_bwd_f32", ops._p(dy), ops._p(masks[l - 1]), dy.numel(), p_drop, st)
        d_emb = _embedding_grad(mode, dy, tokens, x0, vocab, B, L, st) if mode != 0 else (None, None)
        return (None,) * 7 + tuple(grads) + d_emb


class GRU(nn.Module):
    def __init__(self, hidden_dim, vocab_size, embed_size, num_layers, drop_out, bidirectional, use_onehot, root,
                 vocab_dict=None):
        super().__init__()
        if num_layers < 1 or not bidirectional:
            raise NotImplementedError("HIP text encoder covers the bidirectional GRU (any depth): no config builds a unidirectional one")
        self.use_onehot = use_onehot
        # word embedding: the three forms of gru.py:22-34
        if use_onehot == "yes":
            self.embed = nn.Embedding(vocab_size, embed_size, padding_idx=0)  # a trainable table (parameter holder: its forward is never called)
            self.vocab_dict = None
            self.embed_mode = 1
        else:
            self.embed = None if vocab_size == embed_size else nn.Linear(vocab_size, embed_size)
            self.embed_mode = 0 if self.embed is None else 2
            if vocab_dict is None:
                vocab_dict = load_vocab_dict(root, use_onehot)
            vocab_dict = torch.as_tensor(vocab_dict).float()
            assert vocab_size == vocab_dict.shape[1]
            dev = "cuda" if torch.cuda.is_available() else "cpu"
            self.vocab_dict = vocab_dict.to(dev).contiguous()  # plain attribute, as gru.py:34
        self.gru = nn.GRU(embed_size, hidden_dim, num_layers=num_layers, dropout=drop_out,
                          bidirectional=bidirectional, bias=False)
        self.out_channels = hidden_dim * 2
        # inter-layer dropout (num_layers > 1): the generator's (seed, offset) pair lives on the device, one per encoder
        # instance, a plain attribute (not in the state_dict); made the first time a training forward needs it
        self._dropout_state = None
        self._seq_bounds = {}
        self.last_dropout_masks = None  # after a forward: the keep masks it drew, uint8 [B, L, 2H] per layer boundary
        self.last_layer_inputs = []     # ... and the inputs [B, L, 2H] of the layers above the first

    def dropout_state(self, device):
        """int64 [seed, offset] on `device`.  The seed is drawn from torch's default CPU generator on first use
        (`torch.manual_seed` makes a run repeatable); the offset is advanced by a kernel behind every forward's masks, so a
        recorded step draws fresh masks on every replay."""
        s = self._dropout_state
        if s is None:
            seed = int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).item())
            s = self._dropout_state = torch.tensor([seed, 0], dtype=torch.int64).to(device)
        elif s.device != device:
            s = self._dropout_state = s.to(device)
        return s

    def _seq_bound(self, p, device):
        """device scalar 1 / (1 - p): the bound of a layer's (dropped-out) output sequence, |h| < 1 (p = 0: the cached 1.0)"""
        t = self._seq_bounds.get((p, device))
        if t is None:
            t = self._seq_bounds[(p, device)] = torch.full((1,), 1.0 / (1.0 - p), device=device)
        return t

    def __deepcopy__(self, memo):
        # (the MoCo key encoder is a deep copy: it gets generator state of its own, and no cached device scalars)
        new = self.__class__.__new__(self.__class__)
        memo[id(self)] = new
        import copy

        for k, v in self.__dict__.items():
            if k in ("_seq_bounds", "last_layer_inputs"):
                new.__dict__[k] = type(v)()
            elif k in ("_dropout_state", "last_dropout_masks"):
                new.__dict__[k] = None
            else:
                new.__dict__[k] = copy.deepcopy(v, memo)
        return new

    def forward(self, captions):
        cb = CaptionBatch.from_list(captions)
        if not cb.tokens.is_cuda:
            raise RuntimeError("textreid_amd.GRU runs on the HIP kernel library only (CUDA tensors); no CPU fallback")
        if self.vocab_dict is not None and self.vocab_dict.device != cb.tokens.device:
            self.vocab_dict = self.vocab_dict.to(cb.tokens.device)
        g = self.gru
        ws = tuple(getattr(g, "weight_%s_l%d%s" % (kind, k, sfx)) for k in range(g.num_layers) for sfx in ("", "_reverse") for kind in ("ih", "hh"))
        extra = () if self.embed is None else ((self.embed.weight, None) if self.embed_mode == 1 else (self.embed.weight, self.embed.bias))
        save = torch.is_grad_enabled() and any(w.requires_grad for w in ws + tuple(e for e in extra if e is not None))
        # cb.max_len is the time-loop length; when it is only an upper BOUND of the batch maximum (bound_only: a recorded
        # step replayed on other captions) the zero-pad quirk of gru.py:63 takes the true maximum from the device
        lmax_dev = cb.lengths.max().reshape(1) if getattr(cb, "bound_only", False) else None
        # nn.GRU's rule: dropout between the layers iff the nn.GRU itself is in training mode (MODEL.FREEZE puts it in eval
        # mode); one layer has no boundary to drop at
        p_drop = float(g.dropout) if g.training and g.num_layers > 1 else 0.0
        return _BiGRUFn.apply(self, cb.tokens.contiguous(), cb.lengths.contiguous(), cb.max_len, lmax_dev, save, p_drop, *ws,
                              *(extra if extra else (None, None)))


def build_gru(cfg, bidirectional, vocab_dict=None):
    model = GRU(cfg.MODEL.GRU.NUM_UNITS, cfg.MODEL.GRU.VOCABULARY_SIZE, cfg.MODEL.GRU.EMBEDDING_SIZE,
                cfg.MODEL.GRU.NUM_LAYER, 1 - cfg.MODEL.GRU.DROPOUT_KEEP_PROB, bidirectional, cfg.MODEL.GRU.ONEHOT,
                cfg.ROOT, vocab_dict=vocab_dict)
    if cfg.MODEL.FREEZE:
        model.gru.eval()
        for p in model.gru.parameters():
            p.requires_grad = False
    return model
