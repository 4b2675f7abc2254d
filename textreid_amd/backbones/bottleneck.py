"""What the two image encoders (``m_resnet.py``: CLIP ModifiedResNet, ``resnet.py``: ImageNet ResNet-50/101) share: ONE fp32
Bottleneck data flow, ONE eval-mode P16 block body, ONE parameter-only eval plan, ONE ``autograd.Function`` and the module base
class that carries them, with the pure helpers they need (filter views, BatchNorm coefficients, conv arithmetic, P16 filters).

A Bottleneck is ``conv1 -> bn1 -> ReLU -> conv2 -> bn2 -> ReLU -> conv3 -> bn3 (+ identity | downsample) -> ReLU``.  The holder
classes state where the two encoders differ; the flows below read it from them:

* ``blk.down_conv`` / ``blk.down_bn``: the downsample branch's convolution and BatchNorm (``downsample[1]`` / ``[2]`` behind
  CLIP's ``AvgPool2d``, ``downsample[0]`` / ``[1]`` in the ImageNet form);
* ``blk.pooled_stride``: how stride 2 is realised.  True (CLIP): every convolution runs at stride 1 and a 2x2 average pool follows
  bn2 + ReLU and precedes the downsample convolution.  False (ImageNet): the stride is ON the 3x3 convolution and on the 1x1
  downsample convolution, which reads the even pixels (``ops.subsample2``).

Every kernel wrapper is reached as ``ops.<name>`` at call time (tests count calls by replacing them there).  The weight-gradient
side stream, the P16 TRAINING flow and every schedule / fusion switch live in ``m_resnet.py``.
"""

import torch
from torch import nn

from .. import ops


def _w3x3(conv):
    """[N,C,3,3] parameter -> [N, 9*C] tap-major/channel-minor view (a free view
    when the parameter is channels_last, which build/ctor arrange)."""
    w = conv.weight
    N, C = w.shape[0], w.shape[1]
    return w.permute(0, 2, 3, 1).contiguous().reshape(N, 9 * C)


def _g3x3(dw, N, C):
    """[N, 9*C] gradient -> [N,C,3,3]-shaped (channels_last strided) tensor."""
    return dw.view(N, 3, 3, C).permute(0, 3, 1, 2)


def _pix(t):
    return t.numel() // t.shape[-1]


def _bn_coeffs(bn, partials, M, training, counters=None):
    """Per-layer BatchNorm coefficients.  Training also advances `num_batches_tracked`; with `counters`
    (a list) the increment is deferred so the caller can bump all 55 counters in one launch."""
    if training:
        st = ops.bn_finalize(partials, M, bn.weight, bn.bias, bn.running_mean, bn.running_var)
        if counters is None:
            bn.num_batches_tracked += 1
        else:
            counters.append(bn.num_batches_tracked)
        return st
    return ops.bn_eval_coeffs(bn.weight, bn.bias, bn.running_mean, bn.running_var)


class ConvArith:
    """Conv arithmetic of one encoder pass.  With the fp16 two-plane split (ops.conv_precision() == 16) every GEMM
    operand travels with its largest magnitude as a device scalar: `WA` maps id(conv weight) -> max|w| (weight_amax),
    `slot()` hands out zeroed scalars for the amax side outputs of the BatchNorm kernels that produce activations."""

    def __init__(self, device, WA, PB=None):
        self.device, self.WA = device, WA
        # P: arithmetic of the stem convolutions - 16 (fp16 two-plane split, needs WA) or None (the library's default);
        # PB: arithmetic of the residual blocks' convolutions - the same, or 1: operands rounded to bf16 where the conv
        # reads them (configs[3]'s arithmetic, TRID_CONV_PRECISION=1; oracle: oracle.visual.bf16_conv)
        self.P = 16 if WA else None
        self.PB = self.P if PB is None else PB

    def slot(self):
        return ops.amax_slot(self.device) if self.WA else None

    def wam(self, conv):
        return self.WA.get(id(conv.weight))


def _conv_weights(mod):
    """The conv filters under `mod` in module order (the order of weight_amax's scalars).  The module tree is static: walked once
    (nn.Module.modules() cost 1.8 ms of host time per train step when walked on every pass)."""
    ent = mod.__dict__.get("_conv_weight_list")
    # (Parameter OBJECTS are stable under .to() / load_state_dict / optimizer steps; a caller that assigns new nn.Parameters
    # is caught by the identity of the first and last filter)
    if ent is None or ent[1].weight is not ent[0][0] or ent[2].weight is not ent[0][-1]:
        cm = [m for m in mod.modules() if isinstance(m, nn.Conv2d)]
        ent = ([m.weight for m in cm], cm[0], cm[-1])
        mod.__dict__["_conv_weight_list"] = ent
        mod.__dict__.pop("_block_conv_weight_list", None)
    return ent[0]


def weight_amax(mod):
    """{id(conv weight): device scalar max|w|} for every conv filter under `mod`, ONE multi-tensor launch (fp16-split
    arithmetic, ops.CONV_PRECISION == 16).  The pointer table is rebuilt only when a parameter moves."""
    convs = _conv_weights(mod)
    key = tuple(w.data_ptr() for w in convs)
    plan = getattr(mod, "_wamax_plan", None)
    if plan is None or plan[0] != key:
        dev = convs[0].device
        ptrs = torch.tensor(list(key), dtype=torch.int64, device=dev)
        sizes = torch.tensor([w.numel() for w in convs], dtype=torch.int64, device=dev)
        plan = (key, ptrs, sizes)
        mod._wamax_plan = plan
    out = torch.zeros(len(convs), dtype=torch.float32, device=convs[0].device)
    ops.call("trid_amax_multi_f32", ops._p(plan[1]), ops._p(plan[2]), len(convs), ops._p(out), ops.stream())
    WA = {id(w): out[i : i + 1] for i, w in enumerate(convs)}
    WA["all"] = out  # the scalars as one array, in module order of the conv filters (p16_weights)
    return WA


def p16_eligible(mod, mult=32):
    """The residual blocks run on pre-split (P16) operands when every block channel count is a multiple of the 32-wide
    K group - 64 for the bf16 form - (all CLIP ModifiedResNets at width 64; not the width-16 test encoders)."""
    cache = mod.__dict__.setdefault("_p16_ok", {})
    if mult not in cache:
        cache[mult] = all(isinstance(m, nn.Conv2d) is False or (m.in_channels % mult == 0 and m.out_channels % mult == 0)
                          for blk in mod.blocks() for m in blk.modules())
    return cache[mult]


def stem_p16_channels(mod):
    """The P16 stem flow covers the CLIP stem's channel counts: 3 -> 32 -> 32 -> 64."""
    if not hasattr(mod, "conv3"):  # (the ImageNet ResNet's one-convolution stem: backbones/resnet.py)
        return False
    return (mod.conv1.in_channels, mod.conv1.out_channels, mod.conv2.out_channels, mod.conv3.out_channels) == (3, 32, 32, 64)


def p16_weights(mod, WA, transposed, fmt=1, stem_only=False):
    """{id(conv weight): ops.P16} for every residual-block filter of `mod`, ONE multi-tensor launch: the forward
    operands [N][taps*C] (filters as stored: 3x3 in OHWI) or, transposed, the data-gradient operands [C][taps*N] with
    the taps reversed.  fmt 1: P16 (scaled by WA's amax scalars); fmt 2: plain bf16.  Destination buffers and the
    pointer table are persistent per module."""
    convs = _conv_weights(mod)  # weight_amax's order
    index = {id(w): i for i, w in enumerate(convs)}
    mine = mod.__dict__.get("_block_conv_weight_list")
    if mine is None:
        blocks = mod.blocks() if hasattr(mod, "blocks") else [mod]  # (a single Bottleneck: per-block parity tests)
        mine = [m.weight for blk in blocks for m in blk.modules() if isinstance(m, nn.Conv2d)]
        mod.__dict__["_block_conv_weight_list"] = mine
    if fmt == 1 and hasattr(mod, "blocks") and stem_p16_channels(mod):
        mine = [mod.conv2.weight, mod.conv3.weight] + mine  # the stem's 3x3 convolutions run on P16 operands too (stem_forward_p16)
    if stem_only:  # bf16 mode: the residual blocks read bf16 filters, the stem stays fp32-class on ITS two P16 filters
        mine = [mod.conv2.weight, mod.conv3.weight]
    key = tuple(w.data_ptr() for w in mine)
    plans = mod.__dict__.setdefault("_p16_plans", {})
    plan = plans.get((transposed, fmt, stem_only))
    if plan is None or plan[0] != key:
        dev = mine[0].device
        dsts, rows = [], []
        for w in mine:
            N, C, T = w.shape[0], w.shape[1], w.shape[2] * w.shape[3]
            if T > 1 and not w.is_contiguous(memory_format=torch.channels_last):
                raise RuntimeError("3x3 filters must live in channels_last (OHWI) memory")
            d = ops.p16_empty((C, T * N) if transposed else (N, T * C), w, fmt)
            dsts.append(d)
            rows.append([w.data_ptr(), d.data_ptr(), N, T, C, index[id(w)]])
        plan = (key, torch.tensor(rows, dtype=torch.int64, device=dev), dsts)
        plans[(transposed, fmt, stem_only)] = plan
    ops.call("trid_p16_pack_multi_f32", ops._p(plan[1]), ops._p(WA["all"]), len(mine), 1 if transposed else 0, fmt, ops.stream())
    return {id(w): ops.P16(d, WA[id(w)] if fmt == 1 else None, fmt) for w, d in zip(mine, plan[2])}


def _pre_mask(y, st):
    """bool [..., C]: the ReLU decision of relu(bn(y)) where only the pooled activation is kept, taken by the SAME
    kernel arithmetic as the forward / backward passes (parity tests only)."""
    return ops.bn_apply(y, st, relu=True) > 0


# --------------------------------------------------------------------------- the fp32 Bottleneck flow
def block_forward(blk, x, ax, ar, training, save, nbt, masks=None):
    """One Bottleneck (reference m_resnet.py:54-67, resnet.py:78-98) on NHWC activations.  x: block input, ax: its amax scalar
    (or None).  Returns (out, amax scalar of out, record for block_backward or None).  masks (a list, parity tests): receives
    the block's three ReLU decision masks in execution order."""
    P = ar.PB
    stride = blk.stride
    cs = 1 if blk.pooled_stride else stride  # the 3x3 convolution's own stride
    pooled = stride > cs                     # ... and what is left to a 2x2 average pool
    wa = blk.conv1.weight.view(blk.conv1.out_channels, -1)
    kwa = dict(prec=P, aa=ax, ba=ar.wam(blk.conv1))
    ya, pa = ops.conv1x1(x, wa, stats=True, **kwa) if training else (ops.conv1x1(x, wa, **kwa), None)
    sta = _bn_coeffs(blk.bn1, pa, _pix(ya), training, nbt)
    a_aa = ar.slot()
    aa = ops.bn_apply(ya, sta, relu=True, amax=a_aa)
    wb = _w3x3(blk.conv2)
    kwb = dict(prec=P, aa=a_aa, ba=ar.wam(blk.conv2), stride=cs)
    yb, pb = ops.conv3x3(aa, wb, stats=True, **kwb) if training else (ops.conv3x3(aa, wb, **kwb), None)
    stb = _bn_coeffs(blk.bn2, pb, _pix(yb), training, nbt)
    a_ab = ar.slot()
    ab = ops.bn_apply_pool2(yb, stb, relu=True, amax=a_ab) if pooled else ops.bn_apply(yb, stb, relu=True, amax=a_ab)
    wc = blk.conv3.weight.view(blk.conv3.out_channels, -1)
    kwc = dict(prec=P, aa=a_ab, ba=ar.wam(blk.conv3))
    yc, pc = ops.conv1x1(ab, wc, stats=True, **kwc) if training else (ops.conv1x1(ab, wc, **kwc), None)
    stc = _bn_coeffs(blk.bn3, pc, _pix(yc), training, nbt)
    xd = yd = std = a_xd = None
    a_out = ar.slot()
    if blk.downsample is not None:
        a_xd = ar.slot() if stride > 1 else ax
        if stride == 1:
            xd = x
        elif pooled:
            xd = ops.bn_apply_pool2(x, None, amax=a_xd)
        else:
            xd = ops.subsample2(x, amax=a_xd)  # the pixels a stride-2 1x1 convolution reads
        wd = blk.down_conv.weight.view(blk.down_conv.out_channels, -1)
        kwd = dict(prec=P, aa=a_xd, ba=ar.wam(blk.down_conv))
        yd, pd = ops.conv1x1(xd, wd, stats=True, **kwd) if training else (ops.conv1x1(xd, wd, **kwd), None)
        std = _bn_coeffs(blk.down_bn, pd, _pix(yd), training, nbt)
        out = ops.bn_apply(yc, stc, relu=True, res=yd, res_st=std, want_mask=save, amax=a_out)
    else:
        out = ops.bn_apply(yc, stc, relu=True, res=x, want_mask=save, amax=a_out)
    rec = None
    if save:
        out, rmask = out  # 1-bit ReLU mask of the block output for the backward pass
        rec = (x, ya, sta, aa, yb, stb, ab, yc, stc, xd, yd, std, rmask, (ax, a_aa, a_ab, a_xd))
    if masks is not None:
        masks.extend([aa > 0, _pre_mask(yb, stb) if pooled else ab > 0, out > 0])
    return out, a_out, rec


def block_backward(blk, rec, g, ar, ws, G):
    """Backward of block_forward.  g: dL/d(out).  Fills G[id(param)] for the block's parameters (weight gradients on
    the side stream `ws`) and returns dL/d(x)."""
    x, ya, sta, aa, yb, stb, ab, yc, stc, xd, yd, std, rmask, (ax, a_aa, a_ab, a_xd) = rec
    P = ar.PB
    stride = blk.stride
    cs = 1 if blk.pooled_stride else stride
    pooled = stride > cs
    has_down = blk.downsample is not None
    a_dyc = ar.slot()
    dyc, dg, db, dres = ops.bn_bwd(g, yc, stc, None, 3, act=rmask, want_dres=not has_down, amax=a_dyc)
    G[id(blk.bn3.weight)], G[id(blk.bn3.bias)] = dg, db
    if has_down:
        a_dyd = ar.slot()
        dyd, dg, db, _ = ops.bn_bwd(g, yd, std, None, 3, act=rmask, amax=a_dyd)
        G[id(blk.down_bn.weight)], G[id(blk.down_bn.bias)] = dg, db
    wc = blk.conv3.weight.view(blk.conv3.out_channels, -1)
    dab = ops.matmul_nn(dyc.view(-1, dyc.shape[-1]), wc, prec=P, aa=a_dyc, ba=ar.wam(blk.conv3)).view(ab.shape)
    G[id(blk.conv3.weight)] = ws.run(lambda d_, x_: ops.conv1x1_wgrad(d_, x_, prec=P, aa=a_dyc, ba=a_ab), dyc, ab, keep=(a_dyc, a_ab)).view_as(blk.conv3.weight)
    a_dyb = ar.slot()
    dyb, dg, db, _ = ops.bn_bwd(dab, yb, stb, None, 1, pooled=pooled, amax=a_dyb)
    G[id(blk.bn2.weight)], G[id(blk.bn2.bias)] = dg, db
    planes = blk.conv2.out_channels
    if cs > 1:
        # rows of the data-gradient product are the INPUT pixels; each gathers the taps of dyb that reach it (forward taps: no flip)
        wbt = ops.weight_transpose(_w3x3(blk.conv2), planes, 9, planes, flip=False)
        daa = ops.conv3x3_dgrad_s2(dyb, wbt, aa.shape[1], aa.shape[2], prec=P, aa=a_dyb, ba=ar.wam(blk.conv2))
    else:
        wbt = ops.weight_transpose(_w3x3(blk.conv2), planes, 9, planes, flip=True)
        daa = ops.conv3x3(dyb, wbt, prec=P, aa=a_dyb, ba=ar.wam(blk.conv2))
    G[id(blk.conv2.weight)] = _g3x3(ws.run(lambda d_, x_: ops.conv3x3_wgrad(d_, x_, prec=P, aa=a_dyb, ba=a_aa, stride=cs), dyb, aa, keep=(a_dyb, a_aa)),
                                    planes, planes)
    a_dya = ar.slot()
    dya, dg, db, _ = ops.bn_bwd(daa, ya, sta, None, 1, amax=a_dya)
    G[id(blk.bn1.weight)], G[id(blk.bn1.bias)] = dg, db
    wa = blk.conv1.weight.view(blk.conv1.out_channels, -1)
    if has_down:
        wd = blk.down_conv.weight.view(blk.down_conv.out_channels, -1)
        dxd = ops.matmul_nn(dyd.view(-1, dyd.shape[-1]), wd, prec=P, aa=a_dyd, ba=ar.wam(blk.down_conv)).view(xd.shape)
        G[id(blk.down_conv.weight)] = ws.run(lambda d_, x_: ops.conv1x1_wgrad(d_, x_, prec=P, aa=a_dyd, ba=a_xd), dyd, xd, keep=(a_dyd, a_xd)).view_as(blk.down_conv.weight)
        if stride == 1:
            dx = dxd
        else:
            dx = ops.avgpool2_bwd(dxd) if pooled else ops.subsample2_bwd(dxd, x.shape[1], x.shape[2])
    else:
        dx = dres
    ops.matmul_nn(dya.view(-1, dya.shape[-1]), wa, out=dx.view(-1, dx.shape[-1]), accumulate=True, prec=P, aa=a_dya, ba=ar.wam(blk.conv1))
    G[id(blk.conv1.weight)] = ws.run(lambda d_, x_: ops.conv1x1_wgrad(d_, x_, prec=P, aa=a_dya, ba=ax), dya, x, keep=(a_dya, ax)).view_as(blk.conv1.weight)
    return dx


# --------------------------------------------------------------------------- the eval-mode P16 block body
def blocks_eval_p16(mod, x, E, log=None):
    """The residual blocks of an eval-mode P16 pass (ModifiedResNet / ResNet ``_run_forward_eval_p16``): x, the P16 output of the
    stem's pool, through conv1 -> conv2 -> optional downsample -> conv3 + residual of every block, each convolution ONE launch
    with its fused eval epilogue (E: the encoder's _eval_plan).  log (a list, tools/eval_bounds.py): receives (layer, P16 output)
    of every fused epilogue."""

    def note(name, t):
        if log is not None:
            log.append((name, t))
        return t

    for bi, blk in enumerate(mod.blocks()):
        stride = blk.stride
        aa = note("block%d.conv1" % bi, ops.conv_eval_p16(x, *E[id(blk.conv1.weight)], relu=True))
        if stride > 1 and not blk.pooled_stride:
            ab = ops.conv3x3_s2_eval_p16(aa, *E[id(blk.conv2.weight)], relu=True)
        elif stride > 1 and ops.conv_eval_pool_ok(aa.shape[1], aa.shape[2], blk.conv2.out_channels):
            ab = ops.conv_eval_p16(aa, *E[id(blk.conv2.weight)], relu=True, conv3=True, pool=True)  # conv2 + bn2 + ReLU + AvgPool2d(2)
        else:
            ab = ops.conv_eval_p16(aa, *E[id(blk.conv2.weight)], relu=True, conv3=True)  # (CLIP layer1: the ring-of-rows kernel)
            if stride > 1:
                ab = ops.bn_apply_pool2_p16(ab, None, ab.amax)
        note("block%d.conv2" % bi, ab)
        ident = x
        if blk.downsample is not None:
            if stride == 1:
                xd = x
            elif blk.pooled_stride:
                xd = ops.bn_apply_pool2_p16(x, None, x.amax)
            else:
                xd = ops.subsample2_p16(x)  # the pixels a stride-2 1x1 convolution reads
            ident = note("block%d.downsample" % bi, ops.conv_eval_p16(xd, *E[id(blk.down_conv.weight)], relu=False))
        x = note("block%d.conv3" % bi, ops.conv_eval_p16(ab, *E[id(blk.conv3.weight)], relu=True, res=ident))
    return x


# --------------------------------------------------------------------------- one Function, one base class
class EncoderFn(torch.autograd.Function):
    """forward(images, module, save, *params) -> the encoder's output; grads for every parameter.
    `save` (activations kept for backward) is decided by the caller: inside forward() grad mode is
    always off and ctx.needs_input_grad ignores torch.no_grad()."""

    @staticmethod
    def forward(ctx, images, mod, save, *params):
        if save and not mod.training:
            # eval-mode BatchNorm (running statistics) has a different backward (dy = g * scale, no batch terms);
            # only the train-mode backward is implemented - refuse rather than return batch-statistics gradients
            raise NotImplementedError("%s: gradients through an eval-mode (running-statistics) forward are not "
                                      "implemented; call under torch.no_grad() or in train() mode" % type(mod).__name__)
        out, saved = mod._run_forward(images, save)
        ctx.mod = mod
        ctx.saved = saved
        return out

    @staticmethod
    def backward(ctx, gout):
        mod, saved = ctx.mod, ctx.saved
        ctx.saved = None
        if saved is None:
            raise RuntimeError("backward through an encoder forward that did not save activations")
        return (None, None, None) + tuple(mod._run_backward(saved, gout.contiguous()))


class BottleneckEncoder(nn.Module):
    """Base of the two encoders: a stem, ``layer1`` .. ``layer4`` of Bottlenecks and a pool.  A subclass supplies
    ``_stem_pairs()`` (the stem's (conv, bn) pairs), ``_run_forward(images, save) -> (out, saved)`` and
    ``_run_backward(saved, gout) -> gradients in parameters() order``."""

    def _to_channels_last(self):
        # 3x3 filters live in OHWI memory (channels_last) so the kernels read them in place (the 3-channel filter of CLIP's conv1
        # and the ImageNet 7x7 stem filter are read as stored)
        for m in self.modules():
            if isinstance(m, nn.Conv2d) and m.kernel_size == (3, 3) and m.in_channels % 4 == 0:
                m.weight.data = m.weight.data.contiguous(memory_format=torch.channels_last)

    def blocks(self):
        for layer in (self.layer1, self.layer2, self.layer3, self.layer4):
            for blk in layer:
                yield blk

    def forward(self, x):
        if not x.is_cuda:
            raise RuntimeError("textreid_amd.%s runs on the HIP kernel library only (CUDA tensors); no CPU fallback" % type(self).__name__)
        x = x.type(self.conv1.weight.dtype).contiguous()
        params = list(self.parameters())
        save = torch.is_grad_enabled() and any(p.requires_grad for p in params)
        return EncoderFn.apply(x, self, save, *params)

    def _eval_plan(self, device):
        """Everything of the eval-mode P16 pass that depends on the parameters only, kept until a parameter or BatchNorm buffer is
        replaced or written (ops.parameter_generation(): the library's own writers go through raw pointers): the P16 filters
        (one pack launch), the running-statistics BatchNorm coefficients of every layer and the output-bound coefficients
        (max_n |scale_n| ||w_n||_1, max_n |shift_n|) of every convolution (one launch)."""
        key = (device, ops.parameter_generation()) + tuple((t.data_ptr(), t._version) for t in list(self.parameters()) + list(self.buffers()))
        plan = getattr(self, "_eval_plan_cache", None)
        if plan is not None and plan[0] == key:
            return plan[1]
        WA = weight_amax(self)
        WP = p16_weights(self, WA, False, 1)
        pairs = list(self._stem_pairs())
        for blk in self.blocks():
            pairs += [(blk.conv1, blk.bn1), (blk.conv2, blk.bn2), (blk.conv3, blk.bn3)]
            if blk.downsample is not None:
                pairs.append((blk.down_conv, blk.down_bn))
        sts = {id(bn): _bn_coeffs(bn, None, 0, False) for _, bn in pairs}
        coef = ops.eval_bound_coefs([(conv.weight.detach(), sts[id(bn)].scale, sts[id(bn)].shift) for conv, bn in pairs], device)
        # (the first convolution multiplies its fp32 filter as stored: no P16 copy)
        E = {id(conv.weight): (WP.get(id(conv.weight)), sts[id(bn)], coef[i]) for i, (conv, bn) in enumerate(pairs)}
        self._eval_plan_cache = (key, E, WA, coef)  # (WA / coef own the scalars the P16 filters and rows refer to)
        return E
