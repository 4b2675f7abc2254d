"""ImageNet ResNet-50/101 image encoder on the MI355X kernel library (the rn50 baseline config).

Operator surface of the reference ``lib/models/backbones/resnet.py`` (``Bottleneck`` :54-98, ``ResNet`` :101-175,
``remove_fc`` :178-183, ``model_archs`` :186-212, ``build_resnet`` :215-235): same module tree, parameter and buffer
names, shapes and ``out_channels``, so reference / torchvision state dicts load unchanged.  As in ``m_resnet.py`` the
torch modules are parameter holders only; the whole encoder is ONE ``autograd.Function`` whose forward and backward
are explicit launch sequences on NHWC fp32 activations:

* stem: 7x7 stride-2 convolution straight from the NCHW batch (``ops.stem7_conv``), BatchNorm + ReLU + 3x3 stride-2 max
  pool in one pass (``ops.bn_relu_maxpool``);
* bottlenecks: the fp32-tensor data flow of ``m_resnet.block_forward`` with the stride ON the 3x3 convolution
  (``ops.conv3x3(stride=2)``, ``ops.conv3x3_dgrad_s2``, ``ops.conv3x3_wgrad(stride=2)``) and on the 1x1 downsample
  convolution (``ops.subsample2`` + the existing 1x1 GEMM);
* global average pool (``ops.global_avgpool``); the output is ``[B, 2048, 1, 1]`` as the reference returns it.

Convolutions run in ``ops.conv_precision()`` arithmetic, weight gradients on the ``_WgradStream`` side stream.

Eval mode without gradients (``engine.inference``, ``Model.encode_images``) runs the pre-split (P16) data flow of the CLIP
encoder's eval pass (``ResNet._run_forward_eval_p16``): a cached parameter-only plan, every convolution ONE
launch whose epilogue applies the running-statistics BatchNorm, adds the residual, clamps and writes the next P16 operand scaled
by an analytic bound - stem (``ops.stem7_eval_p16``), max pool on the P16 tensor (``ops.maxpool3s2_p16``), stride-2 3x3
convolutions (``ops.conv3x3_s2_eval_p16``), ``ops.subsample2_p16`` in front of the stride-2 downsample convolutions, everything
else ``ops.conv_eval_p16``, and ``ops.global_avgpool_p16``.  ``TRID_EVAL_P16=0``, the other arithmetic modes and shapes
``eval_p16_ok`` declines run the training data flow on running-statistics coefficients (``ops.bn_eval_coeffs``, one ``bn_apply``
pass per convolution).  The training pass itself keeps fp32 activations: the P16 TRAINING flow of the CLIP encoder is not built
for this one.
"""

import logging
import os
from collections import namedtuple

import torch
from torch import nn

from .. import ops
from .m_resnet import ConvArith, _bn_coeffs, _g3x3, _w3x3, _WgradStream, p16_eligible, p16_weights, weight_amax


class Bottleneck(nn.Module):
    expansion = 4

    def __init__(self, inplanes, planes, stride=1, downsample=None, dilation=1):
        super().__init__()
        if dilation != 1:
            raise NotImplementedError("MODEL.RESNET.RES5_DILATION != 1: dilated 3x3 convolutions are not implemented")
        assert stride in (1, 2), "3x3 convolutions are implemented for stride 1 and 2"
        self.conv1 = nn.Conv2d(inplanes, planes, kernel_size=1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = nn.Conv2d(planes, planes, kernel_size=3, stride=stride, padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.conv3 = nn.Conv2d(planes, planes * 4, kernel_size=1, bias=False)
        self.bn3 = nn.BatchNorm2d(planes * 4)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = downsample
        self.stride = stride

    def forward(self, x):  # pragma: no cover - the encoder runs as one fused Function
        raise RuntimeError("Bottleneck is a parameter holder; call ResNet.forward")


def _pix(t):
    return t.numel() // t.shape[-1]


def block_forward(blk, x, ax, ar, training, save, nbt):
    """One Bottleneck (resnet.py:78-98) on NHWC activations.  x: block input, ax: its amax scalar (or None).  Returns
    (out, amax scalar of out, record for block_backward or None)."""
    P = ar.PB
    stride = blk.stride
    wa = blk.conv1.weight.view(blk.conv1.out_channels, -1)
    kwa = dict(prec=P, aa=ax, ba=ar.wam(blk.conv1))
    ya, pa = ops.conv1x1(x, wa, stats=True, **kwa) if training else (ops.conv1x1(x, wa, **kwa), None)
    sta = _bn_coeffs(blk.bn1, pa, _pix(ya), training, nbt)
    a_aa = ar.slot()
    aa = ops.bn_apply(ya, sta, relu=True, amax=a_aa)
    wb = _w3x3(blk.conv2)
    kwb = dict(prec=P, aa=a_aa, ba=ar.wam(blk.conv2), stride=stride)
    yb, pb = ops.conv3x3(aa, wb, stats=True, **kwb) if training else (ops.conv3x3(aa, wb, **kwb), None)
    stb = _bn_coeffs(blk.bn2, pb, _pix(yb), training, nbt)
    a_ab = ar.slot()
    ab = ops.bn_apply(yb, stb, relu=True, amax=a_ab)
    wc = blk.conv3.weight.view(blk.conv3.out_channels, -1)
    kwc = dict(prec=P, aa=a_ab, ba=ar.wam(blk.conv3))
    yc, pc = ops.conv1x1(ab, wc, stats=True, **kwc) if training else (ops.conv1x1(ab, wc, **kwc), None)
    stc = _bn_coeffs(blk.bn3, pc, _pix(yc), training, nbt)
    xd = yd = std = a_xd = None
    a_out = ar.slot()
    if blk.downsample is not None:
        a_xd = ar.slot() if stride > 1 else ax
        xd = ops.subsample2(x, amax=a_xd) if stride > 1 else x  # the pixels a stride-2 1x1 convolution reads
        wd = blk.downsample[0].weight.view(blk.downsample[0].out_channels, -1)
        kwd = dict(prec=P, aa=a_xd, ba=ar.wam(blk.downsample[0]))
        yd, pd = ops.conv1x1(xd, wd, stats=True, **kwd) if training else (ops.conv1x1(xd, wd, **kwd), None)
        std = _bn_coeffs(blk.downsample[1], pd, _pix(yd), training, nbt)
        out = ops.bn_apply(yc, stc, relu=True, res=yd, res_st=std, want_mask=save, amax=a_out)
    else:
        out = ops.bn_apply(yc, stc, relu=True, res=x, want_mask=save, amax=a_out)
    rec = None
    if save:
        out, rmask = out  # 1-bit ReLU mask of the block output for the backward pass
        rec = (x, ya, sta, aa, yb, stb, ab, yc, stc, xd, yd, std, rmask, (ax, a_aa, a_ab, a_xd))
    return out, a_out, rec


def block_backward(blk, rec, g, ar, ws, G):
    """Backward of block_forward.  g: dL/d(out).  Fills G[id(param)] for the block's parameters (weight gradients on the
    side stream `ws`) and returns dL/d(x)."""
    x, ya, sta, aa, yb, stb, ab, yc, stc, xd, yd, std, rmask, (ax, a_aa, a_ab, a_xd) = rec
    P = ar.PB
    stride = blk.stride
    has_down = blk.downsample is not None
    a_dyc = ar.slot()
    dyc, dg, db, dres = ops.bn_bwd(g, yc, stc, None, 3, act=rmask, want_dres=not has_down, amax=a_dyc)
    G[id(blk.bn3.weight)], G[id(blk.bn3.bias)] = dg, db
    if has_down:
        a_dyd = ar.slot()
        dyd, dg, db, _ = ops.bn_bwd(g, yd, std, None, 3, act=rmask, amax=a_dyd)
        G[id(blk.downsample[1].weight)], G[id(blk.downsample[1].bias)] = dg, db
    wc = blk.conv3.weight.view(blk.conv3.out_channels, -1)
    dab = ops.matmul_nn(dyc.view(-1, dyc.shape[-1]), wc, prec=P, aa=a_dyc, ba=ar.wam(blk.conv3)).view(ab.shape)
    G[id(blk.conv3.weight)] = ws.run(lambda d_, x_: ops.conv1x1_wgrad(d_, x_, prec=P, aa=a_dyc, ba=a_ab), dyc, ab, keep=(a_dyc, a_ab)).view_as(blk.conv3.weight)
    a_dyb = ar.slot()
    dyb, dg, db, _ = ops.bn_bwd(dab, yb, stb, None, 1, amax=a_dyb)
    G[id(blk.bn2.weight)], G[id(blk.bn2.bias)] = dg, db
    planes = blk.conv2.out_channels
    if stride > 1:
        # rows of the data-gradient product are the INPUT pixels; each gathers the taps of dyb that reach it (forward taps: no flip)
        wbt = ops.weight_transpose(_w3x3(blk.conv2), planes, 9, planes, flip=False)
        daa = ops.conv3x3_dgrad_s2(dyb, wbt, aa.shape[1], aa.shape[2], prec=P, aa=a_dyb, ba=ar.wam(blk.conv2))
    else:
        wbt = ops.weight_transpose(_w3x3(blk.conv2), planes, 9, planes, flip=True)
        daa = ops.conv3x3(dyb, wbt, prec=P, aa=a_dyb, ba=ar.wam(blk.conv2))
    G[id(blk.conv2.weight)] = _g3x3(ws.run(lambda d_, x_: ops.conv3x3_wgrad(d_, x_, prec=P, aa=a_dyb, ba=a_aa, stride=stride), dyb, aa, keep=(a_dyb, a_aa)),
                                    planes, planes)
    a_dya = ar.slot()
    dya, dg, db, _ = ops.bn_bwd(daa, ya, sta, None, 1, amax=a_dya)
    G[id(blk.bn1.weight)], G[id(blk.bn1.bias)] = dg, db
    wa = blk.conv1.weight.view(blk.conv1.out_channels, -1)
    if has_down:
        wd = blk.downsample[0].weight.view(blk.downsample[0].out_channels, -1)
        dxd = ops.matmul_nn(dyd.view(-1, dyd.shape[-1]), wd, prec=P, aa=a_dyd, ba=ar.wam(blk.downsample[0])).view(xd.shape)
        G[id(blk.downsample[0].weight)] = ws.run(lambda d_, x_: ops.conv1x1_wgrad(d_, x_, prec=P, aa=a_dyd, ba=a_xd), dyd, xd, keep=(a_dyd, a_xd)).view_as(blk.downsample[0].weight)
        dx = ops.subsample2_bwd(dxd, x.shape[1], x.shape[2]) if stride > 1 else dxd
    else:
        dx = dres
    ops.matmul_nn(dya.view(-1, dya.shape[-1]), wa, out=dx.view(-1, dx.shape[-1]), accumulate=True, prec=P, aa=a_dya, ba=ar.wam(blk.conv1))
    G[id(blk.conv1.weight)] = ws.run(lambda d_, x_: ops.conv1x1_wgrad(d_, x_, prec=P, aa=a_dya, ba=ax), dya, x, keep=(a_dya, ax)).view_as(blk.conv1.weight)
    return dx


P16_LIMIT_BYTES = 1 << 31  # the P16 kernels address their operands with 31-bit byte offsets


def eval_p16_shape_ok(B, Hi, Wi):
    """Do the eval-mode P16 kernels take a [B, 3, Hi, Wi] batch?  True while the image batch and the two largest activations of
    the pass - the stem's output [B, Ho, Wo, 64] and layer1's block outputs [B, Hp, Wp, 256], 4 bytes per element, with
    Ho = (Hi - 1) // 2 + 1 and Hp = (Ho - 1) // 2 + 1 (likewise Wo, Wp) - each stay below P16_LIMIT_BYTES (2 GB: B <= 682 at
    384 x 128); every map size, odd ones included, is covered.  Larger batches are declined (the unfused path takes them)."""
    if B < 1 or Hi < 1 or Wi < 1:
        return False
    Ho, Wo = (Hi - 1) // 2 + 1, (Wi - 1) // 2 + 1
    Hp, Wp = (Ho - 1) // 2 + 1, (Wo - 1) // 2 + 1
    return max(B * 3 * Hi * Wi, B * Ho * Wo * 64, B * Hp * Wp * 256) * 4 < P16_LIMIT_BYTES


def eval_p16_ok(mod, images):
    """The eligibility predicate of ResNet._run_forward_eval_p16: a contiguous fp32 [B, 3, Hi, Wi] batch of a size
    eval_p16_shape_ok accepts, on a module whose block channel counts are multiples of the 32-wide K group (every Bottleneck
    architecture) behind the 3 -> 64 channel 7x7 stem."""
    return (images.dim() == 4 and images.shape[1] == 3 and images.dtype == torch.float32 and images.is_contiguous()
            and tuple(mod.conv1.weight.shape) == (64, 3, 7, 7) and mod.conv1.weight.is_contiguous() and p16_eligible(mod, 32)
            and eval_p16_shape_ok(images.shape[0], images.shape[2], images.shape[3]))


class _EncoderFn(torch.autograd.Function):
    """forward(images, module, save, *params) -> [B, 2048, 1, 1]; grads for every parameter (m_resnet._EncoderFn's contract)."""

    @staticmethod
    def forward(ctx, images, mod, save, *params):
        if save and not mod.training:
            raise NotImplementedError("ResNet: gradients through an eval-mode (running-statistics) forward are not "
                                      "implemented; call under torch.no_grad() or in train() mode")
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


class ResNet(nn.Module):
    def __init__(self, model_arch, res5_stride=2, res5_dilation=1, pretrained=None, root="./"):
        """pretrained: a checkpoint path (``torch.load`` -> ``remove_fc`` -> ``load_state_dict``), or None: the architecture's
        ImageNet file under ``root``/pretrained/imagenet/ when it is there, else the ``_init_weight`` initialisation with a
        warning.  Nothing is ever downloaded."""
        super().__init__()
        if res5_stride not in (1, 2):
            raise NotImplementedError("MODEL.RESNET.RES5_STRIDE must be 1 or 2")
        if res5_dilation != 1:
            raise NotImplementedError("MODEL.RESNET.RES5_DILATION != 1: dilated 3x3 convolutions are not implemented")
        block, layers = model_arch.block, model_arch.stage
        if block is not Bottleneck:
            raise NotImplementedError("only the Bottleneck architectures (resnet50 / resnet101) run on the kernel library")
        self.inplanes = 64
        self.conv1 = nn.Conv2d(3, 64, kernel_size=7, stride=2, padding=3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(kernel_size=3, stride=2, padding=1)
        self.layer1 = self._make_layer(block, 64, layers[0])
        self.layer2 = self._make_layer(block, 128, layers[1], stride=2)
        self.layer3 = self._make_layer(block, 256, layers[2], stride=2)
        self.layer4 = self._make_layer(block, 512, layers[3], stride=res5_stride)
        self._init_weight()
        self._load_pretrained(model_arch, pretrained, root)
        self.avgpool = nn.AdaptiveAvgPool2d((1, 1))
        self.out_channels = 512 * block.expansion
        self._to_channels_last()

    def _make_layer(self, block, planes, blocks, stride=1):
        downsample = None
        if stride != 1 or self.inplanes != planes * block.expansion:
            downsample = nn.Sequential(
                nn.Conv2d(self.inplanes, planes * block.expansion, kernel_size=1, stride=stride, bias=False),
                nn.BatchNorm2d(planes * block.expansion),
            )
        layers = [block(self.inplanes, planes, stride, downsample)]
        self.inplanes = planes * block.expansion
        layers += [block(self.inplanes, planes) for _ in range(1, blocks)]
        return nn.Sequential(*layers)

    def _init_weight(self):
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
            elif isinstance(m, nn.BatchNorm2d):
                nn.init.constant_(m.weight, 1)
                nn.init.constant_(m.bias, 0)

    def _load_pretrained(self, model_arch, pretrained, root):
        path = pretrained
        if path is None:
            path = os.path.join(root, "pretrained", "imagenet", model_arch.file) if model_arch.file else None
            if path is None or not os.path.exists(path):
                logging.getLogger("PersonSearch.train").warning("ImageNet weights %s not found: random init", path)
                return
        self.load_state_dict(remove_fc(torch.load(path, map_location="cpu")))

    def _to_channels_last(self):
        # 3x3 filters live in OHWI memory (channels_last) so the kernels read them in place; the 7x7 stem filter is read as stored
        for m in self.modules():
            if isinstance(m, nn.Conv2d) and m.kernel_size == (3, 3):
                m.weight.data = m.weight.data.contiguous(memory_format=torch.channels_last)

    def blocks(self):
        for layer in (self.layer1, self.layer2, self.layer3, self.layer4):
            for blk in layer:
                yield blk

    # ------------------------------------------------------------------ forward
    def forward(self, x):
        if not x.is_cuda:
            raise RuntimeError("textreid_amd.ResNet runs on the HIP kernel library only (CUDA tensors); no CPU fallback")
        x = x.type(self.conv1.weight.dtype).contiguous()
        params = list(self.parameters())
        save = torch.is_grad_enabled() and any(p.requires_grad for p in params)
        return _EncoderFn.apply(x, self, save, *params)

    def _eval_plan(self, device):
        """Everything of the eval-mode pass that depends on the parameters only, kept until a parameter or BatchNorm buffer is
        replaced or written (m_resnet.ModifiedResNet._eval_plan's key: ops.parameter_generation(), data pointers, versions): the
        P16 filters (one pack launch), the running-statistics BatchNorm coefficients of the 53 / 104 layers and the output-bound
        coefficients of every convolution (one launch)."""
        key = (device, ops.parameter_generation()) + tuple((t.data_ptr(), t._version) for t in list(self.parameters()) + list(self.buffers()))
        plan = getattr(self, "_eval_plan_cache", None)
        if plan is not None and plan[0] == key:
            return plan[1]
        WA = weight_amax(self)
        WP = p16_weights(self, WA, False, 1)
        pairs = [(self.conv1, self.bn1)]
        for blk in self.blocks():
            pairs += [(blk.conv1, blk.bn1), (blk.conv2, blk.bn2), (blk.conv3, blk.bn3)]
            if blk.downsample is not None:
                pairs.append((blk.downsample[0], blk.downsample[1]))
        sts = {id(bn): _bn_coeffs(bn, None, 0, False) for _, bn in pairs}
        coef = ops.eval_bound_coefs([(conv.weight.detach(), sts[id(bn)].scale, sts[id(bn)].shift) for conv, bn in pairs], device)
        # (the stem multiplies its fp32 filter as stored: no P16 copy)
        E = {id(conv.weight): (WP.get(id(conv.weight)), sts[id(bn)], coef[i]) for i, (conv, bn) in enumerate(pairs)}
        self._eval_plan_cache = (key, E, WA, coef)  # (WA / coef own the scalars the P16 filters and rows refer to)
        return E

    def _run_forward_eval_p16(self, images):
        """Eval mode (test_net.py / inference.py:14-26) on pre-split (P16) activations from the stem to the pool, the data flow of
        m_resnet.ModifiedResNet._run_forward_eval_p16: every convolution is ONE launch whose epilogue applies the running-statistics
        BatchNorm, adds the P16 identity / downsample branch, clamps and writes the next operand as a P16 tensor scaled by the
        analytic bound of csrc/gemm_common.h EvalBound; each epilogue folds the TRUE maximum of what it wrote into a device scalar
        for the next bound.  No fp32 activation, no amax pass, no BatchNorm pass between the first and the last kernel; the only
        passes that are not convolutions are the max pool, the three even-pixel subsamples and the global average pool."""
        E = self._eval_plan(images.device)
        _, st1, c1 = E[id(self.conv1.weight)]
        a1 = ops.stem7_eval_p16(images, self.conv1.weight.detach(), st1, c1, ops.amax(images))
        x = ops.maxpool3s2_p16(a1)
        for blk in self.blocks():
            aa = ops.conv_eval_p16(x, *E[id(blk.conv1.weight)], relu=True)
            if blk.stride > 1:
                ab = ops.conv3x3_s2_eval_p16(aa, *E[id(blk.conv2.weight)], relu=True)
            else:
                ab = ops.conv_eval_p16(aa, *E[id(blk.conv2.weight)], relu=True, conv3=True)
            ident = x
            if blk.downsample is not None:
                xd = ops.subsample2_p16(x) if blk.stride > 1 else x  # the pixels a stride-2 1x1 convolution reads
                ident = ops.conv_eval_p16(xd, *E[id(blk.downsample[0].weight)], relu=False)
            x = ops.conv_eval_p16(ab, *E[id(blk.conv3.weight)], relu=True, res=ident)
        feat = ops.global_avgpool_p16(x)
        return feat.view(feat.shape[0], feat.shape[1], 1, 1)

    def _run_forward(self, images, save):
        training = self.training
        cp = ops.conv_precision()
        if not training and not save and ops.USE_EVAL_P16 and ops.USE_P16 and cp == 16 and eval_p16_ok(self, images):
            return self._run_forward_eval_p16(images), None
        ar = ConvArith(images.device, weight_amax(self) if cp in (16, 1) else {}, 1 if cp == 1 else None)
        nbt = []  # num_batches_tracked buffers, incremented together at the end of the pass
        # ---- stem (resnet.py:156-159)
        w1 = self.conv1.weight.detach()
        y1, p1 = ops.stem7_conv(images, w1, stats=True) if training else (ops.stem7_conv(images, w1, stats=False), None)
        st1 = _bn_coeffs(self.bn1, p1, _pix(y1), training, nbt)
        ax = ar.slot()
        x = ops.bn_relu_maxpool(y1, st1, amax=ax)
        S = {"stem": (images, y1, st1), "wamax": ar.WA, "prec": ar.PB, "blocks": []} if save else None
        # ---- residual layers (resnet.py:161-164)
        for blk in self.blocks():
            x, ax, rec = block_forward(blk, x, ax, ar, training, save, nbt)
            if save:
                S["blocks"].append(rec)
        if nbt:
            torch._foreach_add_(nbt, 1)  # one launch instead of one per BatchNorm layer
        # ---- global average pool (resnet.py:165)
        if save:
            S["map"] = (x.shape[1], x.shape[2])
        feat = ops.global_avgpool(x)
        return feat.view(feat.shape[0], feat.shape[1], 1, 1), S

    # ------------------------------------------------------------------ backward
    def _run_backward(self, S, gout):
        G = {}
        ws = _WgradStream(gout.device)
        ar = ConvArith(gout.device, S.get("wamax", {}), S.get("prec"))  # the forward's conv arithmetic (its amax scalars are reused here)
        g = ops.global_avgpool_bwd(gout.reshape(gout.shape[0], gout.shape[1]), *S["map"])
        for blk, rec in zip(reversed(list(self.blocks())), reversed(S["blocks"])):
            g = block_backward(blk, rec, g, ar, ws, G)
        S["blocks"] = None
        images, y1, st1 = S["stem"]
        gy = ops.bn_relu_maxpool_bwd(g, y1, st1)  # gradient of relu(bn1(y1)); bn_bwd applies the ReLU mask
        dy1, dg, db, _ = ops.bn_bwd(gy, y1, st1, None, 1)
        G[id(self.bn1.weight)], G[id(self.bn1.bias)] = dg, db
        G[id(self.conv1.weight)] = ws.run(lambda d_, i_: ops.stem7_conv_wgrad(i_, d_), dy1, images)
        ws.join()
        return [G.get(id(p)) for p in self.parameters()]


def remove_fc(state_dict):
    """The checkpoint without its classifier (``fc.*``): torchvision's ImageNet files carry one, the encoder does not."""
    for key in [k for k in state_dict if k.startswith("fc.")]:
        del state_dict[key]
    return state_dict


# (block, blocks per stage, file name of the ImageNet checkpoint under ROOT/pretrained/imagenet/)
resnet = namedtuple("resnet", ["block", "stage", "file"])
model_archs = {
    "resnet50": resnet(Bottleneck, [3, 4, 6, 3], "resnet50-19c8e357.pth"),
    "resnet101": resnet(Bottleneck, [3, 4, 23, 3], "resnet101-5d3b4d8f.pth"),
}


def build_resnet(cfg):
    arch = cfg.MODEL.VISUAL_MODEL
    if arch not in model_archs:
        raise NotImplementedError(arch)
    if cfg.MODEL.RESNET.RES5_DILATION != 1:
        raise NotImplementedError("MODEL.RESNET.RES5_DILATION = %r: dilated 3x3 convolutions are not implemented" % (cfg.MODEL.RESNET.RES5_DILATION,))
    if cfg.MODEL.FREEZE:
        raise NotImplementedError("MODEL.FREEZE = True: a partly frozen image encoder is not implemented")
    return ResNet(model_archs[arch], cfg.MODEL.RESNET.RES5_STRIDE, cfg.MODEL.RESNET.RES5_DILATION,
                  pretrained=cfg.MODEL.RESNET.PRETRAINED, root=cfg.ROOT)
