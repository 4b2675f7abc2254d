"""ImageNet ResNet-50/101 image encoder on the MI355X kernel library (the rn50 baseline config).

Operator surface of the reference ``lib/models/backbones/resnet.py`` (``Bottleneck`` :54-98, ``ResNet`` :101-175,
``remove_fc`` :178-183, ``model_archs`` :186-212, ``build_resnet`` :215-235): same module tree, parameter and buffer
names, shapes and ``out_channels``, so reference / torchvision state dicts load unchanged.  As in ``m_resnet.py`` the
torch modules are parameter holders only; the whole encoder is ONE ``autograd.Function`` whose forward and backward
are explicit launch sequences on NHWC fp32 activations:

* stem: 7x7 stride-2 convolution straight from the NCHW batch (``ops.stem7_conv``), BatchNorm + ReLU + 3x3 stride-2 max
  pool in one pass (``ops.bn_relu_maxpool``);
* bottlenecks: ``bottleneck.block_forward`` / ``block_backward``, the fp32-tensor data flow both image encoders call; this
  ``Bottleneck`` states ``pooled_stride = False``: the stride is ON the 3x3 convolution (``ops.conv3x3(stride=2)``,
  ``ops.conv3x3_dgrad_s2``, ``ops.conv3x3_wgrad(stride=2)``) and on the 1x1 downsample convolution (``ops.subsample2`` + the
  existing 1x1 GEMM);
* global average pool (``ops.global_avgpool``); the output is ``[B, 2048, 1, 1]`` as the reference returns it.

Convolutions run in ``ops.conv_precision()`` arithmetic, weight gradients on the ``_WgradStream`` side stream.

Eval mode without gradients (``engine.inference``, ``Model.encode_images``) runs the pre-split (P16) data flow of the CLIP
encoder's eval pass (``ResNet._run_forward_eval_p16``) - the same plan builder
(``BottleneckEncoder._eval_plan``) and the same block body (``bottleneck.blocks_eval_p16``): a cached parameter-only plan, every convolution ONE
launch whose epilogue applies the running-statistics BatchNorm, adds the residual, clamps and writes the next P16 operand scaled
by an analytic bound - stem (``ops.stem7_eval_p16``), max pool on the P16 tensor (``ops.maxpool3s2_p16``), stride-2 3x3
convolutions (``ops.conv3x3_s2_eval_p16``), ``ops.subsample2_p16`` in front of the stride-2 downsample convolutions, everything
else ``ops.conv_eval_p16``, and ``ops.global_avgpool_p16``.  ``TRID_EVAL_P16=0``, the other arithmetic modes and shapes
``eval_p16_ok`` declines run the training data flow on running-statistics coefficients (``ops.bn_eval_coeffs``, one ``bn_apply``
pass per convolution).  The training pass itself keeps fp32 activations: the P16 TRAINING flow of the CLIP encoder is not built
for this one.

This file holds what is the ImageNet encoder's own: the holder classes, the stem, the max pool and global pool passes, the size
predicates of the eval pass and the checkpoint loaders.  ``forward``, ``blocks``, the eval plan and the ``autograd.Function`` come
from ``bottleneck.BottleneckEncoder``.
"""

import logging
import os
from collections import namedtuple

import torch
from torch import nn

from .. import ops
from .bottleneck import BottleneckEncoder, ConvArith, _bn_coeffs, _pix, block_backward, block_forward, blocks_eval_p16, p16_eligible, weight_amax
from .m_resnet import _WgradStream  # (the weight-gradient side stream reads m_resnet's schedule switches: it stays there)


class Bottleneck(nn.Module):
    expansion = 4
    pooled_stride = False  # stride 2 is ON the 3x3 convolution and on the 1x1 downsample convolution

    down_conv = property(lambda self: self.downsample[0])
    down_bn = property(lambda self: self.downsample[1])

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


class ResNet(BottleneckEncoder):
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

    def _stem_pairs(self):
        return [(self.conv1, self.bn1)]

    # ------------------------------------------------------------------ forward
    def _run_forward_eval_p16(self, images):
        """Eval mode (test_net.py / inference.py:14-26) on pre-split (P16) activations from the stem to the pool, the data flow of
        ModifiedResNet._run_forward_eval_p16 (the residual blocks: bottleneck.blocks_eval_p16): every convolution is ONE launch whose epilogue applies the running-statistics
        BatchNorm, adds the P16 identity / downsample branch, clamps and writes the next operand as a P16 tensor scaled by the
        analytic bound of csrc/gemm_common.h EvalBound; each epilogue folds the TRUE maximum of what it wrote into a device scalar
        for the next bound.  No fp32 activation, no amax pass, no BatchNorm pass between the first and the last kernel; the only
        passes that are not convolutions are the max pool, the three even-pixel subsamples and the global average pool."""
        E = self._eval_plan(images.device)
        _, st1, c1 = E[id(self.conv1.weight)]
        a1 = ops.stem7_eval_p16(images, self.conv1.weight.detach(), st1, c1, ops.amax(images))
        feat = ops.global_avgpool_p16(blocks_eval_p16(self, ops.maxpool3s2_p16(a1), E))
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
