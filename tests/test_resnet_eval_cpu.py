"""Host-side tests of the eval-mode P16 data flow of the ImageNet ResNet image encoder (textreid_amd/backbones/resnet.py,
csrc/resnet_eval.hip, the A_CONV_S2 loader of csrc/gemm_p16.hip): the built library exports the new entry points, ops has the
wrappers, the eligibility predicate answers what its docstring says, and the fp64 restatement the GPU tests compare against agrees
with torch's own operators."""

import pytest
import torch
import torch.nn.functional as F

NEW_ENTRIES = ["trid_stem7_eval_p16", "trid_maxpool3s2_p16", "trid_conv3x3_s2_eval_p16", "trid_conv3x3_s2_eval_p16_ok",
               "trid_subsample2_p16", "trid_global_avgpool_p16"]
NEW_WRAPPERS = ["stem7_eval_p16", "maxpool3s2_p16", "conv3x3_s2_eval_p16", "conv3x3_s2_eval_ok", "subsample2_p16", "global_avgpool_p16"]


def test_library_exports_the_eval_entry_points_and_ops_has_the_wrappers():
    import textreid_amd.lib as L
    from textreid_amd import ops

    lib = L.load()
    for name in NEW_ENTRIES:
        assert name in L.EXPORTS, name          # declared in include/textreid_hip.h
        assert hasattr(lib, name), name         # exported by the built library
    for name in NEW_WRAPPERS:
        assert callable(getattr(ops, name, None)), name
    # a pure shape query needs no GPU: channel counts in multiples of 32, tensors below 2 GB
    assert lib.trid_conv3x3_s2_eval_p16_ok(2, 9, 5, 128, 128) == 1
    assert lib.trid_conv3x3_s2_eval_p16_ok(128, 48, 16, 256, 256) == 1
    assert lib.trid_conv3x3_s2_eval_p16_ok(2, 9, 5, 48, 128) == 0
    assert lib.trid_conv3x3_s2_eval_p16_ok(2, 9, 5, 128, 100) == 0
    assert lib.trid_conv3x3_s2_eval_p16_ok(4096, 96, 32, 128, 128) == 0  # 6.4 GB of input


def test_eligibility_predicate_is_what_its_docstring_says():
    from textreid_amd.backbones import resnet as R

    assert R.P16_LIMIT_BYTES == 1 << 31
    # the rn50 baseline's geometry: 384 x 128 -> stem 192 x 64 x 64 channels = 3 MB per image: B <= 682
    assert R.eval_p16_shape_ok(128, 384, 128) and R.eval_p16_shape_ok(512, 384, 128) and R.eval_p16_shape_ok(682, 384, 128)
    assert not R.eval_p16_shape_ok(683, 384, 128) and not R.eval_p16_shape_ok(1024, 384, 128)
    # odd sizes at every stride-2 step, and the smallest maps, are covered
    assert R.eval_p16_shape_ok(2, 72, 40) and R.eval_p16_shape_ok(3, 37, 21) and R.eval_p16_shape_ok(1, 1, 1)
    assert not R.eval_p16_shape_ok(0, 72, 40)
    m = R.ResNet(R.resnet(R.Bottleneck, [1, 1, 1, 1], None))
    x = torch.zeros(2, 3, 72, 40)
    assert R.eval_p16_ok(m, x)
    assert not R.eval_p16_ok(m, x.double())                                   # fp32 batches only
    assert not R.eval_p16_ok(m, x.permute(0, 1, 3, 2))                        # ... contiguous NCHW
    assert not R.eval_p16_ok(m, torch.zeros(2, 4, 72, 40))                    # ... with 3 channels


def test_module_has_the_plan_and_the_eval_forward():
    from textreid_amd.backbones.resnet import ResNet

    assert callable(getattr(ResNet, "_eval_plan", None)) and callable(getattr(ResNet, "_run_forward_eval_p16", None))


@pytest.mark.parametrize("H,W", [(9, 5), (8, 4), (2, 1)])
def test_restatement_agrees_with_torch_operators(H, W):
    """tests/resnet_eval_ref.py against F.conv2d / F.max_pool2d in fp64 (the restatement is what the GPU tests trust)."""
    import resnet_eval_ref as ref

    g = torch.Generator().manual_seed(11)
    x = torch.randn(2, H, W, 8, generator=g, dtype=torch.float64)
    w3 = torch.randn(6, 3, 3, 8, generator=g, dtype=torch.float64)
    want = F.conv2d(x.permute(0, 3, 1, 2), w3.permute(0, 3, 1, 2), stride=2, padding=1).permute(0, 2, 3, 1)
    assert torch.allclose(ref.conv(x, w3, 2, 1), want, rtol=0, atol=1e-12)
    w1 = torch.randn(6, 1, 1, 8, generator=g, dtype=torch.float64)
    want = F.conv2d(x.permute(0, 3, 1, 2), w1.permute(0, 3, 1, 2), stride=2).permute(0, 2, 3, 1)
    assert torch.allclose(ref.conv(x, w1, 2, 0), want, rtol=0, atol=1e-12)
    w7 = torch.randn(6, 7, 7, 8, generator=g, dtype=torch.float64)
    want = F.conv2d(x.permute(0, 3, 1, 2), w7.permute(0, 3, 1, 2), stride=2, padding=3).permute(0, 2, 3, 1)
    assert torch.allclose(ref.conv(x, w7, 2, 3), want, rtol=0, atol=1e-12)
    xn = x - 10.0  # all negative: a zero-padded pool would return zeros at the border
    want = F.max_pool2d(xn.permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1)
    assert torch.equal(ref.maxpool3s2(xn), want)


def test_restated_encoder_is_the_torch_module_graph():
    """The fp64 encoder restatement against the same graph written with torch.nn.functional on the module's own tensors."""
    import resnet_eval_ref as ref
    from textreid_amd.backbones.resnet import Bottleneck, ResNet, resnet

    torch.manual_seed(5)
    m = ResNet(resnet(Bottleneck, [1, 1, 1, 1], None), 2).double().eval()
    for bn in [b for b in m.modules() if isinstance(b, torch.nn.BatchNorm2d)]:
        bn.running_mean.normal_(0, 0.3)
        bn.running_var.uniform_(0.5, 2.0)
    x = torch.randn(2, 3, 37, 21, dtype=torch.float64)

    def cb(t, conv, bn, relu):
        t = F.batch_norm(F.conv2d(t, conv.weight, None, conv.stride, conv.padding), bn.running_mean, bn.running_var, bn.weight, bn.bias, False, 0.0, bn.eps)
        return F.relu(t) if relu else t

    with torch.no_grad():
        t = F.max_pool2d(cb(x, m.conv1, m.bn1, True), 3, 2, 1)
        for blk in m.blocks():
            a = cb(cb(cb(t, blk.conv1, blk.bn1, True), blk.conv2, blk.bn2, True), blk.conv3, blk.bn3, False)
            t = F.relu(a + (t if blk.downsample is None else cb(t, blk.downsample[0], blk.downsample[1], False)))
        want = t.mean(dim=(2, 3))
    got = ref.encoder(m, x)
    assert float((got - want).abs().max()) <= 1e-10 * float(want.abs().max())
