"""GPU tests of the ImageNet ResNet-50/101 image encoder (textreid_amd/backbones/resnet.py, csrc/resnet_ops.hip and the
stride-2 gathers of csrc/gemm.hip / gemm_bf16.hip).

Kernel cases compare against torch on the CPU in fp64 at test_kernels_gpu.TOL (2e-5 of the output scale), or exactly where
both sides are exact (dyadic data: the pools, the subsample).  The encoder is held to tests/golden/resnet.npz (captured from
the reference module, tests/golden/make_golden_resnet.py) at the project's flat TOL = 1e-3; the full-size and bitwise checks
follow tests/test_baseline_gpu.py."""

import hashlib
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import oracle.fill as OF  # noqa: E402
from oracle.fill import digest, digest_err, grad_floor  # noqa: E402

TOL_KERNEL = 2e-5  # tests/test_kernels_gpu.py:38
TOL = 1e-3         # tests/test_model_gpu.py:19


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import textreid_amd  # noqa: F401

    return torch.device("cuda")


@pytest.fixture(scope="module", autouse=True)
def stream_state_left_as_found():
    """This module records steps and opens side streams: torch's capture stream and the position of its 32-stream pool are put
    back as they were found (see tests/test_baseline_gpu.py)."""
    if not torch.cuda.is_available():
        yield
        return
    made = [0]
    orig_new = torch.cuda.Stream.__new__
    had_capture_stream = torch.cuda.graph.default_capture_stream

    def counting_new(cls, *a, **kw):
        if not ({"stream_ptr", "stream_id"} & set(kw)):
            made[0] += 1
        return orig_new(cls, *a, **kw)

    torch.cuda.Stream.__new__ = staticmethod(counting_new)
    try:
        yield
    finally:
        torch.cuda.Stream.__new__ = staticmethod(orig_new)
        torch.cuda.synchronize()
        torch.cuda.graph.default_capture_stream = had_capture_stream
        for _ in range(-made[0] % 32):
            torch.cuda.Stream()


def rel(a, b):
    a = torch.as_tensor(a).detach().double().cpu()
    b = torch.as_tensor(b).detach().double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


# --------------------------------------------------------------------------- stem convolution
@pytest.mark.parametrize("shape", [(2, 3, 96, 32), (3, 3, 90, 30), (1, 3, 13, 9)], ids=["96x32", "90x30", "13x9"])
def test_stem7_conv_forward_wgrad_and_partials(gpu, shape):
    """nn.Conv2d(3, 64, 7, stride=2, padding=3) from the NCHW batch: output, weight gradient (autograd) and the per-128-row
    (mean, M2) partials finalised by bn_finalize against the batch mean / biased variance.  1536 rows (whole tiles), 2025 rows
    (odd maps, a partial last tile) and 35 rows (less than one wave's worth of pixels in the last wave)."""
    from textreid_amd import ops

    x = OF.randn("stem7:x%s" % (shape,), shape, 3)
    w = OF.randn("stem7:w", (64, 3, 7, 7), 3, 0.1)
    xr, wr = x.double(), w.double().requires_grad_(True)
    yr = F.conv2d(xr, wr, stride=2, padding=3)
    gy = OF.randn("stem7:g%s" % (shape,), tuple(yr.shape), 3)
    (yr * gy.double()).sum().backward()
    y, parts = ops.stem7_conv(x.to(gpu), w.to(gpu))
    Ho, Wo = (shape[2] - 1) // 2 + 1, (shape[3] - 1) // 2 + 1
    assert tuple(y.shape) == (shape[0], Ho, Wo, 64) and tuple(parts.shape) == ((shape[0] * Ho * Wo + 127) // 128, 64, 2)
    errs = {"y": rel(nchw(y), yr)}
    dw = ops.stem7_conv_wgrad(x.to(gpu), nhwc(gy).to(gpu))
    assert tuple(dw.shape) == (64, 3, 7, 7) and dw.is_contiguous()
    errs["dw"] = rel(dw, wr.grad)
    gamma, beta = torch.ones(64, device=gpu), torch.zeros(64, device=gpu)
    st = ops.bn_finalize(parts, shape[0] * Ho * Wo, gamma, beta, None, None)
    mean, var = yr.detach().mean(dim=(0, 2, 3)), yr.detach().var(dim=(0, 2, 3), unbiased=False)
    errs["mean"] = float((st.mean.double().cpu() - mean).abs().max() / yr.detach().abs().max())
    errs["invstd"] = rel(st.invstd, 1.0 / torch.sqrt(var + ops.BN_EPS))
    print(shape, {k: "%.1e" % v for k, v in errs.items()})
    bad = {k: v for k, v in errs.items() if not v < TOL_KERNEL}
    assert not bad, bad


# --------------------------------------------------------------------------- stride-2 3x3 convolution
S2_CASES = [(128, 128, 24, 8), (128, 128, 23, 7), (64, 32, 12, 4)]


def conv_operands(Cin, Cout, H, W, B=3):
    x = OF.randn("s2:x%d_%d_%d_%d" % (Cin, Cout, H, W), (B, Cin, H, W), 4)
    w = OF.randn("s2:w%d_%d" % (Cin, Cout), (Cout, Cin, 3, 3), 4, (2.0 / (9 * Cin)) ** 0.5)
    return x, w


@pytest.mark.parametrize("prec", [0, 16])
@pytest.mark.parametrize("Cin,Cout,H,W", S2_CASES)
def test_conv3x3_stride2_forward_dgrad_wgrad(gpu, Cin, Cout, H, W, prec):
    """F.conv2d(stride=2, padding=1) and its autograd: B = 3 gives 144 output rows at 24x8 (one full 128-row tile and a partial
    one) and odd maps at 23x7; exact fp32 MFMA (precision 0) and the fp16 two-plane split (16).  The BatchNorm partials of the
    forward epilogue are finalised as well (they cover OUTPUT rows)."""
    from textreid_amd import ops

    B = 3
    x, w = conv_operands(Cin, Cout, H, W)
    xr, wr = x.double().requires_grad_(True), w.double().requires_grad_(True)
    yr = F.conv2d(xr, wr, stride=2, padding=1)
    gy = OF.randn("s2:g%d_%d_%d_%d" % (Cin, Cout, H, W), tuple(yr.shape), 4)
    (yr * gy.double()).sum().backward()
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    xg, gg = nhwc(x).to(gpu), nhwc(gy).to(gpu)
    w2 = w.permute(0, 2, 3, 1).reshape(Cout, 9 * Cin).contiguous().to(gpu)  # [N][tap][C]
    y, parts = ops.conv3x3(xg, w2, stats=True, prec=prec, stride=2)
    assert tuple(y.shape) == (B, Ho, Wo, Cout)
    errs = {"y": rel(nchw(y), yr)}
    st = ops.bn_finalize(parts, B * Ho * Wo, torch.ones(Cout, device=gpu), torch.zeros(Cout, device=gpu), None, None)
    errs["mean"] = float((st.mean.double().cpu() - yr.detach().mean(dim=(0, 2, 3))).abs().max() / yr.detach().abs().max())
    wt = ops.weight_transpose(w2, Cout, 9, Cin, flip=False)
    dx = ops.conv3x3_dgrad_s2(gg, wt, H, W, prec=prec)
    assert tuple(dx.shape) == (B, H, W, Cin)
    errs["dx"] = rel(nchw(dx), xr.grad)
    dw = ops.conv3x3_wgrad(gg, xg, prec=prec, stride=2)
    errs["dw"] = rel(dw.view(Cout, 3, 3, Cin).permute(0, 3, 1, 2), wr.grad)
    print((Cin, Cout, H, W, prec), {k: "%.1e" % v for k, v in errs.items()})
    bad = {k: v for k, v in errs.items() if not v < TOL_KERNEL}
    assert not bad, bad


def _sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


@pytest.mark.parametrize("prec", [0, 6, 16])
@pytest.mark.parametrize("Cin,Cout,H,W", S2_CASES)
def test_conv3x3_stride1_bits_are_those_of_the_parent_kernels(gpu, golden_dir, Cin, Cout, H, W, prec):
    """The stride-1 gathers share their kernel templates with the stride-2 ones: forward, data gradient (flipped filter) and weight
    gradient at stride 1 give the SAME BITS as the library built from the commit before the stride was added (sha256 of the
    outputs recorded there, tests/golden/conv3x3_s1_parent.json) - and stride=1 passed explicitly is the default call."""
    from textreid_amd import ops

    ref = json.load(open(os.path.join(golden_dir, "conv3x3_s1_parent.json")))
    x, w = conv_operands(Cin, Cout, H, W)
    gy = OF.randn("s1:g%d_%d_%d_%d" % (Cin, Cout, H, W), (3, Cout, H, W), 4)
    xg, gg = nhwc(x).to(gpu), nhwc(gy).to(gpu)
    w2 = w.permute(0, 2, 3, 1).reshape(Cout, 9 * Cin).contiguous().to(gpu)
    y, parts = ops.conv3x3(xg, w2, stats=True, prec=prec)
    dx = ops.conv3x3(gg, ops.weight_transpose(w2, Cout, 9, Cin, flip=True), prec=prec)
    dw = ops.conv3x3_wgrad(gg, xg, prec=prec)
    y1, parts1 = ops.conv3x3(xg, w2, stats=True, prec=prec, stride=1)
    assert torch.equal(y, y1) and torch.equal(parts, parts1)
    assert torch.equal(dw, ops.conv3x3_wgrad(gg, xg, prec=prec, stride=1))
    got = {"y": _sha(y), "parts": _sha(parts), "dx": _sha(dx), "dw": _sha(dw)}
    want = ref["%d_%d_%d_%d:p%d" % (Cin, Cout, H, W, prec)]
    assert got == want, [k for k in got if got[k] != want[k]]


# --------------------------------------------------------------------------- max pool
def pool_case(shape, seed):
    """y, g on the grid of integers / 16 and power-of-two scale / shift: relu(scale * y + shift) and every sum of gradients are
    exact on both sides.  y takes few distinct values (positive TIES inside most windows) and whole channels are shifted
    negative (windows that are all <= 0)."""
    B, H, W, C = shape
    y = OF.randint("pool:y%s" % (shape,), -6, 7, (B, H, W, C), seed).float() / 16.0
    g = OF.randint("pool:g%s" % (shape,), -32, 33, (B, (H - 1) // 2 + 1, (W - 1) // 2 + 1, C), seed).float() / 16.0
    scale = torch.tensor([1.0, 2.0, 0.5, -1.0] * (C // 4))
    shift = torch.tensor([0.0, 0.125, -0.25, 0.0, -8.0, 0.25, 0.0, -0.125] * (C // 8))  # channel 4 (mod 8): every value negative
    return y, g, scale, shift


@pytest.mark.parametrize("shape", [(2, 48, 16, 64), (3, 45, 15, 8)], ids=["48x16x64", "45x15x8"])
def test_bn_relu_maxpool_forward_and_backward_exact(gpu, shape):
    """torch.equal to F.max_pool2d(relu(scale * y + shift), 3, 2, 1) and to ITS autograd (first maximum in row-major window order
    wins ties; an all-negative window sends its gradient to its first position), on even and odd maps; the amax side output is
    the exact maximum."""
    from textreid_amd import ops

    y, g, scale, shift = pool_case(shape, 5)
    a = torch.relu(nchw(y) * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)).requires_grad_(True)
    pr = F.max_pool2d(a, kernel_size=3, stride=2, padding=1)
    pr.backward(nchw(g))
    windows = F.unfold(a.detach(), 3, padding=1, stride=2).view(shape[0], shape[3], 9, -1)
    top = windows.max(dim=2, keepdim=True).values
    assert bool(((windows == top).sum(dim=2) > 1)[top[:, :, 0] > 0].any()), "the case must hold positive ties"
    assert bool((top <= 0).any()), "the case must hold windows that are all <= 0"
    st = ops.BNState(shape[3], y.to(gpu))
    st.scale.copy_(scale.to(gpu))
    st.shift.copy_(shift.to(gpu))
    slot = ops.amax_slot(gpu)
    out = ops.bn_relu_maxpool(y.to(gpu), st, amax=slot)
    assert torch.equal(nchw(out).cpu(), pr.detach())
    assert float(slot) == float(pr.detach().max())
    dx = ops.bn_relu_maxpool_bwd(g.to(gpu), y.to(gpu), st)
    assert torch.equal(nchw(dx).cpu(), a.grad)


# --------------------------------------------------------------------------- subsample, global pool
@pytest.mark.parametrize("shape", [(2, 8, 6, 16), (3, 7, 5, 8)], ids=["even", "odd"])
def test_subsample2_and_global_avgpool_exact(gpu, shape):
    from textreid_amd import ops

    B, H, W, C = shape
    x = OF.randint("sub:x%s" % (shape,), -64, 65, shape, 6).float() / 8.0
    xg = x.to(gpu)
    slot = ops.amax_slot(gpu)
    sub = ops.subsample2(xg, amax=slot)
    assert torch.equal(sub.cpu(), x[:, ::2, ::2]) and float(slot) == float(x[:, ::2, ::2].abs().max())
    g = OF.randint("sub:g%s" % (shape,), -64, 65, tuple(sub.shape), 6).float() / 8.0
    want = torch.zeros(shape)
    want[:, ::2, ::2] = g
    assert torch.equal(ops.subsample2_bwd(g.to(gpu), H, W).cpu(), want)
    # integers / 8 sum exactly; the division by H * W is one correctly rounded operation on both sides
    assert torch.equal(ops.global_avgpool(xg).cpu(), x.sum(dim=(1, 2)) / float(H * W))
    gp = OF.randint("gap:g%s" % (shape,), -64, 65, (B, C), 6).float() / 8.0
    assert torch.equal(ops.global_avgpool_bwd(gp.to(gpu), H, W).cpu(), (gp / float(H * W)).view(B, 1, 1, C).expand(B, H, W, C))


# --------------------------------------------------------------------------- the encoder against the reference fixture
def fixture_encoder(g, stride, gpu):
    from textreid_amd.backbones.resnet import Bottleneck, ResNet, resnet

    m = ResNet(resnet(Bottleneck, [int(s) for s in g["stages"]], None), stride)
    m.load_state_dict(OF.fill_state(m.state_dict(), int(g["seed"]), "resnet."))
    return m.to(gpu).train()


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("case", ["96x32", "90x30"])
def test_encoder_against_reference_fixture(gpu, golden_dir, case, stride):
    """Stages [1, 2, 1, 1] (an identity block and all four downsample blocks) filled by name, against the reference module's own
    results: train-mode output, digests of every parameter gradient of loss = sum(out * G), every BatchNorm running buffer, the
    eval-mode output afterwards, and three SGD steps of the encoder alone (losses, final-state digests)."""
    g = np.load(os.path.join(golden_dir, "resnet.npz"))
    seed = int(g["seed"])
    lr, mom, wd = (float(v) for v in g["sgd"])
    tag = "%s:s%d:" % (case, stride)
    shape = tuple(int(v) for v in g[case + ":shape"])
    x = OF.randn("resnet:x" + case, shape, seed).to(gpu)
    errs = {}
    m = fixture_encoder(g, stride, gpu)
    out = m(x)
    assert tuple(out.shape) == (shape[0], 2048, 1, 1)
    errs["out"] = rel(out, g[tag + "out"])
    G = OF.randn("resnet:G" + case, tuple(out.shape), seed, float(g["g_scale"])).to(gpu)
    (out * G).sum().backward()
    names = [k for k, _ in m.named_parameters()]
    assert set(tag + "gdig:" + k for k in names) == {k for k in g.files if k.startswith(tag + "gdig:")}
    gfl = grad_floor([g[tag + "gdig:" + k] for k in names])
    for k, p in m.named_parameters():
        assert p.grad is not None, k
        errs["gdig:" + k] = digest_err(digest("grad:" + k, p.grad), g[tag + "gdig:" + k], gfl)
    for k, b in m.named_buffers():
        if "num_batches_tracked" in k:
            assert int(b) == 1, k
        else:
            errs["buf:" + k] = rel(b, g[tag + "buf:" + k])
    m.eval()
    with torch.no_grad():
        errs["eval"] = rel(m(x), g[tag + "eval"])
    # three SGD steps of the encoder alone, from the filled state
    m = fixture_encoder(g, stride, gpu)
    opt = torch.optim.SGD(m.parameters(), lr=lr, momentum=mom, weight_decay=wd)
    for s in range(3):
        xs = OF.randn("resnet:x%s:step%d" % (case, s), shape, seed).to(gpu)
        out = m(xs)
        loss = (out * G).sum()
        opt.zero_grad()
        loss.backward()
        opt.step()
        errs["loss%d" % s] = rel(loss, g[tag + "loss%d" % s])
    for k, v in m.state_dict().items():
        if "num_batches_tracked" not in k:
            errs["fdig:" + k] = digest_err(digest("final:" + k, v), g[tag + "fdig:" + k])
    worst = sorted(errs.items(), key=lambda kv: -kv[1])[:5]
    print(tag, len(errs), "quantities; worst:", [(k, "%.1e" % v) for k, v in worst])
    bad = {k: v for k, v in errs.items() if not v <= TOL}
    assert not bad, sorted(bad.items(), key=lambda kv: -kv[1])[:8]


# --------------------------------------------------------------------------- the model at full size
def imagenet_model(gpu, visual="resnet50", seed=0):
    from textreid_amd.config import imagenet_cfg
    from textreid_amd.model import build_model

    torch.manual_seed(seed)
    cfg = imagenet_cfg(visual)
    return cfg, build_model(cfg).to(gpu).train()


def batch(B, s, gpu, seed=3):
    import bench
    from textreid_amd.caption import CaptionBatch

    images, tokens, lengths, ids = bench.synth_batch(B, s, gpu, seed, vocab=12000)
    return images, CaptionBatch(tokens, lengths, ids % 11003, max_len=64)


@pytest.mark.parametrize("visual", ["resnet50", "resnet101"])
def test_imagenet_baseline_full_size_smoke(gpu, visual):
    """What configs/cuhkpedes/baseline_gru_rn50_ls_bs128.yaml asks for (and its resnet101 sibling): 384x128, B = 8: one training
    step with finite losses and a finite gradient on EVERY trainable tensor, eval output [8,256] x 2."""
    cfg, model = imagenet_model(gpu, visual)
    assert cfg.MODEL.EMBEDDING.FEATURE_SIZE == 256 and cfg.MODEL.NUM_CLASSES == 11003 and model.embed_type == "normal"
    images, cb = batch(8, 0, gpu)
    ld = model(images, cb)
    assert sorted(ld) == ["global_align_loss", "instance_loss"] and all(bool(torch.isfinite(v)) for v in ld.values())
    sum(ld.values()).backward()
    for k, p in model.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), k
    model.eval()
    with torch.no_grad():
        v, t = model(images, cb)
    assert tuple(v.shape) == (8, 256) and tuple(t.shape) == (8, 256)
    assert bool(torch.isfinite(v).all()) and bool(torch.isfinite(t).all())
    assert torch.equal(v, model.encode_images(images)) and torch.equal(t, model.encode_captions(cb))


def test_imagenet_baseline_step_is_deterministic(gpu):
    """Two runs from the same state give the same bits - losses and the whole state: nothing on the path accumulates with atomics."""
    from textreid_amd.solver import make_optimizer

    outs = []
    for _ in range(2):
        cfg, model = imagenet_model(gpu)
        opt = make_optimizer(cfg, model)
        losses = []
        for s in range(3):
            images, cb = batch(8, s, gpu)
            ld = model(images, cb)
            opt.zero_grad()
            sum(ld.values()).backward()
            opt.step()
            losses.append(torch.stack([v.detach() for v in ld.values()]))
        outs.append((torch.stack(losses), {k: v.detach().clone() for k, v in model.state_dict().items()}))
    assert torch.equal(outs[0][0], outs[1][0]) and bool(torch.isfinite(outs[0][0]).all())
    for k, v in outs[0][1].items():
        assert torch.equal(v, outs[1][1][k]), k


def test_captured_imagenet_step_equals_eager_bitwise(gpu):
    """engine.graph.CapturedTrainStep records the step unchanged: both replay forms give the SAME BITS as the eager step over 4
    steps - losses every step, every parameter and BatchNorm buffer at the end."""
    from textreid_amd.engine.graph import CapturedTrainStep
    from textreid_amd.solver import make_optimizer

    steps = 4
    batches = [batch(8, s, gpu, 5) for s in range(steps)]
    runs = {}
    for mode in ("eager", "graph", "streams"):
        cfg, model = imagenet_model(gpu)
        opt = make_optimizer(cfg, model)
        runner = CapturedTrainStep(model, opt, warmup=2, caption_bound=64, launch="graph" if mode == "eager" else mode)
        losses = []
        for images, cb in batches:
            ld = runner._eager(images, cb) if mode == "eager" else runner(images, cb)
            losses.append(torch.stack([v.detach().clone() for v in ld.values()]))
        torch.cuda.synchronize()
        if mode != "eager":
            assert runner.graph is not None and not runner.disabled and runner.recaptures == 0
        runs[mode] = (torch.stack(losses), {k: v.detach().clone() for k, v in model.state_dict().items()})
        del model, opt, runner
    assert bool(torch.isfinite(runs["eager"][0]).all())
    for other in ("graph", "streams"):
        assert torch.equal(runs["eager"][0], runs[other][0]), (other, (runs["eager"][0] - runs[other][0]).abs().max())
        for k, v in runs["eager"][1].items():
            assert torch.equal(v, runs[other][1][k]), (other, k)


def test_imagenet_train_step_has_no_host_device_sync(gpu):
    """After warm-up a whole step does not synchronise the host with the device (torch's sync debug mode raises)."""
    from textreid_amd.solver import make_optimizer

    cfg, model = imagenet_model(gpu)
    opt = make_optimizer(cfg, model)
    batches = [batch(8, s, gpu, 5) for s in range(2)]

    def step(i):
        images, cb = batches[i % 2]
        loss = sum(model(images, cb).values())
        opt.zero_grad()
        loss.backward()
        opt.step()
        return loss

    for i in range(3):
        step(i)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        last = step(3)
        last = step(4)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert bool(torch.isfinite(last))
