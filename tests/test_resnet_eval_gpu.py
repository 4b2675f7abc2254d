"""GPU tests of the eval-mode P16 data flow of the ImageNet ResNet image encoder (textreid_amd/backbones/resnet.py
ResNet._run_forward_eval_p16, csrc/resnet_eval.hip, the A_CONV_S2 loader of csrc/gemm_p16.hip).

Kernel cases compare against the fp64 restatement tests/resnet_eval_ref.py at the smallest shapes where their indexing can go
wrong, relative to the largest output magnitude: the arithmetic kernels (stem, stride-2 3x3) at TOL_KERNEL = 2e-5, the bound of
tests/test_resnet_gpu.py / DESIGN 7b for this encoder's kernels in precision 16; the copying kernels (max pool, subsample) bit for
bit.  The encoder is held to 1e-3 of max|out| (the project's bound for embeddings) against fp64 AND against today's unfused path.

Measured on an MI355X (worst over the cases of each test; every test prints its figures before it asserts them):
    stem7_eval_p16                 4.6e-7    (bound 2e-5)
    conv3x3_s2_eval_p16            7.3e-7    (bound 2e-5)
    encoder, fused path vs fp64    1.0e-6    (bound 1e-3)   unfused path vs fp64 8.3e-7, fused vs unfused 1.3e-6"""

import pytest
import torch

pytestmark = pytest.mark.gpu

import resnet_eval_ref as ref  # noqa: E402

TOL_KERNEL = 2e-5  # tests/test_resnet_gpu.py:23
TOL = 1e-3         # tests/test_model_gpu.py:19
# The folded maximum `tmax` is that of the fp32 values BEFORE they are split into two fp16 planes; the planes carry 22 significand
# bits, so the maximum of the unpacked tensor lies within 2^-22 of it (relative).  Twice that is the bound.
TOL_TMAX = 2.0 ** -21
NEW_WRAPPERS = ["stem7_eval_p16", "maxpool3s2_p16", "conv3x3_s2_eval_p16", "subsample2_p16", "global_avgpool_p16", "conv_eval_p16"]


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import textreid_amd  # noqa: F401

    return torch.device("cuda")


def rel(a, b):
    a = torch.as_tensor(a).detach().double().cpu()
    b = torch.as_tensor(b).detach().double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def gen(seed):
    return torch.Generator().manual_seed(seed)


def signed(n, lo, hi, g):
    """n values of both signs with magnitudes in [lo, hi]"""
    mag = lo + (hi - lo) * torch.rand(n, generator=g)
    return mag * (torch.randint(0, 2, (n,), generator=g).float() * 2 - 1)


def bn_state(scale, shift, gpu):
    from textreid_amd import ops

    st = ops.BNState(scale.numel(), scale.to(gpu))
    st.scale.copy_(scale.to(gpu))
    st.shift.copy_(shift.to(gpu))
    return st


def bits(t):
    return t.contiguous().view(torch.int32)


def check_published_scalars(out, want):
    """out: the kernel's P16 result, want: fp64.  The published bound is >= the true max|output|, the folded maximum is the true
    maximum of the unpacked output (TOL_TMAX)."""
    un = out.unpack().double().cpu()
    true_max = float(un.abs().max())
    assert float(out.amax) >= true_max and float(out.amax) >= float(want.abs().max())
    assert abs(float(out.tmax) - true_max) <= TOL_TMAX * true_max, (float(out.tmax), true_max)


# --------------------------------------------------------------------------- stem
@pytest.mark.parametrize("H,W", [(36, 20), (37, 21)])
def test_stem7_eval_p16_against_fp64(gpu, H, W):
    """relu(scale * conv7x7s2(x) + shift) from the NCHW batch as a P16 tensor: 18x10 maps (360 rows: two whole 128-row slabs and a
    partial one) and odd 19x11 maps (418 rows)."""
    from textreid_amd import ops

    g = gen(21)
    x = torch.randn(2, 3, H, W, generator=g)
    w = torch.randn(64, 3, 7, 7, generator=g) * 0.1
    scale, shift = signed(64, 0.3, 3.0, g), signed(64, 0.05, 1.0, g)
    want = torch.relu(ref.conv(x.permute(0, 2, 3, 1), w.permute(0, 2, 3, 1), 2, 3) * scale.double() + shift.double())
    xg, wg = x.to(gpu), w.to(gpu)
    st = bn_state(scale, shift, gpu)
    coef = ops.eval_bound_coefs([(wg, st.scale, st.shift)], gpu)
    out = ops.stem7_eval_p16(xg, wg, st, coef[0], ops.amax(xg))
    assert tuple(out.shape) == (2, (H - 1) // 2 + 1, (W - 1) // 2 + 1, 64)
    err = rel(out.unpack(), want)
    print("stem7_eval_p16 %dx%d: %.1e" % (H, W, err))
    assert err < TOL_KERNEL
    check_published_scalars(out, want)


# --------------------------------------------------------------------------- max pool on P16
@pytest.mark.parametrize("H,W", [(18, 10), (5, 3)])
def test_maxpool3s2_p16_is_exact(gpu, H, W):
    """18x10 -> 9x5 and 5x3 -> 3x2; channel 4 (mod 8) is negative everywhere (a zero-padded pool would answer 0 at the border where
    the padding is -inf).  No arithmetic: the result equals F.max_pool2d of the unpacked input, packed at the input's scale."""
    import torch.nn.functional as F

    from textreid_amd import ops

    g = gen(22)
    x = torch.randn(2, H, W, 64, generator=g)
    x[..., 4::8] = -x[..., 4::8].abs() - 0.25
    x16 = ops.p16_pack(x.to(gpu))
    xin = x16.unpack()
    want = F.max_pool2d(xin.permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1).contiguous()
    assert bool((want[..., 4::8] < 0).all())
    out = ops.maxpool3s2_p16(x16)
    assert tuple(out.shape) == (2, (H - 1) // 2 + 1, (W - 1) // 2 + 1, 64) and out.amax is x16.amax
    assert torch.equal(out.unpack(), want)
    assert torch.equal(bits(out.data), bits(ops.p16_pack(want, x16.amax).data))
    assert float(out.tmax) == float(want.abs().max())
    assert torch.equal(want.cpu(), ref.maxpool3s2(xin.cpu()))  # (the restatement the encoder reference uses)


# --------------------------------------------------------------------------- subsample of P16
def test_subsample2_p16_is_a_copy(gpu):
    """9x5 -> 5x3: the even rows and columns, bit for bit, under the source's scale scalar."""
    from textreid_amd import ops

    x = torch.randn(2, 9, 5, 64, generator=gen(23))
    x16 = ops.p16_pack(x.to(gpu))
    out = ops.subsample2_p16(x16)
    assert tuple(out.shape) == (2, 5, 3, 64) and out.amax is x16.amax and out.tmax is x16.tmax
    assert torch.equal(bits(out.data), bits(x16.data[:, ::2, ::2]))
    assert torch.equal(out.unpack(), x16.unpack()[:, ::2, ::2])


# --------------------------------------------------------------------------- global average pool of P16
@pytest.mark.parametrize("H,W", [(3, 2), (1, 1)])
def test_global_avgpool_p16(gpu, H, W):
    """2048 channels: the unpacked values summed in pixel order.  On integers / 8 the sums are exact and the division is one
    correctly rounded operation on both sides; on random data the result is that of ops.global_avgpool on the unpacked tensor."""
    from textreid_amd import ops

    g = gen(24)
    x = torch.randint(-64, 65, (2, H, W, 2048), generator=g).float() / 8.0
    x16 = ops.p16_pack(x.to(gpu))
    assert torch.equal(x16.unpack().cpu(), x)
    assert torch.equal(ops.global_avgpool_p16(x16).cpu(), x.sum(dim=(1, 2)) / float(H * W))
    r16 = ops.p16_pack(torch.randn(2, H, W, 2048, generator=g).to(gpu))
    got = ops.global_avgpool_p16(r16)
    assert torch.equal(got, ops.global_avgpool(r16.unpack()))
    assert rel(got, r16.unpack().double().mean(dim=(1, 2))) < 1e-6


# --------------------------------------------------------------------------- stride-2 3x3 convolution, eval epilogue
@pytest.mark.parametrize("H,W,N", [(9, 5, 128), (8, 4, 128), (2, 1, 128), (9, 5, 256)], ids=["9x5", "8x4", "2x1", "9x5_N256"])
def test_conv3x3_s2_eval_p16_against_fp64(gpu, H, W, N):
    """B = 2, Cin = 128: 30, 16 and 2 output rows - far below one 128-row tile, so the masked rows are live; odd x odd 9x5 maps
    (the last output row and column have in-range taps on one side only); N = 256 runs two column tiles."""
    from textreid_amd import ops

    C = 128
    g = gen(25)
    x = torch.relu(torch.randn(2, H, W, C, generator=g)) + 0.1 * torch.randn(2, H, W, C, generator=g)
    w = torch.randn(N, 3, 3, C, generator=g) * (2.0 / (9 * C)) ** 0.5  # [N][ky][kx][C]
    scale, shift = signed(N, 0.3, 3.0, g), signed(N, 0.05, 1.0, g)
    want = torch.relu(ref.conv(x, w, 2, 1) * scale.double() + shift.double())
    x16 = ops.p16_pack(x.to(gpu))
    wg = w.reshape(N, 9 * C).contiguous().to(gpu)
    w16 = ops.p16_pack(wg)
    st = bn_state(scale, shift, gpu)
    coef = ops.eval_bound_coefs([(wg, st.scale, st.shift)], gpu)
    assert ops.conv3x3_s2_eval_ok(2, H, W, C, N)
    out = ops.conv3x3_s2_eval_p16(x16, w16, st, coef[0], relu=True)
    assert tuple(out.shape) == (2, (H - 1) // 2 + 1, (W - 1) // 2 + 1, N)
    err = rel(out.unpack(), want)
    print("conv3x3_s2_eval_p16 %dx%d N=%d: %.1e" % (H, W, N, err))
    assert err < TOL_KERNEL
    check_published_scalars(out, want)


# --------------------------------------------------------------------------- the encoder
def make_encoder(stride, seed, gpu):
    """Stages [1, 1, 1, 1]: running_var spread over two decades, running_mean and the affine parameters of both signs."""
    from textreid_amd.backbones.resnet import Bottleneck, ResNet, resnet

    torch.manual_seed(seed)
    m = ResNet(resnet(Bottleneck, [1, 1, 1, 1], None), stride)
    g = gen(seed + 1)
    for bn in [b for b in m.modules() if isinstance(b, torch.nn.BatchNorm2d)]:
        n = bn.num_features
        bn.running_var.copy_(10.0 ** (2.0 * torch.rand(n, generator=g) - 1.0))
        bn.running_mean.copy_(signed(n, 0.05, 0.5, g))
        with torch.no_grad():
            bn.weight.copy_(signed(n, 0.5, 1.5, g))
            bn.bias.copy_(signed(n, 0.05, 0.5, g))
    return m.to(gpu).eval()


def count_calls(monkeypatch, names):
    from textreid_amd import ops

    calls = {k: 0 for k in names}

    def wrap(name, fn):
        def counted(*a, **kw):
            calls[name] += 1
            return fn(*a, **kw)
        return counted

    for k in names:
        monkeypatch.setattr(ops, k, wrap(k, getattr(ops, k)))
    return calls


ENC_CASES = [(2, 72, 40), (3, 64, 32)]
_enc_cache = {}


def encoder_case(gpu, shape, stride):
    """(module, images, fp64 reference) of one case, computed once"""
    key = (shape, stride)
    if key not in _enc_cache:
        m = make_encoder(stride, 31, gpu)
        x = torch.randn(shape[0], 3, shape[1], shape[2], generator=gen(32))
        _enc_cache[key] = (m, x.to(gpu), ref.encoder(m, x))
    return _enc_cache[key]


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("shape", ENC_CASES, ids=["2x72x40", "3x64x32"])
def test_encoder_eval_p16_against_fp64_and_the_unfused_path(gpu, monkeypatch, shape, stride):
    """72x40 inputs: maps 36x20 -> 18x10 -> 9x5 -> 5x3 -> 3x2, odd at every stride-2 step; RES5_STRIDE 1 and 2.  The default path
    calls bn_apply zero times; with ops.USE_EVAL_P16 off no new-kernel wrapper is called (the launch sequence of the unfused path
    is the one it was)."""
    from textreid_amd import ops

    m, x, want = encoder_case(gpu, shape, stride)
    calls = count_calls(monkeypatch, NEW_WRAPPERS + ["bn_apply", "bn_relu_maxpool", "global_avgpool"])
    with torch.no_grad():
        fused = m(x)
    assert tuple(fused.shape) == (shape[0], 2048, 1, 1)
    assert calls["bn_apply"] == 0 and calls["bn_relu_maxpool"] == 0 and calls["global_avgpool"] == 0
    n_s2 = 2 + (stride == 2)
    assert (calls["stem7_eval_p16"], calls["maxpool3s2_p16"], calls["global_avgpool_p16"]) == (1, 1, 1)
    assert calls["conv3x3_s2_eval_p16"] == n_s2 and calls["subsample2_p16"] == n_s2 and calls["conv_eval_p16"] == 16 - n_s2
    for k in calls:
        calls[k] = 0
    monkeypatch.setattr(ops, "USE_EVAL_P16", False)
    with torch.no_grad():
        unfused = m(x)
    assert all(calls[k] == 0 for k in NEW_WRAPPERS), calls
    assert calls["bn_apply"] == 12 and calls["bn_relu_maxpool"] == 1 and calls["global_avgpool"] == 1
    e_f, e_u, e_fu = rel(fused.view(shape[0], -1), want), rel(unfused.view(shape[0], -1), want), rel(fused, unfused)
    print("encoder %s stride %d: fused vs fp64 %.1e, unfused vs fp64 %.1e, fused vs unfused %.1e" % (shape, stride, e_f, e_u, e_fu))
    assert e_f < TOL and e_fu < TOL


def test_plan_is_invalidated_by_buffer_and_parameter_writes(gpu):
    """Encode, overwrite one running_mean in place and one conv weight through load_state_dict, encode again: the result is that
    of a freshly built module holding the new state, and differs from the first."""
    m = make_encoder(2, 41, gpu)
    x = torch.randn(2, 3, 72, 40, generator=gen(42)).to(gpu)
    with torch.no_grad():
        first = m(x).clone()
        again = m(x)
    assert torch.equal(first, again) and getattr(m, "_eval_plan_cache", None) is not None
    m.layer2[0].bn2.running_mean.add_(0.5)
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    sd["layer3.0.conv1.weight"] = sd["layer3.0.conv1.weight"] * 1.5
    m.load_state_dict(sd)
    with torch.no_grad():
        second = m(x).clone()
    fresh = make_encoder(2, 7, gpu)
    fresh.load_state_dict(sd)
    with torch.no_grad():
        want = fresh(x)
    assert torch.equal(second, want)
    assert not torch.equal(second, first)
    assert rel(second.view(2, -1), ref.encoder(fresh, x)) < TOL


def test_other_precisions_and_declined_shapes_take_the_unfused_path(gpu, monkeypatch):
    """conv_precision() != 16 and a shape the predicate declines: no new-kernel wrapper runs and the module returns the unfused
    path's result."""
    from textreid_amd import ops
    from textreid_amd.backbones import resnet as R

    m, x, want = encoder_case(gpu, ENC_CASES[0], 2)
    calls = count_calls(monkeypatch, NEW_WRAPPERS)
    # precision 6
    with monkeypatch.context() as mp:
        mp.setattr(ops, "CONV_PRECISION", 6)
        assert ops.conv_precision() == 6
        with torch.no_grad():
            got = m(x)
        mp.setattr(ops, "USE_EVAL_P16", False)
        with torch.no_grad():
            unfused = m(x)
    assert all(v == 0 for v in calls.values()), calls
    assert torch.equal(got, unfused) and rel(got.view(2, -1), want) < TOL
    # a declined shape: batches whose activations pass the kernels' 31-bit offsets (here: the limit lowered below this batch)
    with monkeypatch.context() as mp:
        mp.setattr(R, "P16_LIMIT_BYTES", 1 << 16)
        assert not R.eval_p16_ok(m, x)
        with torch.no_grad():
            got = m(x)
    assert all(v == 0 for v in calls.values()), calls
    with monkeypatch.context() as mp:
        mp.setattr(ops, "USE_EVAL_P16", False)
        with torch.no_grad():
            unfused = m(x)
    assert torch.equal(got, unfused) and rel(got.view(2, -1), want) < TOL
    with torch.no_grad():
        m(x)
    assert calls["stem7_eval_p16"] == 1  # (and the default is back)
