"""The CPU helpers of tests/bn_pool_ref.py checked on their own (no GPU): the P16 encoder / decoder, the ReLU-bit words, the
statistics partials, and the derivation of the tolerances tests/test_bn_pool_gpu.py holds the kernels to - including that the
stated bounds are sharp: a P16 tensor without its low plane, or bits laid out in another order, does not pass them."""

import pytest
import torch

import bn_pool_ref as ref
import oracle.fill as OF


def R(name, *shape, scale=1.0):
    return OF.randn(name, shape, 0, scale)


def with_amax(t, amax):
    """t rescaled so that its largest magnitude is exactly amax"""
    return (t.double() / t.double().abs().max() * amax).float()


# --------------------------------------------------------------------------- P16
@pytest.mark.parametrize("amax", [1.0, 2.0 ** -114, 2.0 ** 100, 0.0], ids=["1", "2^-114", "2^100", "0"])
@pytest.mark.parametrize("M,C", [(37, 32), (67, 96)])
def test_p16_round_trip(amax, M, C):
    """encode -> decode reproduces fp32 inputs to 2^-22 of amax; the same tensor decoded WITHOUT its low plane (2^-11 of an
    element: 2000x the bound) does not"""
    x = with_amax(R("rt", M, C), amax) if amax > 0 else torch.zeros(M, C)
    assert float(x.abs().max()) == amax
    enc = ref.p16_encode(x, amax)
    assert enc.shape == x.shape and enc.dtype == torch.float32
    got = ref.p16_decode(enc, amax)
    assert bool(torch.isfinite(got).all())
    e = ref.p16_excess(got, x, amax)
    print("p16 round trip amax %-8g %dx%d: error / (2^-22 amax) = %.3f" % (amax, M, C, e))
    assert e <= 1.0
    if amax > 0:
        assert ref.p16_excess(ref.p16_decode(enc, amax, lo_plane=False), x, amax) > 100.0


def test_p16_scale_and_layout():
    """scale = 2^(13 - floor(log2 amax)) capped at 2^127, 1 for zero / denormal / non-finite; per row and 32-channel group
    [hi x 32 | lo x 32] fp16"""
    for amax, want in ((1.0, 2.0 ** 13), (1.999, 2.0 ** 13), (2.0, 2.0 ** 12), (0.75, 2.0 ** 14), (2.0 ** -114, 2.0 ** 127), (2.0 ** -120, 2.0 ** 127),
                       (2.0 ** 100, 2.0 ** -87), (0.0, 1.0), (2.0 ** -130, 1.0), (float("inf"), 1.0), (float("nan"), 1.0)):
        assert float(ref.p16_scale(amax)) == want, amax
    x = torch.arange(1, 2 * 64 + 1, dtype=torch.float32).reshape(2, 64) + 0.5 ** 12  # (hi = the integer, lo = 2^-12, both * scale)
    h = ref.p16_encode(x, 128.0 + 0.5 ** 12).numpy().view("float16").reshape(2, 2, 2, 32)  # scale 2^6
    for row in range(2):
        for grp in range(2):
            first = 64 * row + 32 * grp + 1
            assert h[row, grp, 0].tolist() == [(first + k) * 64.0 for k in range(32)]
            assert h[row, grp, 1].tolist() == [2.0 ** -6] * 32


# --------------------------------------------------------------------------- ReLU-bit words
@pytest.mark.parametrize("M,C", [(37, 32), (67, 96), (193, 4), (2, 32), (64, 16)])
def test_bit_words_round_trip(M, C):
    """pack -> unpack is the identity, also where M * C / 4 is no multiple of 64; the words are the ones the suite's other
    packer builds; a layout with component and group swapped is told apart"""
    from test_kernels_gpu import _relu_mask_words

    keep = R("bits%d.%d" % (M, C), M, C) > -0.25
    words = ref.pack_bits(keep)
    n4 = M * C // 4
    assert words.dtype == torch.int64 and words.numel() == (n4 + 63) // 64 * 4
    assert torch.equal(ref.unpack_bits(words, M, C), keep)
    assert torch.equal(words, _relu_mask_words(keep).reshape(-1))
    # quad i = 70, component 2 of a [37, 32] tensor: word (70 / 64) * 4 + 2, bit 70 % 64
    one = torch.zeros(37, 32, dtype=torch.bool)
    one.view(-1)[4 * 70 + 2] = True
    w = ref.pack_bits(one)
    assert int(w[6]) == 1 << 6 and int(w.ne(0).sum()) == 1
    if n4 > 64:
        wrong = words.reshape(-1, 4).flip(1).reshape(-1)  # components in the opposite order
        assert not torch.equal(ref.unpack_bits(wrong, M, C), keep)


# --------------------------------------------------------------------------- statistics partials
@pytest.mark.parametrize("M,C,rows", [(3, 4, 3), (50, 24, 3), (2306, 64, 3), (4627, 4, 3), (515, 64, 128)])
def test_partials_merge_to_the_direct_statistics(M, C, rows):
    y = R("part%d" % M, M, C) * 1.5 + 20.0 * R("partm", C)
    st = ref.bn_stats(y, torch.ones(C), torch.zeros(C))
    for minmax in (False, True):
        p = ref.partials(y, rows, minmax)
        assert tuple(p.shape) == ((M + rows - 1) // rows, C, 4 if minmax else 2) and p.dtype == torch.float32
        m = ref.merge_partials(p, rows, M)
        # (the partials are fp32: 6e-8 of a mean of ~20 standard deviations)
        assert float((m["mean"] - st["mean"]).abs().max()) <= 1e-7 * float(st["mean"].abs().max())
        assert float(((m["var"] - st["var"]) / st["var"]).abs().max()) <= 1e-5
        if minmax:
            assert torch.equal(m["lo"].float(), y.min(0).values) and torch.equal(m["hi"].float(), y.max(0).values)


def test_reference_against_its_own_formulas():
    """autograd's gradients are the closed form the kernels implement; running buffers; pooled and residual forms"""
    B, H, W, C = 3, 6, 10, 8
    d = ref.inputs(B, H, W, C)
    r = ref.bn_reference(d["y"], d["gamma"], d["beta"], True, res=d["res"], g=d["g"])
    st = ref.bn_stats(d["y"], d["gamma"], d["beta"])
    y2, g2, M = d["y"].double().reshape(-1, C), d["g"].double().reshape(-1, C), B * H * W
    z = y2 * st["scale"] + st["shift"] + d["res"].double().reshape(-1, C)
    gm = g2 * (z > 0)
    xh = (y2 - st["mean"]) * st["invstd"]
    dy = st["scale"] * (gm - gm.sum(0) / M - xh * (gm * xh).sum(0) / M)
    assert float((r["z"].reshape(-1, C) - z).abs().max()) < 1e-12
    assert float((r["dy"].reshape(-1, C) - dy).abs().max()) < 1e-12 and float((r["dres"].reshape(-1, C) - gm).abs().max()) == 0
    assert float((r["dgamma"] - (gm * xh).sum(0)).abs().max()) < 1e-11 and float((r["dbeta"] - gm.sum(0)).abs().max()) < 1e-11
    p = ref.bn_reference(d["y"], d["gamma"], d["beta"], False, pool=True, g=d["gp"])
    zz = (y2 * st["scale"] + st["shift"]).reshape(B, H, W, C)
    pooled = 0.25 * (zz[:, 0::2, 0::2] + zz[:, 0::2, 1::2] + zz[:, 1::2, 0::2] + zz[:, 1::2, 1::2])
    assert float((p["out"] - pooled).abs().max()) < 1e-12
    rm, rv = ref.running_update(d["y"], d["rmean"], d["rvar"])
    assert float((rm - (0.9 * d["rmean"].double() + 0.1 * st["mean"])).abs().max()) < 1e-12
    assert float((rv - (0.9 * d["rvar"].double() + 0.1 * st["var"] * M / (M - 1))).abs().max()) < 1e-12


def test_a_carried_channel_quad_that_does_not_wrap_fails_the_fp32_bound():
    """(67, 96): C/4 = 24 does not divide the 512 threads of the two workgroups, so the channel quad a thread carries from trip
    to trip moves by step_c = 8 and must wrap at 24.  The same walk with the wrap left out (the index clamped to stay inside the
    coefficient vectors) misses the fp32 bound by five orders of magnitude; the correct walk meets it."""
    M, C, T = 67, 96, 512
    CQ, total4 = C // 4, M * C // 4
    d = ref.inputs(1, 1, M, C)
    st = ref.bn_stats(d["y"], d["gamma"], d["beta"])
    want = ref.bn_reference(d["y"], d["gamma"], d["beta"], False)["out"].reshape(total4, 4)
    y4 = d["y"].reshape(total4, 4)
    sc, sh = st["scale"].float().reshape(CQ, 4), st["shift"].float().reshape(CQ, 4)
    step_c = T % CQ
    assert step_c == 8
    i = torch.arange(total4)
    i0, trip = i % T, i // T
    walked = i0 % CQ + trip * step_c
    top = float(want.abs().max())
    for wraps, cq in ((True, walked % CQ), (False, walked.clamp(max=CQ - 1))):
        out = y4 * sc[cq] + sh[cq]
        e = float((out.double() - want).abs().max()) / top
        assert (e <= ref.TOL_F32) == wraps, (wraps, e)
        assert wraps or e > 1e-1


# --------------------------------------------------------------------------- where the tolerances come from
def test_tolerances_are_four_times_the_fp32_yardstick():
    """TOL_STAT / TOL_SUM / TOL_DY = 4x what a left-to-right fp32 evaluation of the same sums loses against fp64 on the very
    inputs of the GPU test (rounded up, never above the suite's former 2e-5); fp32 outputs: the yardstick stays 5x below 1e-6"""
    worst = dict(out=0.0, stat=0.0, sum=0.0, dy=0.0)
    for (B, H, W, C) in ref.emulation_cases():
        d = ref.inputs(B, H, W, C)
        for relu in (False, True):
            e = ref.fp32_emulation(d["y"].reshape(-1, C), d["gamma"], d["beta"], d["g"].reshape(-1, C), relu)
            worst = {k: max(v, e[k]) for k, v in worst.items()}
    print("fp32 yardstick:", {k: "%.2e" % v for k, v in worst.items()})
    assert worst["out"] <= 1.7e-7 < ref.TOL_F32 / 5
    for tol, k in ((ref.TOL_STAT, "stat"), (ref.TOL_SUM, "sum"), (ref.TOL_DY, "dy")):
        assert 4 * worst[k] <= tol <= 4.2 * worst[k] and tol <= 2e-5, (k, worst[k], tol)


def test_band_share_of_the_reference():
    """the share of pre-activations within 1e-5 of the largest one stays below the 0.1 % the GPU test allows (the largest
    share is one element of the 1440 of a [3, 6, 10, 8] tensor; the large tensors stay at or below 1.7e-4)"""
    top = 0.0
    for (B, H, W, C) in ref.emulation_cases():
        d = ref.inputs(B, H, W, C)
        for kw in ({}, dict(res=d["res"]), dict(res=d["res"], res_gamma=d["gamma2"], res_beta=d["beta2"])):
            top = max(top, ref.relu_band(ref.bn_reference(d["y"], d["gamma"], d["beta"], True, **kw)["z"])[1])
    print("largest band share %.1e" % top)
    assert top <= ref.BAND_SHARE
