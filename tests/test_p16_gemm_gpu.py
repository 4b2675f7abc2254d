"""Sharp fp64 parity of the pre-split (P16) GEMM kernels of csrc/gemm_p16.hip at edge shapes: `trid_gemm_p16` - forward and
data gradient, 1x1 and 3x3 gather (A_CONV) form - and `trid_gemm_p16_wgrad` - 1x1 (B_NC) and 3x3 (B_CONV) form, forced
split counts, bf16 operands.

Every case is compared with a plain fp64 CPU reference of the same operation (F.conv2d / a matrix product in double,
autograd for both gradients) on inputs seeded through oracle.fill.  The bound is 2e-6 of the reference's maximum: a CPU
emulation of correct two-plane fp16 arithmetic (fp16 planes, three products, fp32 sums) stays below 8e-7 at these shapes
(measured on the MI355X: 1.2e-6 at most, the 3x3 data gradient with K = 1152), the same product with the low plane of the
operands lost is 2.6e-4 or more.  Each case runs on the tile kernel (the streaming and ring-of-rows kernels switched off) and
once more through the library's own dispatch, and prints what it measured."""

import contextlib
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import oracle.fill as OF  # noqa: E402
from test_kernels_gpu import _relu_mask_words  # noqa: E402

TOL = 2e-6  # P16: two fp16 planes, three products, fp32 sums; bf16 cases: fp32 sums only (products of bf16 values are exact)
F32_TINY = 2.0 ** -126  # fp32's smallest normal


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from textreid_amd import ops as o

    return o


def R(name, *shape, scale=1.0):
    return OF.randn(name, shape, 0, scale)


def dev(t):
    return t.cuda().contiguous()


def rel(got, ref):
    """largest absolute error over the reference's largest magnitude"""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return float((got - ref).abs().max() / (ref.abs().max() + 1e-300))


def report(group, case, what, err):
    print("p16 parity %-8s %-24s %-22s %.2e" % (group, case, what, err))
    return err


@contextlib.contextmanager
def kernels(ops, tile):
    """tile: the tile kernel of gemm_p16.hip whatever the shape; else the library's own choice"""
    old = ops.USE_STREAM, ops.USE_HALO_BLOCKS
    try:
        if tile:
            ops.USE_STREAM = ops.USE_HALO_BLOCKS = False
        yield "tile" if tile else "dispatch"
    finally:
        ops.USE_STREAM, ops.USE_HALO_BLOCKS = old


def _round(t, bf16):
    return t.bfloat16().float() if bf16 else t


# --------------------------------------------------------------------------- fp64 references (computed once, never written to)
@functools.lru_cache(maxsize=None)
def ref1x1(M, N, K, bf16=False):
    """y [M,N] = x [M,K] . w [N,K]^T with both gradients for the output gradient g [M,N]; bf16: of operands rounded to bf16"""
    x, w, g = _round(R("p1x", M, K), bf16), _round(R("p1w", N, K, scale=0.2), bf16), _round(R("p1g", M, N), bf16)
    xr, wr = x.double().requires_grad_(True), w.double().requires_grad_(True)
    y = xr @ wr.t()
    y.backward(g.double())
    return dict(x=x, w=w, g=g, y=y.detach(), dx=xr.grad, dw=wr.grad)


@functools.lru_cache(maxsize=None)
def ref3x3(B, H, W, C, N, bf16=False):
    """F.conv2d(padding=1) in double with autograd; everything returned channels-last: x [B,H,W,C], w [N,(tap,c)], g, y [B,H,W,N],
    dx [B,H,W,C], dw [N][tap][c]"""
    x, w, g = _round(R("p3x", B, C, H, W), bf16), _round(R("p3w", N, C, 3, 3, scale=0.1), bf16), _round(R("p3g", B, N, H, W), bf16)
    xr, wr = x.double().requires_grad_(True), w.double().requires_grad_(True)
    y = F.conv2d(xr, wr, padding=1)
    y.backward(g.double())
    nhwc = lambda t: t.detach().permute(0, 2, 3, 1).contiguous()  # noqa: E731
    ohwi = lambda t: t.detach().permute(0, 2, 3, 1).reshape(N, 9 * C).contiguous()  # noqa: E731
    return dict(x=nhwc(x), w=ohwi(w), g=nhwc(g), y=nhwc(y), dx=nhwc(xr.grad), dw=ohwi(wr.grad))


# (M, N, K): the 256x32, 128x64 and 128x128 tiles, a row count below a tile and ragged ones, N that does not fill the last column
# tile, 1, 2, 3, 5 and 32 K tiles; (300, 32, 96): a 256-row tile that emits 128-row partials
FWD1 = [(1, 32, 32), (300, 32, 96), (129, 64, 32), (130, 96, 64), (383, 160, 32), (128, 128, 64), (300, 288, 160), (70, 256, 1024)]
# (B, H, W, Cin, Cout): a single pixel, odd widths through the fast division, a tile boundary inside an image and inside an image
# row, three 32-channel groups per tap, H = 1 and W = 1
CONV3 = [(1, 1, 1, 32, 32), (3, 5, 3, 32, 64), (2, 7, 5, 64, 128), (5, 9, 3, 96, 160), (3, 12, 8, 32, 256), (2, 1, 37, 64, 96), (2, 37, 1, 32, 128)]


def check_partials(ops, group, case, st, y_ref, tile):
    """The (mean, M2, min, max) partials of a statistics epilogue: their count, the batch statistics bn_finalize_minmax folds
    them into (1e-5, as everywhere in test_kernels_gpu.py) and the per-part extremes (values of y: y's own bound)."""
    N = y_ref.shape[-1]
    y2 = y_ref.reshape(-1, N)
    M = y2.shape[0]
    if tile:
        assert st.rows == ops.gemm_p16_rows(M, N)
    assert tuple(st.shape) == ((M + st.rows - 1) // st.rows, N, 4)
    gamma, beta = R("p16gamma", N).abs() + 0.5, R("p16beta", N)
    fin = ops.bn_finalize_minmax(st, M, dev(gamma), dev(beta), None, None, False, ops.amax_slot(st.data.device))
    mean, var = y2.mean(0), y2.var(0, unbiased=False)
    e_mean, e_istd = rel(fin.mean, mean), rel(fin.invstd, 1 / torch.sqrt(var + 1e-5))
    parts = y2.split(st.rows)
    lo, hi = torch.stack([q.min(0).values for q in parts]), torch.stack([q.max(0).values for q in parts])
    ymax = float(y2.abs().max())
    got = st.data.double().cpu()
    e_ext = max(float((got[:, :, 2] - lo).abs().max()), float((got[:, :, 3] - hi).abs().max())) / ymax
    report(group, case, "mean / invstd / extremes", max(e_mean, e_istd, e_ext))
    assert e_mean < 1e-5 and e_istd < 1e-5 and e_ext < TOL, (e_mean, e_istd, e_ext)


# --------------------------------------------------------------------------- 1. forward 1x1, statistics epilogue
@pytest.mark.parametrize("M,N,K", FWD1)
def test_p16_forward_1x1(ops, M, N, K):
    r = ref1x1(M, N, K)
    xp, wp = ops.p16_pack(dev(r["x"])), ops.p16_pack(dev(r["w"]))
    for tile in (True, False):
        with kernels(ops, tile) as how:
            y, st = ops.conv_p16(xp, wp)
        case = "%dx%dx%d %s" % (M, N, K, how)
        assert tuple(y.shape) == (M, N) and y.dtype == torch.float32
        assert report("fwd1x1", case, "y", rel(y, r["y"])) < TOL
        check_partials(ops, "fwd1x1", case, st, r["y"], tile)


# --------------------------------------------------------------------------- 2. forward 3x3, statistics epilogue
@pytest.mark.parametrize("B,H,W,C,N", CONV3)
def test_p16_forward_3x3(ops, B, H, W, C, N):
    r = ref3x3(B, H, W, C, N)
    xp, wp = ops.p16_pack(dev(r["x"])), ops.p16_pack(dev(r["w"]))
    for tile in (True, False):
        with kernels(ops, tile) as how:
            y, st = ops.conv_p16(xp, wp, conv3=True)
        case = "%dx%dx%d %d>%d %s" % (B, H, W, C, N, how)
        assert tuple(y.shape) == (B, H, W, N) and y.dtype == torch.float32
        assert report("fwd3x3", case, "y", rel(y, r["y"])) < TOL
        check_partials(ops, "fwd3x3", case, st, r["y"], tile)


# --------------------------------------------------------------------------- 3. data gradient
def check_dgrad(ops, group, case, gp, wt, want, M, Nout, K, conv):
    """gemm_p16 on the transposed (3x3: rotated) filters against autograd's input gradient: plain, accumulated onto a random
    dx0, and accumulated under a ReLU bit mask (grad + where(bit, dx0, 0))."""
    dx0 = R("p16dx0", M, Nout)
    keep = R("p16keep", M, Nout) > -0.25  # ~ 60 % of the bits set
    mask = _relu_mask_words(keep).cuda()
    want = want.reshape(M, Nout)
    for tile in (True, False):
        with kernels(ops, tile) as how:
            dx = ops.empty((M, Nout), gp.data)
            ops.gemm_p16(gp, wt, dx, M, Nout, K, Nout, conv=conv)
            acc = dev(dx0)
            ops.gemm_p16(gp, wt, acc, M, Nout, K, Nout, conv=conv, accumulate=True)
            msk = dev(dx0)
            ops.gemm_p16(gp, wt, msk, M, Nout, K, Nout, conv=conv, accumulate=True, cmask=mask)
        e = (report(group, case + " " + how, "plain", rel(dx, want)),
             report(group, case + " " + how, "accumulate", rel(acc, want + dx0.double())),
             report(group, case + " " + how, "masked accumulate", rel(msk, want + torch.where(keep, dx0.double(), torch.zeros(())))))
        assert max(e) < TOL, e


# the geometries of CONV3 as they are (reduction over 9 * Cout, Cin columns) and with the channel counts swapped
@pytest.mark.parametrize("B,H,W,C,N", CONV3 + [(B, H, W, N, C) for (B, H, W, C, N) in CONV3 if C != N])
def test_p16_dgrad_3x3(ops, B, H, W, C, N):
    r = ref3x3(B, H, W, C, N)
    wd = dev(r["w"])
    gp, wt = ops.p16_pack(dev(r["g"])), ops.p16_pack_wt(wd, N, 9, C, True, ops.amax(wd))
    check_dgrad(ops, "dgrad3x3", "%dx%dx%d %d>%d" % (B, H, W, C, N), gp, wt, r["dx"], B * H * W, C, 9 * N, (H, W, N))


@pytest.mark.parametrize("M,N,K", FWD1)
def test_p16_dgrad_1x1(ops, M, N, K):
    r = ref1x1(M, N, K)
    wd = dev(r["w"])
    gp, wt = ops.p16_pack(dev(r["g"])), ops.p16_pack_wt(wd, N, 1, K, False, ops.amax(wd))
    check_dgrad(ops, "dgrad1x1", "%dx%dx%d" % (M, N, K), gp, wt, r["dx"], M, K, N, None)


# --------------------------------------------------------------------------- 4. weight gradient
# (pixels, N_out, C): the 64-row and the 128-row instantiation, dead waves in the last row and column tile, 1 to 4 and 32 K tiles
# with tails of 1, 13 and 31 pixels
WGRAD1 = [(1, 32, 32), (31, 32, 64), (33, 64, 32), (45, 96, 160), (97, 128, 128), (1000, 160, 288)]


@pytest.mark.parametrize("P,N,C", WGRAD1)
def test_p16_wgrad_1x1(ops, P, N, C):
    r = ref1x1(P, N, C)
    gp, xp = ops.p16_pack(dev(r["g"])), ops.p16_pack(dev(r["x"]))
    for tile in (True, False):
        with kernels(ops, tile) as how:
            dw = ops.wgrad_p16(gp, xp)
        assert tuple(dw.shape) == (N, C)
        assert report("wgrad1x1", "%dx%dx%d %s" % (P, N, C, how), "dw", rel(dw, r["dw"])) < TOL


@pytest.mark.parametrize("B,H,W,C,N", CONV3)
def test_p16_wgrad_3x3(ops, B, H, W, C, N):
    r = ref3x3(B, H, W, C, N)
    gp, xp = ops.p16_pack(dev(r["g"])), ops.p16_pack(dev(r["x"]))
    for tile in (True, False):
        with kernels(ops, tile) as how:
            dw = ops.wgrad_p16(gp, xp, conv=(H, W, C))
        assert tuple(dw.shape) == (N, 9 * C)
        assert report("wgrad3x3", "%dx%dx%d %d>%d %s" % (B, H, W, C, N, how), "dw", rel(dw, r["dw"])) < TOL


# --------------------------------------------------------------------------- 5. forced split counts
# splits >= 8 take the XCD-owned grid; 9 leaves idle workgroups; (100, 96, 64) x 8: splits 4 to 7 own no pixel; 288 pixels x 16:
# seven empty splits; 45 pixels x 3: the last split is empty
SPLITS = ([("1x1", (1000, 160, 288), s) for s in (1, 2, 3, 8, 9, 16)] + [("3x3", (3, 12, 8, 32, 256), s) for s in (1, 2, 3, 8, 9, 16)]
          + [("1x1", (100, 96, 64), 8), ("3x3", (3, 5, 3, 32, 64), 3)])
GUARD = 8  # slabs of poison kept behind the ones the kernel may write


@pytest.mark.parametrize("form,shape,splits", SPLITS)
def test_p16_wgrad_forced_splits(ops, monkeypatch, form, shape, splits):
    """Every split count gives the fp64 result.  Every buffer the wrapper allocates is NaN first, so a split that owns no
    pixel must WRITE its zeros (checked exactly), and the slabs behind the last one must stay untouched (idle workgroups of
    the XCD-owned grid return without writing)."""
    if form == "1x1":
        P, N, C = shape
        r, conv, J = ref1x1(P, N, C), None, C
    else:
        B, H, W, C, N = shape
        r, conv, J, P = ref3x3(B, H, W, C, N), (H, W, C), 9 * C, B * H * W
    gp, xp = ops.p16_pack(dev(r["g"])), ops.p16_pack(dev(r["x"]))
    slabs = []

    def poisoned(shp, like=None, dtype=torch.float32, device=None):
        shp = tuple(shp)
        full = torch.full((shp[0] + GUARD,) + shp[1:], float("nan"), dtype=dtype, device=device if device is not None else like.device)
        if len(shp) == 3:
            slabs.append(full)
        return full[: shp[0]]

    monkeypatch.setattr(ops, "_WGRAD_SPLITS_OVERRIDE", splits)
    monkeypatch.setattr(ops, "empty", poisoned)
    dw = ops.wgrad_p16(gp, xp, conv=conv)
    monkeypatch.undo()
    torch.cuda.synchronize()
    assert tuple(dw.shape) == (N, J)
    assert report("splits", "%s %s x%d" % (form, "x".join(map(str, shape)), splits), "dw", rel(dw, r["dw"])) < TOL
    assert len(slabs) == (1 if splits > 1 else 0)
    if splits > 1:
        slab = slabs[0].cpu()
        chunk = ((P + splits - 1) // splits + 31) // 32 * 32  # pixels per split: whole 32-pixel K tiles
        empty = [s for s in range(splits) if s * chunk >= P]
        for s in empty:
            assert bool((slab[s] == 0).all()), "split %d owns no pixel: its slab must hold zeros" % s
        assert bool(torch.isnan(slab[splits:]).all()), "a workgroup wrote behind the last split's slab"
        assert rel(slab[:splits].double().sum(0), r["dw"]) < TOL


# --------------------------------------------------------------------------- 6. bf16 operands (fmt 2)
@pytest.mark.parametrize("M,N,K", [(130, 64, 64), (257, 192, 128)])
def test_bf16_forward_1x1(ops, monkeypatch, M, N, K):
    monkeypatch.setattr(ops, "BF16_Y", False)  # fp32 output
    r = ref1x1(M, N, K, True)
    xp, wp = ops.p16_pack(dev(r["x"]), fmt=2), ops.p16_pack(dev(r["w"]), fmt=2)
    assert torch.equal(xp.data.float().cpu(), r["x"])  # the packed operand is the rounding the reference assumed
    for tile in (True, False):
        with kernels(ops, tile) as how:
            y, st = ops.conv_p16(xp, wp)
        assert y.dtype == torch.float32 and tuple(st.shape) == ((M + 127) // 128, N, 2)
        assert report("bf16", "fwd1x1 %dx%dx%d %s" % (M, N, K, how), "y", rel(y, r["y"])) < TOL


@pytest.mark.parametrize("N", [128, 64])  # (64: the 128x64 instantiation of the gather form)
def test_bf16_forward_3x3(ops, monkeypatch, N):
    monkeypatch.setattr(ops, "BF16_Y", False)
    B, H, W, C = 2, 7, 5, 64
    r = ref3x3(B, H, W, C, N, True)
    xp, wp = ops.p16_pack(dev(r["x"]), fmt=2), ops.p16_pack(dev(r["w"]), fmt=2)
    for tile in (True, False):
        with kernels(ops, tile) as how:
            y, st = ops.conv_p16(xp, wp, conv3=True)
        assert y.dtype == torch.float32 and tuple(y.shape) == (B, H, W, N)
        assert report("bf16", "fwd3x3 %dx%dx%d %d>%d %s" % (B, H, W, C, N, how), "y", rel(y, r["y"])) < TOL


@pytest.mark.parametrize("P,N,C", [(65, 64, 64), (200, 128, 192)])
def test_bf16_wgrad_1x1(ops, P, N, C):
    r = ref1x1(P, N, C, True)
    gp, xp = ops.p16_pack(dev(r["g"]), fmt=2), ops.p16_pack(dev(r["x"]), fmt=2)
    for tile in (True, False):
        with kernels(ops, tile) as how:
            dw = ops.wgrad_p16(gp, xp)
        assert dw.dtype == torch.float32
        assert report("bf16", "wgrad1x1 %dx%dx%d %s" % (P, N, C, how), "dw", rel(dw, r["dw"])) < TOL


@pytest.mark.parametrize("N", [64, 128])  # (128: the 128-row instantiation of the gather form)
def test_bf16_wgrad_3x3(ops, N):
    B, H, W, C = 2, 7, 5, 64
    r = ref3x3(B, H, W, C, N, True)
    gp, xp = ops.p16_pack(dev(r["g"]), fmt=2), ops.p16_pack(dev(r["x"]), fmt=2)
    for tile in (True, False):
        with kernels(ops, tile) as how:
            dw = ops.wgrad_p16(gp, xp, conv=(H, W, C))
        assert report("bf16", "wgrad3x3 %dx%dx%d %d>%d %s" % (B, H, W, C, N, how), "dw", rel(dw, r["dw"])) < TOL


# --------------------------------------------------------------------------- 7. refused arguments
def test_p16_entry_points_refuse_bad_arguments(ops):
    """What trid_gemm_p16 / trid_gemm_p16_wgrad check on the host before any launch: a non-zero return with a message in
    trid_last_error_string, and a library that still works afterwards."""
    from textreid_amd import lib as L

    lib = L.load()
    buf = [torch.zeros(64 * 320, device="cuda") for _ in range(3)]  # (room for every shape below, were it launched)

    def desc(a_mode, b_mode, M, N, K, lda, ldb, ldc, **kw):
        d = L.GemmDesc()
        d.A, d.B, d.C = (b.data_ptr() for b in buf)
        d.M, d.N, d.K, d.lda, d.ldb, d.ldc = M, N, K, lda, ldb, ldc
        d.batch, d.splits, d.a_mode, d.b_mode, d.alpha, d.precision = 1, 1, a_mode, b_mode, 1.0, 16
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    def refused(name, d, message, *extra):
        rc = getattr(lib, name)(ctypes.addressof(d), *extra, ops.stream())
        assert rc != 0 and message in L.last_error(), (name, rc, L.last_error())

    wg, fw = "trid_gemm_p16_wgrad", "trid_gemm_p16"
    refused(wg, desc(ops.A_MC, ops.B_NC, 48, 32, 64, 64, 32, 32), "multiples of 32")  # 48 output channels
    refused(wg, desc(ops.A_MC, ops.B_CONV, 32, 288, 50, 32, 32, 288, H=7, W=5, Cin=32), "K a multiple of H*W")  # 50 pixels of 7x5 images
    refused(wg, desc(ops.A_MC, ops.B_NC, 32, 32, 64, 32, 32, 32, accumulate=1), "plain or split-K output only")
    refused(fw, desc(ops.A_KC, ops.B_KC, 64, 32, 48, 64, 64, 32), "K must be a positive multiple of 32", -1)
    refused(fw, desc(ops.A_CONV, ops.B_KC, 35, 32, 288, 32, 288, 32, H=7, W=5, Cin=32, splits=2, strideSplit=35 * 32), "splits == 1", -1)
    torch.cuda.synchronize()
    r = ref1x1(33, 64, 32)
    xp, wp, gp = ops.p16_pack(dev(r["x"])), ops.p16_pack(dev(r["w"])), ops.p16_pack(dev(r["g"]))
    with kernels(ops, True):
        assert rel(ops.conv_p16(xp, wp, stats=False), r["y"]) < TOL
    assert rel(ops.wgrad_p16(gp, xp), r["dw"]) < TOL


# --------------------------------------------------------------------------- operands that have underflowed to ~1e-35
@pytest.mark.parametrize("side", ["A", "B"])
@pytest.mark.parametrize("exp", [116, 120])
def test_p16_scale_of_a_tiny_amax(ops, exp, side):
    """A tensor whose largest magnitude is a NORMAL fp32 number below 2^-114 (a gradient that has underflowed to ~1e-35):
    its power-of-two fp16 scale must stay a finite positive number - packing, unpacking and the products against an
    ordinary operand give finite, fp32-class results.  (Before f16_scale_of capped the scale at 2^127: +inf or a negative
    scale - non-finite values at 2^-116, an all-zero tensor at 2^-120.)"""
    M, N, K = 130, 96, 64

    def tiny(t):
        return (t.double() / t.double().abs().max() * 2.0 ** -exp).float()

    def ok(what, got, ref):
        got, ref = got.double().cpu(), ref.double()
        assert bool(torch.isfinite(got).all()), what
        top = float(ref.abs().max())
        e = report("tinyamax", "2^-%d %s" % (exp, side), what, float((got - ref).abs().max()) / top)
        assert e < TOL or (top < F32_TINY and float(got.abs().max()) < F32_TINY), (what, e)

    x, w, g = R("tx", M, K), R("tw", N, K, scale=0.2), R("tg", M, N)
    t = tiny(x)
    assert float(t.abs().max()) == 2.0 ** -exp
    tp = ops.p16_pack(dev(t))
    ok("pack / unpack", tp.unpack(), t)
    # forward y = x . w^T, the tiny tensor as the A or as the B operand
    a, b = (t, w) if side == "A" else (x, tiny(w))
    ap, bp = ops.p16_pack(dev(a)), ops.p16_pack(dev(b))
    for tile in (True, False):
        with kernels(ops, tile) as how:
            ok("forward " + how, ops.conv_p16(ap, bp, stats=False), a.double() @ b.double().t())
    # weight gradient dw = g^T . x
    a, b = (tiny(g), x) if side == "A" else (g, t)
    ok("wgrad", ops.wgrad_p16(ops.p16_pack(dev(a)), ops.p16_pack(dev(b))), a.double().t() @ b.double())
