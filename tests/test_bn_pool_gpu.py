"""fp64 parity of the BatchNorm and pool kernels of csrc/bn_pool.hip at edge shapes, in all three storage formats (fp32, P16,
plain bf16): bn_finalize / bn_finalize_minmax, bn_apply, bn_apply_pool2, bn_bwd / bn_bwd_p16, bn_bwd_dual_p16, avgpool2_bwd,
and P16.unpack (trid_p16_unpack_f32), which the P16 results of every other test in the suite are decoded with.

Every case is compared with the plain fp64 CPU reference of tests/bn_pool_ref.py (F.batch_norm / F.relu / F.avg_pool2d in
double, autograd for the gradients) on inputs seeded through oracle.fill; P16 results are decoded by the CPU decoder of that
module, not by the library.  The statistics every pass reads come from bn_finalize_minmax on raw partials built in fp64.

Shapes (M rows x C channels): (2, 32) smallest batch with a variance; (37, 32) M*C/4 = 296 is no multiple of 64 - a partial last
ReLU-bit word and a ragged last trip; (67, 96) C/4 = 24 does not divide 256 - the carried (row, channel quad) counters wrap with
step_c = 8, three 32-channel P16 groups per row, forward only (the backward refuses this C); (1029, 64) several trips per thread,
odd M; (515, 1024) C/4 = 256, the CW boundary; (130, 2048) two channel-quad slices; (300, 8), (193, 4) fp32 forms only.  Pooled
forms (B, H, W): (1, 2, 2), (3, 6, 10) - W/2 = 5 and the fast division by 10 and 6 - and (2, 4, 2), with C = 32, 64 and (fp32) 8.

Every output and the bit-word buffer is a slice of a larger tensor pre-filled with a sentinel (NaN; 0x5A.. for words), with
64 elements of it in front and behind: after the test those must be unchanged, and an element the kernel did not write fails the
comparison as NaN.  This is a plain comparison after normal runs.

Bounds (tests/bn_pool_ref.py TOL_*; the worst value measured on the MI355X beside each):
  group                      bound                                                                        measured
  a  finalize                mean / invstd / scale / shift / running buffers: TOL_STAT = 3.6e-6 of each    1.8e-7 (running_mean); bound / max 1.000
                             vector's largest entry = 4x the fp32 yardstick (8.95e-7); the reference is
                             the exact merge of the fp32 partials the kernel is given (its input).  Bound:
                             >= true max (1 - 1e-6) and <= 2 true max.
  b  bn_apply                fp32: TOL_F32 = 1e-6 of max|ref| (yardstick 1.43e-7).  P16: that + 2^-22 of   fp32 1.7e-7; P16 0.19 of the bound
                             the tensor's amax scalar (11 + 11 bits below 2^14, x2 for amax's place in
                             its binade; without the low plane: 2^-11, 2000x).  bf16: that + 2^-8 |ref|
                             per element.  Published amax == max|out| exactly.  Bits == (ref > 0) outside
                             |z| < 1e-5 max|z|, at most 0.1 % of the elements inside.
  c  bn_apply_pool2          as b                                                                          fp32 1.0e-7; P16 0.17; bf16 0.996
  d  bn_bwd / bn_bwd_p16     dgamma / dbeta: TOL_SUM = 4.9e-6 of each vector's largest entry (yardstick     sums 8.1e-7; dy 0.28 / P16 0.29 / bf16 0.995
                             1.22e-6); dy: TOL_DY = 4.1e-7 of max|scale| max|g| (0.25 g when pooled;
                             yardstick 1.00e-7) + the format's term; dres as b.  P16 bound >= true max|dy|
                             (1 - 1e-6); its ratio to the true maximum is printed, not bounded.
  e  bn_bwd_dual_p16         as d, for both layers                                                         sums 1.7e-7; dy 0.22 of the bound
  f  avgpool2_bwd            as b (fp32, bf16)                                                             fp32 5.1e-8; bf16 0.996
  g  P16.unpack              bit-equal to the CPU decoder                                                  exact
The incoming gradient is zeroed at the elements inside the ReLU band, so that the masked sums and dy do not depend on a
decision fp32 cannot make.  With a residual the published amax scalar must be exactly bound + bound_res; that this sum stays
within 2x of the true maximum holds for these inputs (terms of unequal size; largest ratio 1.66), it is no property of a kernel.

Not covered: the non-temporal access path (tensors of 128 MB and more, or TRID_BN_NT, read once per process) - a reference of
that size does not fit a test of a few seconds; the fused forms (GEMM-epilogue statistics, presummed backward sums,
conv1x1_bn_res_p16) are covered where they are."""

import functools
import math
import re

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import bn_pool_ref as ref  # noqa: E402
import oracle.fill as OF  # noqa: E402
from bn_pool_ref import BAND_SHARE, TOL_DY, TOL_F32, TOL_STAT, TOL_SUM  # noqa: E402


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from textreid_amd import ops as o

    yield o
    reference.cache_clear()  # (the fp64 references of this file: nothing for the rest of the suite to carry)
    ref.inputs.cache_clear()


def R(name, *shape, scale=1.0):
    return OF.randn(name, shape, 0, scale)


def dev(t):
    return t.cuda().contiguous()


def rel(got, ref_):
    """largest absolute error over the reference's largest magnitude"""
    got, ref_ = got.detach().double().cpu(), ref_.detach().double().cpu()
    return float((got - ref_).abs().max() / (ref_.abs().max() + 1e-300))


def report(group, case, what, err, used=None):
    print("bn/pool parity %-9s %-26s %-34s %.2e%s" % (group, case, what, err, "" if used is None else "  (%.3f of the bound)" % used))
    return err


def scalar(v):
    return torch.tensor([float(v)], dtype=torch.float32, device="cuda")


def bf(t):
    return t.bfloat16().float()


# --------------------------------------------------------------------------- guard regions
GUARD = 64  # sentinel elements in front of and behind every buffer the wrappers allocate


def _sentinel(n, dtype, device):
    if dtype.is_floating_point:
        return torch.full((n,), float("nan"), dtype=dtype, device=device)
    return torch.full((n,), 0x5A5A5A5A5A5A5A5A if dtype == torch.int64 else 0x5A, dtype=dtype, device=device)


def _raw(t):
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


class GuardedTorch:
    """stands in for the `torch` module inside textreid_amd.ops: empty / empty_like hand out the middle of a sentinel-filled
    buffer (same dtype, 16-byte aligned), everything else is torch's own"""

    def __init__(self, log):
        self._log = log

    def __getattr__(self, name):
        return getattr(torch, name)

    def empty(self, *shape, dtype=torch.float32, device=None):
        if len(shape) == 1 and not isinstance(shape[0], int):
            shape = tuple(shape[0])
        n = math.prod(shape)
        full = _sentinel(n + 2 * GUARD, dtype, device)
        self._log.append((full, n))
        return full[GUARD : GUARD + n].view(shape)

    def empty_like(self, t):
        return self.empty(tuple(t.shape), dtype=t.dtype, device=t.device)


@pytest.fixture(autouse=True)
def guard(ops, monkeypatch):
    log = []
    proxy = GuardedTorch(log)
    monkeypatch.setattr(ops, "torch", proxy)
    yield proxy
    torch.cuda.synchronize()
    assert log, "no allocation of the wrappers went through the guard"
    for k, (full, n) in enumerate(log):
        want = _raw(_sentinel(1, full.dtype, full.device))[0]
        raw = _raw(full)
        assert bool((raw[:GUARD] == want).all()), "allocation %d (%s x %d): written in front of the buffer" % (k, full.dtype, n)
        assert bool((raw[GUARD + n :] == want).all()), "allocation %d (%s x %d): written behind the buffer" % (k, full.dtype, n)


def gdev(guard, t):
    """a guarded device copy of t (buffers the test itself hands to a kernel as an output)"""
    out = guard.empty(tuple(t.shape), dtype=t.dtype, device="cuda")
    out.copy_(t)
    return out


# --------------------------------------------------------------------------- fp64 references (computed once, never written to)
@functools.lru_cache(maxsize=24)
def reference(shape, variant, pool=False, y16=False, r16=False, g16=False, rp16=False):
    """variant: plain | relu | res (identity residual) | resbn (BatchNorm of the residual); y16 / r16 / g16: that tensor rounded
    to bf16 first; rp16: the residual as the P16 encoder stores it.  The gradient is zero inside the ReLU band."""
    d = ref.inputs(*shape)
    y = bf(d["y"]) if y16 else d["y"]
    res = bf(d["res"]) if r16 else d["res"]
    if rp16:
        ramax = float(res.abs().max())
        res = ref.p16_decode(ref.p16_encode(res, ramax), ramax)
    kw = dict(res=res) if variant in ("res", "resbn") else {}
    if variant == "resbn":
        kw.update(res_gamma=d["gamma2"], res_beta=d["beta2"])
    relu = variant != "plain"
    z = ref.bn_reference(y, d["gamma"], d["beta"], relu, pool=pool, **kw)["z"]
    band, share = ref.relu_band(z) if relu else (torch.zeros_like(z, dtype=torch.bool), 0.0)
    g = d["gp"] if pool else d["g"]
    g = bf(g) if g16 else g
    hit = F.max_pool2d(band.permute(0, 3, 1, 2).float(), 2).permute(0, 2, 3, 1) > 0 if pool else band
    g = torch.where(hit, torch.zeros(()), g)
    r = ref.bn_reference(y, d["gamma"], d["beta"], relu, pool=pool, g=g, **kw)
    r.update(y=y, res=res, g=g, band=band, share=share, keep=r["z"] > 0, st=ref.bn_stats(y, d["gamma"], d["beta"]),
             st2=ref.bn_stats(res, d["gamma2"], d["beta2"]))
    C = shape[-1]
    xh = ((y.double() - r["st"]["mean"]) * r["st"]["invstd"]).reshape(-1, C)
    dz = r["dz"].reshape(-1, C).abs()
    r.update(l1_dgamma=float((dz * xh.abs()).sum(0).max()), l1_dbeta=float(dz.sum(0).max()), rows=dz.shape[0])
    return r


def finalize(ops, y, gamma, beta, relu=False):
    """(BNState, bound) of y [.., C] from raw fp64-built (mean, M2, min, max) partials of 128 rows"""
    C = y.shape[-1]
    raw = dev(ref.partials(y.float(), 128, True))
    bound = ops.amax_slot(raw.device)
    st = ops.bn_finalize_minmax(raw, y.numel() // C, dev(gamma), dev(beta), None, None, relu, bound, rows_per_part=128)
    return st, bound


# --------------------------------------------------------------------------- comparisons
def check_out(group, case, what, got, want, f32_term=None):
    """got: an fp32 tensor, a bf16 tensor or an ops.P16 of either format, against the fp64 `want` under the format's bound"""
    want = want.double()
    top = float(want.abs().max())
    term = TOL_F32 * top if f32_term is None else f32_term
    fmt = getattr(got, "fmt", None)
    data = got.data if fmt is not None else got
    assert tuple(data.shape) == tuple(want.shape), (tuple(data.shape), tuple(want.shape))
    if fmt == 1:
        amax = float(got.amax)
        val = ref.p16_decode(data, amax)
        used, kind = ref.p16_excess(val, want, amax, term), " [P16]"
    elif data.dtype == torch.bfloat16:
        val = data.float().cpu()
        used, kind = ref.bf16_excess(val, want, term), " [bf16]"
    else:
        assert data.dtype == torch.float32
        val = data.cpu()
        err = float((val.double() - want).abs().max())
        used, kind = (err / term if term > 0 else (0.0 if err == 0 else float("inf"))), ""
    report(group, case, what + kind, float((val.double() - want).abs().max()) / (top + 1e-300), used)
    assert used <= 1.0, (group, case, what, used)  # (NaN - an element that was never written - fails too)
    return used


def check_vec(group, case, what, got, want, tol, l1=None, rows=0):
    """|got - want| <= tol * the vector's largest entry.  l1: the largest sum over the rows of the terms' MAGNITUDES.  A vector
    whose largest entry is below ONE fp32 rounding of that (2^-24 l1) vanishes analytically - the pooled 1x2x2 case without a
    mask: dgamma = g * sum(xhat) = 0 - and has no entry to be relative to: it is held to the a-priori bound of an fp32 sum of
    `rows` rounded terms, (rows + 1) 2^-24 l1, instead (4 rows: measured 1.2e-7 of a bound of 5e-7)."""
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    err, top = float((got - want).abs().max()), float(want.abs().max())
    if l1 is not None and top < 2.0 ** -24 * l1:
        used = report(group, case, what + " (vanishing: of (rows + 1) 2^-24 l1)", err / ((rows + 1) * 2.0 ** -24 * l1))
        assert used <= 1.0, (group, case, what, err, l1)
        return
    e = report(group, case, what, err / (top + 1e-300))
    assert e <= tol, (group, case, what, e)


def check_bits(group, case, words, r):
    M, C = r["z"].numel() // r["z"].shape[-1], r["z"].shape[-1]
    assert words.dtype == torch.int64 and words.numel() == (M * C // 4 + 63) // 64 * 4
    got = ref.unpack_bits(words, M, C).reshape(r["keep"].shape)
    wrong = int(((got != r["keep"]) & ~r["band"]).sum())
    report(group, case, "bits: share inside the band", r["share"])
    assert r["share"] <= BAND_SHARE and wrong == 0, (group, case, r["share"], wrong)


def check_amax_exact(slot, out):
    assert float(slot) == float(out.abs().max()), (float(slot), float(out.abs().max()))


def check_bound(group, case, what, pub, true, upper=2.0):
    """a published bound against the true fp64 maximum; upper=None: only the upper-bound property, the ratio is printed"""
    pub = float(pub)
    report(group, case, what + ": bound / true max", pub / true if true > 0 else float(pub > 0))
    assert pub >= true * (1 - 1e-6), (group, case, what, pub, true)
    if upper is not None:
        assert pub <= upper * true, (group, case, what, pub, true)


# --------------------------------------------------------------------------- a. finalize
FIN_PARTS = [(1, 3), (16, 48), (17, 50), (768, 2304), (769, 2307), (769 * 2 + 5, 4627)]  # (parts of 3 rows, M): 50, 4627 leave a short last part


def _finalize_both(ops, raw2, raw4, M, gamma, beta, rm0, rv0, relu):
    """-> [(name, BNState, running_mean, running_var, bound or None)] of bn_finalize and bn_finalize_minmax on the raw partials"""
    out = []
    for name, raw in (("finalize", raw2), ("minmax", raw4)):
        rm, rv = (dev(rm0), dev(rv0)) if rm0 is not None else (None, None)
        if name == "finalize":
            st, bound = ops.bn_finalize(ops.Partials(dev(raw), 3), M, dev(gamma), dev(beta), rm, rv), None
        else:
            bound = ops.amax_slot(torch.device("cuda", torch.cuda.current_device()))
            st = ops.bn_finalize_minmax(dev(raw), M, dev(gamma), dev(beta), rm, rv, relu, bound, rows_per_part=3)
        out.append((name, st, rm, rv, bound))
    return out


@pytest.mark.parametrize("C", [4, 24, 64])
@pytest.mark.parametrize("parts,M", FIN_PARTS)
def test_finalize_from_raw_partials(ops, parts, M, C):
    """16 channels per workgroup (C = 4, 24: a partly filled one), one launch up to 768 parts, range sums + merge above; the
    running-statistics update; the published bound for relu 0 / 1"""
    d = ref.inputs(1, 1, M, C)
    y, gamma, beta, rm0, rv0 = d["y"].reshape(M, C), d["gamma"], d["beta"], d["rmean"], d["rvar"]
    raw2, raw4 = ref.partials(y, 3, False), ref.partials(y, 3, True)
    assert raw4.shape[0] == parts and torch.equal(raw2, raw4[:, :, :2].contiguous())
    m = ref.merge_partials(raw4, 3, M)  # the exact statistics of the kernel's input
    invstd = 1.0 / torch.sqrt(m["var"] + ref.EPS)
    scale = gamma.double() * invstd
    shift = beta.double() - m["mean"] * scale
    rm_ref, rv_ref = ref.running_update(y, rm0, rv0)
    z = y.double() * scale + shift
    case = "%d parts M=%d C=%d" % (parts, M, C)
    for relu in (False, True):
        for running in (False, True):
            for name, st, rm, rv, bound in _finalize_both(ops, raw2, raw4, M, gamma, beta, rm0 if running else None, rv0, relu):
                if name == "finalize" and relu:
                    continue  # (no relu argument: ran with relu = False already)
                for what, got, want in (("mean", st.mean, m["mean"]), ("invstd", st.invstd, invstd), ("scale", st.scale, scale), ("shift", st.shift, shift)):
                    check_vec("finalize", case, "%s %s" % (name, what), got, want, TOL_STAT)
                if running:
                    check_vec("finalize", case, name + " running_mean", rm, rm_ref, TOL_STAT)
                    check_vec("finalize", case, name + " running_var", rv, rv_ref, TOL_STAT)
                if bound is not None:
                    check_bound("finalize", case, "relu=%d" % relu, bound, float((z.clamp(min=0) if relu else z).abs().max()))


@pytest.mark.parametrize("parts", [17, 769])
def test_finalize_channel_means_300_sigma_out(ops, parts):
    """channel means at +-300 standard deviations, raw partials of 3 rows (one launch; range sums + merge): only means may ever
    be subtracted.  (Against the direct fp64 statistics of y the fp32 rounding of the partial MEANS - the kernel's input -
    shows as ~1e-6 of invstd; that figure is printed.)"""
    C, M = 64, parts * 3 - 1
    sigma = torch.linspace(0.5, 2.0, C)
    y = (R("off%d" % parts, M, C) + torch.linspace(-300.0, 300.0, C)) * sigma
    raw2, raw4 = ref.partials(y, 3, False), ref.partials(y, 3, True)
    m = ref.merge_partials(raw4, 3, M)
    invstd = 1.0 / torch.sqrt(m["var"] + ref.EPS)
    direct = ref.bn_stats(y, torch.ones(C), torch.zeros(C))
    report("finalize", "300 sigma, %d parts" % parts, "input rounding: invstd(partials) vs invstd(y)", rel(invstd, direct["invstd"]))
    for name, st, _, _, _ in _finalize_both(ops, raw2, raw4, M, torch.ones(C), torch.zeros(C), None, None, False):
        check_vec("finalize", "300 sigma, %d parts" % parts, name + " mean", st.mean, m["mean"], TOL_STAT)
        check_vec("finalize", "300 sigma, %d parts" % parts, name + " invstd", st.invstd, invstd, TOL_STAT)


# --------------------------------------------------------------------------- b. bn_apply
VARIANTS = ("plain", "relu", "res", "resbn")


def _res_args(ops, d, variant, r, st2):
    """(res tensor on the device, res_st) of a variant for an fp32 residual"""
    if variant == "res":
        return dev(r["res"]), None
    if variant == "resbn":
        return dev(r["res"]), st2
    return None, None


@pytest.mark.parametrize("M,C", ref.SHAPES + ref.SHAPES_F32)
def test_bn_apply_fp32(ops, M, C):
    shape = (1, 1, M, C)
    d = ref.inputs(*shape)
    yd = dev(d["y"])
    st, _ = finalize(ops, d["y"], d["gamma"], d["beta"])
    st2, _ = finalize(ops, d["res"], d["gamma2"], d["beta2"])
    for variant in VARIANTS:
        r = reference(shape, variant)
        res, res_st = _res_args(ops, d, variant, r, st2)
        case = "%dx%d %s" % (M, C, variant)
        slot = ops.amax_slot(yd.device)
        out, bits = ops.bn_apply(yd, st, relu=variant != "plain", res=res, res_st=res_st, want_mask=True, amax=slot)
        check_out("apply", case, "out", out, r["out"])
        check_amax_exact(slot, out)
        if variant != "plain":
            check_bits("apply", case, bits, r)
        assert torch.equal(ops.bn_apply(yd, st, relu=variant != "plain", res=res, res_st=res_st), out)  # (no mask, no amax: the same values)
    # eval-mode coefficients from the running buffers
    ste = ops.bn_eval_coeffs(dev(d["gamma"]), dev(d["beta"]), dev(d["rmean"]), dev(d["rvar"]))
    sc = d["gamma"].double() / torch.sqrt(d["rvar"].double() + ref.EPS)
    check_vec("apply", "%dx%d eval" % (M, C), "scale", ste.scale, sc, TOL_F32)
    check_vec("apply", "%dx%d eval" % (M, C), "shift", ste.shift, d["beta"].double() - d["rmean"].double() * sc, TOL_F32)
    want = F.relu(F.batch_norm(d["y"].double().reshape(M, C), d["rmean"].double(), d["rvar"].double(), d["gamma"].double(), d["beta"].double(), False, 0.1, ref.EPS))
    check_out("apply", "%dx%d eval" % (M, C), "out", ops.bn_apply(yd, ste, relu=True), want.reshape(shape))
    # an all-zero output publishes 0
    zero = ops.BNState(C, yd)
    zero.scale.zero_()
    zero.shift.fill_(-1.0)
    slot = ops.amax_slot(yd.device)
    out = ops.bn_apply(yd, zero, relu=True, amax=slot)
    assert float(out.abs().max()) == 0.0 and float(slot) == 0.0


@pytest.mark.parametrize("M,C", ref.SHAPES)
def test_bn_apply_p16(ops, M, C):
    """P16 out with an fp32 residual and with a P16 residual; bound / bound_res from the fp64 reference's true maxima and from
    bn_finalize_minmax"""
    shape = (1, 1, M, C)
    d = ref.inputs(*shape)
    yd = dev(d["y"])
    st, b_plain = finalize(ops, d["y"], d["gamma"], d["beta"])
    _, b_relu = finalize(ops, d["y"], d["gamma"], d["beta"], relu=True)
    st2, b2 = finalize(ops, d["res"], d["gamma2"], d["beta2"])
    zmax = float((d["y"].double() * reference(shape, "plain")["st"]["scale"] + reference(shape, "plain")["st"]["shift"]).abs().max())
    for variant in VARIANTS:
        r = reference(shape, variant)
        res, res_st = _res_args(ops, d, variant, r, st2)
        true = float(r["out"].abs().max())
        if variant in ("plain", "relu"):
            sources = {"true": (scalar(true), None), "minmax": (b_plain if variant == "plain" else b_relu, None)}
            check_bound("apply", "%dx%d %s" % (M, C, variant), "bn_finalize_minmax", sources["minmax"][0], true)
        elif variant == "res":
            sources = {"true": (scalar(zmax), scalar(r["res"].abs().max())), "minmax": (b_plain, ops.amax(res))}
        else:
            s2 = r["st2"]
            rmax = float((r["res"].double() * s2["scale"] + s2["shift"]).abs().max())
            sources = {"true": (scalar(zmax), scalar(rmax)), "minmax": (b_plain, b2)}
            check_bound("apply", "%dx%d %s" % (M, C, variant), "bn_finalize_minmax of the residual", b2, rmax)
        for src, (bound, bound_res) in sources.items():
            case = "%dx%d %s %s" % (M, C, variant, src)
            out, bits = ops.bn_apply_p16(yd, st, bound, relu=variant != "plain", res=res, res_st=res_st, bound_res=bound_res, want_mask=True, fmt=1)
            check_out("apply", case, "out", out, r["out"])
            if variant != "plain":
                check_bits("apply", case, bits, r)
            if bound_res is not None:
                assert float(out.amax) == float((bound + bound_res).float()), "the published scalar is bound + bound_res"
            check_bound("apply", case, "published amax", out.amax, true)
    # a P16 identity residual (decoded on the fly), written by the CPU encoder
    r = reference(shape, "res", rp16=True)
    ramax = float(d["res"].abs().max())
    resp = ops.P16(dev(ref.p16_encode(d["res"], ramax)), scalar(ramax))
    for src, bound in (("true", scalar(zmax)), ("minmax", b_plain)):
        out, bits = ops.bn_apply_p16(yd, st, bound, relu=True, res=resp, bound_res=resp.amax, want_mask=True, fmt=1)
        case = "%dx%d P16 res %s" % (M, C, src)
        check_out("apply", case, "out", out, r["out"])
        check_bits("apply", case, bits, r)
        assert float(out.amax) == float((bound + resp.amax).float())
        check_bound("apply", case, "published amax", out.amax, float(r["out"].abs().max()))


@pytest.mark.parametrize("M,C", ref.SHAPES)
def test_bn_apply_bf16(ops, M, C):
    """bf16 out with fp32 y, with bf16 y, and with a bf16 residual (identity: a fmt-2 P16 record; raw conv output: with res_st)"""
    shape = (1, 1, M, C)
    d = ref.inputs(*shape)
    for y16 in (False, True):
        y = bf(d["y"]) if y16 else d["y"]
        yd = dev(y.bfloat16()) if y16 else dev(y)
        st, _ = finalize(ops, y, d["gamma"], d["beta"])
        for variant in VARIANTS:
            for r16 in ((False, True) if variant in ("res", "resbn") else (False,)):
                r = reference(shape, variant, y16=y16, r16=r16)
                st2, _ = finalize(ops, r["res"], d["gamma2"], d["beta2"])
                res, res_st = _res_args(ops, d, variant, r, st2)
                if r16:
                    res = ops.P16(res.bfloat16(), None, 2) if variant == "res" else res.bfloat16()
                out, bits = ops.bn_apply_p16(yd, st, None, relu=variant != "plain", res=res, res_st=res_st, want_mask=True, fmt=2)
                case = "%dx%d %s%s%s" % (M, C, variant, " y16" if y16 else "", " r16" if r16 else "")
                assert out.fmt == 2 and out.data.dtype == torch.bfloat16
                check_out("apply", case, "out", out, r["out"])
                if variant != "plain":
                    check_bits("apply", case, bits, r)


# --------------------------------------------------------------------------- c. bn_apply_pool2
POOL_CASES = [(B, H, W, C) for (B, H, W) in ref.POOLED for C in (8, 32, 64)]


@pytest.mark.parametrize("B,H,W,C", POOL_CASES)
def test_bn_apply_pool2(ops, B, H, W, C):
    shape = (B, H, W, C)
    d = ref.inputs(*shape)
    yd = dev(d["y"])
    name = "%dx%dx%dx%d" % shape
    pool64 = lambda t: F.avg_pool2d(t.double().permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1)  # noqa: E731
    for relu in (False, True):
        r = reference(shape, "relu" if relu else "plain", pool=True)
        st, bound = finalize(ops, d["y"], d["gamma"], d["beta"], relu=relu)
        case = "%s relu=%d" % (name, relu)
        slot = ops.amax_slot(yd.device)
        out = ops.bn_apply_pool2(yd, st, relu=relu, amax=slot)
        check_out("pool", case, "fp32 -> fp32", out, r["out"])
        check_amax_exact(slot, out)
        if C % 32:
            continue
        act = r["z"].clamp(min=0) if relu else r["z"]
        for src, b in (("true", scalar(act.abs().max())), ("minmax", bound)):
            check_out("pool", case + " " + src, "fp32 -> P16", ops.bn_apply_pool2_p16(yd, st, b, relu=relu, fmt=1), r["out"])
        check_out("pool", case, "fp32 -> bf16", ops.bn_apply_pool2_p16(yd, st, None, relu=relu, fmt=2), r["out"])
        r16 = reference(shape, "relu" if relu else "plain", pool=True, y16=True)
        st16, _ = finalize(ops, r16["y"], d["gamma"], d["beta"])
        check_out("pool", case, "bf16 -> bf16", ops.bn_apply_pool2_p16(dev(r16["y"].bfloat16()), st16, None, relu=relu, fmt=2), r16["out"])
    # plain pooling (st = None): fp32; a P16 input written by the CPU encoder (the output keeps its scale); a bf16 input
    check_out("pool", name + " plain", "fp32 -> fp32", ops.bn_apply_pool2(yd, None), pool64(d["y"]))
    if C % 32 == 0:
        amax = float(d["y"].abs().max())
        yp = ops.P16(dev(ref.p16_encode(d["y"], amax)), scalar(amax))
        out = ops.bn_apply_pool2_p16(yp, None, yp.amax, fmt=1)
        assert float(out.amax) == amax
        check_out("pool", name + " plain", "P16 -> P16", out, pool64(ref.p16_decode(yp.data, amax)))
        y16 = d["y"].bfloat16()
        check_out("pool", name + " plain", "bf16 -> bf16", ops.bn_apply_pool2_p16(ops.P16(dev(y16), None, 2), None, None, fmt=2), pool64(y16.float()))


# --------------------------------------------------------------------------- d. bn_bwd / bn_bwd_p16
MODES = ((0, "plain"), (1, "relu"), (2, "res"), (3, "res"), (3, "resbn"))
BWD_CASES = [(1, 1, M, C) for (M, C) in ref.SHAPES + ref.SHAPES_F32 if C != 96] + POOL_CASES


@pytest.mark.parametrize("B,H,W,C", BWD_CASES)
def test_bn_bwd(ops, B, H, W, C):
    """mask modes 0, 1, 2 (the forward's fp32 output) and 3 (the forward's bit words), plain and pooled, with and without dres;
    fp32, P16 (fmt 1), bf16 (fmt 2) dy, bf16 g, bf16 y"""
    shape = (B, H, W, C)
    d = ref.inputs(*shape)
    flavours = [("fp32", {})] + ([("P16", {}), ("bf16", {}), ("bf16 g", dict(g16=True)), ("bf16 y", dict(y16=True))] if C % 32 == 0 else [])
    fwd = {}  # (y16, variant) -> (BNState, forward output, bit words)
    for pooled in ((False, True) if H > 1 else (False,)):
        for mode, variant in MODES:
            for flavour, flags in flavours:
                r = reference(shape, variant, pool=pooled, **flags)
                y16 = bool(flags.get("y16"))
                key = (y16, variant)
                if key not in fwd:
                    st, _ = finalize(ops, r["y"], d["gamma"], d["beta"])
                    st2, _ = finalize(ops, r["res"], d["gamma2"], d["beta2"])
                    res, res_st = _res_args(ops, d, variant, r, st2)
                    o, bits = ops.bn_apply(dev(r["y"]), st, relu=variant != "plain", res=res, res_st=res_st, want_mask=True)
                    fwd[key] = (st, o, bits)
                st, o, bits = fwd[key]
                act = o if mode == 2 else bits if mode == 3 else None
                yd = dev(r["y"].bfloat16()) if y16 else dev(r["y"])
                gd = dev(r["g"].bfloat16()) if flags.get("g16") else dev(r["g"])
                geff = float(r["g"].abs().max()) * (0.25 if pooled else 1.0)
                dy_term = TOL_DY * float(r["st"]["scale"].abs().max()) * geff
                for want_dres in ((False, True) if flavour in ("fp32", "P16") else (mode >= 2,)):
                    case = "%dx%dx%dx%d m%d %s%s%s" % (B, H, W, C, mode, variant, " pooled" if pooled else "", " dres" if want_dres else "")
                    if flavour == "fp32":
                        slot = ops.amax_slot(yd.device)
                        dy, dg, db, dres = ops.bn_bwd(gd, yd, st, None, mode, act=act, pooled=pooled, want_dres=want_dres, amax=slot)
                        check_amax_exact(slot, dy)
                    else:
                        dy, dg, db, dres = ops.bn_bwd_p16(gd, yd, st, mode, act=act, pooled=pooled, want_dres=want_dres, fmt=1 if flavour == "P16" else 2)
                        assert dy.fmt == (1 if flavour == "P16" else 2)
                    check_out("bwd", case, flavour + " dy", dy, r["dy"], dy_term)
                    check_vec("bwd", case, flavour + " dgamma", dg, r["dgamma"], TOL_SUM, r["l1_dgamma"], r["rows"])
                    check_vec("bwd", case, flavour + " dbeta", db, r["dbeta"], TOL_SUM, r["l1_dbeta"], r["rows"])
                    assert (dres is not None) == want_dres
                    if want_dres:
                        assert dres.dtype == gd.dtype
                        check_out("bwd", case, flavour + " dres", dres, r["dz"], TOL_F32 * geff)
                    if flavour == "P16":
                        check_bound("bwd", case, "P16 dy", dy.amax, float(r["dy"].abs().max()), upper=None)


# --------------------------------------------------------------------------- e. bn_bwd_dual_p16
@pytest.mark.parametrize("M,C", ref.DUAL)
def test_bn_bwd_dual(ops, M, C):
    """relu(bn1(y1) + bn2(y2)): the fp64 gradient with respect to y1, y2 and both affine pairs; the bits come from the forward"""
    shape = (1, 1, M, C)
    d = ref.inputs(*shape)
    r = reference(shape, "resbn")
    y1, y2, gd = dev(r["y"]), dev(r["res"]), dev(r["g"])
    st1, _ = finalize(ops, r["y"], d["gamma"], d["beta"])
    st2, _ = finalize(ops, r["res"], d["gamma2"], d["beta2"])
    out, bits = ops.bn_apply(y1, st1, relu=True, res=y2, res_st=st2, want_mask=True)
    case = "%dx%d" % (M, C)
    check_out("dual", case, "forward", out, r["out"])
    check_bits("dual", case, bits, r)
    assert ops.bn_bwd_dual_ok(gd, y1, y2)
    dy1, dg1, db1, dy2, dg2, db2 = ops.bn_bwd_dual_p16(gd, bits, y1, st1, y2, st2)
    gmax = float(r["g"].abs().max())
    check_out("dual", case, "dy1", dy1, r["dy"], TOL_DY * float(r["st"]["scale"].abs().max()) * gmax)
    check_out("dual", case, "dy2", dy2, r["dres"], TOL_DY * float(r["st2"]["scale"].abs().max()) * gmax)
    for what, got, want in (("dgamma1", dg1, r["dgamma"]), ("dbeta1", db1, r["dbeta"]), ("dgamma2", dg2, r["dgamma2"]), ("dbeta2", db2, r["dbeta2"])):
        check_vec("dual", case, what, got, want, TOL_SUM)
    check_bound("dual", case, "P16 dy1", dy1.amax, float(r["dy"].abs().max()), upper=None)
    check_bound("dual", case, "P16 dy2", dy2.amax, float(r["dres"].abs().max()), upper=None)


# --------------------------------------------------------------------------- f. avgpool2_bwd
@pytest.mark.parametrize("B,H,W,C", POOL_CASES)
def test_avgpool2_bwd(ops, guard, B, H, W, C):
    d = ref.inputs(B, H, W, C)
    name = "%dx%dx%dx%d" % (B, H, W, C)
    for bf16 in (False, True):
        g, base = (bf(d["gp"]), bf(d["y"])) if bf16 else (d["gp"], d["y"])
        xr = base.double().permute(0, 3, 1, 2).clone().requires_grad_(True)
        F.avg_pool2d(xr, 2).backward(g.double().permute(0, 3, 1, 2))
        up = xr.grad.permute(0, 2, 3, 1)
        cast = (lambda t: t.bfloat16()) if bf16 else (lambda t: t)  # noqa: E731
        kind = "bf16" if bf16 else "fp32"
        dx = ops.avgpool2_bwd(dev(cast(g)))
        assert dx.dtype == (torch.bfloat16 if bf16 else torch.float32)
        check_out("poolbwd", name, kind + " plain", dx, up)
        acc = ops.avgpool2_bwd(dev(cast(g)), dx=gdev(guard, cast(base)), accumulate=True)
        check_out("poolbwd", name, kind + " accumulate", acc, up + base.double())


# --------------------------------------------------------------------------- g. P16.unpack
@pytest.mark.parametrize("M,C", [(37, 32), (67, 96)])
def test_p16_unpack_is_the_cpu_decoder(ops, M, C):
    shape = (1, 1, M, C)
    d = ref.inputs(*shape)
    st, bound = finalize(ops, d["y"], d["gamma"], d["beta"], relu=True)
    for relu, b in ((True, bound), (False, scalar(float(reference(shape, "plain")["out"].abs().max())))):
        out = ops.bn_apply_p16(dev(d["y"]), st, b, relu=relu, fmt=1)
        got, want = out.unpack().cpu(), ref.p16_decode(out.data, float(out.amax))
        assert got.dtype == torch.float32 and float(got.abs().max()) > 0
        differ = report("unpack", "%dx%d relu=%d" % (M, C, relu), "elements that differ", float((got.view(torch.int32) != want.view(torch.int32)).sum()))
        assert differ == 0


# --------------------------------------------------------------------------- refusals
def test_refused_arguments_come_back_as_errors(ops):
    """what the entry points refuse on the host: the library's error through the binding's RuntimeError, message included, and a
    library that still works afterwards"""

    def refused(message, fn, *args, **kw):
        with pytest.raises(RuntimeError, match=re.escape(message)):
            fn(*args, **kw)

    def state(C):
        st = ops.BNState(C, y32)
        for t in (st.mean, st.invstd, st.scale, st.shift):
            t.fill_(1.0)
        return st

    y32 = dev(R("refy", 2, 4, 6, 32))
    st32, one = state(32), scalar(1.0)
    # bn_bwd with C = 96: C/4 = 24 neither divides 256 nor is a multiple of it
    y96 = dev(R("refy96", 1, 1, 67, 96))
    st96 = state(96)
    refused("bn_bwd: C/4 must divide 256 or be a multiple of 256 (C=96)", ops.bn_bwd, y96, y96, st96, None, 1)
    refused("bn_bwd: C/4 must divide 256 or be a multiple of 256 (C=96)", ops.bn_bwd_p16, y96, y96, st96, 1)
    refused("bn_bwd_dual: C/4 must divide 256 or be a multiple of 256 (C=96)", ops.bn_bwd_dual_p16, y96, torch.zeros(112, dtype=torch.int64, device="cuda"), y96, st96, y96, st96)
    # pooled forms with an odd H or W
    for shp in ((2, 3, 6, 32), (2, 4, 5, 32)):
        yo = dev(R("refodd", *shp))
        go = dev(R("refoddg", shp[0], shp[1] // 2, shp[2] // 2, 32))
        refused("trid_bn_apply_pool2_f32: bad arguments", ops.bn_apply_pool2, yo, st32)
        refused("trid_bn_apply_pool2_p16_f32: bad arguments", ops.bn_apply_pool2_p16, yo, st32, one, fmt=1)
        refused("trid_bn_apply_pool2_p16_f32: bad arguments", ops.bn_apply_pool2_p16, yo, st32, None, fmt=2)
        refused("bn_bwd: pooled needs even H,W", ops.bn_bwd, go, yo, st32, None, 1, pooled=True)
        refused("bn_bwd: pooled needs even H,W", ops.bn_bwd_p16, go, yo, st32, 1, pooled=True)
        refused("trid_avgpool2_bwd_f32: bad arguments", ops.call, "trid_avgpool2_bwd_f32", go.data_ptr(), yo.data_ptr(), shp[0], shp[1], shp[2], 32, 0, 0, ops.stream())
    # P16 forms with C % 32 != 0
    y8 = dev(R("refy8", 2, 4, 6, 8))
    st8 = state(8)
    for fmt in (1, 2):
        refused("trid_bn_apply_p16_f32: bad arguments (fmt 1 / 2, C%32)", ops.bn_apply_p16, y8, st8, one, fmt=fmt)
        refused("trid_bn_apply_pool2_p16_f32: bad arguments (fmt 1 / 2, C%32)", ops.bn_apply_pool2_p16, y8, st8, one, fmt=fmt)
        refused("trid_bn_bwd_apply_p16_f32: null pointer, fmt not 1 / 2 or C % 32 != 0", ops.bn_bwd_p16, y8, y8, st8, 1, fmt=fmt)
    y16c = dev(R("refy16", 1, 1, 40, 16))
    st16 = state(16)
    refused("bn_bwd_dual: bad shape (C % 32)", ops.bn_bwd_dual_p16, y16c, torch.zeros(12, dtype=torch.int64, device="cuda"), y16c, st16, y16c, st16)
    # a P16 residual is an identity residual
    resp = ops.p16_pack(y32)
    refused("a P16 residual is an identity residual", ops.bn_apply_p16, y32, st32, one, res=resp, res_st=st32, bound_res=resp.amax)
    # the library is still healthy
    torch.cuda.synchronize()
    d = ref.inputs(1, 1, 37, 32)
    st, _ = finalize(ops, d["y"], d["gamma"], d["beta"])
    check_out("refusals", "37x32 afterwards", "bn_apply", ops.bn_apply(dev(d["y"]), st, relu=True), reference((1, 1, 37, 32), "relu")["out"])
