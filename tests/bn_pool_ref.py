"""Plain CPU references for the BatchNorm / pool kernels of csrc/bn_pool.hip (tests/test_bn_pool_cpu.py checks these helpers,
tests/test_bn_pool_gpu.py compares the kernels with them).  No GPU and no call into the library.

  * bn_reference: BatchNorm with batch statistics (biased variance, eps 1e-5), optional residual (identity or a second BatchNorm
    of a second tensor), ReLU and 2x2 average pool in fp64; the gradients are autograd's, in double.
  * partials / merge_partials: the raw (mean, M2[, min, max]) statistics partials of row blocks, and their exact merge.
  * p16_encode / p16_decode: the P16 storage format, written from the layout comment of csrc/split_common.h - per row and
    32-channel group 128 bytes [hi x 32 | lo x 32] fp16 of x * scale, scale = 2^(13 - floor(log2 amax)) capped at 2^127
    (1 for a zero, denormal or non-finite amax), value = (hi + lo) / scale.
  * pack_bits / unpack_bits: the ReLU-bit words - quad i (four adjacent channels) -> words (i / 64) * 4 + c, bit i % 64.
  * fp32_emulation: what a plain left-to-right fp32 evaluation of the same sums loses against fp64 - the yardstick the GPU
    tolerances for sums and dy are derived from (4x its worst value over the shapes of the GPU test, see TOL_* below).
"""

import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

import oracle.fill as OF

EPS, MOMENTUM = 1e-5, 0.1

# ------------------------------------------------------------------------------------------------ tolerances
# fp32 outputs, element-wise, of the reference's largest magnitude: an fp32 evaluation of scale * y + shift against fp64 stays
# <= 1.7e-7 at the shapes of the GPU test (fp32_emulation's "out")
TOL_F32 = 1e-6
# sums and statistics, of each vector's largest entry; dy, of max_c |scale_c| * max |g| (the size of the terms that cancel).
# 4x the worst error of fp32_emulation over emulation_cases() (test_bn_pool_cpu.py recomputes it: stat 8.95e-7 at 515 x 1024,
# sum 1.22e-6 at 1029 x 64, dy 1.00e-7 at 300 x 8; out 1.43e-7), rounded up to two digits; the ceiling is the suite's former 2e-5.
TOL_STAT = 3.6e-6
TOL_SUM = 4.9e-6
TOL_DY = 4.1e-7
P16_REL = 2.0 ** -22  # of the tensor's own amax scalar: 11 + 11 significand bits below 2^14, a factor 2 for amax's place in its binade
BF16_REL = 2.0 ** -8  # of |ref|: one round-to-nearest-even of an fp32-class result
RELU_BAND = 1e-5  # |z| < RELU_BAND * max|z|: the ReLU decision of an fp32 evaluation is not determined; left out of bit and gradient checks
BAND_SHARE = 1e-3  # ... and at most this share of a tensor may lie there

# (M, C) of the GPU test (flat forms) and (B, H, W) of its pooled forms
SHAPES = [(2, 32), (37, 32), (67, 96), (1029, 64), (515, 1024), (130, 2048)]
SHAPES_F32 = [(300, 8), (193, 4)]
POOLED = [(1, 2, 2), (3, 6, 10), (2, 4, 2)]
DUAL = [(37, 32), (1029, 256), (130, 2048)]


def emulation_cases():
    """(B, H, W, C) of every input set the GPU test runs a backward pass on"""
    flat = sorted(set(SHAPES + SHAPES_F32 + DUAL))
    return [(1, 1, M, C) for (M, C) in flat] + [(B, H, W, C) for (B, H, W) in POOLED for C in (8, 32, 64)]


@functools.lru_cache(maxsize=None)
def inputs(B, H, W, C):
    """the seeded tensors of a case (never written to): conv outputs y, res [B, H, W, C] with non-zero channel means (the
    residual terms about 0.4 of the main one, as behind a block's bn3), the incoming gradients g (full size) and gp (pooled
    size; even H, W), two affine pairs, running buffers.
    A channel whose batch variance comes out below a quarter of the nominal one (it happens at 2 to 16 rows only) has its
    deviations stretched to that: two rows that nearly coincide give invstd up to 316 and |scale * y|, |shift| >> |z|, and ANY
    fp32 evaluation of scale * y + shift then loses 6e-8 |shift| - the 1e-6 bound on fp32 outputs presumes inputs on which a
    plain fp32 evaluation stays at 1.7e-7 (fp32_emulation's "out")."""
    tag = "bnp%d.%d.%d.%d" % (B, H, W, C)
    R = lambda name, *shape, scale=1.0: OF.randn(tag + name, shape, 0, scale)  # noqa: E731

    def spread(t, sigma):
        t2 = t.double().reshape(-1, C)
        m, v = t2.mean(0), t2.var(0, unbiased=False)
        k = torch.clamp(torch.sqrt(0.25 * sigma * sigma / v), min=1.0)
        return (m + (t2 - m) * k).float().reshape(t.shape)

    d = dict(y=spread(R("y", B, H, W, C) * 1.5 + R("ym", C, scale=0.7), 1.5), res=spread(R("r", B, H, W, C) * 0.4 + R("rm", C, scale=0.2), 0.4),
             g=R("g", B, H, W, C),
             gamma=R("ga", C).abs() + 0.5, beta=R("be", C, scale=0.3), gamma2=0.4 * (R("ga2", C).abs() + 0.5), beta2=R("be2", C, scale=0.1),
             rmean=R("rme", C, scale=0.2), rvar=R("rva", C).abs() + 0.5)
    if H % 2 == 0 and W % 2 == 0:
        d["gp"] = R("gp", B, H // 2, W // 2, C)
    return d


def _nchw(t):
    return t.double().permute(0, 3, 1, 2)


def _nhwc(t):
    return t.detach().permute(0, 2, 3, 1).contiguous()


# ------------------------------------------------------------------------------------------------ fp64 BatchNorm
def bn_stats(y, gamma, beta):
    """y [..., C] -> mean, var (biased), invstd, scale, shift in fp64"""
    C = y.shape[-1]
    y2 = y.double().reshape(-1, C)
    mean, var = y2.mean(0), y2.var(0, unbiased=False)
    invstd = 1.0 / torch.sqrt(var + EPS)
    scale = gamma.double() * invstd
    return dict(mean=mean, var=var, invstd=invstd, scale=scale, shift=beta.double() - mean * scale)


def running_update(y, running_mean, running_var):
    """the running buffers after one training step of F.batch_norm in double (momentum 0.1, unbiased variance)"""
    C = y.shape[-1]
    rm, rv = running_mean.double().clone(), running_var.double().clone()
    F.batch_norm(y.double().reshape(-1, C), rm, rv, None, None, True, MOMENTUM, EPS)
    return rm, rv


def bn_reference(y, gamma, beta, relu, res=None, res_gamma=None, res_beta=None, pool=False, g=None):
    """out = pool?(relu?(bn(y) [+ res | + bn2(res)])) for y, res [B, H, W, C]; with g (the gradient of out) also dy, dgamma,
    dbeta, dz (the gradient of the pre-activation z: what the kernels return as `dres`) and - with a residual - dres (the
    gradient of `res`) and dgamma2 / dbeta2."""
    leaf = lambda t: t.double().clone().requires_grad_(True)  # noqa: E731
    yr, ga, be = leaf(_nchw(y)), leaf(gamma), leaf(beta)
    z = F.batch_norm(yr, None, None, ga, be, True, MOMENTUM, EPS)
    if res is not None:
        rr = leaf(_nchw(res))
        if res_gamma is not None:
            ga2, be2 = leaf(res_gamma), leaf(res_beta)
            z = z + F.batch_norm(rr, None, None, ga2, be2, True, MOMENTUM, EPS)
        else:
            z = z + rr
    z.retain_grad()
    a = F.relu(z) if relu else z
    out = F.avg_pool2d(a, 2) if pool else a
    r = dict(z=_nhwc(z), out=_nhwc(out))
    if g is not None:
        out.backward(_nchw(g))
        r.update(dy=_nhwc(yr.grad), dgamma=ga.grad, dbeta=be.grad, dz=_nhwc(z.grad))
        if res is not None:
            r["dres"] = _nhwc(rr.grad)
            if res_gamma is not None:
                r.update(dgamma2=ga2.grad, dbeta2=be2.grad)
    return r


def relu_band(z):
    """bool mask of the elements whose ReLU decision an fp32 evaluation may take either way, and their share"""
    band = z.abs() < RELU_BAND * float(z.abs().max())
    return band, float(band.double().mean())


# ------------------------------------------------------------------------------------------------ statistics partials
def partials(y, rows_per_part, minmax):
    """rows of y [M, C] in blocks of rows_per_part (the last one short) -> fp32 [parts][C][2] (mean, M2) or [parts][C][4]
    (mean, M2, min, max), each computed in fp64"""
    C = y.shape[-1]
    out = []
    for q in y.double().reshape(-1, C).split(rows_per_part):
        m = q.mean(0)
        cols = [m, ((q - m) ** 2).sum(0)]
        if minmax:
            cols += [q.min(0).values, q.max(0).values]
        out.append(torch.stack(cols, dim=-1))
    return torch.stack(out).float().contiguous()


def merge_partials(p, rows_per_part, M):
    """exact (fp64) statistics of the rows behind the partials p: mean, biased variance, M2 and (4 columns) min, max"""
    p = p.double()
    parts = p.shape[0]
    n = torch.full((parts, 1), float(rows_per_part), dtype=torch.float64)
    n[-1] = M - (parts - 1) * rows_per_part
    mean = (n * p[:, :, 0]).sum(0) / M
    m2 = p[:, :, 1].sum(0) + (n * (p[:, :, 0] - mean) ** 2).sum(0)
    r = dict(mean=mean, var=m2 / M, m2=m2)
    if p.shape[-1] == 4:
        r.update(lo=p[:, :, 2].min(0).values, hi=p[:, :, 3].max(0).values)
    return r


# ------------------------------------------------------------------------------------------------ P16
def p16_scale(amax):
    amax = float(amax)
    if not math.isfinite(amax) or amax < 2.0 ** -126:
        return np.float32(1.0)
    _, ex = math.frexp(amax)  # amax = m * 2^ex, 0.5 <= m < 1: floor(log2 amax) = ex - 1
    return np.float32(2.0 ** min(13 - (ex - 1), 127))


def p16_encode(x, amax):
    """fp32 [..., C] (C % 32 == 0) -> the P16 tensor (an fp32 container of the same shape) scaled for amax"""
    x = x.detach().float().contiguous()
    C = x.shape[-1]
    assert C % 32 == 0
    with np.errstate(over="ignore", invalid="ignore"):
        xs = x.numpy().reshape(-1, C // 32, 32) * p16_scale(amax)
        hi = xs.astype(np.float16)
        lo = (xs - hi.astype(np.float32)).astype(np.float16)
    packed = np.ascontiguousarray(np.stack([hi, lo], axis=2))  # [rows][groups][hi | lo][32]
    return torch.from_numpy(packed.reshape(-1).view(np.float32).reshape(tuple(x.shape)).copy())


def p16_decode(data, amax, lo_plane=True):
    """the fp32 values of a P16 tensor; lo_plane=False drops the low parts (what a kernel that lost them would store)"""
    data = data.detach().cpu().contiguous()
    C = data.shape[-1]
    assert data.dtype == torch.float32 and C % 32 == 0
    h = data.numpy().view(np.float16).reshape(-1, C // 32, 2, 32)
    v = h[:, :, 0].astype(np.float32)
    if lo_plane:
        v = v + h[:, :, 1].astype(np.float32)
    v = v * (np.float32(1.0) / p16_scale(amax))
    return torch.from_numpy(np.ascontiguousarray(v).reshape(tuple(data.shape)))


def p16_excess(got, ref, amax, f32_term=0.0):
    """largest |got - ref| over the P16 bound f32_term + 2^-22 * amax (<= 1: within the bound); an all-zero tensor: 0 if exact"""
    err = float((got.double() - ref.double()).abs().max())
    allowed = f32_term + P16_REL * float(amax)
    return err / allowed if allowed > 0 else (0.0 if err == 0 else float("inf"))


def bf16_excess(got, ref, f32_term):
    """largest |got - ref| / (2^-8 |ref| + f32_term), element-wise"""
    got, ref = got.double(), ref.double()
    return float(((got - ref).abs() / (BF16_REL * ref.abs() + f32_term + 1e-300)).max())


# ------------------------------------------------------------------------------------------------ ReLU-bit words
def pack_bits(keep):
    """bool [M, C] -> int64 words: quad i = elements 4i .. 4i + 3 (row-major), component c -> word (i / 64) * 4 + c, bit i % 64;
    the padding bits of a partial last group are 0"""
    flat = keep.reshape(-1).numpy().astype(np.uint64)
    assert flat.size % 4 == 0
    flat = np.concatenate([flat, np.zeros((-flat.size) % 256, dtype=np.uint64)])
    b = flat.reshape(-1, 64, 4)  # [group][bit][component]
    words = np.bitwise_or.reduce(b << np.arange(64, dtype=np.uint64)[None, :, None], axis=1)
    return torch.from_numpy(np.ascontiguousarray(words).reshape(-1).view(np.int64).copy())


def unpack_bits(words, M, C):
    """the first M * C bits of the words pack_bits lays out, as bool [M, C]"""
    w = words.detach().cpu().contiguous().numpy().view(np.uint64).reshape(-1, 1, 4)
    bits = (w >> np.arange(64, dtype=np.uint64)[None, :, None]) & np.uint64(1)  # [group][bit][component]
    return torch.from_numpy(bits.reshape(-1)[: M * C].astype(np.bool_).reshape(M, C))


# ------------------------------------------------------------------------------------------------ fp32 yardstick
def _seq_sum(a):
    """left-to-right fp32 sum over the rows"""
    return np.add.accumulate(a.astype(np.float32), axis=0, dtype=np.float32)[-1]


def fp32_emulation(y, gamma, beta, g, relu):
    """BatchNorm forward and backward of y, g [M, C] evaluated in fp32 with left-to-right sums (the ReLU mask taken from the
    fp64 pre-activation, so no decision can differ) against fp64: dict of errors - out (of max|z|), stat (mean, invstd), sum
    (dgamma, dbeta: of each vector's largest entry), dy (of max|scale| * max|g|)."""
    M, C = y.shape
    st = bn_stats(y, gamma, beta)
    yd, gd = y.double(), g.double()
    zd = yd * st["scale"] + st["shift"]
    keep = (zd > 0) if relu else torch.ones_like(zd, dtype=torch.bool)
    gmd = gd * keep
    xhd = (yd - st["mean"]) * st["invstd"]
    dbd, dgd = gmd.sum(0), (gmd * xhd).sum(0)
    dyd = st["scale"] * (gmd - dbd / M - xhd * dgd / M)

    f = np.float32
    yn, gn, km = y.numpy().astype(f), g.numpy().astype(f), keep.numpy()
    mean32 = _seq_sum(yn) / f(M)
    invstd32 = f(1.0) / np.sqrt(_seq_sum((yn - mean32) ** 2) / f(M) + f(EPS))
    # the passes behind the statistics read the coefficients bn_finalize rounded from its fp64 merge
    mean, invstd = st["mean"].numpy().astype(f), st["invstd"].numpy().astype(f)
    scale = gamma.numpy().astype(f) * invstd
    shift = beta.numpy().astype(f) - mean * scale
    z = yn * scale + shift
    gm = np.where(km, gn, f(0))
    xh = (yn - mean) * invstd
    db, dg = _seq_sum(gm), _seq_sum(gm * xh)
    inv = f(1.0) / f(M)
    dy = scale * (gm - db * inv - xh * dg * inv)

    def e(a, b, top=None):
        b = b.numpy()
        return float(np.abs(a.astype(np.float64) - b).max() / (top if top is not None else np.abs(b).max()))

    return dict(out=e(z, zd), stat=max(e(mean32, st["mean"]), e(invstd32, st["invstd"])), sum=max(e(db, dbd), e(dg, dgd)),
                dy=e(dy, dyd, float(st["scale"].abs().max()) * float(gd.abs().max())))
