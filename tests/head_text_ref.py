"""Plain CPU references for the kernels of csrc/head_loss.hip and csrc/attn_text.hip (tests/test_head_text_cpu.py checks these
helpers, tests/test_head_text_gpu.py compares the kernels with them).  No GPU and no call into the library.

  * Every numerical operation is ONE function of (inputs, dtype), written from the formulas in the kernel comments and in
    oracle/losses.py, with autograd for every gradient.  In torch.float64 it is the reference; the very same function in
    torch.float32 is the yardstick: what a plain fp32 evaluation of the formula loses against fp64.
  * Every function returns (outputs, spec): spec[key] = (mode, scale) says how an output is measured (`measure`):
      "max"   largest |error| over max(largest |reference|, scale)
      "rows"  the same per row (first axis), scale per row; the worst row counts
    `scale` is the size of the terms that enter where the result itself may cancel (the L1 sum of a dot product's terms, the
    largest logit behind lse - logit, ...), so that the figure says how well the formula was evaluated and not how lucky the
    cancellation was.  A reference NaN (the mean of nothing) must be a NaN; a reference that is all zero with no scale must be
    met exactly.
  * runs_<group>() lists the cases of a tolerance group - the inputs (seeded through oracle.fill, never written to), the
    function, and what the GPU test needs to lay the buffers out.  YARDSTICK[group] is the worst fp32-vs-fp64 figure over those
    runs, TOL[group] = 4 x that (recorded inside [4, 4.2] x): the factor covers another summation order and the device's expf /
    logf.  test_head_text_cpu.py recomputes every yardstick and asserts the constants recorded here.
  * Exact restatements where the result is a copy, a decision or a fixed-order fp32 sum: gather with id clamping, the hit mask
    on full int64 ids, argmax with lowest-index ties, relu_bwd, zero padding, and the embedding gradient as a sequential numpy
    float32 sum in position order.
"""

import collections
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

import oracle.fill as OF

F64, F32 = torch.float64, torch.float32
INF = float("inf")
INV_T = float(np.float32(1.0 / 0.07))  # the scalar the kernels are handed
INFONCE_SEG = 4096  # columns per workgroup of the InfoNCE kernels
GEMM_VALUE, GEMM_GRAD = 1e-5, 1e-4  # the project's bounds where a case goes through the split-bf16 GEMMs (test_model_gpu.py::test_losses)

# ------------------------------------------------------------------------------------------------ yardsticks and bounds
# worst error of the fp32 evaluation against fp64 over runs_<group>() (test_head_text_cpu.py::test_yardsticks recomputes them)
YARDSTICK = dict(
    softmax=1.127e-7,   # softmax rows and their backward
    infonce=5.487e-7,   # InfoNCE rows, both forms, unit-norm range: |logit| <= 1 / 0.07 = 14 in front of the exp
    infonce5=2.767e-6,  # ... |S| <= 5: |logit| <= 71
    ce=1.073e-7,        # label-smoothed cross entropy rows, logit scale 1
    ce28=1.974e-5,      # ... logit scale 28: lse ~ 130, one rounding of it is 7.6e-6 in the exponent
    cmpm=3.864e-6,      # CMPM rows: (log p - log(q + eps)) reaches 40 beside a probability near 1
    align=2.009e-7,     # global-align rows
    norm=4.027e-7,      # l2norm, colnorm, cross projection and their backwards
    sum=8.050e-8,       # sum, colsum, rowdot, pair means: of the L1 sum of the terms
    elem=1.495e-7,      # axpby3, rowscale_add: of the sum of the terms' magnitudes, per element
    tokens=1.922e-7,    # attention-pool token tensor and its backward
)
# 4 x the yardstick, rounded into [4, 4.2] x so that the last digits of another CPU's fp32 sums do not matter
TOL = dict(softmax=4.62e-7, infonce=2.25e-6, infonce5=1.13e-5, ce=4.40e-7, ce28=8.09e-5, cmpm=1.58e-5, align=8.24e-7, norm=1.65e-6, sum=3.30e-7,
           elem=6.13e-7, tokens=7.88e-7)
TOL_SOFTMAX, TOL_INFONCE, TOL_INFONCE5, TOL_CE, TOL_CE28, TOL_CMPM = TOL["softmax"], TOL["infonce"], TOL["infonce5"], TOL["ce"], TOL["ce28"], TOL["cmpm"]
TOL_ALIGN, TOL_NORM, TOL_SUM, TOL_ELEM, TOL_TOKENS = TOL["align"], TOL["norm"], TOL["sum"], TOL["elem"], TOL["tokens"]


def R(name, *shape, scale=1.0):
    return OF.randn("ht:" + name, shape, 0, scale)


def RI(name, lo, hi, *shape):
    return OF.randint("ht:" + name, lo, hi, shape, 0)


Run = collections.namedtuple("Run", "name fn kw meta")


def ref_of(run, dtype=F64):
    return run.fn(dtype=dtype, **run.kw)


# ------------------------------------------------------------------------------------------------ measuring
def measure(got, ref, mode="max", scale=None):
    got, ref = torch.as_tensor(got).detach().double().cpu(), torch.as_tensor(ref).detach().double().cpu()
    assert got.shape == ref.shape, (tuple(got.shape), tuple(ref.shape))
    nan = torch.isnan(ref)
    if not torch.equal(torch.isnan(got), nan):
        return INF
    zero = torch.zeros((), dtype=F64)
    err, mag = torch.where(nan, zero, (got - ref).abs()), torch.where(nan, zero, ref.abs())
    if err.numel() == 0:
        return 0.0
    if mode == "max":
        top, e = max(float(mag.max()), float(scale or 0.0)), float(err.max())
        return e / top if top > 0 else (0.0 if e == 0 else INF)
    assert mode == "rows"
    rows = ref.shape[0]
    err, top = err.reshape(rows, -1).max(1).values, mag.reshape(rows, -1).max(1).values
    if scale is not None:
        top = torch.maximum(top, torch.nan_to_num(torch.as_tensor(scale).double().reshape(rows), nan=0.0))
    if bool(((top == 0) & (err > 0)).any()):
        return INF
    return float((err / top.clamp(min=1e-300)).max())


def compare(got, want, spec):
    """worst figure of a dict of outputs against the reference outputs of the same keys"""
    return max(measure(got[k], want[k], *spec.get(k, ("max", None))) for k in want)


def yardstick(runs):
    worst = 0.0
    for run in runs:
        want, spec = ref_of(run, F64)
        got, _ = ref_of(run, F32)
        worst = max(worst, compare(got, want, spec))
    return worst


def _leaf(t, dtype):
    return t.detach().to(dtype).clone().requires_grad_(True)


def _c(t, dtype):
    return None if t is None else t.detach().to(dtype)


def same_ids(ids):
    return ids.view(-1, 1) == ids.view(1, -1)


def id_patterns(B):
    """all equal, all distinct (beyond 32 bits), duplicates in groups of up to four"""
    return dict(equal=torch.full((B,), 7, dtype=torch.int64), distinct=torch.arange(B, dtype=torch.int64) * 3 + (1 << 33) - 5,
                dup=(torch.arange(B, dtype=torch.int64) // 4) * 7 - 3)


# ------------------------------------------------------------------------------------------------ InfoNCE
def infonce(S, hit, invT, gscale, dtype, pos=None, q=None, key=None, masked=True):
    """rows_b = CE([pos_b | S_b without the masked columns] * invT, label 0); dS, dpos (or dq0 = dL/dq through pos = <q, key>)
    of gscale * mean_b rows_b.  masked=False: the wrong form that leaves the masked columns in the log-sum-exp."""
    Sl = _leaf(S, dtype)
    if pos is not None:
        pl = _leaf(pos, dtype)
        p = pl
    else:
        pl = _leaf(q, dtype)
        p = (pl * _c(key, dtype)).sum(1)
    z = Sl * invT
    if masked:
        z = z.masked_fill(hit.bool()[None, :], -INF)
    z = torch.cat([(p * invT)[:, None], z], dim=1)
    rows = torch.logsumexp(z, dim=1) - z[:, 0]
    (gscale * rows.mean()).backward()
    dS = Sl.grad if masked else Sl.grad.masked_fill(hit.bool()[None, :], 0.0)
    gs = gscale * invT / S.shape[0]
    top = float(z.detach()[torch.isfinite(z.detach())].abs().max())  # rows = lse - logit: terms of the largest logit's size
    out = dict(rows=rows.detach(), dS=dS, dpos=pl.grad)
    return out, dict(rows=("max", top), dS=("max", gs), dpos=("max", gs * (1.0 if pos is not None else float(key.abs().max()))))


def infonce_segment_fold(S, hit, pos, invT, skip, dtype=F32):
    """loss rows through per-segment (max, sum) partials folded by a running maximum seeded with (-inf, 0).  skip=True leaves
    out a segment whose columns are all masked (m = -inf); skip=False folds it in as exp(-inf - m) * l, which with the running
    maximum still at -inf is exp(nan) * 0 = NaN."""
    z = (_c(S, dtype) * invT).masked_fill(hit.bool()[None, :], -INF)
    B, K = z.shape
    m, l = torch.full((B,), -INF, dtype=dtype), torch.zeros(B, dtype=dtype)
    for k0 in range(0, K, INFONCE_SEG):
        seg = z[:, k0 : k0 + INFONCE_SEG]
        ms = seg.max(1).values
        live = ms > -INF
        ls = torch.where(live, torch.exp(seg - torch.where(live, ms, torch.zeros_like(ms))[:, None]).sum(1), torch.zeros_like(ms))
        if skip and not bool(live.any()):
            continue
        mn = torch.maximum(m, ms)
        l = l * torch.exp(m - mn) + ls * torch.exp(ms - mn)
        m = mn
    p = _c(pos, dtype) * invT
    mn = torch.maximum(m, p)
    l = l * torch.exp(m - mn) + torch.exp(p - mn)
    return mn + torch.log(l) - p


INFONCE_CASES = [(1, 1, 1, 0), (3, 5, 8, 0), (2, 4096, 4096, 0), (2, 4097, 4100, 0), (3, 8197, 8197, 0), (2, 4100, 4100, 1)]  # (B, K, ldS, floats off alignment)
QUEUE_C = (1, 256, 260)


def infonce_masks(K):
    k = torch.arange(K)
    m = dict(none=k < 0, every7=k % 7 == 0, all=k >= 0)
    if K > INFONCE_SEG:  # (up to 4096 columns segment 0 is the whole row)
        m.update(seg0=k < INFONCE_SEG, seg1=(k >= INFONCE_SEG) & (k < 2 * INFONCE_SEG))
    return m


def runs_infonce(forms=("rows", "queue"), amps=(1.0, 5.0)):
    for B, K, ld, off in INFONCE_CASES:
        base = torch.tanh(R("nce.S%d.%d.%d" % (B, K, off), B, K))
        for mname, hit in infonce_masks(K).items():
            for amp in amps:  # unit-norm range; |S| <= 5, where exp(S / T) without the maximum subtracted overflows
                S = amp * base
                tag = "B%d K%d ld%d%s %s |S|<=%g" % (B, K, ld, "+1" if off else "", mname, amp)
                meta = dict(B=B, K=K, ld=ld, off=off)
                if "rows" in forms:
                    pos = amp * torch.tanh(R("nce.p%d.%d" % (B, K), B) * 0.5 + 0.5)
                    yield Run("rows " + tag, infonce, dict(S=S, hit=hit, invT=INV_T, gscale=2.0, pos=pos), meta)
                for C in QUEUE_C if "queue" in forms else ():
                    q = amp * torch.tanh(R("nce.q%d.%d.%d" % (B, K, C), B, C)) / math.sqrt(C)
                    key = torch.tanh(R("nce.k%d.%d.%d" % (B, K, C), B, C) * 0.5 + 0.5) / math.sqrt(C)
                    yield Run("queue C%d " % C + tag, infonce, dict(S=S, hit=hit, invT=INV_T, gscale=2.0, q=q, key=key), dict(meta, C=C))


# ------------------------------------------------------------------------------------------------ smooth CE
def smooth_ce(logits, labels, eps, gscale, dtype, uniform_term=True):
    """rows_i = -sum_j t_ij log softmax(z_i)_j, t = (1 - eps) onehot + eps / n; dlogits of gscale * sum_i rows_i.
    uniform_term=False: the wrong form without the eps / n term."""
    z = _leaf(logits, dtype)
    n = z.shape[1]
    lp = F.log_softmax(z, dim=1)
    rows = -(1.0 - eps) * lp.gather(1, labels.view(-1, 1))[:, 0]
    if uniform_term:
        rows = rows - (eps / n) * lp.sum(1)
    (gscale * rows.sum()).backward()
    return dict(rows=rows.detach(), dlogits=z.grad), dict(rows=("max", float(logits.abs().max())), dlogits=("max", gscale))


CE_CASES = [(1, 1, 16, 0.0), (3, 5, 16, 0.1), (4, 255, 256, 0.1), (2, 256, 256, 0.0), (3, 257, 272, 0.1), (2, 11003, 11008, 0.1)]  # (rows, n, ld, eps)


def runs_ce(scales=(1.0, 28.0)):
    for rows, n, ld, eps in CE_CASES:
        for scale in scales:
            labels = RI("ce.y%d.%d" % (rows, n), 0, n, rows)
            labels[0] = 0
            labels[-1] = n - 1
            logits = R("ce.z%d.%d" % (rows, n), rows, n) * scale
            yield Run("%dx%d ld%d eps%g scale%g" % (rows, n, ld, eps, scale), smooth_ce, dict(logits=logits, labels=labels, eps=eps, gscale=1.0 / rows),
                      dict(rows=rows, n=n, ld=ld))


# ------------------------------------------------------------------------------------------------ CMPM, pair means
def cmpm_rows(S, ids, eps, gs, dtype, count_per_row=True):
    """p = softmax(S_i), q_ij = [id_i == id_j] / sqrt(n_i), rows_i = sum_j p_ij (log p_ij - log(q_ij + eps)); dS of gs * sum_i
    rows_i.  count_per_row=False: the wrong form with n taken over the whole batch (every same-id pair of the matrix).
    Measured of max(., 1): log(q + eps) at q = 1 carries an absolute rounding error of 2^-24 however small the row's loss is
    (B = 1: the loss is -log(1 + 1e-8))."""
    z = _leaf(S, dtype)
    same = same_ids(ids)
    cnt = same.sum(1, keepdim=True) if count_per_row else same.sum()
    qq = same.to(dtype) / torch.sqrt(cnt.to(dtype))
    lp = F.log_softmax(z, dim=1)
    rows = (lp.exp() * (lp - torch.log(qq + eps))).sum(1)
    (gs * rows.sum()).backward()
    return dict(rows=rows.detach(), dS=z.grad), dict(rows=("max", 1.0), dS=("max", gs))


CMPM_CASES = [(1, 4), (3, 4), (63, 64), (64, 64), (65, 68), (256, 256), (257, 260), (300, 300)]  # (B, ldS)


def runs_cmpm():
    for B, ld in CMPM_CASES:
        S = R("cmpm.S%d" % B, B, B) * 5.0  # the left operand is not normalised: entries up to about 20
        for pname, ids in id_patterns(B).items():
            yield Run("B%d ld%d ids %s" % (B, ld, pname), cmpm_rows, dict(S=S, ids=ids, eps=1e-8, gs=1.0 / B), dict(B=B, ld=ld))


def pair_sim_means(S, ids, row_scale, dtype):
    """mean of row_scale_i * S_ij over the same-id pairs and over the others (NaN for an empty set, as torch.mean of nothing)"""
    s = _c(S, dtype)
    if row_scale is not None:
        s = s * _c(row_scale, dtype)[:, None]
    same = same_ids(ids)
    out = torch.stack([s[same].mean(), s[~same].mean()])
    return dict(means=out), dict(means=("rows", torch.stack([s[same].abs().mean(), s[~same].abs().mean()])))


PAIR_B = (1, 3, 130, 300)


def runs_pair_means():
    for B in PAIR_B:
        S = torch.tanh(R("pair.S%d" % B, B, B) * 0.5 + 0.3)
        for pname, ids in id_patterns(B).items():
            for scaled in (False, True):
                rs = R("pair.r%d" % B, B).abs() + 0.5 if scaled else None
                yield Run("pair means B%d ids %s%s" % (B, pname, " scaled" if scaled else ""), pair_sim_means, dict(S=S, ids=ids, row_scale=rs), dict(B=B, ld=B + (-B) % 4))


# ------------------------------------------------------------------------------------------------ global align
def global_align_rows(S, ids, gscale, dtype, alpha=0.6, beta=0.4, sp=10.0, sn=40.0):
    """rows_i = 2 / B * sum_j (same id: log(1 + exp(-sp (s - alpha))), else log(1 + exp(sn (s - beta)))); dS of gscale * sum rows"""
    z = _leaf(S, dtype)
    B = z.shape[0]
    l = torch.where(same_ids(ids), torch.log(1.0 + torch.exp(-sp * (z - alpha))), torch.log(1.0 + torch.exp(sn * (z - beta))))
    rows = l.sum(1) * 2.0 / B
    (gscale * rows.sum()).backward()
    return dict(rows=rows.detach(), dS=z.grad), {}


ALIGN_CASES = [(1, 4), (3, 4), (5, 8), (256, 256), (257, 260), (300, 300)]


def runs_align():
    for B, ld in ALIGN_CASES:
        S = torch.tanh(R("ga.S%d" % B, B, B))
        S.view(-1)[0] = 1.0  # exact +1 and -1 present
        S.view(-1)[-1] = -1.0
        if B > 1:
            S[0, 1], S[1, 0] = -1.0, 1.0
        for pname, ids in id_patterns(B).items():
            yield Run("B%d ld%d ids %s" % (B, ld, pname), global_align_rows, dict(S=S, ids=ids, gscale=0.5), dict(B=B, ld=ld))


# ------------------------------------------------------------------------------------------------ norm group
def _inv_norm(x, dim, eps):
    return 1.0 / torch.clamp(torch.linalg.vector_norm(x, dim=dim, keepdim=True), min=eps)


def l2norm(x, dtype, dy=None, eps=1e-12):
    """y = x / max(|x_row|, eps), inv = 1 / max(|x_row|, eps); dx for the upstream gradient dy"""
    xl = _leaf(x, dtype)
    inv = _inv_norm(xl, 1, eps)
    y = xl * inv
    out = dict(y=y.detach(), inv=inv.detach()[:, 0])
    if dy is not None:
        y.backward(_c(dy, dtype))
        out["dx"] = xl.grad
    # dx = (dy - y <dy, y>) inv vanishes analytically at C = 1: measured of the terms' size max|dy_row| inv_row
    return out, dict(y=("rows", None), inv=("rows", None), dx=("rows", None if dy is None else dy.double().abs().max(1).values * inv.detach().double()[:, 0]))


ROW_CASES = [(1, 1), (3, 5), (5, 64), (6, 65), (37, 256), (2, 1000)]  # (rows, C)


def row_inputs(rows, C):
    """rows scaled by 1e-3 and 1e3, one zero row (from three rows on)"""
    x = R("row.x%d.%d" % (rows, C), rows, C)
    if rows >= 3:
        x[0] *= 1e-3
        x[1] *= 1e3
        x[2] = 0.0
    return x


def runs_l2norm():
    for rows, C in ROW_CASES:
        yield Run("l2norm %dx%d" % (rows, C), l2norm, dict(x=row_inputs(rows, C), dy=R("row.dy%d.%d" % (rows, C), rows, C)), dict(rows=rows, C=C))


def colnorm(proj, dtype, dpnt=None):
    """pnt [N, C] = (proj / max(|proj column|, 1e-12))^T, inv [N]; dprojT [N, C] = (dL/dproj)^T for the upstream gradient dpnt"""
    pl = _leaf(proj, dtype)
    inv = _inv_norm(pl, 0, 1e-12)
    pnt = (pl * inv).t()
    out = dict(pnt=pnt.detach(), inv=inv.detach()[0])
    if dpnt is not None:
        pnt.backward(_c(dpnt, dtype))
        out["dprojT"] = pl.grad.t()
    return out, dict(pnt=("rows", None), inv=("rows", None), dprojT=("rows", None if dpnt is None else dpnt.double().abs().max(1).values * inv.detach().double()[0]))


def colnorm_rows_instead(proj, dtype=F64):
    """the wrong form: rows normalised instead of columns"""
    p = _c(proj, dtype)
    return (p * _inv_norm(p, 1, 1e-12)).t()


COLNORM_CASES = [(1, 1, 16), (5, 3, 16), (64, 64, 64), (65, 70, 80), (256, 130, 144)]  # (C, N, ldn)


def runs_colnorm():
    for C, N, ldn in COLNORM_CASES:
        proj = OF.fill("ht:cn%d.%d.projection" % (C, N), (C, N))
        yield Run("colnorm %dx%d ldn%d" % (C, N, ldn), colnorm, dict(proj=proj, dpnt=R("cn.d%d.%d" % (C, N), N, C)), dict(C=C, N=N, ldn=ldn))
        if N >= 3:
            pz = proj.clone()
            pz[:, 1] = 0.0  # one all-zero column: inv = 1e12, outputs 0 (forward only)
            yield Run("colnorm %dx%d ldn%d zero column" % (C, N, ldn), colnorm, dict(proj=pz), dict(C=C, N=N, ldn=ldn))


def cross_project(v, t, dtype, G=None):
    """X [2B, C] = [(v . t^) t^ ; (t . v^) v^], dots = [v . t^ ; t . v^], inv = [1 / max(|v|, 1e-12) ; 1 / max(|t|, 1e-12)];
    dv, dt for the upstream gradient G [2B, C]"""
    vl, tl = _leaf(v, dtype), _leaf(t, dtype)
    iv, it = _inv_norm(vl, 1, 1e-12), _inv_norm(tl, 1, 1e-12)
    d = (vl * tl).sum(1, keepdim=True)
    a, b = d * it, d * iv
    X = torch.cat([a * it * tl, b * iv * vl])
    out = dict(X=X.detach(), dots=torch.cat([a, b]).detach()[:, 0], inv=torch.cat([iv, it]).detach()[:, 0])
    if G is not None:
        X.backward(_c(G, dtype))
        out.update(dv=vl.grad, dt=tl.grad)
    return out, dict(inv=("rows", None))


CROSS_CASES = [(1, 1, 0), (3, 5, 0), (5, 4, 0), (4, 256, 0), (3, 260, 0), (2, 1000, 0), (2, 1024, 1)]  # (B, C, floats v is off alignment)


def runs_cross():
    for B, C, off in CROSS_CASES:
        v = R("cp.v%d.%d" % (B, C), B, C)
        t = R("cp.t%d.%d" % (B, C), B, C) + 0.5 * v  # correlated pairs, as trained embeddings are
        if B >= 3:
            v[1] = 0.0  # a zero row in v
        yield Run("cross %dx%d%s" % (B, C, " v+1" if off else ""), cross_project, dict(v=v, t=t, G=R("cp.g%d.%d" % (B, C), 2 * B, C)), dict(B=B, C=C, off=off))


def runs_norm():
    yield from runs_l2norm()
    yield from runs_colnorm()
    yield from runs_cross()


# ------------------------------------------------------------------------------------------------ sums
def sum_(x, scale, out0, dtype):
    s = _c(x, dtype).sum() * scale
    if out0 is not None:
        s = s + _c(out0, dtype)[0]
    return dict(out=s.reshape(1)), dict(out=("max", float(x.double().abs().sum()) * abs(scale) + (abs(float(out0[0])) if out0 is not None else 0.0)))


def colsum(x, out0, dtype):
    s = _c(x, dtype).sum(0)
    l1 = x.double().abs().sum(0)
    if out0 is not None:
        s, l1 = s + _c(out0, dtype), l1 + out0.double().abs()
    return dict(out=s), dict(out=("rows", l1))


def rowdot(x, y, dtype):
    return dict(out=(_c(x, dtype) * _c(y, dtype)).sum(1)), dict(out=("rows", (x.double() * y.double()).abs().sum(1)))


SUM_N = (1, 255, 257, 1000)
COLSUM_CASES = [(1, 1, 1), (3, 5, 7), (4, 64, 64), (5, 65, 80), (1029, 130, 130)]  # (M, N, ld)


def runs_sum():
    for n in SUM_N:
        x = R("sum.x%d" % n, n) + 0.25
        yield Run("sum n%d" % n, sum_, dict(x=x, scale=1.0, out0=None), dict(n=n))
        yield Run("sum n%d scale accumulate" % n, sum_, dict(x=x, scale=-0.37, out0=torch.tensor([1.5])), dict(n=n))
    for M, N, ld in COLSUM_CASES:
        x = R("cs.x%d.%d" % (M, N), M, N)
        yield Run("colsum %dx%d ld%d" % (M, N, ld), colsum, dict(x=x, out0=None), dict(M=M, N=N, ld=ld))
        yield Run("colsum %dx%d ld%d accumulate" % (M, N, ld), colsum, dict(x=x, out0=R("cs.o%d.%d" % (M, N), N)), dict(M=M, N=N, ld=ld))
    for rows, C in ROW_CASES:
        yield Run("rowdot %dx%d" % (rows, C), rowdot, dict(x=row_inputs(rows, C), y=R("row.y%d.%d" % (rows, C), rows, C)), dict(rows=rows, C=C))
    yield from runs_pair_means()


# ------------------------------------------------------------------------------------------------ element-wise
def rowscale_add(s, y, dx0, dtype):
    v = _c(s, dtype)[:, None] * _c(y, dtype)
    l1 = (s.double()[:, None] * y.double()).abs()
    if dx0 is not None:
        v, l1 = v + _c(dx0, dtype), l1 + dx0.double().abs()
    return dict(dx=v.reshape(-1)), dict(dx=("rows", l1.reshape(-1)))


def axpby3(a, b, c, g, dtype, third=True):
    """g0 a + g1 b + g2 c (b, c optional).  third=False: the wrong form that drops the third term."""
    v = _c(g, dtype)[0] * _c(a, dtype)
    l1 = (g[0].double() * a.double()).abs()
    if b is not None:
        v, l1 = v + _c(g, dtype)[1] * _c(b, dtype), l1 + (g[1].double() * b.double()).abs()
    if c is not None and third:
        v = v + _c(g, dtype)[2] * _c(c, dtype)
    if c is not None:
        l1 = l1 + (g[2].double() * c.double()).abs()
    return dict(out=v), dict(out=("rows", l1))


ELEM_N = (1, 1023, 1025, 2048 * 1024 + 3)  # (the last one is past the grid cap of 2048 workgroups x 1024 elements)
ROWSCALE_BIG = (1050, 1000)  # rows * C = 1 050 000 > 4096 workgroups x 256: a second grid-stride trip


def runs_elem():
    for rows, C in ROW_CASES + [ROWSCALE_BIG]:
        s, y = R("rs.s%d.%d" % (rows, C), rows), (row_inputs(rows, C) if rows * C < 10 ** 6 else R("rs.y", rows, C))
        yield Run("rowscale_add %dx%d" % (rows, C), rowscale_add, dict(s=s, y=y, dx0=None), dict(rows=rows, C=C))
        yield Run("rowscale_add %dx%d accumulate" % (rows, C), rowscale_add, dict(s=s, y=y, dx0=R("rs.d%d.%d" % (rows, C), rows, C)), dict(rows=rows, C=C))
    g = torch.tensor([0.75, -1.25, 3.0])
    for n in ELEM_N:
        a, b, c = (R("ax.%s%d" % (k, n), n) for k in "abc")
        for have in ("a", "ab", "ac", "abc"):
            yield Run("axpby3 n%d %s" % (n, have), axpby3, dict(a=a, b=b if "b" in have else None, c=c if "c" in have else None, g=g), dict(n=n))


# ------------------------------------------------------------------------------------------------ attention-pool tokens
def tokens(x, pos, dtype, dtok=None, divisor=None):
    """mean [B, C] = mean_t x + pos[0], rest [B, T, C] = x + pos[1:]; dx, dpos for the upstream gradient dtok [B, T + 1, C].
    divisor: the wrong form that divides the token sum by something other than T (ldt)."""
    xl, pl = _leaf(x, dtype), _leaf(pos, dtype)
    T = x.shape[1]
    mean = xl.sum(1) / (divisor or T) + pl[0]
    rest = xl + pl[1:]
    out = dict(mean=mean.detach(), rest=rest.detach())
    if dtok is not None:
        torch.cat([mean[:, None], rest], dim=1).backward(_c(dtok, dtype))
        out.update(dx=xl.grad, dpos=pl.grad)
    return out, {}


TOKEN_CASES = [(2, 3, 32, 4), (3, 5, 32, 8), (1, 7, 256, 8), (2, 48, 288, 52)]  # (B, T, C, ldt), all formats
TOKEN_F32_ONLY = [(1, 1, 4, 2)]
TOKEN_BWD_BIG = (8, 130, 4096, 132)  # dx past the grid cap (4096 workgroups x 512 channel quads)


@functools.lru_cache(maxsize=None)
def token_inputs(B, T, C):
    return dict(x=R("tok.x%d.%d.%d" % (B, T, C), B, T, C), pos=OF.fill("ht:tok%d.%d.positional_embedding" % (T, C), (T + 1, C)),
                dtok=R("tok.d%d.%d.%d" % (B, T, C), B, T + 1, C))


def runs_tokens(big=True):
    for B, T, C, ldt in TOKEN_CASES + TOKEN_F32_ONLY + ([TOKEN_BWD_BIG] if big else []):
        d = token_inputs(B, T, C)
        meta = dict(B=B, T=T, C=C, ldt=ldt)
        yield Run("tokens %dx%dx%d ldt%d" % (B, T, C, ldt), tokens, dict(d), meta)
        if C % 32 == 0 and (B, T, C, ldt) != TOKEN_BWD_BIG:
            yield Run("tokens %dx%dx%d ldt%d bf16 x" % (B, T, C, ldt), tokens, dict(x=d["x"].bfloat16().float(), pos=d["pos"]), meta)


# ------------------------------------------------------------------------------------------------ softmax
def softmax(s, dtype, dp=None, n_sum=None):
    """p = softmax over the row; ds for the upstream gradient dp.  n_sum: the wrong form whose sum runs over n_sum > n columns
    (the padding's zeros read as logits)."""
    sl = _leaf(s, dtype)
    if n_sum is None:
        p = F.softmax(sl, dim=1)
    else:
        pad = torch.cat([sl, torch.zeros(s.shape[0], n_sum - s.shape[1], dtype=dtype)], dim=1)
        p = F.softmax(pad, dim=1)[:, : s.shape[1]]
    out = dict(p=p.detach())
    spec = dict(p=("rows", None))
    if dp is not None:
        p.backward(_c(dp, dtype))
        out["ds"] = sl.grad
        spec["ds"] = ("rows", p.detach().double().max(1).values * dp.double().abs().max(1).values)  # ds = p (dp - <p, dp>): the terms' size
    return out, spec


SOFTMAX_CASES = [(1, 1, 1), (3, 5, 8), (5, 64, 64), (4, 65, 68), (7, 193, 196), (2, 1000, 1000)]  # (rows, n, ld)


def runs_softmax():
    for rows, n, ld in SOFTMAX_CASES:
        for scale in (1.0, 30.0):
            s = R("sm.s%d.%d" % (rows, n), rows, n) * scale
            if n > 1:
                s[-1] = -80.0  # one row holding a single +80 among -80
                s[-1, n // 2] = 80.0
            yield Run("softmax %dx%d ld%d scale%g" % (rows, n, ld, scale), softmax, dict(s=s, dp=R("sm.d%d.%d" % (rows, n), rows, n)), dict(rows=rows, n=n, ld=ld))


# (the logit range decides what an fp32 exp(z - lse) can deliver - one rounding of lse is 2^-24 |lse| in the exponent - so the
# unit-norm range and the wide one are groups of their own, as are logit scale 1 and 28 of the cross entropy)
GROUP_RUNS = dict(softmax=runs_softmax, infonce=functools.partial(runs_infonce, amps=(1.0,)), infonce5=functools.partial(runs_infonce, amps=(5.0,)),
                  ce=functools.partial(runs_ce, scales=(1.0,)), ce28=functools.partial(runs_ce, scales=(28.0,)), cmpm=runs_cmpm, align=runs_align,
                  norm=runs_norm, sum=runs_sum, elem=runs_elem, tokens=runs_tokens)


# ------------------------------------------------------------------------------------------------ exact restatements
def gather(table, tokens_, L):
    """x [B, L, E] = table[clamp(tokens[:, :L], 0, vocab - 1)]; the columns L..ldtok of `tokens` are no positions"""
    ids = tokens_[:, :L].clamp(0, table.shape[0] - 1)
    return table[ids]


def hit_mask(id_queue, ids):
    """flag[k] = 1 where id_queue[k] equals any of ids, on the full 64 bits"""
    return (id_queue.view(-1, 1) == ids.view(1, -1)).any(1).to(torch.uint8)


def argmax_rows(x):
    """index of each row's maximum, the lowest index on ties; an all -inf row answers 0"""
    return torch.from_numpy(np.argmax(x.numpy(), axis=1).astype(np.int64))


def relu_bwd(dy, act):
    return torch.where(act > 0, dy, torch.zeros_like(dy))


def padded(t, ld, fill=0.0):
    """t [rows, n] in a [rows, ld] matrix whose columns n..ld hold `fill`"""
    out = torch.full((t.shape[0], ld), fill, dtype=t.dtype)
    out[:, : t.shape[1]] = t
    return out


def embedding_bwd(dX, tokens_, L, vocab, pad=0, lose_second_chunk=False):
    """dT [vocab, E]: the first position that holds a token owns its row (a copy of that position's dX row), the later positions
    are added in ascending order, in float32.  Pad and out-of-range ids are ignored; unused rows stay zero.
    lose_second_chunk: the wrong form that loses the positions p + 257 .. p + 512 behind the owner p (its second chunk of 256)."""
    d = dX.numpy().astype(np.float32)
    dT = np.zeros((vocab, d.shape[1]), dtype=np.float32)
    toks = tokens_[:, :L].reshape(-1).tolist()
    owner = {}
    for p, tok in enumerate(toks):
        if tok == pad or tok < 0 or tok >= vocab:
            continue
        if tok not in owner:
            owner[tok] = p
            dT[tok] = d[p]
        elif not (lose_second_chunk and 256 <= p - owner[tok] - 1 < 512):
            dT[tok] = dT[tok] + d[p]
    return torch.from_numpy(dT)


EMB_BWD_CASES = [(1, 1, 1, 2), (2, 3, 5, 7), (3, 100, 32, 5), (2, 140, 300, 9), (4, 130, 8, 3)]  # (B, L, E, vocab)


def emb_bwd_inputs(B, L, E, vocab, kind="mixed", ldtok=None):
    """kind mixed: random ids with pad tokens and out-of-range ids; one: every position the same token; pad: all pad"""
    ldtok = ldtok or L
    if kind == "mixed":
        tok = RI("emb.t%d.%d.%d" % (B, L, vocab), 0, vocab, B, ldtok)
        if B * L >= 6:
            tok[0, 1], tok[-1, L - 1], tok[0, 2] = -1, vocab, vocab + 5
        if B * L == 1:
            tok[0, 0] = 1
    else:
        tok = torch.full((B, ldtok), 1 if kind == "one" else 0, dtype=torch.int64)
    if ldtok > L:
        tok[:, L:] = vocab - 1  # (no positions: must not be counted)
    return R("emb.d%d.%d.%d" % (B, L, E), B * L, E), tok
