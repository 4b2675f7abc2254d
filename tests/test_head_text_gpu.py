"""fp64 parity of the kernels of csrc/head_loss.hip and csrc/attn_text.hip at edge shapes: every loss row and dL/dlogits the
training step back-propagates, the attention pool's token tensor, the embedding gather and the embedding-table gradient.

The entry points are called directly through the C ABI (ops.call / ops._p / ops.stream), so leading dimensions, alignment and
null pointers are the test's to choose.  Every case is compared with the plain fp64 CPU reference of tests/head_text_ref.py
(torch in double, autograd for every gradient) on inputs seeded through oracle.fill; copies, decisions and the fixed-order
embedding sum are compared bit for bit with that module's exact restatements.  Backward kernels that read a forward result are
handed the fp64 reference's, rounded to fp32 - never a kernel's own output.

Every output is a slice of a larger tensor pre-filled with a sentinel (NaN; 0x5A bytes for integers) with 64 elements of it in
front and behind: after the test those must be unchanged, and an element the kernel did not write fails the comparison as NaN.
In-place matrices carry a finite marker in their padding columns where the kernel must leave them alone (infonce, cmpm,
global_align) and must hold zeros there afterwards where the kernel's contract is to clear them (smooth_ce, softmax, colnorm,
attnpool).  Every numerical case runs twice on fresh buffers and must give the same bits: these kernels have no atomics.

Shapes: each is the smallest that enters the branch it is there for - InfoNCE (B, K, ldS): (3, 5, 8) vector path with a tail,
(2, 4096, 4096) exactly one segment, (2, 4097, 4100) a one-column second segment, (3, 8197, 8197) scalar path and three
segments, (2, 4100, 4100) one float off alignment; masks none / every 7th / a whole segment / everything; CMPM 256 | 257 the
register and the re-read path; rows of 255 | 256 | 257 and 11003 for the 256-thread row kernels; colnorm with C and N no
multiples of 64 and ldn > N; the cross projection's scalar form by C % 4 and by alignment; embedding gradients over more than
256 positions, E > 256, E % 4 != 0; token tensors with T < 4, T % 4 != 0, C / 4 % 64 != 0, ldt > T + 1 in all three input
formats; the grid-stride kernels once past their grid cap.

Bounds (tests/head_text_ref.py: TOL[group] = 4 x YARDSTICK[group], the error of an fp32 CPU evaluation of the same formula
against fp64 over the same runs; measured "of" = relative to the larger of the reference's largest magnitude and the size of
the terms that enter).  The worst value measured on the MI355X beside each:
  group     kernels                                                         bound     measured
  softmax   softmax_rows, softmax_rows_bwd                                  4.62e-7   1.13e-7
  infonce   infonce_rows, infonce_queue_rows, |logit| <= 14                 2.25e-6   5.27e-7
  infonce5  ... |logit| <= 71                                               1.13e-5   3.20e-6
  ce        smooth_ce_rows, logit scale 1                                   4.40e-7   1.13e-7
  ce28      ... logit scale 28                                              8.09e-5   3.45e-6
  cmpm      cmpm_rows                                                       1.58e-5   9.65e-6
  align     global_align_rows                                               8.24e-7   2.01e-7
  norm      l2norm_rows, colnorm, cross_project_rows and their backwards    1.65e-6   2.21e-7
  sum       sum, colsum, rowdot, pair_sim_means (of the terms' L1 sum)      3.30e-7   7.88e-8
  elem      axpby3, rowscale_add (per element, of the terms' magnitudes)    6.13e-7   1.31e-7
  tokens    attnpool_tokens (wide: fp32, P16, bf16; narrow), its backward   7.88e-7   2.62e-7
  gemm      cmpm / cmpc / instance / global_align losses through the GEMMs  1e-5 value, 1e-4 of the gradient's maximum: value 2.1e-7, gradient 7.4e-6
  exact     embedding_gather, embedding_bwd, queue_hit_mask, argmax_rows, relu_bwd, token rows 1..T (fp32, bf16), padding: bit for bit
"""

import math

import pytest
import torch

pytestmark = pytest.mark.gpu

import bn_pool_ref as BP  # noqa: E402
import head_text_ref as H  # noqa: E402
import oracle.fill as OF  # noqa: E402
import oracle.losses as OL  # noqa: E402
from head_text_ref import F64, R, RI  # noqa: E402

MARK = 7.5  # finite marker in the padding columns a kernel must not touch
NAN = float("nan")
WORST = {}


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from textreid_amd import ops as o

    yield o
    H.token_inputs.cache_clear()
    print("\nhead/text parity: worst value per group")
    for group in sorted(WORST):
        print("  %-9s %.2e  (bound %s)  %s" % (group, WORST[group][0], "%.2e" % H.TOL[group] if group in H.TOL else "-", WORST[group][1]))


def dev(t):
    return None if t is None else t.cuda().contiguous()


class Args:
    """device copies of CPU tensors as kernel arguments: they stay alive until the outputs of the launch have been read back (a
    temporary whose address alone is kept would be freed, and its memory handed to the next copy, before the kernel runs)"""

    def __init__(self):
        self.keep = []

    def __call__(self, t):
        if t is None:
            return None
        self.keep.append(dev(t))
        return self.keep[-1].data_ptr()


def dev_off(t, off):
    """a device copy of t that starts `off` elements past an allocation's (256-byte aligned) start"""
    flat = torch.empty(t.numel() + off, dtype=t.dtype, device="cuda")
    out = flat[off:].view(t.shape)
    out.copy_(t)
    return out


def report(group, case, what, err):
    print("head/text parity %-9s %-46s %-10s %.2e%s" % (group, case, what, err, "  (%.3f of the bound)" % (err / H.TOL[group]) if group in H.TOL else ""))
    if group not in WORST or not err <= WORST[group][0]:
        WORST[group] = (err, "%s %s" % (case, what))
    return err


def check(group, case, got, want, spec):
    for k in want:
        e = report(group, case, k, H.measure(got[k], want[k], *spec.get(k, ("max", None))))
        assert e <= H.TOL[group], (group, case, k, e)  # (NaN - an element that was never written - fails too)


def bits(t):
    t = t.contiguous()
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


def twice(once):
    """two runs on fresh buffers: equal bits; the first one's outputs (CPU tensors)"""
    a, b = once(), once()
    for k in a:
        assert same_bits(a[k], b[k]), "two runs differ in " + k
    return a


# --------------------------------------------------------------------------- guard regions
GUARD = 64  # sentinel elements in front of and behind every output buffer


def _sentinel(n, dtype):
    if dtype.is_floating_point:
        return torch.full((n,), NAN, dtype=dtype, device="cuda")
    return torch.full((n,), 0x5A5A5A5A5A5A5A5A if dtype == torch.int64 else 0x5A, dtype=dtype, device="cuda")


class Guard:
    def __init__(self):
        self.log = []

    def buf(self, shape, dtype=torch.float32, init=None, off=0):
        """the middle of a sentinel-filled buffer (`off` elements past its aligned position), optionally holding `init`"""
        shape = (shape,) if isinstance(shape, int) else tuple(shape)
        n = math.prod(shape)
        full = _sentinel(n + 2 * GUARD + off, dtype)
        out = full[GUARD + off : GUARD + off + n].view(shape)
        if init is not None:
            out.copy_(init)
        self.log.append((full, GUARD + off, n))
        return out

    def check(self):
        torch.cuda.synchronize()
        for k, (full, start, n) in enumerate(self.log):
            want = bits(_sentinel(1, full.dtype))[0]
            raw = bits(full)
            assert bool((raw[:start] == want).all()), "buffer %d (%s x %d): written in front of it" % (k, full.dtype, n)
            assert bool((raw[start + n :] == want).all()), "buffer %d (%s x %d): written behind it" % (k, full.dtype, n)
        self.log.clear()


@pytest.fixture(autouse=True)
def g(ops):
    guard = Guard()
    yield guard
    guard.check()


def all_equal(t, value):
    return bool((t == value).all())


# --------------------------------------------------------------------------- InfoNCE
def _infonce_case(ops, g, B, K, off, forms):
    lib = ops.L.load()
    for run in H.runs_infonce(forms=forms):
        m, kw = run.meta, run.kw
        if (m["B"], m["K"], m["off"]) != (B, K, off):
            continue
        ld, C = m["ld"], m.get("C")
        group = "infonce5" if "|S|<=5" in run.name else "infonce"
        S0 = H.padded(kw["S"], ld, MARK)

        def once():
            a = Args()
            S = g.buf((B, ld), init=S0, off=off)
            hit = g.buf(K, torch.uint8, init=kw["hit"].to(torch.uint8))  # exactly K bytes, sentinel behind them
            rows, ws = g.buf(B), g.buf(int(lib.trid_infonce_ws_floats(B, K)))
            if C is None:
                pos, dpos = dev(kw["pos"]), g.buf(B)
                ops.call("trid_infonce_rows_f32", ops._p(S), ops._p(pos), ops._p(hit), ops._p(rows), ops._p(dpos), B, K, ld, kw["invT"], kw["gscale"],
                         ops._p(ws), ops.stream())
            else:
                q, key, dpos = dev(kw["q"]), dev(kw["key"]), g.buf((B, C))
                ops.call("trid_infonce_queue_rows_f32", ops._p(S), ops._p(q), ops._p(key), ops._p(hit), ops._p(rows), ops._p(dpos), B, K, ld, C,
                         kw["invT"], kw["gscale"], ops._p(ws), ops.stream())
            return dict(rows=rows.cpu(), S=S.cpu(), dpos=dpos.cpu())

        out = twice(once)
        assert all_equal(out["S"][:, K:], MARK), "columns beyond K were written"
        got = dict(rows=out["rows"], dS=out["S"][:, :K], dpos=out["dpos"])
        want, spec = H.ref_of(run)
        check(group, run.name, got, want, spec)
        if " all " in run.name:  # every column masked: the loss row is 0 and so is the whole gradient
            assert all(all_equal(got[k], 0.0) for k in got), run.name


@pytest.mark.parametrize("B,K,ld,off", H.INFONCE_CASES)
def test_infonce_rows(ops, g, B, K, ld, off):
    _infonce_case(ops, g, B, K, off, ("rows",))


@pytest.mark.parametrize("B,K,ld,off", H.INFONCE_CASES)
def test_infonce_queue_rows(ops, g, B, K, ld, off):
    """the positive logit <q, key> computed in the kernel, dq0 = dL/dpos * key; C = 1, 256, 260"""
    _infonce_case(ops, g, B, K, off, ("queue",))


# --------------------------------------------------------------------------- in-place [B, ldS] row kernels: CMPM, global align
def _square_rows(ops, g, group, runs, B, launch):
    for run in runs:
        if run.meta["B"] != B:
            continue
        ld, kw = run.meta["ld"], run.kw
        S0 = H.padded(kw["S"], ld, MARK)

        def once():
            a = Args()
            S, ids, rows = g.buf((B, ld), init=S0), dev(kw["ids"]), g.buf(B)
            launch(S, ids, rows, ld, kw)
            return dict(rows=rows.cpu(), S=S.cpu())

        out = twice(once)
        assert all_equal(out["S"][:, B:], MARK), "columns beyond B were written"
        want, spec = H.ref_of(run)
        check(group, run.name, dict(rows=out["rows"], dS=out["S"][:, :B]), want, spec)


@pytest.mark.parametrize("B,ld", H.CMPM_CASES)
def test_cmpm_rows(ops, g, B, ld):
    """B <= 256: the row in registers; 257, 300: the re-read path"""
    _square_rows(ops, g, "cmpm", H.runs_cmpm(), B,
                 lambda S, ids, rows, ld_, kw: ops.call("trid_cmpm_rows_f32", ops._p(S), ops._p(ids), ops._p(rows), B, ld_, kw["eps"], kw["gs"], ops.stream()))


@pytest.mark.parametrize("B,ld", H.ALIGN_CASES)
def test_global_align_rows(ops, g, B, ld):
    _square_rows(ops, g, "align", H.runs_align(), B,
                 lambda S, ids, rows, ld_, kw: ops.call("trid_global_align_rows_f32", ops._p(S), ops._p(ids), ops._p(rows), B, ld_, 0.6, 0.4, 10.0, 40.0,
                                                        kw["gscale"], ops.stream()))


@pytest.mark.parametrize("B", H.PAIR_B)
def test_pair_sim_means(ops, g, B):
    """B = 1 (and one id everywhere): the different-id mean is NaN, as torch.mean of nothing - the output is pre-filled with a
    finite value here, so that a NaN is one the kernel wrote"""
    for run in H.runs_pair_means():
        if run.meta["B"] != B:
            continue
        ld, kw = run.meta["ld"], run.kw
        S = dev(H.padded(kw["S"], ld, NAN))

        def once():
            a = Args()
            out = g.buf(2, init=torch.full((2,), 777.0))
            ops.call("trid_pair_sim_means_f32", ops._p(S), a(kw["row_scale"]), a(kw["ids"]), ops._p(out), B, ld, ops.stream())
            return dict(means=out.cpu())

        want, spec = H.ref_of(run)
        check("sum", run.name, twice(once), want, spec)
        assert bool(torch.isnan(want["means"][1])) == all_equal(kw["ids"], int(kw["ids"][0])) and not bool(torch.isnan(want["means"][0]))


# --------------------------------------------------------------------------- smooth CE
@pytest.mark.parametrize("rows,n,ld,eps", H.CE_CASES)
def test_smooth_ce_rows(ops, g, rows, n, ld, eps):
    """rows longer than one 256-thread trip with a ragged tail, ld > n (zeros written in columns n..ld), labels 0 and n - 1"""
    for run in H.runs_ce():
        if (run.meta["rows"], run.meta["n"]) != (rows, n):
            continue
        kw = run.kw
        z0 = H.padded(kw["logits"], ld, MARK)

        def once():
            a = Args()
            z, lr = g.buf((rows, ld), init=z0), g.buf(rows)
            ops.call("trid_smooth_ce_rows_f32", ops._p(z), a(kw["labels"]), ops._p(lr), rows, n, ld, kw["eps"], kw["gscale"], ops.stream())
            return dict(rows=lr.cpu(), z=z.cpu())

        out = twice(once)
        assert all_equal(out["z"][:, n:], 0.0), "columns n..ld must be zero"
        want, spec = H.ref_of(run)
        check("ce28" if "scale28" in run.name else "ce", run.name, dict(rows=out["rows"], dlogits=out["z"][:, :n]), want, spec)
        if n == 1:
            assert all_equal(out["rows"], 0.0)


# --------------------------------------------------------------------------- colnorm
@pytest.mark.parametrize("C,N,ldn", H.COLNORM_CASES)
def test_colnorm(ops, g, C, N, ldn):
    """C, N no multiples of 64, ldn > N: rows N..ldn of pnt and columns N..ldn of pn are zero (they are GEMM operands); pn null
    and given; an all-zero column: inv = 1e12, outputs 0"""
    for run in H.runs_colnorm():
        if (run.meta["C"], run.meta["N"]) != (C, N):
            continue
        kw = run.kw
        want, spec = H.ref_of(run)
        for with_pn in (False, True):
            def once():
                a = Args()
                pn, pnt, inv = (g.buf((C, ldn)) if with_pn else None), g.buf((ldn, C)), g.buf(N)
                ops.call("trid_colnorm_f32", a(kw["proj"]), ops._p(pn), ops._p(pnt), ops._p(inv), C, N, ldn, ops.stream())
                return dict(pnt=pnt.cpu(), inv=inv.cpu(), **(dict(pn=pn.cpu()) if with_pn else {}))

            out = twice(once)
            assert all_equal(out["pnt"][N:], 0.0), "rows N..ldn of pnt must be zero"
            check("norm", run.name + (" +pn" if with_pn else ""), dict(pnt=out["pnt"][:N], inv=out["inv"]), {k: want[k] for k in ("pnt", "inv")}, spec)
            if with_pn:
                assert all_equal(out["pn"][:, N:], 0.0) and same_bits(out["pn"][:, :N].t().contiguous(), out["pnt"][:N].contiguous())
            if "zero column" in run.name:
                assert all_equal(out["pnt"][1], 0.0) and float(out["inv"][1]) == float(torch.tensor(1e12, dtype=torch.float32))
        if "dpnt" not in kw:
            continue
        pnt32 = torch.full((ldn, C), NAN)  # (rows N..ldn are not the backward's to read)
        pnt32[:N] = want["pnt"].float()
        dpnt = torch.full((ldn, C), NAN)
        dpnt[:N] = kw["dpnt"]

        def once_bwd():
            a = Args()
            dproj = g.buf((C, N))
            ops.call("trid_colnorm_bwd_f32", a(dpnt), a(pnt32), a(want["inv"].float()), ops._p(dproj), C, N, ldn, ops.stream())
            return dict(dprojT=dproj.cpu().t().contiguous())

        check("norm", run.name + " bwd", twice(once_bwd), dict(dprojT=want["dprojT"]), spec)


# --------------------------------------------------------------------------- cross projection
@pytest.mark.parametrize("B,C,off", H.CROSS_CASES)
def test_cross_project_rows(ops, g, B, C, off):
    """C % 4 != 0 or v one float off alignment: the scalar kernel; C > 256 in the backward; a zero row in v (the 1e-12 clamp)"""
    (run,) = [r for r in H.runs_cross() if (r.meta["B"], r.meta["C"], r.meta["off"]) == (B, C, off)]
    kw = run.kw
    want, spec = H.ref_of(run)

    def once():
        a = Args()
        v, t = dev_off(kw["v"], off), dev(kw["t"])
        X, dots, inv = g.buf((2 * B, C)), g.buf(2 * B), g.buf(2 * B)
        ops.call("trid_cross_project_rows_f32", ops._p(v), ops._p(t), ops._p(X), ops._p(dots), ops._p(inv), B, C, ops.stream())
        dv, dt = g.buf((B, C)), g.buf((B, C))
        ops.call("trid_cross_project_rows_bwd_f32", a(kw["G"]), ops._p(v), ops._p(t), a(want["dots"].float()), a(want["inv"].float()),
                 ops._p(dv), ops._p(dt), B, C, ops.stream())
        return dict(X=X.cpu(), dots=dots.cpu(), inv=inv.cpu(), dv=dv.cpu(), dt=dt.cpu())

    out = twice(once)
    check("norm", run.name, out, want, spec)
    if B >= 3:  # the zero row of v: nothing of it in X, dots 0, inv 1e12
        assert all_equal(out["X"][1], 0.0) and all_equal(out["X"][B + 1], 0.0) and float(out["dots"][1]) == 0.0 and float(out["inv"][1]) == float(torch.tensor(1e12, dtype=torch.float32))


# --------------------------------------------------------------------------- argmax, hit mask
def _argmax_variants(rows, n):
    """name -> x [rows, n]: ties inside a lane's trips (j and j + 256), across lanes, across waves; all equal; all -inf; the
    maximum in the last column"""
    base = R("am.x%d.%d" % (rows, n), rows, n)
    out = dict(random=base)
    ties = base.clone()
    pairs = [(a, b) for (a, b) in ((3, 259), (5, 20), (10, 200), (0, n - 1)) if b < n and a < b]
    for r in range(rows):
        if pairs:
            a, b = pairs[r % len(pairs)]
            ties[r, a] = ties[r, b] = 9.0
    out["ties"] = ties
    out["all equal"] = torch.full((rows, n), -2.5)
    out["all -inf"] = torch.full((rows, n), -H.INF)
    last = base.clone()
    last[:, n - 1] = 11.0
    out["last column"] = last
    return out


@pytest.mark.parametrize("rows,n,ld", [(1, 1, 1), (3, 5, 8), (2, 256, 256), (2, 257, 260), (2, 1000, 1000)])
def test_argmax_rows(ops, g, rows, n, ld):
    for k, (name, x) in enumerate(_argmax_variants(rows, n).items()):
        want = H.argmax_rows(x)
        if name in ("all equal", "all -inf"):
            assert all_equal(want, 0)
        if name == "last column":
            assert all_equal(want, n - 1)
        labels = want.clone()
        if k % 2:
            labels[0] = (labels[0] + 1) % max(n, 2)
        a = Args()
        xd = dev(H.padded(x, ld, 100.0))  # (the padding columns are no candidates)
        for mode in ("idx", "hit", "both"):
            idx = g.buf(rows, torch.int64) if mode != "hit" else None
            hit = g.buf(rows) if mode != "idx" else None
            ops.call("trid_argmax_rows_f32", ops._p(xd), a(labels) if hit is not None else None, ops._p(idx), ops._p(hit), rows, n, ld, ops.stream())
            if idx is not None:
                assert torch.equal(idx.cpu(), want), (name, mode, idx.cpu().tolist(), want.tolist())
            if hit is not None:
                assert torch.equal(hit.cpu(), (want == labels).float()), (name, mode)
        report("exact", "argmax %dx%d ld%d %s" % (rows, n, ld, name), "idx, hit", 0.0)


@pytest.mark.parametrize("K,B", [(1, 1), (5, 3), (256, 1), (257, 130), (1000, 8192)])
def test_queue_hit_mask(ops, g, K, B):
    """negative ids; ids that agree in their low 32 bits only do not hit"""
    ids = RI("hm.i%d.%d" % (K, B), -40, 40, B) * 3
    queue = RI("hm.q%d.%d" % (K, B), -60, 60, K) * 2  # (multiples of 6 can hit)
    queue[0] = ids[0]
    if K >= 5:
        queue[1] = ids[-1] + (1 << 32)
        queue[2] = ids[0] - (1 << 32)
        queue[3] = -ids[0] - 1 if int(ids[0]) != 0 else 1
        queue[K - 1] = ids[B // 2]
    want = H.hit_mask(queue, ids)
    assert int(want[0]) == 1 and (K < 5 or (int(want[1]) == 0 and int(want[2]) == 0))

    def once():
        a = Args()
        flag = g.buf(K, torch.uint8)
        ops.call("trid_queue_hit_mask", a(queue), a(ids), ops._p(flag), K, B, ops.stream())
        return dict(flag=flag.cpu())

    got = twice(once)["flag"]
    assert torch.equal(got, want), (got.tolist(), want.tolist())
    report("exact", "hit mask K%d B%d" % (K, B), "%d hits" % int(want.sum()), 0.0)


# --------------------------------------------------------------------------- row kernels: l2norm, rowdot, rowscale_add
@pytest.mark.parametrize("rows,C", H.ROW_CASES)
def test_l2norm_rows(ops, g, rows, C):
    """one wave per row: C = 1, 5, 64 | 65, 256, 1000; one zero row, rows scaled by 1e-3 and 1e3; inv_norm null; accumulate"""
    (run,) = [r for r in H.runs_l2norm() if (r.meta["rows"], r.meta["C"]) == (rows, C)]
    kw = run.kw
    want, spec = H.ref_of(run)
    x, dy, d0 = dev(kw["x"]), dev(kw["dy"]), R("row.d0%d.%d" % (rows, C), rows, C)
    y32, inv32 = dev(want["y"].float()), dev(want["inv"].float())

    def once():
        a = Args()
        y, inv, y2 = g.buf((rows, C)), g.buf(rows), g.buf((rows, C))
        ops.call("trid_l2norm_rows_f32", ops._p(x), ops._p(y), ops._p(inv), rows, C, 1e-12, ops.stream())
        ops.call("trid_l2norm_rows_f32", ops._p(x), ops._p(y2), None, rows, C, 1e-12, ops.stream())
        dx, dxa = g.buf((rows, C)), g.buf((rows, C), init=d0)
        ops.call("trid_l2norm_rows_bwd_f32", ops._p(dy), ops._p(y32), ops._p(inv32), ops._p(dx), rows, C, 0, ops.stream())
        ops.call("trid_l2norm_rows_bwd_f32", ops._p(dy), ops._p(y32), ops._p(inv32), ops._p(dxa), rows, C, 1, ops.stream())
        return dict(y=y.cpu(), inv=inv.cpu(), y2=y2.cpu(), dx=dx.cpu(), dxa=dxa.cpu())

    out = twice(once)
    assert same_bits(out["y"], out["y2"]), "inv_norm null changes y"
    check("norm", run.name, out, want, spec)
    check("norm", run.name + " accumulate", dict(dx=out["dxa"]), dict(dx=want["dx"] + d0.double()), dict(dx=("rows", spec["dx"][1] + d0.double().abs().max(1).values)))
    if rows >= 3:
        assert all_equal(out["y"][2], 0.0) and float(out["inv"][2]) == float(torch.tensor(1e12, dtype=torch.float32))


def _sum_runs(ops, g, word, launch):
    for run in H.runs_sum():
        if run.name.startswith(word):
            want, spec = H.ref_of(run)
            check("sum", run.name, twice(lambda: launch(run)), want, spec)


def test_rowdot(ops, g):
    def launch(run):
        a = Args()
        rows, C = run.meta["rows"], run.meta["C"]
        out = g.buf(rows)
        ops.call("trid_rowdot_f32", a(run.kw["x"]), a(run.kw["y"]), ops._p(out), rows, C, ops.stream())
        return dict(out=out.cpu())

    _sum_runs(ops, g, "rowdot", launch)


def test_sum(ops, g):
    """n = 1, 255, 257, 1000 over one 256-thread workgroup; scale and accumulate"""
    def launch(run):
        a = Args()
        out0 = run.kw["out0"]
        out = g.buf(1, init=out0)
        ops.call("trid_sum_f32", a(run.kw["x"]), ops._p(out), run.meta["n"], run.kw["scale"], 0 if out0 is None else 1, ops.stream())
        return dict(out=out.cpu())

    _sum_runs(ops, g, "sum", launch)


def test_colsum(ops, g):
    """N = 1, 5, 64 | 65, 130 columns over 64-column workgroups, M = 1029 rows over four row lanes, ld > N; accumulate"""
    def launch(run):
        a = Args()
        M, N, ld = run.meta["M"], run.meta["N"], run.meta["ld"]
        out = g.buf(N, init=run.kw["out0"])
        ops.call("trid_colsum_f32", a(H.padded(run.kw["x"], ld, NAN)), ops._p(out), M, N, ld, 0 if run.kw["out0"] is None else 1, ops.stream())
        return dict(out=out.cpu())

    _sum_runs(ops, g, "colsum", launch)


def _elem_runs(ops, g, word, launch):
    for run in H.runs_elem():
        if run.name.startswith(word):
            want, spec = H.ref_of(run)
            check("elem", run.name, twice(lambda: launch(run)), want, spec)


def test_rowscale_add(ops, g):
    """the row shapes, and once rows * C = 1 050 000: past 4096 workgroups x 256, the grid-stride loop's second trip"""
    def launch(run):
        a = Args()
        rows, C = run.meta["rows"], run.meta["C"]
        dx0 = run.kw["dx0"]
        dx = g.buf((rows, C), init=dx0)
        ops.call("trid_rowscale_add_f32", a(run.kw["s"]), a(run.kw["y"]), ops._p(dx), rows, C, 0 if dx0 is None else 1, ops.stream())
        return dict(dx=dx.cpu().reshape(-1))

    _elem_runs(ops, g, "rowscale_add", launch)


def test_axpby3(ops, g):
    """n = 1, 1023 | 1025 and 2048 * 1024 + 3 (past the grid cap); b / c null and given"""
    def launch(run):
        a = Args()
        n, kw = run.meta["n"], run.kw
        out = g.buf(n)
        ops.call("trid_axpby3_f32", ops._p(out), a(kw["a"]), a(kw["b"]), a(kw["c"]), a(kw["g"]), n, ops.stream())
        return dict(out=out.cpu())

    _elem_runs(ops, g, "axpby3", launch)


@pytest.mark.parametrize("n", H.ELEM_N)
def test_relu_bwd(ops, g, n):
    """dx = act > 0 ? dy : 0, with act holding 0 and -0; exact"""
    dy, act = R("rb.dy%d" % n, n), R("rb.a%d" % n, n)
    act[::7] = 0.0
    act[3::11] = -0.0
    want = H.relu_bwd(dy, act)

    def once():
        a = Args()
        dx = g.buf(n)
        ops.call("trid_relu_bwd_f32", a(dy), a(act), ops._p(dx), n, ops.stream())
        return dict(dx=dx.cpu())

    assert same_bits(twice(once)["dx"], want)
    report("exact", "relu_bwd n%d" % n, "dx", 0.0)


# --------------------------------------------------------------------------- attention-pool tokens
def _token_formats(ops, x):
    """fmt -> (device tensor, amax scalar or None, the fp32 values it holds): 0 fp32; 1 P16 written by ops.p16_pack and read back
    by the CPU decoder, so that only the token kernel is measured; 2 plain bf16"""
    xd = dev(x)
    out = {0: (xd, None, x)}
    if x.shape[-1] % 32 == 0:
        p1, p2 = ops.p16_pack(xd), ops.p16_pack(xd, fmt=2)
        out[1] = (p1.data, p1.amax, BP.p16_decode(p1.data.cpu(), float(p1.amax)))
        out[2] = (p2.data, None, p2.data.float().cpu())
    return out


@pytest.mark.parametrize("B,T,C,ldt", H.TOKEN_CASES + H.TOKEN_F32_ONLY)
def test_attnpool_tokens(ops, g, B, T, C, ldt):
    """T < 4 (idle token lanes), T % 4 != 0, C / 4 = 8, 64, 72 (a partly live second block), ldt > T + 1 (zeroed rows), fmt 0 / 1 /
    2; the narrow fp32 form: rows 1..T bit-equal to the wide one"""
    d = H.token_inputs(B, T, C)
    pos = dev(d["pos"])
    wide0 = None
    for fmt, (xd, amax, xval) in _token_formats(ops, d["x"]).items():
        def once():
            a = Args()
            tok = g.buf((B, ldt, C))
            ops.call("trid_attnpool_tokens_fmt_f32", ops._p(xd), fmt, ops._p(amax), ops._p(pos), ops._p(tok), B, T, C, ldt, ops.stream())
            return dict(tok=tok.cpu())

        tok = twice(once)["tok"]
        case = "tokens %dx%dx%d ldt%d fmt%d" % (B, T, C, ldt, fmt)
        want, spec = H.tokens(xval, d["pos"], F64)
        assert all_equal(tok[:, T + 1 :], 0.0), "token rows T+1..ldt must be zero"
        check("tokens", case, dict(mean=tok[:, 0], rest=tok[:, 1 : T + 1]), want, spec)
        if fmt != 1:
            assert same_bits(tok[:, 1 : T + 1].contiguous(), xval + d["pos"][1:]), "rows 1..T are the fp32 sum x + pos"
        if fmt == 0:
            wide0 = tok

    def narrow():
        a = Args()
        tok = g.buf((B, ldt, C))
        ops.call("trid_attnpool_tokens_f32", a(d["x"]), ops._p(pos), ops._p(tok), B, T, C, ldt, ops.stream())
        return dict(tok=tok.cpu())

    tok = twice(narrow)["tok"]
    want, spec = H.tokens(d["x"], d["pos"], F64)
    assert all_equal(tok[:, T + 1 :], 0.0) and same_bits(tok[:, 1 : T + 1].contiguous(), wide0[:, 1 : T + 1].contiguous())
    check("tokens", "tokens %dx%dx%d ldt%d narrow" % (B, T, C, ldt), dict(mean=tok[:, 0]), dict(mean=want["mean"]), spec)


@pytest.mark.parametrize("B,T,C,ldt", H.TOKEN_CASES + H.TOKEN_F32_ONLY + [H.TOKEN_BWD_BIG])
def test_attnpool_tokens_bwd(ops, g, B, T, C, ldt):
    """dx = dtok[1 + t] + dtok[0] / T, dpos = sum_b dtok; (8, 130, 4096, 132): dx past the grid cap"""
    (run,) = [r for r in H.runs_tokens() if r.meta == dict(B=B, T=T, C=C, ldt=ldt) and "bf16" not in r.name]
    dtok = torch.full((B, ldt, C), NAN)  # (rows T+1..ldt are not read)
    dtok[:, : T + 1] = run.kw["dtok"]
    dtokd = dev(dtok)

    def once():
        a = Args()
        dx, dpos = g.buf((B, T, C)), g.buf((T + 1, C))
        ops.call("trid_attnpool_tokens_bwd_f32", ops._p(dtokd), ops._p(dx), ops._p(dpos), B, T, C, ldt, ops.stream())
        return dict(dx=dx.cpu(), dpos=dpos.cpu())

    want, spec = H.ref_of(run)
    check("tokens", run.name + " bwd", twice(once), {k: want[k] for k in ("dx", "dpos")}, spec)


# --------------------------------------------------------------------------- softmax
@pytest.mark.parametrize("rows,n,ld", H.SOFTMAX_CASES)
def test_softmax_rows(ops, g, rows, n, ld):
    """one wave per row: n = 1, 5, 64 | 65, 193, 1000; ld > n (zeros in columns n..ld, forward and backward); scale 1 and 30; a row
    holding a single +80 among -80"""
    for run in H.runs_softmax():
        if (run.meta["rows"], run.meta["n"]) != (rows, n):
            continue
        kw = run.kw
        want, spec = H.ref_of(run)
        s0 = H.padded(kw["s"], ld, MARK)
        p32, dp = dev(H.padded(want["p"].float(), ld, NAN)), dev(H.padded(kw["dp"], ld, NAN))  # (the backward reads columns 0..n only)

        def once():
            a = Args()
            s, ds = g.buf((rows, ld), init=s0), g.buf((rows, ld))
            ops.call("trid_softmax_rows_f32", ops._p(s), rows, n, ld, ops.stream())
            ops.call("trid_softmax_rows_bwd_f32", ops._p(p32), ops._p(dp), ops._p(ds), rows, n, ld, ops.stream())
            return dict(s=s.cpu(), ds=ds.cpu())

        out = twice(once)
        assert all_equal(out["s"][:, n:], 0.0) and all_equal(out["ds"][:, n:], 0.0), "columns n..ld must be zero"
        check("softmax", run.name, dict(p=out["s"][:, :n], ds=out["ds"][:, :n]), want, spec)


# --------------------------------------------------------------------------- embedding gather and gradient
@pytest.mark.parametrize("B,L,ldtok,E,vocab", [(1, 1, 1, 4, 2), (3, 5, 8, 32, 11), (2, 7, 7, 300, 50), (64, 64, 64, 1028, 100)])
def test_embedding_gather(ops, g, B, L, ldtok, E, vocab):
    """an exact copy; ids -1, vocab, vocab + 5 are clamped; tokens in columns L..ldtok are no positions; the last case is past the
    grid cap (4096 workgroups x 512 quads)"""
    table = R("eg.t%d.%d" % (vocab, E), vocab, E)
    tok = RI("eg.i%d.%d" % (B, L), 0, vocab, B, ldtok)
    if B * L >= 15:
        tok[0, 0], tok[1, 2], tok[B - 1, L - 1] = -1, vocab, vocab + 5
    if ldtok > L:
        tok[:, L:] = (tok[:, :1] + 1) % vocab
    want = H.gather(table, tok, L)

    def once():
        a = Args()
        x = g.buf((B, L, E))
        ops.call("trid_embedding_gather_f32", a(table), a(tok), ops._p(x), B, L, ldtok, E, vocab, ops.stream())
        return dict(x=x.cpu())

    assert same_bits(twice(once)["x"], want)
    report("exact", "gather %dx%d ldtok%d E%d vocab%d" % (B, L, ldtok, E, vocab), "x", 0.0)


@pytest.mark.parametrize("B,L,E,vocab", H.EMB_BWD_CASES)
def test_embedding_bwd(ops, g, B, L, E, vocab):
    """bit-equal to the sequential fp32 sum in position order: 300 positions (a second ballot chunk), E = 300 (a second channel
    pass), E % 4 != 0, every position one token (519 adds over three chunks), all pad (all zero), out-of-range ids, ldtok > L"""
    for kind, ldtok in (("mixed", L), ("mixed", L + 3), ("one", L), ("pad", L)):
        dX, tok = H.emb_bwd_inputs(B, L, E, vocab, kind=kind, ldtok=ldtok)
        want = H.embedding_bwd(dX, tok, L, vocab)

        def once():
            a = Args()
            dT = g.buf((vocab, E))
            ops.call("trid_embedding_bwd_f32", a(dX), a(tok), B, L, ldtok, E, ops._p(dT), vocab, 0, ops.stream())
            return dict(dT=dT.cpu())

        got = twice(once)["dT"]
        assert same_bits(got, want), (kind, ldtok, float((got.double() - want.double()).abs().max()))
        used = set(t for t in tok[:, :L].reshape(-1).tolist() if 0 < t < vocab)
        assert all(all_equal(got[v], 0.0) for v in range(vocab) if v not in used) and (kind != "pad" or not used)
        report("exact", "embedding_bwd %dx%d E%d vocab%d %s ldtok%d" % (B, L, E, vocab, kind, ldtok), "dT", 0.0)


# --------------------------------------------------------------------------- the public losses, through the split-bf16 GEMMs
def _gemm_check(case, got, want, grads_got, grads_want):
    e = report("gemm", case, "value", H.measure(got.detach().reshape(-1), want.detach().reshape(-1)))
    assert e <= H.GEMM_VALUE, (case, e)
    for k, (a, b) in enumerate(zip(grads_got, grads_want)):
        e = report("gemm", case, "grad %d" % k, H.measure(a, b))
        assert e <= H.GEMM_GRAD, (case, k, e)


def _embeds(tag, B, C):
    """correlated pairs with a common component, as trained embeddings are (no cosine mean that cancels)"""
    common = R(tag + ".c", 1, C)
    v = R(tag + ".v", B, C) * 0.5 + 0.5 * common
    return v, R(tag + ".t", B, C) * 0.5 + 0.5 * v


def _leaves(*ts, cuda=False):
    return [(t.cuda() if cuda else t.double()).clone().requires_grad_(True) for t in ts]


@pytest.mark.parametrize("B", [257, 300])
def test_cmpm_loss_reread_path(ops, B):
    """cmpm_loss(verbose=True) above 256 rows: both CMPM matrices take the re-read path, the pair means read B * B entries"""
    import torch.nn.functional as F

    from textreid_amd import losses as L

    v0, t0 = _embeds("g.cmpm%d" % B, B, 64)
    lab = (torch.arange(B) // 4) * 7

    def want(v, t):
        vn, tn = F.normalize(v, dim=1), F.normalize(t, dim=1)
        same = H.same_ids(lab)
        q = same.double() / same.double().sum(1, keepdim=True).sqrt()
        loss = 0.0
        for S in (v @ tn.t(), t @ vn.t()):
            lp = F.log_softmax(S, dim=1)
            loss = loss + (lp.exp() * (lp - torch.log(q + 1e-8))).sum(1).mean()
        cos = vn @ tn.t()
        return loss, cos[same].mean(), cos[~same].mean()

    rv, rt = _leaves(v0, t0)
    wl, wp, wn = want(rv, rt)
    (wl * 2.0).backward()
    gv, gt = _leaves(v0, t0, cuda=True)
    loss, pos, neg = L.cmpm_loss(gv, gt, lab.cuda(), verbose=True)
    (loss * 2.0).backward()
    _gemm_check("cmpm_loss B%d" % B, torch.stack([loss, pos, neg]).cpu(), torch.stack([wl, wp, wn]), (gv.grad.cpu(), gt.grad.cpu()), (rv.grad, rt.grad))
    for k, (a, b) in enumerate(((loss, wl), (pos, wp), (neg, wn))):
        assert abs(float(a.detach()) - float(b.detach())) <= H.GEMM_VALUE * abs(float(b.detach())), (B, k, float(a.detach()), float(b.detach()))


def test_global_align_losses_reread_rows(ops):
    """global_align_loss and global_align_loss_from_sim at B = 257: rows of two 256-thread trips, ldS = 260"""
    from textreid_amd import losses as L

    B = 257
    v0, t0 = _embeds("g.ga", B, 64)
    lab = (torch.arange(B) // 4) * 7
    rv, rt = _leaves(v0, t0)
    want = OL.global_align_loss(rv, rt, lab)
    (want * 2.0).backward()
    gv, gt = _leaves(v0, t0, cuda=True)
    got = L.global_align_loss(gv, gt, lab.cuda())
    (got * 2.0).backward()
    _gemm_check("global_align_loss B257", got.cpu(), want, (gv.grad.cpu(), gt.grad.cpu()), (rv.grad, rt.grad))
    sim0 = torch.tanh(R("g.sim", B, B) * 0.5)
    (rs,) = _leaves(sim0)
    rows = H.global_align_rows(rs.detach(), lab, 2.0, F64)[0]
    (gs,) = _leaves(sim0, cuda=True)
    got = L.global_align_loss_from_sim(gs, lab.cuda())
    (got * 2.0).backward()
    _gemm_check("global_align_loss_from_sim B257", got.cpu(), rows["rows"].sum(), (gs.grad.cpu(),), (rows["dS"],))


def test_instance_and_cmpc_losses_ragged_projection(ops):
    """instance_loss(norm=True, scale=28) and cmpc_loss(verbose=True) with a (65, 70) projection, B = 5: colnorm with C and N
    no multiples of 64 and ldn = 80, cross projection with C % 4 != 0"""
    import torch.nn.functional as F

    from textreid_amd import losses as L

    C, N, B = 65, 70, 5
    v0, t0 = _embeds("g.inst", B, C)
    p0 = OF.fill("ht:g.inst.projection", (C, N))
    lab = torch.tensor([0, 69, 33, 33, 7])
    p0[:, lab] += 0.5 * (F.normalize(v0, dim=1) + F.normalize(t0, dim=1)).t()  # some rows classify correctly: a precision that is not 0
    rp, rv, rt = _leaves(p0, v0, t0)
    want = OL.instance_loss(rp, rv, rt, lab, 0.1, scale=28, norm=True)
    (want * 2.0).backward()
    gp, gv, gt = _leaves(p0, v0, t0, cuda=True)
    got = L.instance_loss(gp, gv, gt, lab.cuda(), scale=28, norm=True, epsilon=0.1)
    (got * 2.0).backward()
    _gemm_check("instance_loss 65x70 B5", got.cpu(), want, [x.grad.cpu() for x in (gp, gv, gt)], [x.grad for x in (rp, rv, rt)])

    def cmpc(p, v, t):  # losses.py:65-99
        vn, tn, pn = F.normalize(v, dim=1), F.normalize(t, dim=1), F.normalize(p, dim=0)
        il, tl = ((v * tn).sum(1, keepdim=True) * tn) @ pn, ((t * vn).sum(1, keepdim=True) * vn) @ pn
        return F.cross_entropy(il, lab) + F.cross_entropy(tl, lab), (il.argmax(1) == lab).double().mean(), (tl.argmax(1) == lab).double().mean()

    rp, rv, rt = _leaves(p0, v0, t0)
    want, wip, wtp = cmpc(rp, rv, rt)
    (want * 2.0).backward()
    gp, gv, gt = _leaves(p0, v0, t0, cuda=True)
    got, ip, tp = L.cmpc_loss(gp, gv, gt, lab.cuda(), verbose=True)
    (got * 2.0).backward()
    assert float(wip) > 0 and float(wtp) > 0
    _gemm_check("cmpc_loss 65x70 B5", torch.stack([got, ip, tp]).cpu(), torch.stack([want, wip, wtp]), [x.grad.cpu() for x in (gp, gv, gt)], [x.grad for x in (rp, rv, rt)])
    assert float(ip) == pytest.approx(float(wip), rel=1e-6) and float(tp) == pytest.approx(float(wtp), rel=1e-6)
