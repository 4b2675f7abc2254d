"""The CPU references of tests/head_text_ref.py checked on their own (no GPU): the fp64 restatements against oracle/losses.py and
torch.nn.functional, the exact forms against what they claim, the derivation of every bound tests/test_head_text_gpu.py holds
the kernels of csrc/head_loss.hip and csrc/attn_text.hip to, and that each bound is sharp: one plausible wrong variant per
tolerance group, computed on the CPU, misses its bound by at least 10x."""

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import head_text_ref as H
import oracle.losses as OL
from head_text_ref import F32, F64, R, RI

SHARP = 10.0


def close(a, b, tol=1e-12):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max()))


def grads(fn, *xs):
    leaves = [x.double().clone().requires_grad_(True) for x in xs]
    fn(*leaves).backward()
    return [x.grad for x in leaves]


# --------------------------------------------------------------------------- the fp64 forms are the formulas they restate
def test_infonce_is_the_oracle_loss():
    B, K, T = 5, 37, 0.07
    S, pos = torch.tanh(R("t.S", B, K)).double(), torch.tanh(R("t.p", B)).double()
    none = torch.zeros(K, dtype=torch.bool)
    out, _ = H.infonce(S, none, 1.0 / T, 3.0, F64, pos=pos)
    want = lambda p, s: 3.0 * OL.infonce_loss(p[:, None], s, p[:, None], s, T) / 2.0  # noqa: E731  (v + t of the same logits)
    assert close(out["rows"].mean() * 3.0, want(pos, S))
    dpos, dS = grads(want, pos, S)
    assert close(out["dpos"], dpos) and close(out["dS"], dS)
    # masked columns: the oracle on the matrix without them; their gradient is zero
    hit = torch.arange(K) % 3 == 1
    out, _ = H.infonce(S, hit, 1.0 / T, 3.0, F64, pos=pos)
    assert close(out["rows"].mean() * 3.0, want(pos, S[:, ~hit]))
    assert close(out["dS"][:, ~hit], grads(want, pos, S[:, ~hit])[1]) and float(out["dS"][:, hit].abs().max()) == 0.0
    # the queue form: pos = <q, key>, dq0 = dL/dpos * key
    q, key = R("t.q", B, 9).double(), R("t.k", B, 9).double()
    outq, _ = H.infonce(S, hit, 1.0 / T, 3.0, F64, q=q, key=key)
    outp, _ = H.infonce(S, hit, 1.0 / T, 3.0, F64, pos=(q * key).sum(1))
    assert close(outq["rows"], outp["rows"]) and close(outq["dpos"], outp["dpos"][:, None] * key) and close(outq["dS"], outp["dS"])
    # every column masked: the loss row and every gradient are exactly zero
    out, _ = H.infonce(S, ~none, 1.0 / T, 3.0, F64, pos=pos)
    assert all(float(out[k].abs().max()) == 0.0 for k in ("rows", "dS", "dpos"))
    # the segment fold that skips is the plain form
    S2, hit2 = torch.tanh(R("t.S2", 2, 4100)), torch.arange(4100) < 4096
    want2, _ = H.infonce(S2, hit2, 1.0 / T, 1.0, F64, pos=pos[:2])
    assert close(H.infonce_segment_fold(S2, hit2, pos[:2], 1.0 / T, True, F64), want2["rows"])


def test_smooth_ce_is_the_oracle_loss():
    rows, n = 6, 11
    z, y = R("t.z", rows, n).double() * 3, RI("t.y", 0, n, rows)
    for eps in (0.0, 0.1, 0.3):
        out, _ = H.smooth_ce(z, y, eps, 1.0 / rows, F64)
        want = lambda x: OL.label_smooth_ce(x, y, eps)  # noqa: E731
        assert close(out["rows"].mean(), want(z)) and close(out["dlogits"], grads(want, z)[0])
    assert close(H.smooth_ce(z, y, 0.0, 1.0, F64)[0]["rows"], F.cross_entropy(z, y, reduction="none"))


def test_global_align_is_the_oracle_loss():
    B = 7
    v, t, lab = R("t.v", B, 16).double(), R("t.t", B, 16).double(), torch.tensor([0, 1, 0, 2, 2, 2, 5])
    S = F.normalize(v, dim=1) @ F.normalize(t, dim=1).t()
    out, _ = H.global_align_rows(S, lab, 1.0, F64)
    assert close(out["rows"].sum(), OL.global_align_loss(v, t, lab))
    same = H.same_ids(lab)
    want = lambda s: (F.softplus(-10 * (s[same] - 0.6)).sum() + F.softplus(40 * (s[~same] - 0.4)).sum()) * 2.0 / B  # noqa: E731
    assert close(out["dS"], grads(want, S)[0], 1e-8)  # (softplus switches to the identity above 20: 2e-9)


def test_cmpm_rows_is_the_reference_form():
    """losses.py:156-203 with its broadcast quirk (element [i, j] divided by the norm of mask row j) is the per-row form"""
    B = 9
    lab = torch.tensor([3, 1, 3, 3, 4, 1, 7, 4, 3])
    S = R("t.cm", B, B).double() * 4

    def want(s):
        mask = H.same_ids(lab).double()
        qq = mask / mask.norm(dim=1)
        lp = F.log_softmax(s, dim=1)
        return (F.softmax(s, dim=1) * (lp - torch.log(qq + 1e-8))).sum(1).mean()

    out, _ = H.cmpm_rows(S, lab, 1e-8, 1.0 / B, F64)
    assert close(out["rows"].mean(), want(S)) and close(out["dS"], grads(want, S)[0])
    s = S * R("t.rs", B).double()[:, None]
    same = H.same_ids(lab)
    assert close(H.pair_sim_means(S, lab, R("t.rs", B), F64)[0]["means"], torch.stack([s[same].mean(), s[~same].mean()]))
    one = H.pair_sim_means(S[:1, :1], lab[:1], None, F64)[0]["means"]
    assert float(one[0]) == float(S[0, 0]) and bool(torch.isnan(one[1]))


def test_norm_forms_are_normalize():
    x, dy = R("t.x", 6, 13).double(), R("t.dy", 6, 13).double()
    out, _ = H.l2norm(x, F64, dy=dy)
    assert close(out["y"], F.normalize(x, dim=1)) and close(out["inv"], 1.0 / x.norm(dim=1))
    assert close(out["dx"], grads(lambda a: (F.normalize(a, dim=1) * dy).sum(), x)[0])
    zero, _ = H.l2norm(torch.zeros(2, 5), F64, dy=torch.ones(2, 5))
    assert float(zero["y"].abs().max()) == 0.0 and zero["inv"].tolist() == [1e12, 1e12] and close(zero["dx"], torch.full((2, 5), 1e12, dtype=F64))
    p, dpnt = R("t.p", 13, 6).double(), R("t.dp", 6, 13).double()
    out, _ = H.colnorm(p, F64, dpnt=dpnt)
    assert close(out["pnt"], F.normalize(p, dim=0).t()) and close(out["dprojT"].t(), grads(lambda a: (F.normalize(a, dim=0).t() * dpnt).sum(), p)[0])
    v, t, G = R("t.v", 4, 13).double(), R("t.t", 4, 13).double(), R("t.G", 8, 13).double()
    out, _ = H.cross_project(v, t, F64, G=G)

    def X(a, b):  # losses.py:73-82
        an, bn = F.normalize(a, dim=1), F.normalize(b, dim=1)
        return torch.cat([(a * bn).sum(1, keepdim=True) * bn, (b * an).sum(1, keepdim=True) * an])

    assert close(out["X"], X(v, t)) and close(out["dots"], torch.cat([(v * F.normalize(t, dim=1)).sum(1), (t * F.normalize(v, dim=1)).sum(1)]))
    dv, dt = grads(lambda a, b: (X(a, b) * G).sum(), v, t)
    assert close(out["dv"], dv) and close(out["dt"], dt) and close(out["inv"], torch.cat([1 / v.norm(dim=1), 1 / t.norm(dim=1)]))


def test_instance_loss_is_its_parts():
    """colnorm -> (l2norm) -> scale * embed @ pn -> smooth CE is oracle.losses.instance_loss"""
    C, N, B = 12, 7, 5
    p, v, t, lab = R("t.ip", C, N).double(), R("t.iv", B, C).double(), R("t.it", B, C).double(), RI("t.il", 0, N, B)
    pnt = H.colnorm(p, F64)[0]["pnt"]
    e2 = H.l2norm(torch.cat([v, t]), F64)[0]["y"]
    rows = H.smooth_ce(28.0 * e2 @ pnt.t(), torch.cat([lab, lab]), 0.1, 1.0 / B, F64)[0]["rows"]
    assert close(rows.sum() / B, OL.instance_loss(p, v, t, lab, 0.1, scale=28, norm=True))


def test_softmax_tokens_and_small_sums():
    s, dp = R("t.s", 4, 9).double() * 5, R("t.dp", 4, 9).double()
    out, _ = H.softmax(s, F64, dp=dp)
    assert close(out["p"], F.softmax(s, dim=1)) and close(out["ds"], grads(lambda a: (F.softmax(a, dim=1) * dp).sum(), s)[0])
    x, pos, dtok = R("t.tx", 2, 5, 8).double(), R("t.tp", 6, 8).double(), R("t.td", 2, 6, 8).double()
    out, _ = H.tokens(x, pos, F64, dtok=dtok)
    assert close(out["mean"], x.mean(1) + pos[0]) and torch.equal(out["rest"], x + pos[1:])
    assert close(out["dx"], dtok[:, 1:] + dtok[:, :1] / 5) and close(out["dpos"], dtok.sum(0))
    a = R("t.a", 3, 7).double()
    assert close(H.colsum(a, None, F64)[0]["out"], a.sum(0)) and close(H.rowdot(a, a, F64)[0]["out"], (a * a).sum(1))
    assert close(H.sum_(a.reshape(-1), -2.0, torch.tensor([1.0]), F64)[0]["out"], 1.0 - 2.0 * a.sum())
    assert close(H.rowscale_add(a[:, 0], a, a, F64)[0]["dx"], (a[:, :1] * a + a).reshape(-1))
    g = torch.tensor([2.0, -1.0, 0.5])
    assert close(H.axpby3(a, a * a, None, g, F64)[0]["out"], 2 * a - a * a) and close(H.axpby3(a, None, a * a, g, F64)[0]["out"], 2 * a + 0.5 * a * a)


def test_measure():
    ref = torch.tensor([[1.0, -4.0], [0.0, 0.0], [1e-3, 0.0]], dtype=F64)
    got = ref + torch.tensor([[4e-6, 0.0], [0.0, 0.0], [0.0, 1e-9]], dtype=F64)
    assert H.measure(got, ref) == pytest.approx(1e-6) and H.measure(got, ref, "rows") == pytest.approx(1e-6)
    assert H.measure(got, ref, "max", 8.0) == pytest.approx(5e-7) and H.measure(got, ref, "rows", torch.tensor([0.0, 0.0, 1.0])) == pytest.approx(1e-6)
    got[1, 1] = 1e-30  # a row that must be met exactly
    assert H.measure(got, ref, "rows") == H.INF and H.measure(got, ref, "rows", torch.tensor([0.0, 1.0, 0.0])) < 1e-5
    nan = torch.tensor([1.0, float("nan")])
    assert H.measure(nan, nan) == 0.0 and H.measure(torch.tensor([1.0, 2.0]), nan) == H.INF and H.measure(nan, torch.tensor([1.0, 2.0])) == H.INF
    assert H.measure(torch.zeros(3), torch.zeros(3)) == 0.0 and H.measure(torch.full((3,), 1e-30), torch.zeros(3)) == H.INF


# --------------------------------------------------------------------------- the exact forms do what they say
def test_exact_forms():
    # argmax: the lowest index wins a tie; an all-equal and an all -inf row answer 0
    x = torch.tensor([[1.0, 5.0, 5.0, 2.0], [3.0, 3.0, 3.0, 3.0], [-H.INF] * 4, [0.0, 1.0, 2.0, 9.0]])
    assert H.argmax_rows(x).tolist() == [1, 0, 0, 3]
    # gather: ids below 0 read row 0, ids from vocab on read the last row; the columns L.. of `tokens` are not read
    table = torch.arange(12.0).reshape(4, 3)
    tok = torch.tensor([[-1, 4, 9, 2], [1, 0, 3, 2]])
    assert torch.equal(H.gather(table, tok, 3), table[torch.tensor([[0, 3, 3], [1, 0, 3]])])
    # hit mask: two ids that differ only in their upper 32 bits do not hit
    queue = torch.tensor([5, 5 + (1 << 32), -5, (-5) + (1 << 40), 6])
    assert H.hit_mask(queue, torch.tensor([5, -5])).tolist() == [1, 0, 1, 0, 0]
    assert H.hit_mask(queue, torch.tensor([5 + (1 << 32)])).tolist() == [0, 1, 0, 0, 0]
    # relu_bwd: zero and minus zero pass nothing
    assert H.relu_bwd(torch.tensor([1.0, 2.0, 3.0, 4.0]), torch.tensor([0.0, -0.0, 1e-30, -1.0])).tolist() == [0.0, 0.0, 3.0, 0.0]
    assert torch.equal(H.padded(torch.ones(2, 3), 5, 7.5), torch.tensor([[1, 1, 1, 7.5, 7.5]] * 2))


def test_embedding_bwd_is_a_sequential_fp32_sum():
    """the first position of a token owns the row, later positions are added ascending: an order fp32 can tell from another"""
    dX = torch.tensor([[1.0], [2.0 ** -24], [2.0 ** -24], [9.0], [5.0]])
    tok = torch.tensor([[2, 2, 2, 0, 7, 99]])  # position 3 is the pad token, 4 is out of range, column 5 is beyond L
    got = H.embedding_bwd(dX, tok, 5, 4)
    assert got.shape == (4, 1) and got[2, 0] == 1.0 and float(got.abs().sum()) == 1.0  # ((1 + 2^-24) + 2^-24 = 1 in fp32; 1 + 2^-23 otherwise)
    assert H.embedding_bwd(dX.flip(0), torch.tensor([[7, 0, 2, 2, 2]]), 5, 4)[2, 0] == np.float32(1.0 + 2.0 ** -23)
    for case in H.EMB_BWD_CASES:
        for kind in ("mixed", "one", "pad"):
            d, t = H.emb_bwd_inputs(*case, kind=kind)
            B, L, E, vocab = case
            got = H.embedding_bwd(d, t, L, vocab)
            live = (t.reshape(-1) > 0) & (t.reshape(-1) < vocab)
            want = torch.zeros(vocab, E, dtype=F64).index_add_(0, t.reshape(-1)[live], d.double()[live])
            assert H.measure(got, want, "max", float(d.abs().max())) < 1e-5, (case, kind)
            assert kind != "pad" or float(got.abs().max()) == 0.0
            assert float(got[0].abs().max()) == 0.0


# --------------------------------------------------------------------------- where the bounds come from
@pytest.mark.parametrize("group", sorted(H.GROUP_RUNS))
def test_yardsticks(group):
    """TOL[group] = 4 x the worst error of the fp32 evaluation of the group's formula against fp64 over the very runs of the GPU
    test (recorded within [4, 4.2] x), and the recorded yardstick is that worst error to 2.5 %"""
    worst = H.yardstick(H.GROUP_RUNS[group]())
    print("fp32 yardstick %-9s %.3e   recorded %.3e   TOL %.2e" % (group, worst, H.YARDSTICK[group], H.TOL[group]))
    assert abs(worst - H.YARDSTICK[group]) <= 0.025 * H.YARDSTICK[group], (group, worst)
    assert 4.0 * H.YARDSTICK[group] <= H.TOL[group] <= 4.2 * H.YARDSTICK[group], group
    assert 4.0 * worst <= H.TOL[group] <= 4.2 * worst, (group, worst)


def test_every_bound_has_a_yardstick():
    assert sorted(H.TOL) == sorted(H.YARDSTICK) == sorted(H.GROUP_RUNS)
    assert (H.GEMM_VALUE, H.GEMM_GRAD) == (1e-5, 1e-4)


# --------------------------------------------------------------------------- the bounds are sharp
def first(runs, word):
    return next(r for r in runs if word in r.name)


def excess(group, got, run):
    """how far outputs computed some other way miss the group's bound on a run of the group (1: at the bound)"""
    want, spec = H.ref_of(run)
    e = H.compare({k: got[k] for k in want if k in got}, {k: want[k] for k in want if k in got}, spec) / H.TOL[group]
    print("sharpness %-9s %-50s %.1f x the bound" % (group, run.name, e))
    return e


def test_sharp_softmax_padding_in_the_sum():
    run = first(H.runs_softmax(), "3x5 ld8 scale1")
    assert excess("softmax", H.softmax(n_sum=8, dtype=F64, **run.kw)[0], run) > SHARP


@pytest.mark.parametrize("group,amp", [("infonce", "|S|<=1"), ("infonce5", "|S|<=5")])
def test_sharp_infonce_masked_columns_left_in(group, amp):
    for form in ("rows", "queue C260"):
        run = first((r for r in H.GROUP_RUNS[group]() if "every7" in r.name and "K8197" in r.name and amp in r.name), form)
        assert excess(group, H.infonce(masked=False, dtype=F64, **run.kw)[0], run) > SHARP


def test_sharp_infonce_masked_segment_folded_in():
    """a running fold that does not skip the all-masked first segment: exp(-inf - -inf) * 0 = NaN in every row"""
    run = first((r for r in H.GROUP_RUNS["infonce"]() if "seg0" in r.name and "K8197" in r.name), "rows")
    kw = {k: run.kw[k] for k in ("S", "hit", "pos", "invT")}
    good, bad = H.infonce_segment_fold(skip=True, **kw), H.infonce_segment_fold(skip=False, **kw)
    assert excess("infonce", dict(rows=good), run) <= 1.0
    assert bool(torch.isnan(bad).all()) and excess("infonce", dict(rows=bad), run) > SHARP


@pytest.mark.parametrize("group", ["ce", "ce28"])
def test_sharp_smooth_ce_without_the_uniform_term(group):
    run = first(H.GROUP_RUNS[group](), "2x11003")
    assert excess(group, H.smooth_ce(uniform_term=False, dtype=F64, **run.kw)[0], run) > SHARP


def test_sharp_cmpm_count_over_the_batch():
    run = first(H.runs_cmpm(), "B65 ld68 ids dup")
    assert excess("cmpm", H.cmpm_rows(count_per_row=False, dtype=F64, **run.kw)[0], run) > SHARP


def test_sharp_align_thresholds_swapped():
    run = first(H.runs_align(), "B5 ld8 ids dup")
    assert excess("align", H.global_align_rows(alpha=0.4, beta=0.6, dtype=F64, **run.kw)[0], run) > SHARP


def test_sharp_colnorm_rows_instead_of_columns():
    run = first(H.runs_colnorm(), "65x70")
    assert excess("norm", dict(pnt=H.colnorm_rows_instead(run.kw["proj"])), run) > SHARP


def test_sharp_sum_without_its_last_trip():
    """a 256-wide sum that stops at the last full trip loses one element of 257"""
    run = first(H.runs_sum(), "sum n257")
    assert excess("sum", dict(out=run.kw["x"][:256].double().sum().reshape(1)), run) > SHARP


def test_sharp_axpby3_without_its_third_term():
    run = first(H.runs_elem(), "axpby3 n1025 abc")
    assert excess("elem", H.axpby3(third=False, dtype=F64, **run.kw)[0], run) > SHARP


def test_sharp_token_mean_over_ldt():
    run = first(H.runs_tokens(big=False), "2x48x288 ldt52")
    assert excess("tokens", H.tokens(divisor=52, dtype=F64, **run.kw)[0], run) > SHARP


def test_sharp_embedding_sum_losing_its_second_chunk():
    """(4, 130, 8, 3) with one token everywhere: 519 adds over three chunks of 256 positions.  Without the second chunk the sum
    is not the sequential one - and not by a rounding: by more than 10 x 2^-24 of it"""
    d, t = H.emb_bwd_inputs(4, 130, 8, 3, kind="one")
    good, bad = H.embedding_bwd(d, t, 130, 3), H.embedding_bwd(d, t, 130, 3, lose_second_chunk=True)
    assert not torch.equal(good, bad) and H.measure(bad, good, "max", float(d.abs().max())) > SHARP * 2.0 ** -24
