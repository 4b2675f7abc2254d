"""GPU tests of the baseline path: cmpm_loss / cmpc_loss / global_align_loss_from_sim against the vectors captured
from the reference (tests/golden/losses_extra.npz) and against an fp64 restatement at full size, the simple head's
trajectory against tests/golden/simple_head.npz, and the engine (eager / captured step, inference, do_train) on a
model built from the baseline configs' keys.

Tolerances are the project's: loss kernels at fixture size as test_model_gpu.test_losses holds instance / global_align
(value 1e-5, gradients 1e-4, max-abs over the reference's max-abs); trajectories and full-size cases the flat 1e-3 of
test_model_gpu.TOL."""

import math
import os
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import oracle.fill as OF  # noqa: E402
import oracle.visual as OV  # noqa: E402
from oracle.fill import digest, digest_err, grad_floor  # noqa: E402

TOL = 1e-3        # tests/test_model_gpu.py:19
TOL_VALUE = 1e-5  # test_model_gpu.test_losses: loss values at fixture size
TOL_GRAD = 1e-4   # ... and their gradients


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import textreid_amd  # noqa: F401

    return torch.device("cuda")


@pytest.fixture(scope="module", autouse=True)
def stream_state_left_as_found():
    """This module is the first of the suite to record a step and to open side streams.  Two pieces of torch's process-wide
    state move with that: `torch.cuda.graph.default_capture_stream` (made on the first capture, kept for the process) and the
    round-robin position of the 32-stream pool `torch.cuda.Stream()` hands out from.  A later test that forks from the capture
    stream to a fresh pool stream gets a real fork only while the two are different pool entries, so both are put back: the
    capture stream to what it was, the pool position by drawing the remainder of a whole round."""
    if not torch.cuda.is_available():
        yield
        return
    made = [0]
    orig_new = torch.cuda.Stream.__new__
    had_capture_stream = torch.cuda.graph.default_capture_stream

    def counting_new(cls, *a, **kw):
        if not ({"stream_ptr", "stream_id"} & set(kw)):  # (ExternalStream and re-wrapped ids draw nothing from the pool)
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
        print("stream pool: %d drawn by this module, %d to complete the round" % (made[0], -made[0] % 32))


def rel(a, b):
    a = torch.as_tensor(a).detach().double().cpu()
    b = torch.as_tensor(b).detach().double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def same_scalar(a, b, tol):
    """rel() for 0-d figures that may be NaN on both sides (the mean over an empty set of pairs)."""
    a, b = float(torch.as_tensor(a)), float(torch.as_tensor(b))
    if math.isnan(a) or math.isnan(b):
        return math.isnan(a) and math.isnan(b)
    return abs(a - b) <= tol * max(abs(b), 1e-30) or (b == 0.0 and a == 0.0)


def load(golden_dir, name):
    return np.load(os.path.join(golden_dir, name))


# --------------------------------------------------------------------------- 6: fixture-size losses
@pytest.mark.parametrize("pattern", ["dup", "distinct", "equal"])
@pytest.mark.parametrize("B", [16, 13])
def test_new_losses_against_reference_vectors(gpu, golden_dir, B, pattern):
    """Values, gradients and `verbose` figures of the three losses against the reference's own (fp32) results.  The upstream
    gradient is 2 (`(loss * 2).backward()`), so the stored gradients are compared doubled: the device-side scaling is on the path."""
    from textreid_amd import losses as L

    g = load(golden_dir, "losses_extra.npz")
    tag = "b%d_%s:" % (B, pattern)
    v0, t0, sim0 = (torch.from_numpy(g["b%d:%s" % (B, k)]).to(gpu) for k in ("v", "t", "sim"))
    p0 = torch.from_numpy(g["proj"]).to(gpu)
    lab = torch.from_numpy(g[tag + "labels"]).to(gpu)
    errs = {}

    v, t = (x.clone().requires_grad_(True) for x in (v0, t0))
    loss = L.cmpm_loss(v, t, lab)
    (loss * 2.0).backward()
    errs["cmpm"] = (rel(loss, g[tag + "cmpm"]), TOL_VALUE)
    errs["cmpm_dv"] = (rel(v.grad, 2.0 * g[tag + "cmpm_dv"]), TOL_GRAD)
    errs["cmpm_dt"] = (rel(t.grad, 2.0 * g[tag + "cmpm_dt"]), TOL_GRAD)
    lv, pos, neg = L.cmpm_loss(v0, t0, lab, verbose=True)
    assert torch.equal(lv, loss.detach()) and pos.dim() == 0 and not pos.requires_grad and pos.is_cuda
    assert same_scalar(pos, g[tag + "cmpm_pos"], 1e-4) and same_scalar(neg, g[tag + "cmpm_neg"], 1e-4), (float(pos), float(neg))

    p, v, t = (x.clone().requires_grad_(True) for x in (p0, v0, t0))
    loss = L.cmpc_loss(p, v, t, lab)
    (loss * 2.0).backward()
    errs["cmpc"] = (rel(loss, g[tag + "cmpc"]), TOL_VALUE)
    errs["cmpc_dproj"] = (rel(p.grad, 2.0 * g[tag + "cmpc_dproj"]), TOL_GRAD)
    errs["cmpc_dv"] = (rel(v.grad, 2.0 * g[tag + "cmpc_dv"]), TOL_GRAD)
    errs["cmpc_dt"] = (rel(t.grad, 2.0 * g[tag + "cmpc_dt"]), TOL_GRAD)
    lv, ip, tp = L.cmpc_loss(p0, v0, t0, lab, verbose=True)
    assert torch.equal(lv, loss.detach()) and ip.dim() == 0 and not ip.requires_grad
    assert float(ip) == float(g[tag + "cmpc_iprec"]) and float(tp) == float(g[tag + "cmpc_tprec"])

    for name, kw in (("gafs", {}), ("gafs_args", dict(alpha=0.5, beta=0.3, scale_pos=8, scale_neg=20))):
        sim = sim0.clone().requires_grad_(True)
        keep = sim.detach().clone()
        loss = L.global_align_loss_from_sim(sim, lab, **kw)
        (loss * 2.0).backward()
        assert torch.equal(sim.detach(), keep)  # the caller's matrix is not modified
        errs[name] = (rel(loss, g[tag + name]), TOL_VALUE)
        errs[name + "_dsim"] = (rel(sim.grad, 2.0 * g[tag + name + "_dsim"]), TOL_GRAD)

    # global_align_loss_from_sim(cosine of v, t) is global_align_loss(v, t)
    cos = F.normalize(v0, dim=1) @ F.normalize(t0, dim=1).t()
    errs["gafs_vs_global_align"] = (rel(L.global_align_loss_from_sim(cos, lab), L.global_align_loss(v0, t0, lab)), TOL_VALUE)
    print({k: "%.1e" % e for k, (e, _) in errs.items()})
    bad = {k: e for k, (e, tol) in errs.items() if not e < tol}
    assert not bad, bad


def test_argmax_rows_ties_take_the_lowest_index(gpu):
    from textreid_amd import ops

    x = OF.randn("amax:x", (37, 1003), 0).to(gpu)
    x[3, 700] = x[3, 20] = 9.0   # a tie across workgroup lanes: index 20 wins
    x[5, 999] = x[5, 1000] = 8.0
    ld = 1008
    xp = torch.zeros(37, ld, device=gpu)
    xp[:, :1003] = x
    xp[:, 1003:] = 100.0  # padding columns are not candidates
    labels = torch.argmax(x, dim=1)
    labels[0] = (labels[0] + 1) % 1003
    idx = torch.empty(37, dtype=torch.int64, device=gpu)
    hit = torch.empty(37, device=gpu)
    ops.call("trid_argmax_rows_f32", ops._p(xp), ops._p(labels), ops._p(idx), ops._p(hit), 37, 1003, ld, ops.stream())
    assert torch.equal(idx, torch.argmax(x, dim=1)) and int(idx[3]) == 20 and int(idx[5]) == 999
    assert hit.tolist() == [0.0] + [1.0] * 36


# --------------------------------------------------------------------------- 7: full size, fp64 restatement
def cmpm_fp64(v, t, lab, eps=1e-8):
    """losses.py:156-203 restated: A = v t^^T, Bm = t v^^T, q = same-id mask over its row norm,
    mean_i sum_j p_ij (log p_ij - log(q_ij + eps)) for both; cosine means over the same-id / other pairs."""
    mask = lab[:, None] == lab[None, :]
    q = mask.double() / mask.double().norm(dim=1, keepdim=True)
    vn, tn = F.normalize(v, dim=1), F.normalize(t, dim=1)
    loss = 0.0
    for S in (v @ tn.t(), t @ vn.t()):
        lp = F.log_softmax(S, dim=1)
        loss = loss + (lp.exp() * (lp - torch.log(q + eps))).sum(dim=1).mean()
    cos = vn @ tn.t()
    return loss, cos[mask].mean(), cos[~mask].mean()


def cmpc_fp64(proj, v, t, lab):
    """losses.py:65-99 restated: each embedding projected onto the other modality's unit vector, logits against the
    column-normalised projection, mean cross entropy summed over the two; arg-max precision of both."""
    vn, tn, pn = F.normalize(v, dim=1), F.normalize(t, dim=1), F.normalize(proj, dim=0)
    il = ((v * tn).sum(dim=1, keepdim=True) * tn) @ pn
    tl = ((t * vn).sum(dim=1, keepdim=True) * vn) @ pn
    loss = F.cross_entropy(il, lab) + F.cross_entropy(tl, lab)
    return loss, (il.argmax(dim=1) == lab).double().mean(), (tl.argmax(dim=1) == lab).double().mean()


def gafs_fp64(sim, lab, alpha=0.6, beta=0.4, sp=10, sn=40):
    """losses.py:131-153 restated: softplus terms of the same-id / other pairs, x2 / B."""
    mask = lab[:, None] == lab[None, :]
    return (F.softplus(-sp * (sim[mask] - alpha)).sum() + F.softplus(sn * (sim[~mask] - beta)).sum()) * 2.0 / lab.shape[0]


@pytest.mark.parametrize("B", [128, 130])
def test_new_losses_full_size_against_fp64(gpu, B):
    """B = 128 and the padding path B = 130, C = 256, NC = 11003, ids in groups of four (the sampler's IMS_PER_ID), against the
    fp64 restatement above, flat 1e-3 (not tightened).  Measured worst errors on an MI355X: 8.8e-7 at B = 128 (cmpc_dproj), 2.3e-6 at
    B = 130 (cmpm_neg, the mean of ~17 k cosines that nearly cancel); every other quantity below 1.2e-6."""
    from textreid_amd import losses as L

    C, NC = 256, 11003
    v0 = OF.randn("full:v%d" % B, (B, C), 1, 0.5)
    t0 = OF.randn("full:t%d" % B, (B, C), 1, 0.5) + 0.5 * v0  # correlated pairs, as trained embeddings are
    p0 = OF.randn("full:p", (C, NC), 1, 0.05)
    lab = (torch.arange(B) // 4) * 7 % NC
    p0.index_add_(1, lab, (F.normalize(v0, dim=1) + F.normalize(t0, dim=1)).t() * 0.5)  # some rows classify correctly: the precisions are not 0
    sim0 = torch.tanh(OF.randn("full:s%d" % B, (B, B), 1, 0.5))
    errs = {}

    ref = [x.double().requires_grad_(True) for x in (v0, t0)]
    want, wpos, wneg = cmpm_fp64(*ref, lab)
    (want * 2.0).backward()
    v, t = (x.to(gpu).requires_grad_(True) for x in (v0, t0))
    got, pos, neg = L.cmpm_loss(v, t, lab.to(gpu), verbose=True)
    (got * 2.0).backward()
    errs.update(cmpm=rel(got, want), cmpm_dv=rel(v.grad, ref[0].grad), cmpm_dt=rel(t.grad, ref[1].grad), cmpm_pos=rel(pos, wpos), cmpm_neg=rel(neg, wneg))

    ref = [x.double().requires_grad_(True) for x in (p0, v0, t0)]
    want, wip, wtp = cmpc_fp64(*ref, lab)
    (want * 2.0).backward()
    p, v, t = (x.to(gpu).requires_grad_(True) for x in (p0, v0, t0))
    got, ip, tp = L.cmpc_loss(p, v, t, lab.to(gpu), verbose=True)
    (got * 2.0).backward()
    errs.update(cmpc=rel(got, want), cmpc_dproj=rel(p.grad, ref[0].grad), cmpc_dv=rel(v.grad, ref[1].grad), cmpc_dt=rel(t.grad, ref[2].grad))
    assert 0.0 < float(wip) and 0.0 < float(wtp)
    errs.update(cmpc_iprec=rel(ip, wip), cmpc_tprec=rel(tp, wtp))

    ref = sim0.double().requires_grad_(True)
    want = gafs_fp64(ref, lab)
    (want * 2.0).backward()
    sim = sim0.to(gpu).requires_grad_(True)
    got = L.global_align_loss_from_sim(sim, lab.to(gpu))
    (got * 2.0).backward()
    errs.update(gafs=rel(got, want), gafs_dsim=rel(sim.grad, ref.grad))
    print("B=%d" % B, {k: "%.1e" % e for k, e in errs.items()})
    bad = {k: e for k, e in errs.items() if not e < TOL}
    assert not bad, bad


# --------------------------------------------------------------------------- 8: simple-head trajectory
def fixture_model(g, gpu):
    """The model of simple_head.npz (tiny visual spec + small BiGRU + simple head) in its `margin`-filled start state."""
    from textreid_amd.backbones.gru import GRU
    from textreid_amd.backbones.m_resnet import ModifiedResNet
    from textreid_amd.embeddings import build_embed
    from textreid_amd.model import Model

    ns = types.SimpleNamespace
    hidden, embed, vocab, Lpad, C, NC, B, seed = (int(x) for x in g["dims"][:8])
    spec = OV.TINY
    m = Model.__new__(Model)
    torch.nn.Module.__init__(m)
    m.visual_model = ModifiedResNet(list(spec.layers), spec.output_dim, spec.heads, spec.last_stride, (spec.height, spec.in_width), spec.width)
    m.textual_model = GRU(hidden, embed, embed, 1, 0.0, True, "clip_vit", "./", vocab_dict=OF.randn("vocab_table_base", (vocab, embed), seed, 0.5))
    cfg = ns(MODEL=ns(EMBEDDING=ns(EMBED_HEAD="simple", FEATURE_SIZE=C, EPSILON=0.1), NUM_CLASSES=NC))
    m.embed_model = build_embed(cfg, m.visual_model.out_channels, m.textual_model.out_channels)
    m.embed_type = "normal"
    m._text_stream = None
    m.load_state_dict(OF.fill_state(m.state_dict(), seed, "base.", style="margin"))
    return m.to(gpu).train()


def swap_in_cmpm_cmpc(model):
    """The one-line edit of the loss evaluator (simple_head/loss.py): {cmpm_loss, cmpc_loss} for the default pair."""
    from textreid_amd import losses as L
    from textreid_amd.caption import CaptionBatch

    ev = model.embed_model.loss_evaluator

    def forward(visual_embed, textual_embed, captions):
        labels = CaptionBatch.from_list(captions).ids.long()
        return {"cmpm_loss": L.cmpm_loss(visual_embed, textual_embed, labels),
                "cmpc_loss": L.cmpc_loss(ev.projection, visual_embed, textual_embed, labels)}

    ev.forward = forward
    return model


def run_trajectory(g, gpu, steps, swap):
    from textreid_amd.caption import CaptionBatch

    hidden, embed, vocab, Lpad, C, NC, B, seed = (int(x) for x in g["dims"][:8])
    lr, mom, wd = (float(x) for x in g["sgd"])
    spec = OV.TINY
    model = fixture_model(g, gpu)
    if swap:
        swap_in_cmpm_cmpc(model)
    groups = [{"params": [p], "lr": 2 * lr if "bias" in k else lr, "weight_decay": 0.0 if "bias" in k else wd}
              for k, p in model.named_parameters() if p.requires_grad]
    opt = torch.optim.SGD(groups, lr=lr, momentum=mom)
    losses, g0 = {}, {}
    for s in range(steps):
        x = OF.randn("img:base%d" % s, (B, 3, spec.height, spec.in_width), seed).to(gpu)
        tok, ln, ids = (torch.from_numpy(g["%s%d" % (k, s)]).to(gpu) for k in ("tokens", "lengths", "ids"))
        cb = CaptionBatch(tok, ln, ids)
        ld = model(x, cb)
        opt.zero_grad()
        sum(ld.values()).backward()
        if s == 0:
            g0 = {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}
        opt.step()
        for k in ld:
            losses["loss%d:%s" % (s, k)] = ld[k].detach()
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    model.eval()
    with torch.no_grad():
        ev = model(x, cb)
    return losses, g0, sd, ev


def test_simple_head_three_steps(gpu, golden_dir):
    """Tiny encoders + simple head wired as the model's "normal" branch, three SGD steps with the reference's per-tensor groups:
    losses per step, EVERY step-0 gradient (digests under the grad_floor rule) and seven full ones, the ENTIRE state after the
    last step (parameters and BatchNorm running statistics) and the eval embeddings against the reference-captured trajectory."""
    from fixture_check import assert_within, head_errors

    g = load(golden_dir, "simple_head.npz")
    steps = int(g["dims"][8])
    losses, g0, sd, ev = run_trajectory(g, gpu, steps, swap=False)
    assert set(losses) == {k for k in g.files if k.startswith("loss")}
    assert set("gdig0:" + k for k in g0) == {k for k in g.files if k.startswith("gdig0:")}  # every trainable tensor has a gradient
    assert any("running_mean" in k for k in g.files if k.startswith("fdig:"))
    assert ev[0].shape == g["eval_v"].shape and ev[1].shape == g["eval_t"].shape
    errs = head_errors(g, losses, lambda k: g0[k], sd, ev)
    worst = sorted(errs.items(), key=lambda kv: -kv[1])[:5]
    print(len(errs), "quantities; worst:", [(k, "%.1e" % v) for k, v in worst])
    assert_within(errs, TOL, exact=())


def test_simple_head_with_cmpm_cmpc_swapped_in(gpu, golden_dir):
    """The same model with the loss evaluator's dict switched to {cmpm_loss, cmpc_loss}: two steps against the second
    trajectory of the fixture - losses, every step-0 gradient digest, the whole final state."""
    g = load(golden_dir, "simple_head.npz")
    steps = int(g["dims"][9])
    losses, g0, sd, _ = run_trajectory(g, gpu, steps, swap=True)
    keys = [k[5:] for k in g.files if k.startswith("swap:")]
    gfl = grad_floor([g["swap:" + k] for k in keys if k.startswith("gdig0:")])
    errs = {}
    for k in keys:
        ref = g["swap:" + k]
        if k.startswith("loss"):
            errs[k] = rel(losses[k], ref)
        elif k.startswith("gdig0:"):
            errs[k] = digest_err(digest("grad0:" + k[6:], g0[k[6:]]), ref, gfl * (100.0 if k.endswith("attnpool.k_proj.bias") else 1.0))
        elif k.startswith("fdig:"):
            errs[k] = digest_err(digest("final:" + k[5:], sd[k[5:]]), ref)
    assert sorted(k for k in errs if k.startswith("loss")) == sorted("loss%d:%s" % (s, n) for s in range(steps) for n in ("cmpm_loss", "cmpc_loss"))
    assert len(errs) == len(keys)
    worst = sorted(errs.items(), key=lambda kv: -kv[1])[:5]
    print(len(errs), "quantities; worst:", [(k, "%.1e" % v) for k, v in worst])
    bad = {k: v for k, v in errs.items() if not v <= TOL}
    assert not bad, sorted(bad.items(), key=lambda kv: -kv[1])[:8]


# --------------------------------------------------------------------------- 9-11: the step
def baseline_model(gpu, visual="m_resnet50", vocab=3000, seed=0):
    from textreid_amd.config import baseline_cfg
    from textreid_amd.model import build_model

    torch.manual_seed(seed)
    cfg = baseline_cfg(visual)
    table = torch.randn(vocab, 512, generator=torch.Generator().manual_seed(1)) * 0.02
    return cfg, build_model(cfg, vocab_dict=table).to(gpu).train()


def test_baseline_step_is_deterministic(gpu):
    """Two runs of the baseline step from the same state give the same bits - losses and the whole state: the text
    encoder's side stream is joined before anything reads its output, and nothing on the path uses atomics."""
    import bench
    from textreid_amd.caption import CaptionBatch
    from textreid_amd.solver import make_optimizer

    outs = []
    for _ in range(2):
        cfg, model = baseline_model(gpu)
        opt = make_optimizer(cfg, model)
        losses = []
        for s in range(3):
            images, tokens, lengths, ids = bench.synth_batch(8, s, gpu, 3, vocab=3000)
            ld = model(images, CaptionBatch(tokens, lengths, ids, max_len=64))
            opt.zero_grad()
            sum(ld.values()).backward()
            opt.step()
            losses.append(torch.stack([v.detach() for v in ld.values()]))
        outs.append((torch.stack(losses), {k: v.detach().clone() for k, v in model.state_dict().items()}))
        assert sorted(ld) == ["global_align_loss", "instance_loss"]
    assert torch.equal(outs[0][0], outs[1][0]) and bool(torch.isfinite(outs[0][0]).all())
    for k, v in outs[0][1].items():
        assert torch.equal(v, outs[1][1][k]), k


@pytest.mark.parametrize("swap", [False, True], ids=["default_losses", "cmpm_cmpc"])
def test_captured_baseline_step_equals_eager_bitwise(gpu, swap):
    """engine.graph.CapturedTrainStep on the baseline model (forward on two streams, the two losses, backward, FusedAdam with a
    learning-rate change in mid-run): both replay forms give the SAME BITS as the eager step - losses every step, every parameter,
    moment and BatchNorm buffer at the end.  Once with the default losses, once with cmpm / cmpc swapped in."""
    import bench
    from textreid_amd.caption import CaptionBatch
    from textreid_amd.engine.graph import CapturedTrainStep
    from textreid_amd.solver import make_optimizer

    B, steps = 8, 6
    batches = [bench.synth_batch(B, s, gpu, 5, vocab=3000) for s in range(steps)]
    runs = {}
    for mode in ("eager", "graph", "streams"):
        cfg, model = baseline_model(gpu)
        if swap:
            swap_in_cmpm_cmpc(model)
        opt = make_optimizer(cfg, model)
        assert len(opt.param_groups) == len([p for p in model.parameters() if p.requires_grad])
        runner = CapturedTrainStep(model, opt, warmup=2, caption_bound=64, launch="graph" if mode == "eager" else mode)
        losses = []
        for i in range(steps):
            images, tokens, lengths, ids = batches[i]
            cb = CaptionBatch(tokens, lengths, ids % 11003, max_len=64)
            if i == 4:  # an LR scheduler step between two training steps
                for grp in opt.param_groups:
                    grp["lr"] *= 0.5
            ld = runner._eager(images, cb) if mode == "eager" else runner(images, cb)
            losses.append(torch.stack([v.detach().clone() for v in ld.values()]))
        torch.cuda.synchronize()
        if mode != "eager":
            assert runner.graph is not None and not runner.disabled and runner.recaptures == 0
        if mode == "streams":
            assert runner.replayer is not None and runner.replay_info["kernels"] == runner.replay_info["nodes"] > 200
        runs[mode] = (torch.stack(losses), {k: v.detach().clone() for k, v in model.state_dict().items()},
                      [opt.state[p]["exp_avg_sq"].clone() for g_ in opt.param_groups for p in g_["params"]])
        del model, opt, runner
    assert bool(torch.isfinite(runs["eager"][0]).all())
    for other in ("graph", "streams"):
        assert torch.equal(runs["eager"][0], runs[other][0]), (other, (runs["eager"][0] - runs[other][0]).abs().max())
        for k, v in runs["eager"][1].items():
            assert torch.equal(v, runs[other][1][k]), (other, k)
        for a, b in zip(runs["eager"][2], runs[other][2]):
            assert torch.equal(a, b), other


@pytest.mark.parametrize("swap", [False, True], ids=["default_losses", "cmpm_cmpc"])
def test_baseline_train_step_has_no_host_device_sync(gpu, swap):
    """After warm-up a whole baseline step - encoders, embed layers, losses, backward, FusedAdam - does not synchronise the host with
    the device (torch's sync debug mode raises on any blocking copy / .item()); with cmpm / cmpc swapped in as well."""
    import bench
    from textreid_amd.caption import CaptionBatch
    from textreid_amd.solver import make_optimizer

    cfg, model = baseline_model(gpu, vocab=49408)
    if swap:
        swap_in_cmpm_cmpc(model)
    opt = make_optimizer(cfg, model)
    batches = [bench.synth_batch(8, s, gpu, 5) for s in range(2)]

    def step(i):
        images, tokens, lengths, ids = batches[i % 2]
        cb = CaptionBatch(tokens, lengths, ids % 11003, max_len=64)
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


# --------------------------------------------------------------------------- 12: do_train + inference
def test_do_train_baseline_plumbing(gpu, tmp_path):
    """A baseline config on the GPU box: 256 synthetic 384x128 images + 64-token captions, ONE epoch (2 steps at bs128) of
    engine.trainer.do_train (the bucketed captured step) + the per-epoch evaluation through engine.inference: losses finite, R@1
    returned and finite, a checkpoint written that loads back through checkpoint.py; each distinct image encoded once."""
    import bench
    from textreid_amd.caption import CaptionBatch
    from textreid_amd.checkpoint import load_checkpoint_file
    from textreid_amd.engine.inference import compute_on_dataset, inference
    from textreid_amd.engine.trainer import do_train
    from textreid_amd.solver import FusedAdam, make_lr_scheduler, make_optimizer

    B, N = 128, 256
    cfg, model = baseline_model(gpu, vocab=49408)
    opt = make_optimizer(cfg, model)
    assert isinstance(opt, FusedAdam) and len(opt.param_groups) == len([n for n, p in model.named_parameters() if p.requires_grad])
    sched = make_lr_scheduler(cfg, opt)
    batches = [bench.synth_batch(B, s, "cpu", 3) for s in range(N // B)]

    class TrainLoader:
        def __len__(self):
            return len(batches)

        def __iter__(self):
            for im, tk, ln, ids in batches:
                yield im, CaptionBatch(tk, ln, ids, max_len=64), None

    vn = 32
    vim, vtk, vln, vids = bench.synth_batch(vn, 9, "cpu", 4)

    class ValDS:
        def get_id_info(self, idx):
            return idx // 2, int(vids[idx])

        def __len__(self):
            return vn

    class ValLoader:
        dataset = ValDS()

        def __iter__(self):
            for s in range(0, vn, 16):
                idx = list(range(s, s + 16))
                yield vim[[i // 2 * 2 for i in idx]], CaptionBatch(vtk[idx], vln[idx]), idx

    class Checkpointer:
        saved = []

        def save(self, name, **kw):
            path = os.path.join(str(tmp_path), name + ".pth")
            torch.save(dict(model=model.state_dict(), **kw), path)
            self.saved.append(path)

    seen = []

    class Meters:
        def update(self, **kw):
            seen.append(kw)

        def __str__(self):
            return str(seen[-1])

    args = {"max_epoch": 1, "epoch": 0, "iteration": 0}
    ck = Checkpointer()
    do_train(model, TrainLoader(), [ValLoader()], opt, sched, ck, Meters(), gpu, checkpoint_period=1, evaluate_period=1,
             arguments=args, log_period=1)
    steps_seen = [kw for kw in seen if "loss" in kw]
    assert args["iteration"] == 2 and args["epoch"] == 1 and len(steps_seen) == 2
    assert all(sorted(kw) == ["global_align_loss", "instance_loss", "loss"] for kw in steps_seen)
    assert any("top1" in kw for kw in seen)
    assert all(np.isfinite(v) for kw in seen for v in kw.values())
    assert any(p.endswith("epoch_1.pth") for p in ck.saved) and all(os.path.getsize(p) > 0 for p in ck.saved)
    # image de-duplication: 32 captions over 16 distinct images, coalesced into one encoder pass
    assert compute_on_dataset.last_stats == {"images_encoded": vn // 2, "samples": vn, "encoder_passes": 1}
    top1 = inference(model, ValLoader(), device=gpu, save_data=False, rerank=False)
    assert np.isfinite(float(top1))
    a = compute_on_dataset(model, ValLoader(), gpu, dedupe=True)
    b = compute_on_dataset(model, ValLoader(), gpu, dedupe=False)
    assert compute_on_dataset.last_stats["images_encoded"] == vn
    for i in range(vn):
        assert torch.allclose(a[i][0], b[i][0], rtol=1e-5, atol=1e-6) and torch.equal(a[i][1], b[i][1])
    # the written checkpoint is a baseline state dict and loads back through checkpoint.py
    _, fresh = baseline_model(gpu, vocab=49408, seed=7)
    rest = load_checkpoint_file(fresh, next(p for p in ck.saved if p.endswith("epoch_1.pth")))
    assert rest["epoch"] == 1
    for k, v in model.state_dict().items():
        assert torch.equal(v, fresh.state_dict()[k]), k


# --------------------------------------------------------------------------- 13: full-size smoke
@pytest.mark.parametrize("visual", ["m_resnet50", "m_resnet101"])
def test_baseline_full_size_smoke(gpu, visual):
    """What the shipped baseline configs ask for: m_resnet50 / m_resnet101, 384x128, B = 8, FEATURE_SIZE 256, NUM_CLASSES 11003:
    one training step with finite losses and a finite gradient on EVERY trainable tensor, eval output [8,256] x 2."""
    import bench
    from textreid_amd.caption import CaptionBatch

    cfg, model = baseline_model(gpu, visual=visual)
    assert cfg.MODEL.EMBEDDING.FEATURE_SIZE == 256 and cfg.MODEL.NUM_CLASSES == 11003
    images, tokens, lengths, ids = bench.synth_batch(8, 0, gpu, 3, vocab=3000)
    cb = CaptionBatch(tokens, lengths, ids, max_len=64)
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
