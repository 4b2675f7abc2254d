"""GPU: the fused multi-tensor SGD (csrc/optim.hip trid_sgd_multi_f32, solver.FusedSGD; lib/solver/build.py:19-22) against
torch.optim.SGD and an fp64 run of it, against the reference-made golden trajectories, and on the recorded train step
(engine.graph) - single process and data parallel."""

import os
import socket
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

import oracle.fill as OF  # noqa: E402
import oracle.head as OH  # noqa: E402
import oracle.visual as OV  # noqa: E402

TOL = 1e-3  # tests/test_model_gpu.py:19, tests/test_baseline_gpu.py:25


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import textreid_amd  # noqa: F401

    return torch.device("cuda")


# --------------------------------------------------------------------------- the kernel against torch.optim.SGD
SHAPES = [(64, 32, 3, 3), (128,), (1000, 17), (5,), (1,), (70001,)]
LATE = 3  # this parameter has no gradient on steps 0-1: its first-update rule fires at step 2


def _params(gpu):
    """The six shapes (the first in channels_last; 70001 = two full chunks of the kernel's 32768 and a ragged tail that is no
    multiple of four) and a parameter whose storage is 4-byte but not 16-byte aligned (the kernel's scalar path)."""
    ps = [torch.nn.Parameter(torch.randn(s, device=gpu)) for s in SHAPES]
    ps[0].data = ps[0].data.contiguous(memory_format=torch.channels_last)
    ps.append(torch.nn.Parameter(torch.randn(4100, device=gpu)[1:]))
    assert ps[-1].data_ptr() % 16 == 4 and ps[0].data_ptr() % 16 == 0
    return ps


def _groups(ps):
    # lr and weight decay alternate between 0 and 4e-2, out of step with each other: all four combinations occur
    return [{"params": [p], "lr": 4e-2 if i % 2 == 0 else 0.0, "weight_decay": 4e-2 if (i // 2) % 2 == 0 else 0.0} for i, p in enumerate(ps)]


@pytest.mark.parametrize("momentum,dampening,nesterov", [(0.9, 0, False), (0.9, 0.1, False), (0.9, 0, True), (0, 0, False)])
def test_fused_sgd_matches_torch_sgd(gpu, momentum, dampening, nesterov):
    """Six steps of FusedSGD, torch.optim.SGD (fp32, same device) and torch.optim.SGD in fp64 on the CPU over the same fp32 inputs.
    (a) a group with weight_decay == 0 at dampening == 0: the momentum buffer is torch's, bit for bit, after every step (its two
    IEEE operations are the same: buf * momentum, + g); with momentum == 0 no state entry exists.
    (b) parameters and the remaining buffers: FusedSGD's worst error against the fp64 run (relative to the tensor's max-abs) is at
    most twice torch-fp32's own worst error plus one fp32 ulp - the only legal difference is whether g + wd*w and w - lr*u were
    contracted on either side, one rounding each."""
    from textreid_amd.solver import FusedSGD

    torch.manual_seed(0)
    pf = _params(gpu)
    pt = [torch.nn.Parameter(p.detach().clone(memory_format=torch.preserve_format)) for p in pf]
    pd = [torch.nn.Parameter(p.detach().double().cpu()) for p in pf]
    kw = dict(lr=4e-2, momentum=momentum, dampening=dampening, nesterov=nesterov)
    of, ot, od = FusedSGD(_groups(pf), **kw), torch.optim.SGD(_groups(pt), **kw), torch.optim.SGD(_groups(pd), **kw)
    exact = [i for i, g in enumerate(of.param_groups) if g["weight_decay"] == 0.0] if dampening == 0 else []
    assert momentum == 0 or dampening != 0 or len(exact) >= 3
    worst_f = worst_t = 0.0

    def err(x, truth):
        truth = truth.detach()
        return float((x.detach().double().cpu() - truth).abs().max() / truth.abs().max().clamp_min(1e-300))

    for it in range(6):
        for i, (a, b, c) in enumerate(zip(pf, pt, pd)):
            if i == LATE and it < 2:
                a.grad = b.grad = c.grad = None
                continue
            gr = torch.randn(4100, device=gpu)[1:] if i == len(pf) - 1 else torch.randn_like(b)
            a.grad, b.grad, c.grad = gr, gr.clone(), gr.double().cpu()
        of.step()
        ot.step()
        od.step()
        for i, (a, b, c) in enumerate(zip(pf, pt, pd)):
            worst_f, worst_t = max(worst_f, err(a, c)), max(worst_t, err(b, c))
            if momentum == 0:
                assert a not in of.state
                continue
            if i == LATE and it < 2:
                assert "momentum_buffer" not in of.state.get(a, {})
                continue
            bf, bt, bd = (o.state[p]["momentum_buffer"] for o, p in ((of, a), (ot, b), (od, c)))
            if i in exact:
                assert torch.equal(bf, bt), (it, i, float((bf - bt).abs().max()))
            else:
                worst_f, worst_t = max(worst_f, err(bf, bd)), max(worst_t, err(bt, bd))
        if it == 2:
            for grp in of.param_groups + ot.param_groups + od.param_groups:
                grp["lr"] *= 0.1  # an LR scheduler changes the per-group lr after step 3
    print("worst error against fp64: FusedSGD %.3e, torch.optim.SGD fp32 %.3e" % (worst_f, worst_t))
    assert worst_t > 0.0
    assert worst_f <= 2.0 * worst_t + 2.0 ** -23, "FusedSGD %.3e vs torch.optim.SGD fp32 %.3e against the fp64 run" % (worst_f, worst_t)


def test_fused_sgd_resume_from_state_dict(gpu):
    """Resume flow of the reference (train_net.py:69-72: build the optimiser, then Checkpointer.resume ->
    optimizer.load_state_dict): a state-dict round trip into a FusedSGD that has ALREADY stepped (stale pointer tables, stale
    buffers) continues exactly as the uninterrupted run does."""
    from textreid_amd.solver import FusedSGD

    torch.manual_seed(1)
    shapes = [(33, 17), (64,), (8, 4, 3, 3), (40000,)]
    base = [torch.randn(s, device=gpu) for s in shapes]
    grads = [[torch.randn(s, device=gpu) for s in shapes] for _ in range(6)]
    mk = lambda: [torch.nn.Parameter(b.clone()) for b in base]
    new = lambda ps: FusedSGD([{"params": [p], "weight_decay": 1e-2 * (i % 2)} for i, p in enumerate(ps)], lr=1e-2, momentum=0.9, dampening=0.1)

    def run(opt, ps, its):
        for it in its:
            for p, g in zip(ps, grads[it]):
                p.grad = g.clone()
            opt.step()

    whole_p = mk()
    whole = new(whole_p)
    run(whole, whole_p, range(6))
    first_p = mk()
    first = new(first_p)
    run(first, first_p, range(3))
    saved = first.state_dict()
    second_p = mk()
    second = new(second_p)
    run(second, second_p, [5])       # a step BEFORE loading: its pointer tables and buffers must not survive the load
    for p, q in zip(second_p, first_p):
        p.data.copy_(q.data)
    second.load_state_dict(saved)
    run(second, second_p, range(3, 6))
    for a, b in zip(second_p, whole_p):
        assert torch.equal(a.detach(), b.detach())
        assert torch.equal(second.state[a]["momentum_buffer"], whole.state[b]["momentum_buffer"])


def test_argument_errors_are_reported(gpu):
    from textreid_amd import ops

    t = torch.zeros(8, dtype=torch.int64, device=gpu)
    p, s = ops._p(t), ops.stream()
    for args in ((None, p, p, p, p, p, p, p, p, p, 1, 4, 0.9, 0, s),   # null table
                 (p, p, p, p, p, p, p, p, p, p, 0, 4, 0.9, 0, s),      # no chunks
                 (p, p, p, p, p, p, p, p, p, p, 1, 0, 0.9, 0, s),      # empty chunk
                 (p, p, p, p, p, p, p, p, p, p, 1, 6, 0.9, 0, s),      # chunk_len % 4 != 0
                 (p, p, None, p, p, p, p, p, p, p, 1, 4, 0.9, 1, s)):  # nesterov without buffers
        with pytest.raises(RuntimeError, match="trid_sgd_multi_f32"):
            ops.call("trid_sgd_multi_f32", *args)
    torch.cuda.synchronize()


# --------------------------------------------------------------------------- golden trajectories (reference-made, SGD)
def _sgd_groups(named, lr, wd):
    return [{"params": [p], "lr": 2 * lr if "bias" in k else lr, "weight_decay": 0.0 if "bias" in k else wd} for k, p in named if p.requires_grad]


def test_moco_head_three_steps_with_fused_sgd(gpu, golden_dir):
    """tests/test_model_gpu.py::test_moco_head_three_steps[head.npz] with FusedSGD in torch.optim.SGD's place: the same groups, lr
    and momentum, the same flat 1e-3 bound on everything the reference-captured trajectory pins."""
    from fixture_check import assert_within, head_errors
    from textreid_amd.backbones.gru import GRU
    from textreid_amd.backbones.m_resnet import ModifiedResNet
    from textreid_amd.caption import CaptionBatch
    from textreid_amd.embeddings.moco_head.head import MoCoHead
    from textreid_amd.solver import FusedSGD

    ns = types.SimpleNamespace
    g = np.load(os.path.join(golden_dir, "head.npz"))
    hidden, embed, vocab, Lpad, C, K, NC, B, seed, steps = (int(v) for v in g["dims"])
    lr, mom, wd = (float(v) for v in g["sgd"])
    spec = OV.TINY
    table = OF.randn("vocab_table_head", (vocab, embed), seed, 0.5)
    vis = ModifiedResNet(list(spec.layers), spec.output_dim, spec.heads, spec.last_stride, (spec.height, spec.in_width), spec.width)
    txt = GRU(hidden, embed, embed, 1, 0.0, True, "clip_vit", "./", vocab_dict=table)
    cfg = ns(MODEL=ns(EMBEDDING=ns(FEATURE_SIZE=C, EPSILON=0.1), MOCO=ns(K=K, M=float(g["m"]), FC=False), NUM_CLASSES=NC))
    head = MoCoHead(cfg, vis, txt)
    filled = OF.fill_state(head.state_dict(), seed, "head.", style="margin")
    st = {k: torch.zeros(tuple(s), dtype=torch.int64) if k in ("id_queue", "queue_ptr") else torch.zeros(tuple(s))
          for k, s in OH.state_shapes(spec, K, C, NC, hidden, embed).items() if k in ("t_queue", "v_queue", "id_queue", "queue_ptr")}
    OH.init_queues(st, seed)
    filled.update(st)
    head.load_state_dict(filled)
    head.to(gpu).train()
    opt = FusedSGD(_sgd_groups(head.named_parameters(), lr, wd), lr=lr, momentum=mom)
    losses, g0 = {}, {}
    for s in range(steps):
        x, tok, ln, ids = (torch.from_numpy(g["%s%d" % (k, s)]).to(gpu) for k in ("images", "tokens", "lengths", "ids"))
        cb = CaptionBatch(tok, ln, ids)
        ld = head(x, cb)
        opt.zero_grad()
        sum(ld.values()).backward()
        if s == 0:
            g0 = {k: p.grad.clone() for k, p in head.named_parameters() if p.grad is not None}
        opt.step()
        for k in ld:
            losses["loss%d:%s" % (s, k)] = ld[k].detach()
    sd2 = head.state_dict()
    head.eval()
    with torch.no_grad():
        ev = head(x, cb)
    errs = head_errors(g, losses, lambda k: g0[k], sd2, ev)
    print(len(errs), "quantities; worst:", [(k, "%.1e" % v) for k, v in sorted(errs.items(), key=lambda kv: -kv[1])[:5]])
    assert_within(errs, TOL)


def test_simple_head_three_steps_with_fused_sgd(gpu, golden_dir):
    """tests/test_baseline_gpu.py::test_simple_head_three_steps with FusedSGD in torch.optim.SGD's place, same bound."""
    import test_baseline_gpu as TB
    from fixture_check import assert_within, head_errors
    from textreid_amd.caption import CaptionBatch
    from textreid_amd.solver import FusedSGD

    g = np.load(os.path.join(golden_dir, "simple_head.npz"))
    hidden, embed, vocab, Lpad, C, NC, B, seed = (int(x) for x in g["dims"][:8])
    steps = int(g["dims"][8])
    lr, mom, wd = (float(x) for x in g["sgd"])
    spec = OV.TINY
    model = TB.fixture_model(g, gpu)
    opt = FusedSGD(_sgd_groups(model.named_parameters(), lr, wd), lr=lr, momentum=mom)
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
    assert set(losses) == {k for k in g.files if k.startswith("loss")}
    errs = head_errors(g, losses, lambda k: g0[k], sd, ev)
    print(len(errs), "quantities; worst:", [(k, "%.1e" % v) for k, v in sorted(errs.items(), key=lambda kv: -kv[1])[:5]])
    assert_within(errs, TOL, exact=())


# --------------------------------------------------------------------------- the recorded step
def _model(kind, gpu):
    if kind == "baseline":
        import test_baseline_gpu as TB

        cfg, model = TB.baseline_model(gpu)
    else:
        from textreid_amd.config import moco_cfg
        from textreid_amd.model import build_model

        torch.manual_seed(0)
        cfg = moco_cfg("m_resnet50", K=64)
        table = torch.randn(3000, 512, generator=torch.Generator().manual_seed(1)) * 0.02
        model = build_model(cfg, vocab_dict=table).to(gpu).train()
    cfg.SOLVER.OPTIMIZER = "SGD"
    return cfg, model


def _momentum_buffers(opt):
    return [opt.state[p]["momentum_buffer"].clone() for g_ in opt.param_groups for p in g_["params"]]


@pytest.mark.parametrize("kind", ["moco", "baseline"])
def test_captured_sgd_step_equals_eager_bitwise(gpu, kind):
    """engine.graph.CapturedTrainStep with make_optimizer's FusedSGD: five steps (two eager warm-ups, the recording, two replays;
    the scheduler changes the learning rates between steps 3 and 4) through both replay forms give the SAME BITS as five eager
    steps - losses, every parameter and buffer, every momentum buffer - and the runner did record."""
    import bench
    from textreid_amd.caption import CaptionBatch
    from textreid_amd.engine.graph import CapturedTrainStep
    from textreid_amd.solver import FusedSGD, make_optimizer

    B, steps = 8, 5
    batches = [bench.synth_batch(B, s, gpu, 5, vocab=3000) for s in range(steps)]
    runs = {}
    for mode in ("eager", "graph", "streams"):
        cfg, model = _model(kind, gpu)
        opt = make_optimizer(cfg, model)
        assert isinstance(opt, FusedSGD) and len(opt.param_groups) == len([p for p in model.parameters() if p.requires_grad])
        runner = CapturedTrainStep(model, opt, warmup=2, caption_bound=64, launch="graph" if mode == "eager" else mode)
        losses = []
        for i in range(steps):
            images, tokens, lengths, ids = batches[i]
            cb = CaptionBatch(tokens, lengths, ids % 11003, max_len=64)
            if i == 3:  # an LR scheduler step between steps 3 and 4
                for grp in opt.param_groups:
                    grp["lr"] *= 0.5
            ld = runner._eager(images, cb) if mode == "eager" else runner(images, cb)
            losses.append(torch.stack([v.detach().clone() for v in ld.values()]))
        torch.cuda.synchronize()
        if mode != "eager":
            assert runner.graph is not None and not runner.disabled and runner.recaptures == 0 and runner.calls == steps
            assert runner.plan is opt._plan
        if mode == "streams":
            assert runner.replayer is not None and runner.replay_info["kernels"] == runner.replay_info["nodes"] > 200
        runs[mode] = (torch.stack(losses), {k: v.detach().clone() for k, v in model.state_dict().items()}, _momentum_buffers(opt))
        del model, opt, runner
    assert bool(torch.isfinite(runs["eager"][0]).all())
    assert len(runs["eager"][2]) > 50 and all(bool(b.abs().max() > 0) for b in runs["eager"][2][:4])
    for other in ("graph", "streams"):
        assert torch.equal(runs["eager"][0], runs[other][0]), (other, (runs["eager"][0] - runs[other][0]).abs().max())
        for k, v in runs["eager"][1].items():
            assert torch.equal(v, runs[other][1][k]), (other, k)
        for a, b in zip(runs["eager"][2], runs[other][2]):
            assert torch.equal(a, b), other


def test_captured_step_refuses_an_optimizer_without_the_protocol(gpu):
    """An optimizer that does not implement prepare_capture / finish_capture / advance_for_replay is refused by the recording
    (absorbed as a failed capture: the run stays eager, loudly) - never recorded with its launches left out."""
    import bench
    from textreid_amd.caption import CaptionBatch
    from textreid_amd.engine.graph import CapturedTrainStep, implements_capture_protocol
    from textreid_amd.solver import make_optimizer

    cfg, model = _model("baseline", gpu)
    opt = make_optimizer(cfg, model, fused=False)
    assert type(opt) is torch.optim.SGD and not implements_capture_protocol(opt) and implements_capture_protocol(make_optimizer(cfg, model))
    runner = CapturedTrainStep(model, opt, warmup=1, caption_bound=64)
    images, tokens, lengths, ids = bench.synth_batch(8, 0, gpu, 5, vocab=3000)
    cb = CaptionBatch(tokens, lengths, ids % 11003, max_len=64)
    with pytest.raises(RuntimeError, match="needs textreid_amd.solver.FusedAdam"):
        runner._capture(images, cb)


def test_do_train_records_the_sgd_step(gpu, monkeypatch):
    """engine.trainer.do_train with an SGD config: the step goes through engine.graph.BucketedTrainStep (two eager steps, the
    recording, replays) and ends on the bits of the eager loop (capture=False)."""
    import bench
    from textreid_amd.caption import CaptionBatch
    from textreid_amd.engine import graph as G
    from textreid_amd.engine.trainer import do_train
    from textreid_amd.solver import FusedSGD, make_lr_scheduler, make_optimizer

    batches = [bench.synth_batch(8, s, "cpu", 5, vocab=3000) for s in range(2)]

    class Loader:
        def __len__(self):
            return len(batches)

        def __iter__(self):
            for im, tk, ln, ids in batches:
                yield im, CaptionBatch(tk, ln, ids % 11003, max_len=64), None

    built = []
    real = G.BucketedTrainStep

    class Spy(real):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            built.append(self)

    monkeypatch.setattr(G, "BucketedTrainStep", Spy)
    finals = {}
    for capture in (True, False):
        cfg, model = _model("moco", gpu)
        opt = make_optimizer(cfg, model)
        assert isinstance(opt, FusedSGD)
        sched = make_lr_scheduler(cfg, opt)  # (linear warm-up: another learning rate in each of the three epochs)
        do_train(model, Loader(), None, opt, sched, None, None, gpu, checkpoint_period=10, evaluate_period=10,
                 arguments={"max_epoch": 3, "epoch": 0, "iteration": 0}, capture=capture)
        torch.cuda.synchronize()
        finals[capture] = ({k: v.detach().clone() for k, v in model.state_dict().items()}, _momentum_buffers(opt), [g["lr"] for g in opt.param_groups])
        if capture:
            assert len(built) == 1 and built[0].optimizer is opt
            assert built[0].recorded == {64: 64} and built[0].last.calls == 6 and not built[0].last.disabled
        del model, opt
    assert len(built) == 1  # capture=False built none
    assert finals[True][2] == finals[False][2]
    for k, v in finals[False][0].items():
        assert torch.equal(v, finals[True][0][k]), k
    for a, b in zip(finals[False][1], finals[True][1]):
        assert torch.equal(a, b)


@pytest.mark.parametrize("kind", ["moco", "baseline"])
def test_sgd_train_step_has_no_host_device_sync(gpu, kind):
    """After warm-up a whole SGD step - encoders, losses, backward, FusedSGD - does not synchronise the host with the device
    (torch's sync debug mode raises on any blocking copy / .item()): the eager step, then the recorded one."""
    import bench
    from textreid_amd.caption import CaptionBatch
    from textreid_amd.engine.graph import CapturedTrainStep
    from textreid_amd.solver import make_optimizer

    cfg, model = _model(kind, gpu)
    opt = make_optimizer(cfg, model)
    runner = CapturedTrainStep(model, opt, warmup=3, caption_bound=64)
    batches = [bench.synth_batch(8, s, gpu, 5, vocab=3000) for s in range(2)]

    def step(i):
        images, tokens, lengths, ids = batches[i % 2]
        return sum(runner(images, CaptionBatch(tokens, lengths, ids % 11003, max_len=64)).values())

    step(0)
    step(1)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        last = step(2)  # the third warm-up call: an eager step
        assert runner.graph is None
    finally:
        torch.cuda.set_sync_debug_mode("default")
    step(3)  # (the recording itself synchronises, by design)
    step(4)
    assert runner.graph is not None and not runner.disabled
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        last = last + step(5)
        last = last + step(6)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert bool(torch.isfinite(last))


# --------------------------------------------------------------------------- data parallel
def test_dp_sgd_step_recorded_with_its_rccl_collectives():
    """The data-parallel SGD step on the segmented replay (a one-rank `nccl` group with TRID_DP_FORCE=1 drives every collective):
    five steps equal five eager data-parallel steps bit for bit (tests/dp_sgd_worker.py), in a fresh child under its own timeout."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ, RANK="0", WORLD_SIZE="1", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), OMP_NUM_THREADS="8",
               HSA_ENABLE_IPC_MODE_LEGACY="0", TRID_DIST_BACKEND="nccl", TRID_DP_FORCE="1")
    p = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.join(ROOT, "tests", "dp_sgd_worker.py")], env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-3000:]
    assert "DP_SGD_CAPTURED_OK backend=nccl world=1" in p.stdout, p.stdout[-3000:]
    print([ln for ln in p.stdout.splitlines() if ln.startswith("DP_SGD")])
