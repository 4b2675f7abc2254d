"""Stacked BiGRU text encoder on the GPU (MODEL.GRU.NUM_LAYER > 1 with inter-layer dropout; reference
lib/models/backbones/gru.py:36-43): the sequence-emitting / sequence-gradient GRU steps (csrc/gru_step.hip), the
Philox dropout pass (csrc/dropout_seq.hip) and the whole recorded train step, against vectors captured from the
reference module (tests/golden/text_stack.npz) and the fp64 restatement of tests/gru_stack_ref.py."""

import os
import types

import numpy as np
import pytest
import torch

import gru_stack_ref as GS
import oracle.fill as OF

pytestmark = pytest.mark.gpu

TOL = 1e-3        # tests/test_model_gpu.py's gate against the reference's own fp32 vectors
PER_LAYER = 2e-5  # what the one-layer tests hold the encoder to against fp64 (test_fused_gru_step_vs_oracle); layer errors add


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


class fused_setting:
    def __init__(self, value):
        self.value = value

    def __enter__(self):
        from textreid_amd.backbones import gru as G

        self.old, G.FUSED_GRU_STEP = G.FUSED_GRU_STEP, self.value

    def __exit__(self, *a):
        from textreid_amd.backbones import gru as G

        G.FUSED_GRU_STEP = self.old


def table_encoder(tag, H, E, layers, p, vocab=40):
    """frozen-table form; parameters from oracle.fill names -> (module on the CPU, table, fp64 state)"""
    from textreid_amd.backbones.gru import GRU

    table = OF.randn("gs:table:" + tag, (vocab, E), 1, 0.5)
    m = GRU(H, E, E, layers, p, True, "clip_vit", "./", vocab_dict=table)
    with torch.no_grad():
        for k, p_ in m.named_parameters():
            p_.copy_(OF.randn("gs:%s:%s" % (tag, k), tuple(p_.shape), 2, 1.5 / p_.shape[1] ** 0.5))
    st = {k: p_.detach().double().clone().requires_grad_(True) for k, p_ in m.named_parameters()}
    return m, table, st


def ragged(tag, B, L, vocab=40):
    lengths = OF.randint("gs:len:" + tag, 1, L + 1, (B,), 3)
    lengths[0] = L
    if B > 1:
        lengths[-1] = 1
    return OF.randint("gs:tok:" + tag, 0, vocab, (B, L), 4), lengths


def run_gpu(m, cb, gout):
    for p_ in m.parameters():
        p_.grad = None
    y = m(cb)
    (y * gout).sum().backward()
    return y.detach().clone(), {k: p_.grad.clone() for k, p_ in m.named_parameters()}


# --------------------------------------------------------------------------- 1. the reference's own vectors
@pytest.mark.parametrize("layers", [2, 3])
def test_stacked_encoder_golden(gpu, golden_dir, layers):
    from textreid_amd.backbones.gru import GRU
    from textreid_amd.caption import CaptionBatch

    g = np.load(os.path.join(golden_dir, "text_stack.npz"))
    seed, rs = int(g["seed"]), int(g["row_stride"])
    hidden, embed, vocab, L = (int(v) for v in g["dims"])
    m = GRU(hidden, vocab, embed, layers, 0.0, True, "yes", "./")
    m.load_state_dict(OF.fill_state(m.state_dict(), seed, "stack%d." % layers))
    m.to(gpu)
    cb = CaptionBatch(torch.from_numpy(g["tokens"]).to(gpu), torch.from_numpy(g["lengths"]).to(gpu))
    gout = OF.randn("gout:stack", (cb.tokens.shape[0], 2 * hidden), seed).to(gpu)
    y, grads = run_gpu(m, cb, gout)
    y_again, grads_again = run_gpu(m, cb, gout)
    errs = {"out": rel(y, g["out_l%d" % layers])}
    for k, gr in grads.items():
        errs["grad:" + k] = rel(gr[::rs] if k.startswith("gru.") else gr, g["grad_l%d:%s" % (layers, k)])
        assert torch.equal(gr, grads_again[k]), k  # run to run bit-identical
    assert torch.equal(y, y_again)
    assert set(grads) == {"embed.weight"} | set(GS.gru_keys(layers))
    m.eval()
    with torch.no_grad():
        cb2 = CaptionBatch(torch.from_numpy(g["tokens2"]).to(gpu), torch.from_numpy(g["lengths2"]).to(gpu))
        errs["out2"] = rel(m(cb2), g["out2_l%d" % layers])
    print("golden, %d layers:" % layers, {k: "%.1e" % v for k, v in errs.items()})
    bad = {k: v for k, v in errs.items() if not v < TOL}
    assert not bad, bad


# --------------------------------------------------------------------------- 2. fp64 restatement at other sizes
CASES = [(5, 64, 48, 7, 2), (1, 32, 32, 1, 2), (33, 96, 64, 5, 3), (17, 768, 64, 3, 2), (130, 512, 512, 4, 2)]


def untied_upstream(tag, st, table, tokens, lengths, layers, masks=None, p=0.0):
    """Upstream gradient with zeros at the units whose two largest LAST-layer steps are closer than 1e-4 (their arg-max,
    and with it the whole chain below, is undetermined in fp32), as test_fused_gru_step_vs_oracle does -> (gout, share excluded)"""
    B, L = tokens.shape
    gout = OF.randn("gs:gout:" + tag, (B, st["gru.weight_hh_l0"].shape[1] * 2), 5)
    share = 0.0
    if L > 1:
        with torch.no_grad():
            hs = GS.stack_sequences(st, GS.embed_input(st, table.double(), tokens), lengths, layers, masks, p)[-1]
            top = hs.topk(2, dim=1).values
            tie = ((top[:, 0] - top[:, 1]) < 1e-4) & (top[:, 0] != 0)
        gout = gout * (~tie).float()
        share = float(tie.float().mean())
    return gout, share


@pytest.mark.parametrize("B,H,E,L,layers", CASES)
def test_stacked_encoder_vs_fp64_restatement(gpu, B, H, E, L, layers):
    """Batches that are no multiple of the 16-row tile or of the workgroup's 32 rows, L = 1, the largest H of the fused
    step, E != 2H; ragged lengths including 1 and L; fused and unfused steps.  Bound: layers x 2e-5 of each quantity's maximum.
    Measured on MI355X (worst of output and gradients): 1.1e-6 at H = 768 and H = 512, <= 5.2e-7 elsewhere; CHANGELOG.md has the table."""
    from textreid_amd.caption import CaptionBatch

    tag = "c%d_%d_%d_%d_%d" % (B, H, E, L, layers)
    m, table, st = table_encoder(tag, H, E, layers, 0.0)
    tokens, lengths = ragged(tag, B, L)
    gout, share = untied_upstream(tag, st, table, tokens, lengths, layers)
    assert share <= 0.05, share
    yo = GS.stack_forward(st, table.double(), tokens, lengths, layers)
    (yo * gout.double()).sum().backward()
    m.to(gpu).train()
    cb = CaptionBatch(tokens.to(gpu), lengths.to(gpu), max_len=L)
    for fused in (True, False):
        with fused_setting(fused):
            y, grads = run_gpu(m, cb, gout.to(gpu))
            with torch.no_grad():
                y_nograd = m(cb)  # nothing saved (the key encoder)
        errs = {"out": rel(y, yo), "out_nograd": rel(y_nograd, yo)}
        for k, gr in grads.items():
            errs["grad:" + k] = rel(gr, st[k].grad)
        print("stack vs fp64 %s fused=%d excluded %.4f: worst %.1e" % (tag, fused, share, max(errs.values())), {k: "%.1e" % v for k, v in errs.items()})
        bad = {k: v for k, v in errs.items() if not v < layers * PER_LAYER}
        assert not bad, (fused, bad)


# --------------------------------------------------------------------------- 3. padding
@pytest.mark.parametrize("fused", [True, False])
def test_stacked_encoder_padding_does_not_leak(gpu, fused):
    """bound_only batch: the time loop runs to the bound (12) over captions of at most 7 tokens with GARBAGE tokens behind
    each caption's end.  Output and gradients equal the exact-length run to fp32 rounding (the bound changes launch
    shapes only), and the rows t >= length of every intermediate sequence are exactly zero, in both directions."""
    from textreid_amd.caption import CaptionBatch

    B, H, E, bound, top, layers = 9, 64, 48, 12, 7, 3
    m, table, st = table_encoder("pad", H, E, layers, 0.0)
    tokens, lengths = ragged("pad", B, bound)
    lengths = lengths.clamp(max=top)
    lengths[0] = top
    clean = tokens.clone()
    for i, n in enumerate(lengths.tolist()):
        clean[i, n:] = 0
    assert not torch.equal(clean, tokens)
    gout = OF.randn("gs:gout:pad", (B, 2 * H), 5).to(gpu)
    m.to(gpu).train()
    with fused_setting(fused):
        y0, g0 = run_gpu(m, CaptionBatch(clean[:, :top].contiguous().to(gpu), lengths.to(gpu), max_len=top), gout)
        y1, g1 = run_gpu(m, CaptionBatch(tokens.to(gpu), lengths.to(gpu), max_len=bound, bound_only=True), gout)
        seqs = [s.clone() for s in m.last_layer_inputs]
    assert len(seqs) == layers - 1
    dead = (torch.arange(bound).view(1, -1) >= lengths.view(-1, 1)).to(gpu)  # [B, bound]
    for s in seqs:
        assert tuple(s.shape) == (B, bound, 2 * H)
        assert float(s[dead].abs().max()) == 0.0
        assert float(s[~dead].abs().min()) > 0.0
    errs = {"out": rel(y1, y0)}
    for k in g0:
        errs["grad:" + k] = rel(g1[k], g0[k])
    print("padding fused=%d:" % fused, {k: "%.1e" % v for k, v in errs.items()})
    assert all(v <= 1e-5 for v in errs.values()), errs


# --------------------------------------------------------------------------- 4. dropout, given the mask
@pytest.mark.parametrize("layers", [2, 3])
def test_stacked_encoder_dropout_given_the_mask(gpu, layers):
    from textreid_amd.caption import CaptionBatch

    B, H, E, L, p = 9, 64, 48, 6, 0.3
    tag = "drop%d" % layers
    m, table, st = table_encoder(tag, H, E, layers, p)
    m0, _, _ = table_encoder(tag, H, E, layers, 0.0)  # the same weights without dropout
    tokens, lengths = ragged(tag, B, L)
    m.to(gpu).train()
    m0.to(gpu).train()
    cb = CaptionBatch(tokens.to(gpu), lengths.to(gpu), max_len=L)
    for fused in (True, False):
        with fused_setting(fused):
            for p_ in m.parameters():
                p_.grad = None
            y = m(cb)
            masks = m.last_dropout_masks
            assert masks is not None and len(masks) == layers - 1
            assert all(k.dtype == torch.uint8 and tuple(k.shape) == (B, L, 2 * H) for k in masks)
            cpu_masks = [k.cpu() for k in masks]
            for s_ in st.values():
                s_.grad = None
            gout, share = untied_upstream(tag + "f%d" % fused, st, table, tokens, lengths, layers, cpu_masks, p)
            assert share <= 0.05, share
            (y * gout.to(gpu)).sum().backward()
            yo = GS.stack_forward(st, table.double(), tokens, lengths, layers, cpu_masks, p)
            (yo * gout.double()).sum().backward()
            errs = {"out": rel(y, yo)}
            for k, p_ in m.named_parameters():
                errs["grad:" + k] = rel(p_.grad, st[k].grad)
            print("dropout given the mask, %d layers fused=%d:" % (layers, fused), {k: "%.1e" % v for k, v in errs.items()})
            bad = {k: v for k, v in errs.items() if not v < layers * PER_LAYER}
            assert not bad, (fused, bad)
            # eval mode, and the nn.GRU alone in eval mode (what MODEL.FREEZE does): no dropout, the p = 0 result bit for bit
            with torch.no_grad():
                want = m0(cb)
                m.eval()
                got_eval = m(cb)
                assert m.last_dropout_masks is None
                m.train()
                m.gru.eval()
                got_gru_eval = m(cb)
                assert m.last_dropout_masks is None
                m.train()
            assert torch.equal(got_eval, want) and torch.equal(got_gru_eval, want)
            assert not torch.equal(y.detach(), want)


# --------------------------------------------------------------------------- 5. dropout, the generator
def test_dropout_generator_sequences(gpu):
    """Consecutive training forwards draw different masks, each the one the Philox restatement predicts from the device
    state (seed, offset + layer boundary); the same torch.manual_seed before construction reproduces the sequence."""
    from textreid_amd.caption import CaptionBatch

    B, H, E, L, p, layers = 5, 32, 48, 4, 0.3, 3
    tokens, lengths = ragged("gen", B, L)
    runs = []
    for _ in range(2):
        torch.manual_seed(1234)
        m, _, _ = table_encoder("gen", H, E, layers, p)
        m.to(gpu).train()
        cb = CaptionBatch(tokens.to(gpu), lengths.to(gpu), max_len=L)
        seq = []
        for step in range(3):
            with torch.no_grad():
                m(cb)
            seed, offset = (int(v) for v in m._dropout_state.cpu())
            assert offset == (step + 1) * (layers - 1)
            masks = [k.cpu().clone() for k in m.last_dropout_masks]
            for i, k in enumerate(masks):
                want = GS.keep_mask(k.numel(), p, seed, offset - (layers - 1) + i)
                assert np.array_equal(k.numpy().reshape(-1), want), (step, i)
            seq.append(masks)
        assert "_dropout_state" not in m.state_dict() and not any("dropout" in k for k in m.state_dict())
        runs.append(seq)
    flat = [k for seq in runs[0] for k in seq]
    for i in range(len(flat)):
        for j in range(i + 1, len(flat)):
            assert not torch.equal(flat[i], flat[j]), (i, j)
    for a, b in zip(runs[0], runs[1]):
        assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_dropout_keep_rate(gpu):
    """One mask of 128 x 16 x 1024 elements, p = 0.3: every byte 0 or 1; the keep rate within 4 standard deviations of
    1 - p (binomial: sigma = sqrt(p (1 - p) / n) = 3.2e-4), per column (2048 draws: sigma = 1.0e-2) within 5; the output is
    the input times keep / (1 - p); the backward pass applies the same factor."""
    from textreid_amd import ops

    rows, cols, p = 128 * 16, 1024, 0.3
    n = rows * cols
    y = torch.rand(rows, cols, device=gpu) + 0.5
    x = torch.empty_like(y)
    keep = torch.full((rows, cols), 7, dtype=torch.uint8, device=gpu)
    state = torch.tensor([0x1234567812345, 41], dtype=torch.int64).to(gpu)
    ops.call("trid_dropout_seq_fwd_f32", ops._p(y), ops._p(x), ops._p(keep), n, p, ops._p(state), 1, ops.stream())
    ops.call("trid_dropout_advance", ops._p(state), 2, ops.stream())
    assert state.cpu().tolist() == [0x1234567812345, 43]
    assert int(keep.max()) == 1 and int(keep.min()) == 0
    k = keep.double()
    sigma = (p * (1 - p) / n) ** 0.5
    assert abs(float(k.mean()) - (1 - p)) <= 4 * sigma, (float(k.mean()), sigma)
    sigma_col = (p * (1 - p) / rows) ** 0.5
    worst = float((k.mean(dim=0) - (1 - p)).abs().max())
    assert worst <= 5 * sigma_col, (worst, sigma_col)
    assert np.array_equal(keep.cpu().numpy().reshape(-1), GS.keep_mask(n, p, 0x1234567812345, 42))
    scale = float(np.float32(1) / (np.float32(1) - np.float32(p)))  # the launcher's fp32 arithmetic
    assert torch.equal(x, torch.where(keep.bool(), y * scale, torch.zeros_like(y)))
    dx = y.clone()
    ops.call("trid_dropout_seq_bwd_f32", ops._p(dx), ops._p(keep), n, p, ops.stream())
    assert torch.equal(dx, x)
    # a length that is no multiple of four, in place: the partial last group
    y5 = y.reshape(-1)[:4101].clone()
    k5 = torch.full((4104,), 9, dtype=torch.uint8, device=gpu)
    ops.call("trid_dropout_seq_fwd_f32", ops._p(y5), ops._p(y5), ops._p(k5), 4101, p, ops._p(state), 0, ops.stream())
    assert np.array_equal(k5.cpu().numpy()[:4101], GS.keep_mask(4101, p, 0x1234567812345, 43)) and k5[4101:].tolist() == [9, 9, 9]
    assert torch.equal(y5, torch.where(k5[:4101].bool(), y.reshape(-1)[:4101] * scale, torch.zeros_like(y5)))


def test_moco_query_and_key_encoders_have_their_own_generator_state(gpu):
    import oracle.visual as OV
    from textreid_amd.backbones.gru import GRU
    from textreid_amd.backbones.m_resnet import ModifiedResNet
    from textreid_amd.caption import CaptionBatch
    from textreid_amd.embeddings.moco_head.head import MoCoHead

    spec, hidden, embed, vocab, C, K, NC, B = OV.TINY, 64, 64, 200, 32, 32, 53, 8
    ns = types.SimpleNamespace
    torch.manual_seed(3)
    vis = ModifiedResNet(list(spec.layers), spec.output_dim, spec.heads, spec.last_stride, (spec.height, spec.in_width), spec.width)
    txt = GRU(hidden, embed, embed, 2, 0.3, True, "clip_vit", "./", vocab_dict=OF.randn("gs:moco_table", (vocab, embed), 1, 0.5))
    cfg = ns(MODEL=ns(EMBEDDING=ns(FEATURE_SIZE=C, EPSILON=0.1), MOCO=ns(K=K, M=0.9, FC=False), NUM_CLASSES=NC))
    head = MoCoHead(cfg, vis, txt).to(gpu).train()
    x = OF.randn("gs:moco_img", (B, 3, spec.height, spec.in_width), 1).to(gpu)
    tok, ln = ragged("moco", B, 20, vocab)
    ids = torch.arange(B) // 2
    for step in range(2):
        ld = head(x, CaptionBatch(tok.to(gpu), ln.to(gpu), ids.to(gpu)))
        sum(ld.values()).backward()
        q, k = head.t_encoder_q, head.t_encoder_k
        assert q._dropout_state is not None and k._dropout_state is not None
        assert q._dropout_state.data_ptr() != k._dropout_state.data_ptr()
        sq, sk = q._dropout_state.cpu().tolist(), k._dropout_state.cpu().tolist()
        assert sq[1] == sk[1] == step + 1 and sq[0] != sk[0]  # each advanced its own offset; seeds drawn separately
        assert not torch.equal(q.last_dropout_masks[0], k.last_dropout_masks[0])
    assert not any("dropout" in n for n in head.state_dict())


# --------------------------------------------------------------------------- 6. the whole model
def _two_layer_model(gpu, keep_prob, table):
    from textreid_amd.config import moco_cfg
    from textreid_amd.model import build_model
    from textreid_amd.solver import make_optimizer

    cfg = moco_cfg("m_resnet50", K=64)
    cfg.MODEL.GRU.NUM_LAYER = 2
    cfg.MODEL.GRU.DROPOUT_KEEP_PROB = keep_prob
    model = build_model(cfg, vocab_dict=table).to(gpu).train()
    return cfg, model, make_optimizer(cfg, model)


def test_two_layer_model_captured_step_equals_eager_bitwise(gpu):
    """MODEL.GRU.NUM_LAYER = 2 without dropout: four steps through CapturedTrainStep (two eager warm-ups, the recording,
    replays) as hipGraphLaunch and as stream replay equal the eager steps bit for bit - losses, every parameter and buffer
    (queues, key encoders), Adam moments; the key encoder's second-layer weights follow the query encoder's by the EMA."""
    import bench
    from textreid_amd.caption import CaptionBatch
    from textreid_amd.engine.graph import CapturedTrainStep

    B, steps = 8, 4
    table = torch.randn(3000, 512, generator=torch.Generator().manual_seed(1)) * 0.02
    batches = [bench.synth_batch(B, s, gpu, 5, vocab=3000) for s in range(steps)]
    runs = {}
    for mode in ("eager", "graph", "streams"):
        torch.manual_seed(0)
        cfg, model, opt = _two_layer_model(gpu, 1.0, table)
        k0 = model.embed_model.t_encoder_k.gru.weight_ih_l1.detach().clone()
        assert torch.equal(k0, model.embed_model.t_encoder_q.gru.weight_ih_l1)
        runner = CapturedTrainStep(model, opt, warmup=2, caption_bound=64, launch="graph" if mode == "eager" else mode)
        losses = []
        for images, tokens, lengths, ids in batches:
            cb = CaptionBatch(tokens, lengths, ids % 11003, max_len=64)
            ld = runner._eager(images, cb) if mode == "eager" else runner(images, cb)
            losses.append(torch.stack([v.detach().clone() for v in ld.values()]))
        torch.cuda.synchronize()
        if mode != "eager":
            assert runner.graph is not None and not runner.disabled
        if mode == "streams":
            assert runner.replayer is not None
        names = [n for n, _ in model.named_parameters()]
        assert "textual_model.gru.weight_hh_l1_reverse" in names
        kq = model.embed_model.t_encoder_q.gru.weight_ih_l1.detach()
        kk = model.embed_model.t_encoder_k.gru.weight_ih_l1.detach()
        assert not torch.equal(kk, k0) and not torch.equal(kk, kq)  # moved by the EMA, behind the query encoder
        assert model.embed_model.t_encoder_q.last_dropout_masks is None
        runs[mode] = (torch.stack(losses), {k: v.detach().clone() for k, v in model.state_dict().items()},
                      [opt.state[p][m_].clone() for g_ in opt.param_groups for p in g_["params"] for m_ in ("exp_avg", "exp_avg_sq")])
        del model, opt, runner
    for other in ("graph", "streams"):
        assert torch.equal(runs["eager"][0], runs[other][0]), (other, (runs["eager"][0] - runs[other][0]).abs().max())
        for k, v in runs["eager"][1].items():
            assert torch.equal(v, runs[other][1][k]), (other, k)
        for a, b in zip(runs["eager"][2], runs[other][2]):
            assert torch.equal(a, b), other


@pytest.mark.parametrize("launch", ["graph", "streams"])
def test_two_layer_model_replay_draws_fresh_masks(gpu, launch):
    """DROPOUT_KEEP_PROB = 0.7: two replays of ONE recording on the same batch, the model state restored in between, give
    different losses (the mask's offset lives on the device and the recording advances it); a rerun from the same
    torch.manual_seed gives the same two losses."""
    import bench
    from textreid_amd.caption import CaptionBatch
    from textreid_amd.engine.graph import CapturedTrainStep

    table = torch.randn(3000, 512, generator=torch.Generator().manual_seed(1)) * 0.02
    images, tokens, lengths, ids = bench.synth_batch(8, 0, gpu, 5, vocab=3000)
    cb = CaptionBatch(tokens, lengths, ids % 11003, max_len=64)
    outs = []
    for _ in range(2):
        torch.manual_seed(0)
        cfg, model, _ = _two_layer_model(gpu, 0.7, table)
        state = {k: v.clone() for k, v in model.state_dict().items()}
        runner = CapturedTrainStep(model, None, warmup=1, caption_bound=64, launch=launch)
        got = []
        for call in range(3):  # eager warm-up, then the recording's first and second replay
            model.load_state_dict(state)
            ld = runner(images, cb)
            got.append(torch.stack([v.detach().clone() for v in ld.values()]).cpu())
        assert runner.graph is not None and not runner.disabled and runner.calls == 3
        q = model.embed_model.t_encoder_q
        assert int(q._dropout_state[1]) == 3 and q.last_dropout_masks is not None
        assert not torch.equal(got[1], got[2]), got
        outs.append(got)
        del model, runner
    for a, b in zip(outs[0], outs[1]):
        assert torch.equal(a, b), (outs[0], outs[1])
