#!/usr/bin/env python3
"""Generate the baseline fixtures under tests/golden/ from the IMPORTED reference:

  losses_extra.npz   cmpm_loss / cmpc_loss / global_align_loss_from_sim (lib/models/losses.py:65-99,131-203):
                     values, reference-autograd gradients and both `verbose` tuples, for B = 16 and an odd
                     batch (B = 13), each with duplicate, all-distinct and all-equal labels.
  simple_head.npz    tiny visual encoder + small BiGRU + the reference SimpleHead wired as the reference
                     Model.forward wires its "normal" branch: three SGD steps (losses, step-0 gradients, the
                     whole final state, eval embeddings, state-dict names and shapes), and a second, two-step
                     trajectory with the loss evaluator switched to {cmpm_loss, cmpc_loss}.

Runs only where the reference tree is present (read-only); the same three in-process shims as make_golden.py
(restated here: importing that script would run its own imports and shims as a side effect):
  (i)   torch.Tensor.cuda -> identity
  (ii)  lib.models.backbones.gru.load_vocab_dict -> synthetic table from fill()
  (iii) visual model built directly from a spec (no pretrained file)
Weights are NOT stored: both sides fill every tensor from oracle.fill(name, shape, seed).  Fixtures hold arrays
and name lists only.  Every stored fp32 quantity is asserted to lie within 5e-4 of an fp64 evaluation of the same
reference code (a fixture that fails this gets another seed, never another bound).

Usage:  python tests/golden/make_golden_baseline.py
"""

import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
sys.path.insert(0, ROOT)
sys.path.insert(0, REF)

torch.Tensor.cuda = lambda self, *a, **k: self  # shim (i)
torch.set_num_threads(8)

import oracle.fill as OF  # noqa: E402
from oracle.fill import digest, digest_err, grad_floor  # noqa: E402
import oracle.visual as OV  # noqa: E402

import lib.models.backbones.gru as ref_gru  # noqa: E402
import lib.models.backbones.m_resnet as ref_mr  # noqa: E402
import lib.models.losses as ref_losses  # noqa: E402
from lib.models.embeddings.simple_head.head import SimpleHead  # noqa: E402
from lib.utils.caption import Caption  # noqa: E402

COND = 5e-4  # fp32 reference vs fp64 evaluation of the same code
LR, MOMENTUM, WD = 0.02, 0.9, 4e-5


def ns(**kw):
    return types.SimpleNamespace(**kw)


def rel(a, b):
    a, b = torch.as_tensor(a).detach().double(), torch.as_tensor(b).detach().double()
    if a.numel() == 1 and torch.isnan(a).all() and torch.isnan(b).all():
        return 0.0
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def make_captions(tokens, lengths, ids):
    caps = []
    for i in range(tokens.shape[0]):
        c = Caption([tokens[i, : int(lengths[i])].tolist()], max_length=tokens.shape[1])
        c.add_field("id", ids[i].clone())
        caps.append(c)
    return caps


# -------------------------------------------------------------------------- losses
LABEL_PATTERNS = ("dup", "distinct", "equal")


def labels_of(pattern, B, NC, seed):
    if pattern == "distinct":
        return torch.from_numpy(np.random.RandomState(seed).permutation(NC)[:B].astype(np.int64))
    if pattern == "equal":
        return torch.full((B,), 7, dtype=torch.int64)
    lab = OF.randint("x:lab%d" % B, 0, NC, (B,), seed)
    lab[1] = lab[0]
    lab[5] = lab[0]
    lab[B - 1] = lab[2]
    return lab


def eval_losses(v, t, proj, sim, lab):
    """Every stored quantity of one case, in the dtype of the inputs."""
    out = {}
    v, t, proj, sim = (x.clone().requires_grad_(True) for x in (v, t, proj, sim))
    loss, pos, neg = ref_losses.cmpm_loss(v, t, lab, verbose=True)
    assert float(loss.detach()) == float(ref_losses.cmpm_loss(v, t, lab).detach())
    gv, gt = torch.autograd.grad(loss, (v, t))
    out.update(cmpm=loss, cmpm_pos=pos, cmpm_neg=neg, cmpm_dv=gv, cmpm_dt=gt)
    loss, ip, tp = ref_losses.cmpc_loss(proj, v, t, lab, verbose=True)
    gp, gv, gt = torch.autograd.grad(loss, (proj, v, t))
    out.update(cmpc=loss, cmpc_iprec=ip, cmpc_tprec=tp, cmpc_dproj=gp, cmpc_dv=gv, cmpc_dt=gt)
    loss = ref_losses.global_align_loss_from_sim(sim, lab)
    (gs,) = torch.autograd.grad(loss, (sim,))
    out.update(gafs=loss, gafs_dsim=gs)
    loss = ref_losses.global_align_loss_from_sim(sim, lab, alpha=0.5, beta=0.3, scale_pos=8, scale_neg=20)
    (gs,) = torch.autograd.grad(loss, (sim,))
    out.update(gafs_args=loss, gafs_args_dsim=gs)
    return {k: x.detach() for k, x in out.items()}


def gen_losses_extra(seed=21):
    print("[losses_extra]")
    C, NC = 32, 101
    out = {"dims": np.array([C, NC, seed]), "batches": np.array([16, 13]), "patterns": np.array(LABEL_PATTERNS)}
    worst = 0.0
    for B in (16, 13):
        v = OF.randn("x:v%d" % B, (B, C), seed)
        t = OF.randn("x:t%d" % B, (B, C), seed)
        proj = OF.randn("x:p", (C, NC), seed, 0.3)
        sim = torch.tanh(OF.randn("x:sim%d" % B, (B, B), seed, 0.6))  # a similarity matrix that is NOT a cosine of v, t
        for pat in LABEL_PATTERNS:
            tag = "b%d_%s:" % (B, pat)
            lab = labels_of(pat, B, NC, seed)
            r32 = eval_losses(v, t, proj, sim, lab)
            r64 = eval_losses(v.double(), t.double(), proj.double(), sim.double(), lab)
            for k in r32:
                e = rel(r32[k], r64[k])
                worst = max(worst, e)
                assert e < COND, ("losses_extra is not well conditioned: change the seed", tag + k, e)
                out[tag + k] = r32[k].numpy()
            out[tag + "labels"] = lab.numpy()
        out["b%d:v" % B], out["b%d:t" % B], out["b%d:sim" % B] = v.numpy(), t.numpy(), sim.numpy()
    out["proj"] = proj.numpy()
    out["conditioning"] = np.array(worst)
    print("  fp32 vs fp64: worst %.1e" % worst)
    np.savez_compressed(os.path.join(HERE, "losses_extra.npz"), **out)


# -------------------------------------------------------------------------- simple head
class Baseline(torch.nn.Module):
    """The reference Model's "normal" wiring (lib/models/model.py:19-41) around directly built encoders."""

    def __init__(self, vis, txt, head):
        super().__init__()
        self.visual_model, self.textual_model, self.embed_model = vis, txt, head

    def forward(self, images, captions):
        outputs, losses = self.embed_model(self.visual_model(images), self.textual_model(captions), captions)
        return dict(losses) if self.training else outputs


def swap_losses(evaluator):
    """The one-line edit of the loss evaluator: {cmpm_loss, cmpc_loss} instead of the default pair."""

    def forward(visual_embed, textual_embed, captions):
        labels = torch.stack([c.get_field("id") for c in captions]).long()
        return {"cmpm_loss": ref_losses.cmpm_loss(visual_embed, textual_embed, labels),
                "cmpc_loss": ref_losses.cmpc_loss(evaluator.projection, visual_embed, textual_embed, labels)}

    evaluator.forward = forward


def groups(named):
    """lib/solver/build.py:6-18: one group per tensor, bias lr x2 and no weight decay."""
    return [{"params": [p], "lr": 2 * LR if "bias" in k else LR, "weight_decay": 0.0 if "bias" in k else WD}
            for k, p in named if p.requires_grad]


def step_inputs(s, spec, B, vocab, Lpad, seed):
    x = OF.randn("img:base%d" % s, (B, 3, spec.height, spec.in_width), seed)
    lens = [int(v) for v in OF.randint("len:base%d" % s, 3, 30, (B,), seed)]
    tok = OF.randint("tok:base%d" % s, 1, vocab, (B, Lpad), seed)
    for i, n in enumerate(lens):
        tok[i, n:] = 0
    ids = torch.tensor([10 * s + (i // 2) for i in range(B)], dtype=torch.int64)  # duplicates inside the batch
    return x, tok, torch.tensor(lens, dtype=torch.int64), ids


FULL_GRADS = ("embed_model.visual_embed_layer.weight", "embed_model.textual_embed_layer.bias", "embed_model.loss_evaluator.projection",
              "textual_model.gru.weight_hh_l0", "visual_model.conv1.weight", "visual_model.layer2.0.conv2.weight",
              "visual_model.attnpool.c_proj.bias")


def build_reference(spec, dims, table, seed, dt, swap):
    hidden, embed, vocab, Lpad, C, NC, B = dims
    ref_gru.load_vocab_dict = lambda root, onehot: table.numpy()  # shim (ii)
    vis = ref_mr.ModifiedResNet(layers=list(spec.layers), output_dim=spec.output_dim, heads=spec.heads, last_stride=spec.last_stride,
                                input_resolution=(spec.height, spec.in_width), width=spec.width)  # shim (iii)
    txt = ref_gru.GRU(hidden, embed, embed, 1, 0.0, True, "clip_vit", "./")
    cfg = ns(MODEL=ns(EMBEDDING=ns(FEATURE_SIZE=C, EPSILON=0.1), NUM_CLASSES=NC))
    model = Baseline(vis, txt, SimpleHead(cfg, vis.out_channels, txt.out_channels))
    model.load_state_dict(OF.fill_state(model.state_dict(), seed, "base.", style="margin"))
    if dt == torch.float64:  # the module and the table attribute cast on the instance
        model.double()
        txt.vocab_dict = txt.vocab_dict.double()
    if swap:
        swap_losses(model.embed_model.loss_evaluator)
    return model.train()


def trajectory(spec, dims, table, seed, dt, steps, swap):
    hidden, embed, vocab, Lpad, C, NC, B = dims
    model = build_reference(spec, dims, table, seed, dt, swap)
    opt = torch.optim.SGD(groups(model.named_parameters()), lr=LR, momentum=MOMENTUM)
    out = {}
    for s in range(steps):
        x, tok, ln, ids = step_inputs(s, spec, B, vocab, Lpad, seed)
        ld = model(x.to(dt), make_captions(tok, ln, ids))
        opt.zero_grad()
        sum(ld.values()).backward()
        if s == 0:
            named = dict(model.named_parameters())
            for k, p in named.items():
                out["gdig0:" + k] = digest("grad0:" + k, p.grad)
            if not swap:
                for k in FULL_GRADS:
                    out["grad0:" + k] = named[k].grad.numpy().copy()
        opt.step()
        for k in ld:
            out["loss%d:%s" % (s, k)] = ld[k].detach().numpy()
        if not swap:
            # (the images are not stored: step s reads oracle.fill.randn("img:base<s>", [B, 3, H, W], seed) on both sides)
            out["tokens%d" % s], out["lengths%d" % s], out["ids%d" % s] = tok.numpy(), ln.numpy(), ids.numpy()
    sd = model.state_dict()
    for k, v in sd.items():  # the WHOLE state after the last step: parameters and BatchNorm statistics
        if v.dtype.is_floating_point:
            out["fdig:" + k] = digest("final:" + k, v)
    if not swap:
        for k in ("embed_model.visual_embed_layer.weight", "visual_model.bn1.running_mean", "visual_model.layer4.0.bn3.running_var",
                  "textual_model.gru.weight_ih_l0"):
            out["final:" + k] = sd[k].numpy().copy()
        model.eval()
        with torch.no_grad():
            ev = model(x.to(dt), make_captions(tok, ln, ids))
        out["eval_v"], out["eval_t"] = ev[0].numpy(), ev[1].numpy()
        out["state_names"] = np.array(list(sd.keys()))
        out["state_shapes"] = np.array([",".join(str(int(d)) for d in v.shape) for v in sd.values()])
        out["trainable_names"] = np.array([k for k, p in model.named_parameters() if p.requires_grad])
    return out


def conditioning(r32, r64):
    gfl = grad_floor([v for k, v in r32.items() if k.startswith("gdig0:")])
    errs = {}
    for k, ref in r64.items():
        v = r32[k]
        if k.startswith("gdig0:"):
            errs[k] = digest_err(v, ref, gfl * (100.0 if k.endswith("attnpool.k_proj.bias") else 1.0))
        elif k.startswith("fdig:"):
            errs[k] = digest_err(v, ref)
        elif k.startswith("grad0:"):
            errs[k] = float(np.abs(np.asarray(v, dtype=np.float64) - ref).max() / max(np.abs(ref).max(), gfl))
        elif k.startswith(("loss", "final:", "eval_")):
            errs[k] = rel(v, ref)
    top = sorted(errs.items(), key=lambda kv: -kv[1])[:4]
    print("  reference fp32 vs fp64 (conditioning): worst", [(k, "%.1e" % v) for k, v in top])
    assert top[0][1] < COND, ("fixture is not well conditioned: change the seed", top)
    return top[0][1]


def gen_simple_head(seed=5, steps=3, swap_steps=2):
    print("[simple_head]")
    spec = OV.TINY
    hidden, embed, vocab, Lpad, C, NC, B = 64, 64, 200, 105, 32, 53, 8
    dims = (hidden, embed, vocab, Lpad, C, NC, B)
    table = OF.randn("vocab_table_base", (vocab, embed), seed, 0.5)
    out = {"dims": np.array([hidden, embed, vocab, Lpad, C, NC, B, seed, steps, swap_steps]), "sgd": np.array([LR, MOMENTUM, WD])}
    main = trajectory(spec, dims, table, seed, torch.float32, steps, False)
    c1 = conditioning(main, trajectory(spec, dims, table, seed, torch.float64, steps, False))
    swap = trajectory(spec, dims, table, seed, torch.float32, swap_steps, True)
    c2 = conditioning(swap, trajectory(spec, dims, table, seed, torch.float64, swap_steps, True))
    out.update(main)
    out.update({"swap:" + k: v for k, v in swap.items()})
    out["conditioning"] = np.array(max(c1, c2))
    out = {k: (np.asarray(v).astype(np.float32) if np.asarray(v).dtype == np.float64 and not k.startswith(("gdig0:", "fdig:", "swap:gdig0:", "swap:fdig:", "sgd", "conditioning")) else v)
           for k, v in out.items()}
    np.savez_compressed(os.path.join(HERE, "simple_head.npz"), **out)


if __name__ == "__main__":
    gen_losses_extra()
    gen_simple_head()
    for f in ("losses_extra.npz", "simple_head.npz"):
        print("%-20s %8d bytes" % (f, os.path.getsize(os.path.join(HERE, f))))
