#!/usr/bin/env python3
"""Generate tests/golden/resnet.npz from the IMPORTED reference module lib/models/backbones/resnet.py.

  resnet.npz   the reference ResNet built from its own `resnet(Bottleneck, stages, None)` tuple with stages [1, 2, 1, 1] (an
               identity block and all four downsample blocks), RES5_STRIDE 1 and 2, on inputs [2,3,96,32] and [3,3,90,30]
               (odd maps: 45x15 after the stem, 23x8 after the pool).  Per input and stride: the train-mode output, digests
               of every parameter gradient of loss = sum(out * G), every BatchNorm running buffer after that forward, the
               eval-mode output afterwards, and three SGD steps of the encoder alone (losses, final-state digests).  Also
               the state-dict names and shapes of the real resnet50 / resnet101.

Runs only where the reference tree is present (read-only); one in-process shim: `torch.load` INSIDE the reference module's
namespace hands the constructor a state dict filled by oracle.fill.fill_state for the module being built, and `pretrained` is
always a (non-None) token, so the download branch of the constructor is never reached.
Weights are NOT stored: both sides fill every tensor by name.  Two conditions are asserted (a fixture that fails one gets
another seed, never another bound):
  1. every stored fp32 quantity lies within COND of an fp64 evaluation of the same reference code;
  2. no max-pool window holds two equal positive maxima (the winner of a tie is an implementation's choice of order; the
     smallest relative gap between the two largest values of a window is stored as `min_pool_gap`);
  3. the same fp64 evaluation with every input value perturbed by a relative 1e-6 (the size of ONE fp32 rounding) stays within
     COND of the unperturbed one in every quantity of the three-step trajectory (losses, final state; the single-pass
     quantities are linear in the input in places - the stem's weight gradient - and are held by condition 1).  Condition 1 alone is not enough for the three-step trajectory: an implementation with
     fp32-class arithmetic differs from the reference by perturbations of this size at every layer, and with BatchNorm over as
     few as 9 values per channel (layer4 at [3,3,90,30], RES5_STRIDE 2) the steps amplify them - a fixture can pass 1 by the
     luck of which ReLU / pool decisions flip and still move by 2e-2 under 3 (seed 13 at G_SCALE 0.005 did).

Usage:  python tests/golden/make_golden_resnet.py <path of the reference tree>
"""

import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("TEXTREID_REFERENCE", "")
if not os.path.isdir(os.path.join(REF, "lib", "models", "backbones")):
    sys.exit("usage: make_golden_resnet.py <path of the reference tree>")
sys.path.insert(0, ROOT)
sys.path.insert(0, REF)

torch.set_num_threads(8)

import oracle.fill as OF  # noqa: E402
from oracle.fill import digest, digest_err, grad_floor  # noqa: E402

import lib.models.backbones.resnet as ref_rn  # noqa: E402

COND = 5e-4  # fp32 reference vs fp64 evaluation of the same code
LR, MOMENTUM, WD = 0.02, 0.9, 4e-5
# Scale of the filled upstream gradient G of loss = sum(out * G): it sets the size of the SGD steps, and with it how much the
# three-step trajectory amplifies a rounding-sized perturbation (condition 3; worst case [3,3,90,30] at RES5_STRIDE 2, where a
# single forward pass already turns 1e-6 into 1.3e-5):
#   G_SCALE 1      largest parameter gradient ~66; the reference's own fp32 run ends 3e-2 from its fp64 run
#   G_SCALE 5e-3   1e-6 -> 1.6e-2
#   G_SCALE 1e-3   1e-6 -> 2.6e-3
#   G_SCALE 1e-4   1e-6 -> < 1e-4   (chosen: the first below COND; the figure of the stored fixture is its `sensitivity`)
# The price: at 1e-4 a step moves a filter by ~1e-4 of its size, so the final-state digests of the FILTERS say little about the
# updates; the per-step losses, the BatchNorm biases and running statistics (which the updates dominate) and the single-pass
# gradient digests carry that part of the check.
G_SCALE = 1e-4
STAGES = [1, 2, 1, 1]
CASES = {"96x32": (2, 3, 96, 32), "90x30": (3, 3, 90, 30)}
PREFIX = "resnet."
PERTURB = 1e-6  # condition 3: relative input perturbation, one fp32 rounding


class _TorchWithLoad:
    """`torch` as the reference module sees it: everything is torch's own, except `load`, which returns the state the shim holds."""

    def __init__(self, make_state):
        self._make_state = make_state

    def __getattr__(self, name):
        return getattr(torch, name)

    def load(self, *a, **k):
        return self._make_state(sys._getframe(1).f_locals["self"])  # the half-built ResNet whose constructor is loading


def build_reference(stages, stride, seed, dt=torch.float32, fill=True):
    def make_state(module):
        sd = module.state_dict()
        return OF.fill_state(sd, seed, PREFIX) if fill else {k: v.clone() for k, v in sd.items()}

    ref_rn.torch = _TorchWithLoad(make_state)
    try:
        m = ref_rn.ResNet(ref_rn.resnet(ref_rn.Bottleneck, stages, None), stride, 1, pretrained="filled-by-name")
    finally:
        ref_rn.torch = torch
    return m.to(dt).train()


def rel(a, b):
    a, b = torch.as_tensor(a).detach().double(), torch.as_tensor(b).detach().double()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def pool_gap(a):
    """Smallest relative gap between the two largest values of a 3x3 / stride 2 / pad 1 window with a positive maximum;
    0.0 = an exact tie."""
    B, C = a.shape[:2]
    win = F.unfold(a, 3, padding=1, stride=2).view(B, C, 9, -1)  # (zero padding: never equal to a positive maximum)
    top2 = win.topk(2, dim=2).values
    pos = top2[:, :, 0] > 0
    gap = ((top2[:, :, 0] - top2[:, :, 1]) / top2[:, :, 0].clamp_min(1e-30))[pos]
    return float(gap.min())


def run(case, shape, stride, seed, dt, eps=0.0):
    r = {}
    x = OF.randn("resnet:x" + case, shape, seed).to(dt)
    x = x * (1.0 + eps * OF.randn("resnet:perturb" + case, shape, seed).to(dt))
    m = build_reference(STAGES, stride, seed, dt)
    seen = []
    hook = m.maxpool.register_forward_hook(lambda mod, inp, out: seen.append(inp[0].detach()))
    out = m(x)
    hook.remove()
    r["pool_gap"] = pool_gap(seen[0])
    r["out"] = out.detach().numpy()
    G = OF.randn("resnet:G" + case, tuple(out.shape), seed, G_SCALE).to(dt)
    (out * G).sum().backward()
    for k, p in m.named_parameters():
        r["gdig:" + k] = digest("grad:" + k, p.grad)
    for k, b in m.named_buffers():
        if "num_batches_tracked" not in k:
            r["buf:" + k] = b.detach().clone().numpy()
    m.eval()
    with torch.no_grad():
        r["eval"] = m(x).numpy()
    m = build_reference(STAGES, stride, seed, dt)
    opt = torch.optim.SGD(m.parameters(), lr=LR, momentum=MOMENTUM, weight_decay=WD)
    for s in range(3):
        xs = OF.randn("resnet:x%s:step%d" % (case, s), shape, seed).to(dt)
        xs = xs * (1.0 + eps * OF.randn("resnet:perturb%s:step%d" % (case, s), shape, seed).to(dt))
        loss = (m(xs) * G).sum()
        opt.zero_grad()
        loss.backward()
        opt.step()
        r["loss%d" % s] = np.asarray(float(loss.detach()))
    for k, v in m.state_dict().items():
        if "num_batches_tracked" not in k:
            r["fdig:" + k] = digest("final:" + k, v)
    return r


def conditioning(r32, r64, what="reference fp32 vs fp64 (conditioning)", only=None):
    gfl = grad_floor([v for k, v in r32.items() if k.startswith("gdig:")])
    errs = {}
    for k, ref in r64.items():
        v = r32[k]
        if only is not None and not k.startswith(only):
            continue
        if k.startswith("gdig:"):
            errs[k] = digest_err(v, ref, gfl)
        elif k.startswith("fdig:"):
            errs[k] = digest_err(v, ref)
        elif k != "pool_gap":
            errs[k] = rel(v, ref)
    top = sorted(errs.items(), key=lambda kv: -kv[1])[:4]
    print("  %s: worst" % what, [(k, "%.1e" % v) for k, v in top])
    assert top[0][1] < COND, ("fixture is not well conditioned: change the seed", top)
    return top[0][1]


def gen_resnet(seed=13):
    out = {"seed": np.array(seed), "stages": np.array(STAGES), "sgd": np.array([LR, MOMENTUM, WD]), "g_scale": np.array(G_SCALE)}
    worst, sens, gap = 0.0, 0.0, 1.0
    for case, shape in CASES.items():
        out[case + ":shape"] = np.array(shape)
        for stride in (1, 2):
            tag = "%s:s%d:" % (case, stride)
            print("[resnet %s]" % tag)
            r32 = run(case, shape, stride, seed, torch.float32)
            assert r32["pool_gap"] > 0.0, ("a max-pool window holds two equal positive maxima: change the seed", tag)
            r64 = run(case, shape, stride, seed, torch.float64)
            worst = max(worst, conditioning(r32, r64))
            sens = max(sens, conditioning(run(case, shape, stride, seed, torch.float64, PERTURB), r64, "fp64 with inputs perturbed by 1e-6 vs fp64 (trajectory sensitivity)",
                                              only=("loss", "fdig:")))
            gap = min(gap, r32.pop("pool_gap"))
            print("  smallest relative top-two gap of a pool window: %.1e" % gap)
            for k, v in r32.items():
                v = np.asarray(v)
                out[tag + k] = v if k.startswith(("gdig:", "fdig:")) else v.astype(np.float32)
    out["conditioning"] = np.array(worst)
    out["sensitivity"] = np.array(sens)
    out["min_pool_gap"] = np.array(gap)
    for arch in ("resnet50", "resnet101"):
        sd = build_reference(ref_rn.model_archs[arch].stage, 1, seed, fill=False).state_dict()
        out[arch + ":names"] = np.array(list(sd.keys()))
        out[arch + ":shapes"] = np.array([",".join(str(int(d)) for d in v.shape) for v in sd.values()])
    np.savez_compressed(os.path.join(HERE, "resnet.npz"), **out)


if __name__ == "__main__":
    gen_resnet()
    print("%-20s %8d bytes" % ("resnet.npz", os.path.getsize(os.path.join(HERE, "resnet.npz"))))
