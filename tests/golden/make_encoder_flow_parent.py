#!/usr/bin/env python3
"""Bits and library-call sequences of the two image encoders, recorded at the commit BEFORE their fp32 Bottleneck flow, eval plan
and autograd Function were merged (tests/test_encoder_flow_gpu.py holds every later commit to them).

Run on the GPU in a checkout of that parent commit, twice, in two processes; the two files must be identical:

    python tests/golden/make_encoder_flow_parent.py /tmp/a.json && python tests/golden/make_encoder_flow_parent.py /tmp/b.json
    cmp /tmp/a.json /tmp/b.json && cp /tmp/a.json tests/golden/encoder_flow_parent.json

Only names that exist on both sides of that change are used: the two encoder classes, forward / backward, oracle.fill,
ops.USE_EVAL_P16, fold_eval_bn, _debug_eval_bounds and textreid_amd.lib.TRACE.  Per case (``compute(case, device)``):

* ``out``: sha256 of the train-mode output; ``grad:<name>``: of every parameter gradient of loss = sum(out * G);
  ``buf:<name>``: of every BatchNorm buffer after that step; ``eval:<pass>``: of each eval-mode output;
* ``calls:<pass>``: [number of library calls of the pass, sha256 of their newline-joined entry-point names] (the train pass is
  forward + backward; an eval pass is the FIRST call in that mode, parameter-only plans included).
"""

import hashlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import oracle.fill as OF  # noqa: E402
import oracle.visual as OV  # noqa: E402

SEED = 17
CASES = ["A", "B", "C:96x32:s1", "C:96x32:s2", "C:90x30:s1", "C:90x30:s2", "D"]


def _sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def _traced(fn):
    """(fn(), [number of library calls, sha256 of their names])"""
    from textreid_amd import lib

    lib.TRACE = []
    try:
        out = fn()
        torch.cuda.synchronize()
        names = [entry[0] for entry in lib.TRACE]
    finally:
        lib.TRACE = None
    return out, [len(names), hashlib.sha256("\n".join(names).encode()).hexdigest()]


def _train(m, x, tag, res):
    def step():
        out = m(x)
        G = OF.randn("flow:G" + tag, tuple(out.shape), SEED).to(x.device)
        (out * G).sum().backward()
        return out

    out, res["calls:train"] = _traced(step)
    res["out"] = _sha(out)
    for k, p in m.named_parameters():
        res["grad:" + k] = _sha(p.grad)
    for k, b in m.named_buffers():
        res["buf:" + k] = _sha(b)


def _eval(m, x, name, res):
    with torch.no_grad():
        out, res["calls:eval:" + name] = _traced(lambda: m(x))
    res["eval:" + name] = _sha(out)


def _clip(spec, dev):
    from textreid_amd.backbones.m_resnet import ModifiedResNet

    m = ModifiedResNet(list(spec.layers), spec.output_dim, spec.heads, spec.last_stride, (spec.height, spec.in_width), spec.width)
    m.load_state_dict(OF.fill_state(m.state_dict(), SEED))
    return m.to(dev).train()


def compute(case, dev):
    from textreid_amd import ops

    res = {}
    if case == "A":  # CLIP, fp32 flow (width 16 is not P16-eligible): a stride-1 downsample block, three stride-2 blocks, an identity block
        spec = OV.VisualSpec(layers=(1, 2, 1, 1), width=16, heads=4, output_dim=64, last_stride=2, height=64, in_width=64)
        m = _clip(spec, dev)
        x = OF.randn("flow:imgA", (3, 3, spec.height, spec.in_width), SEED).to(dev)
        _train(m, x, "A", res)
        m.eval()
        m.fold_eval_bn = False
        _eval(m, x, "unfolded", res)
        m.fold_eval_bn = True
        _eval(m, x, "folded", res)
    elif case == "B":  # CLIP, layer4 at stride 1
        spec = OV.TINY
        assert spec.last_stride == 1
        m = _clip(spec, dev)
        _train(m, OF.randn("flow:imgB", (3, 3, spec.height, spec.in_width), SEED).to(dev), "B", res)
    elif case.startswith("C:"):  # ImageNet, the shapes of tests/golden/resnet.npz (90x30: odd at every stride-2 step)
        from textreid_amd.backbones.resnet import Bottleneck, ResNet, resnet

        _, shape, stride = case.split(":")
        g = np.load(os.path.join(ROOT, "tests", "golden", "resnet.npz"))
        m = ResNet(resnet(Bottleneck, [int(s) for s in g["stages"]], None), int(stride[1:]))
        m.load_state_dict(OF.fill_state(m.state_dict(), SEED, "resnet."))
        m.to(dev).train()
        x = OF.randn("flow:img" + case, tuple(int(v) for v in g[shape + ":shape"]), SEED).to(dev)
        _train(m, x, case, res)
        m.eval()
        _eval(m, x, "default", res)
        was = ops.USE_EVAL_P16
        ops.USE_EVAL_P16 = False
        try:
            _eval(m, x, "unfused", res)
        finally:
            ops.USE_EVAL_P16 = was
    elif case == "D":  # CLIP at width 64: the P16 training flow and the P16 eval pass, map sizes of the full-size encoder
        spec = OV.VisualSpec(layers=(1, 2, 1, 1), width=64, heads=32, output_dim=1024, last_stride=1, height=384, in_width=128)
        m = _clip(spec, dev)
        x = OF.randn("flow:imgD", (2, 3, spec.height, spec.in_width), SEED).to(dev)
        _train(m, x, "D", res)
        m.eval()
        m._debug_eval_bounds = []
        try:
            _eval(m, x, "default", res)
            res["eval_p16_taken"] = len(m._debug_eval_bounds) > 0
        finally:
            m._debug_eval_bounds = None
    else:
        raise KeyError(case)
    return res


def state_names(empty_dir):
    """sha256 of the newline-joined parameter names and state-dict keys of the two full-size encoders (CPU; ``empty_dir``: a
    directory without checkpoints, so nothing is loaded)."""
    from textreid_amd.backbones.m_resnet import ModifiedResNet
    from textreid_amd.backbones.resnet import ResNet, model_archs

    res = {}
    for tag, m in (("clip", ModifiedResNet([3, 4, 6, 3], 1024, 32, 1, (384, 128))),
                   ("imagenet", ResNet(model_archs["resnet50"], 2, pretrained=None, root=empty_dir))):
        res[tag + ":parameters"] = hashlib.sha256("\n".join(k for k, _ in m.named_parameters()).encode()).hexdigest()
        res[tag + ":state_dict"] = hashlib.sha256("\n".join(m.state_dict()).encode()).hexdigest()
    return res


if __name__ == "__main__":
    import tempfile

    import textreid_amd  # noqa: F401

    dev = torch.device("cuda")
    out = {case: compute(case, dev) for case in CASES}
    with tempfile.TemporaryDirectory() as tmp:
        out["names"] = state_names(tmp)
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print({k: len(v) for k, v in out.items()})
