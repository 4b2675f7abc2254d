#!/usr/bin/env python3
"""Bits and library-call sequences of the BiGRU text encoder, recorded at the commit BEFORE its two autograd Functions (one
layer / stacked) and its four cell kernels were merged (tests/test_gru_flow_gpu.py holds every later commit to them).

Run on the GPU in a checkout of that parent commit, twice, in two processes; the two files must be identical:

    python tests/golden/make_gru_flow_parent.py /tmp/a.json && python tests/golden/make_gru_flow_parent.py /tmp/b.json
    cmp /tmp/a.json /tmp/b.json && cp /tmp/a.json tests/golden/gru_flow_parent.json

Only names that exist on both sides of that change are used: GRU, CaptionBatch, gru.FUSED_GRU_STEP, ops.CONV_PRECISION,
textreid_amd.lib.TRACE, oracle.fill, last_dropout_masks and last_layer_inputs.  Per case (``compute(case, device)``):

* ``out``: sha256 of the train-mode output; ``grad:<name>``: of every parameter gradient of loss = sum(out * G);
  ``mask:<k>`` / ``input:<k>``: of every keep mask and of every ``last_layer_inputs`` tensor of that forward (``masks``: their
  number, -1 for None); ``out:nograd`` / ``out:eval``: of a following torch.no_grad() forward and of an eval() forward;
* ``calls:<pass>``: [number of library calls of the pass, sha256 of the ordered, newline-joined (entry point, scalar arguments)]
  as lib.TRACE records them (the train pass is forward + backward);
* the dropout cases run the training step twice (``2:`` keys: the offset advance shows) and then the same module with
  ``gru.eval()`` and frozen parameters, as MODEL.FREEZE leaves it (``frozen`` keys: no masks, nothing saved);
* ``error``: the exception text, where the pass raises.
"""

import hashlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import oracle.fill as OF  # noqa: E402

VOCAB = 40
LIN_IN = 56  # width of the frozen table in front of the nn.Linear form
BASE = (5, 64, 48, 7)


def _name(kind, layers, shape, fused, extra=""):
    return "%s:l%d:%s:%s%s" % (kind, layers, "x".join(str(v) for v in shape), "fused" if fused else "unfused", extra)


def _cases():
    """{name: (embed form, layers, (B, H, E, L), FUSED_GRU_STEP, dropout p, CONV_PRECISION or None, bound_only)}"""
    out = {}
    for layers in (1, 2, 3):  # frozen table; (17, 768, ...) is the H ceiling of the step kernels
        for shape in (BASE, (1, 32, 32, 1), (33, 96, 64, 5), (17, 768, 64, 3)):
            for fused in (True, False):
                out[_name("table", layers, shape, fused)] = ("table", layers, shape, fused, 0.0, None, False)
    for kind in ("embedding", "linear"):  # trainable nn.Embedding; nn.Linear on frozen rows
        for layers in (1, 2):
            for fused in (True, False):
                out[_name(kind, layers, BASE, fused)] = (kind, layers, BASE, fused, 0.0, None, False)
    for layers in (2, 3):
        for fused in (True, False):
            out[_name("dropout", layers, BASE, fused)] = ("table", layers, BASE, fused, 0.3, None, False)
    for layers in (1, 2):
        out[_name("splitk", layers, (130, 64, 64, 8), True)] = ("table", layers, (130, 64, 64, 8), True, 0.0, None, False)  # L*B >= 1024
        for fused in (True, False):
            out[_name("bound", layers, BASE, fused)] = ("table", layers, BASE, fused, 0.0, None, True)
        for prec in (16, 6):
            out[_name("precision", layers, BASE, True, ":p%d" % prec)] = ("table", layers, BASE, True, 0.0, prec, False)
        out[_name("h48", layers, (5, 48, 48, 7), True)] = ("table", layers, (5, 48, 48, 7), True, 0.0, None, False)  # the step kernels refuse H = 48
    return out


SPECS = _cases()
CASES = list(SPECS)


def _sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def _traced(fn):
    """(fn(), [number of library calls, sha256 of their (entry point, scalar arguments)])"""
    from textreid_amd import lib

    lib.TRACE = []
    try:
        out = fn()
        torch.cuda.synchronize()
        rows = ["%s %r" % (entry[0], entry[1]) for entry in lib.TRACE]
    finally:
        lib.TRACE = None
    return out, [len(rows), hashlib.sha256("\n".join(rows).encode()).hexdigest()]


def _module(case, kind, layers, shape, p, dev):
    from textreid_amd.backbones.gru import GRU

    B, H, E, L = shape
    if kind == "embedding":
        m = GRU(H, VOCAB, E, layers, p, True, "yes", "./")
    else:
        width = E if kind == "table" else LIN_IN
        m = GRU(H, width, E, layers, p, True, "clip_vit", "./", vocab_dict=OF.randn("gf:table:" + case, (VOCAB, width), 1, 0.5))
    assert m.embed_mode == {"table": 0, "embedding": 1, "linear": 2}[kind]
    with torch.no_grad():
        for k, q in m.named_parameters():
            q.copy_(OF.randn("gf:%s:%s" % (case, k), tuple(q.shape), 2, 1.5 / q.shape[-1] ** 0.5 if q.dim() > 1 else 0.05))
    return m.to(dev).train()


def _batch(case, shape, bound_only, dev):
    """ragged lengths that include 1 and L; a bound_only batch loops L + 2 steps over token rows that wide"""
    from textreid_amd.caption import CaptionBatch

    B, H, E, L = shape
    lengths = OF.randint("gf:len:" + case, 1, L + 1, (B,), 3)
    lengths[0] = L
    if B > 1:
        lengths[-1] = 1
    width = L + 2 if bound_only else L
    tokens = torch.zeros(B, width, dtype=torch.int64)
    tokens[:, :L] = OF.randint("gf:tok:" + case, 0, VOCAB, (B, L), 4)
    return CaptionBatch(tokens.to(dev), lengths.to(dev), max_len=width, bound_only=bound_only)


def _side(m, tag, res):
    masks = m.last_dropout_masks
    res[tag + "masks"] = -1 if masks is None else len(masks)
    for i, k in enumerate(masks or []):
        res["%smask:%d" % (tag, i)] = _sha(k)
    res[tag + "inputs"] = len(m.last_layer_inputs)
    for i, x in enumerate(m.last_layer_inputs):
        res["%sinput:%d" % (tag, i)] = _sha(x)


def _train(m, cb, G, tag, res):
    def step():
        for q in m.parameters():
            q.grad = None
        out = m(cb)
        (out * G).sum().backward()
        return out

    out, res[tag + "calls:train"] = _traced(step)
    res[tag + "out"] = _sha(out)
    for k, q in m.named_parameters():
        res["%sgrad:%s" % (tag, k)] = _sha(q.grad)
    _side(m, tag, res)


def _forward(m, cb, name, res):
    out, res["calls:" + name] = _traced(lambda: m(cb))
    res["out:" + name] = _sha(out)
    _side(m, name + ":", res)


def _run(case, dev):
    kind, layers, shape, fused, p, prec, bound_only = SPECS[case]
    B, H = shape[0], shape[1]
    res = {}
    m = _module(case, kind, layers, shape, p, dev)
    cb = _batch(case, shape, bound_only, dev)
    G = OF.randn("gf:G:" + case, (B, 2 * H), 5).to(dev)
    torch.manual_seed(1234)  # (the dropout seed is drawn from torch's CPU generator by the first training forward)
    _train(m, cb, G, "", res)
    if p > 0:
        _train(m, cb, G, "2:", res)
    with torch.no_grad():
        _forward(m, cb, "nograd", res)
    m.eval()
    _forward(m, cb, "eval", res)
    if p > 0:  # build_gru under MODEL.FREEZE: the nn.GRU in eval mode, its parameters frozen
        m.train()
        m.gru.eval()
        for q in m.gru.parameters():
            q.requires_grad = False
        _forward(m, cb, "frozen", res)
        assert m.last_dropout_masks is None
    return res


def compute(case, dev):
    from textreid_amd import ops
    from textreid_amd.backbones import gru as G

    prec = SPECS[case][5]
    was_fused, was_prec = G.FUSED_GRU_STEP, ops.CONV_PRECISION
    G.FUSED_GRU_STEP = SPECS[case][3]
    if prec is not None:
        ops.CONV_PRECISION = prec
    try:
        return _run(case, dev)
    except RuntimeError as e:
        if "h48" not in case:
            raise
        torch.cuda.synchronize()
        return {"error": str(e)}
    finally:
        G.FUSED_GRU_STEP, ops.CONV_PRECISION = was_fused, was_prec


if __name__ == "__main__":
    import textreid_amd  # noqa: F401

    dev = torch.device("cuda")
    out = {case: compute(case, dev) for case in CASES}
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print({k: len(v) for k, v in out.items()})
