#!/usr/bin/env python3
"""Generate tests/golden/text_stack.npz from the IMPORTED reference text encoder with num_layers = 2 and 3
(lib/models/backbones/gru.py:36-43: nn.GRU(num_layers=..., dropout=...)), with the shims make_golden.py uses for its
text section.  `use_onehot="yes"` (a trainable nn.Embedding) needs no vocabulary file and no .cuda().

hidden 64, embed 48 (neither H nor 2H: a mixed-up layer input width cannot pass), vocab 40, B = 6, L = 9, drop_out 0.
Parameters are filled by oracle.fill names ("stack<layers>." + state_dict key).  Recorded per depth: the output, every
gradient under a filled upstream gradient (every other row of the GRU matrices), the eval-mode output of a second batch.  Arrays and scalars only.

The result is also checked here against the fp64 restatement of tests/gru_stack_ref.py.

Usage:  python tests/golden/make_golden_gru_stack.py <path of the reference checkout>
"""

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if len(sys.argv) != 2:
    sys.exit(__doc__)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, sys.argv[1])

torch.Tensor.cuda = lambda self, *a, **k: self  # shim (i) of make_golden.py

import gru_stack_ref as GS  # noqa: E402
import oracle.fill as OF  # noqa: E402

import lib.models.backbones.gru as ref_gru  # noqa: E402
from lib.utils.caption import Caption  # noqa: E402

HIDDEN, EMBED, VOCAB, L, SEED = 64, 48, 40, 9, 6
LENS = [9, 1, 5, 3, 9, 7]
ROW_STRIDE = 2
LENS2 = [4, 7, 2, 7]  # batch maximum below L: the zero pad enters the max only up to the BATCH maximum


def captions(tok, ln):
    return [Caption([tok[i, : int(ln[i])].tolist()], max_length=tok.shape[1]) for i in range(tok.shape[0])]


def tokens(name, lens):
    tok = OF.randint(name, 1, VOCAB, (len(lens), L), SEED)
    for i, n in enumerate(lens):
        tok[i, n:] = 0
    return tok, torch.tensor(lens, dtype=torch.int64)


def rel(a, b):
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def main():
    tok, ln = tokens("tok:stack", LENS)
    tok2, ln2 = tokens("tok:stack2", LENS2)
    out = {"tokens": tok.numpy(), "lengths": ln.numpy(), "tokens2": tok2.numpy(), "lengths2": ln2.numpy(), "seed": np.array(SEED),
           "dims": np.array([HIDDEN, EMBED, VOCAB, L]), "row_stride": np.array(ROW_STRIDE)}
    for nl in (2, 3):
        pre = "stack%d." % nl
        g = ref_gru.GRU(HIDDEN, VOCAB, EMBED, nl, 0.0, True, "yes", "./")
        g.load_state_dict(OF.fill_state(g.state_dict(), SEED, pre))
        y = g(captions(tok, ln))
        w_out = OF.randn("gout:stack", tuple(y.shape), SEED)
        (y * w_out).sum().backward()
        out["out_l%d" % nl] = y.detach().numpy()
        for k, p in g.named_parameters():
            # (every other row of the GRU matrices, all columns: the whole set would exceed the size limit of a committed file)
            out["grad_l%d:%s" % (nl, k)] = (p.grad[::ROW_STRIDE] if k.startswith("gru.") else p.grad).numpy().copy()
        g.eval()
        with torch.no_grad():
            y2 = g(captions(tok2, ln2))
        out["out2_l%d" % nl] = y2.numpy()
        # the fp64 restatement against what the reference just computed
        st = {k: OF.fill(pre + k, tuple(v.shape), SEED).double().requires_grad_(True) for k, v in g.state_dict().items()}
        yo = GS.stack_forward(st, None, tok, ln, nl)
        (yo * w_out.double()).sum().backward()
        errs = {"out": rel(yo, y), "out2": rel(GS.stack_forward(st, None, tok2, ln2, nl), y2)}
        for k, p in g.named_parameters():
            errs["grad " + k] = rel(st[k].grad, p.grad)
        print(nl, "layers:", {k: "%.1e" % v for k, v in errs.items()})
        assert errs["out"] < 1e-5 and errs["out2"] < 1e-5 and all(v < 1e-4 for v in errs.values()), errs
    np.savez_compressed(os.path.join(HERE, "text_stack.npz"), **out)
    print("wrote text_stack.npz: %d bytes" % os.path.getsize(os.path.join(HERE, "text_stack.npz")))


if __name__ == "__main__":
    main()
