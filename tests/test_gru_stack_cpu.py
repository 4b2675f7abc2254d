"""Stacked BiGRU text encoder (MODEL.GRU.NUM_LAYER > 1, reference lib/models/backbones/gru.py:36-43): what can be
checked without a GPU - the parameter surface, and the fp64 restatement the GPU tests compare against
(tests/gru_stack_ref.py), pinned to vectors captured from the reference module and to torch.nn.GRU's own definition."""

import os

import numpy as np
import pytest
import torch
from torch import nn

import gru_stack_ref as GS
import oracle.fill as OF


def rel(a, b):
    a = torch.as_tensor(a).detach().double()
    b = torch.as_tensor(b).detach().double()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def test_two_layer_encoder_has_nn_gru_parameters():
    from textreid_amd.backbones.gru import GRU

    hidden, embed = 64, 48
    m = GRU(hidden, 40, embed, 2, 0.3, True, "yes", "./")
    want = {"gru." + k: tuple(v.shape) for k, v in nn.GRU(embed, hidden, 2, bias=False, bidirectional=True).state_dict().items()}
    got = {k: tuple(v.shape) for k, v in m.state_dict().items() if k.startswith("gru.")}
    assert got == want and list(got) == list(want)
    assert got == GS.state_shapes(hidden, embed, 2)
    assert set(m.state_dict()) == set(want) | {"embed.weight"}  # the dropout generator's state is not in the state_dict
    assert m.out_channels == 2 * hidden and m.gru.dropout == 0.3 and m.last_dropout_masks is None


def test_build_textual_model_with_two_layers():
    from textreid_amd.backbones import GRU, build_textual_model
    from textreid_amd.config import moco_cfg

    cfg = moco_cfg("m_resnet50", K=64)
    cfg.MODEL.GRU.NUM_LAYER = 2
    cfg.MODEL.GRU.DROPOUT_KEEP_PROB = 0.7
    m = build_textual_model(cfg, vocab_dict=torch.zeros(10, cfg.MODEL.GRU.VOCABULARY_SIZE))
    assert isinstance(m, GRU) and m.gru.num_layers == 2 and abs(m.gru.dropout - 0.3) < 1e-12
    assert tuple(m.gru.weight_ih_l1_reverse.shape) == (3 * cfg.MODEL.GRU.NUM_UNITS, 2 * cfg.MODEL.GRU.NUM_UNITS)


def test_unidirectional_still_refused():
    from textreid_amd.backbones.gru import GRU

    for layers in (1, 2):
        with pytest.raises(NotImplementedError):
            GRU(64, 40, 48, layers, 0.0, False, "yes", "./")


def test_deep_copy_gets_its_own_generator_state():
    import copy

    from textreid_amd.backbones.gru import GRU

    m = GRU(32, 40, 48, 2, 0.3, True, "yes", "./")
    a = m.dropout_state(torch.device("cpu"))
    k = copy.deepcopy(m)
    assert k._dropout_state is None and m._dropout_state is a
    assert all(torch.equal(p, q) and p is not q for p, q in zip(m.parameters(), k.parameters()))


@pytest.mark.parametrize("layers", [2, 3])
def test_restatement_reproduces_reference_fixture(golden_dir, layers):
    """tests/gru_stack_ref.py in fp64 against text_stack.npz (the reference module's output, gradients and eval-mode output),
    at the tolerance tests/test_oracle_golden.py::test_text holds the one-layer oracle to."""
    g = np.load(os.path.join(golden_dir, "text_stack.npz"))
    seed, rs = int(g["seed"]), int(g["row_stride"])
    hidden, embed, vocab, L = (int(v) for v in g["dims"])
    shapes = dict(GS.state_shapes(hidden, embed, layers), **{"embed.weight": (vocab, embed)})
    st = {k: OF.fill("stack%d.%s" % (layers, k), s, seed).requires_grad_(True) for k, s in shapes.items()}
    tok, ln = torch.from_numpy(g["tokens"]), torch.from_numpy(g["lengths"])
    assert int(ln.max()) == L and int(ln.min()) == 1
    y = GS.stack_forward(st, None, tok, ln, layers)
    assert rel(y, g["out_l%d" % layers]) < 1e-5
    (y * OF.randn("gout:stack", tuple(y.shape), seed)).sum().backward()
    for k in st:
        want = g["grad_l%d:%s" % (layers, k)]
        assert rel(st[k].grad[::rs] if k.startswith("gru.") else st[k].grad, want) < 1e-4, k
    with torch.no_grad():
        y2 = GS.stack_forward(st, None, torch.from_numpy(g["tokens2"]), torch.from_numpy(g["lengths2"]), layers)
    assert rel(y2, g["out2_l%d" % layers]) < 1e-5


@pytest.mark.parametrize("layers", [2, 3])
def test_restatement_dropout_is_torch_definition(layers):
    """With GIVEN keep masks the restatement equals single-layer torch.nn.GRU modules run by hand with mask / (1 - p)
    applied between them (nn.GRU: dropout on the outputs of each layer except the last).  Full-length captions, so the
    plain (unpacked) nn.GRU forward is the same computation."""
    B, L, H, E, p = 4, 5, 16, 12, 0.3
    gen = torch.Generator().manual_seed(11)
    x = torch.randn(B, L, E, generator=gen, dtype=torch.float64)
    masks = [(torch.rand(B, L, 2 * H, generator=gen) >= p).to(torch.uint8) for _ in range(layers - 1)]
    st, mods = {}, []
    for k in range(layers):
        m = nn.GRU(E if k == 0 else 2 * H, H, 1, bias=False, bidirectional=True, batch_first=True).double()
        mods.append(m)
        for n, v in m.state_dict().items():
            st["gru." + n.replace("_l0", "_l%d" % k)] = v.clone()
    want = x
    for k, m in enumerate(mods):
        want, _ = m(want)
        if k + 1 < layers:
            want = want * masks[k].double() / (1.0 - p)
    seqs = GS.stack_sequences(st, x, torch.full((B,), L), layers, masks, p)
    assert rel(seqs[-1], want) < 1e-12
    # ... and p = 0 without masks is torch's own stacked module
    full = nn.GRU(E, H, layers, bias=False, bidirectional=True, batch_first=True).double()
    full.load_state_dict({k[4:]: v for k, v in st.items()})
    assert rel(GS.stack_sequences(st, x, torch.full((B,), L), layers)[-1], full(x)[0]) < 1e-12


def test_philox_restatement_known_answers():
    """The numpy Philox4x32-10 the GPU test predicts the keep masks with, against the published known-answer vectors of
    the Random123 library (kat_vectors: philox4x32 10)."""
    kat = [((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
           ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
           ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1))]
    for ctr, key, want in kat:
        got = GS.philox4x32_10(np.array(ctr, dtype=np.uint64), np.array(key, dtype=np.uint64))
        assert tuple(int(v) for v in got) == want
    m = GS.keep_mask(10, 0.3, seed=5, offset=2)
    assert m.shape == (10,) and set(m.tolist()) <= {0, 1}
