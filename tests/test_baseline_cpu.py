"""Host-side checks of the baseline path (``EMBED_HEAD: 'simple'``): construction, state-dict names against the
list captured from the reference (tests/golden/simple_head.npz), optimizer groups, checkpoint ingestion, and the
"no CPU fallback" rule of the three added losses.  No GPU needed."""

import os
from collections import OrderedDict

import numpy as np
import pytest
import torch

import oracle.fill as OF


def _tiny_cfg(head="simple", visual="m_resnet50"):
    """The baseline configs' keys at tiny sizes (a supplied vocab table instead of the CLIP one on disk)."""
    from textreid_amd.config import baseline_cfg

    cfg = baseline_cfg(visual, height=96, width=32, num_classes=53)
    cfg.MODEL.EMBEDDING.EMBED_HEAD = head
    cfg.MODEL.EMBEDDING.FEATURE_SIZE = 32
    cfg.MODEL.GRU.NUM_UNITS = 64
    cfg.MODEL.GRU.VOCABULARY_SIZE = 64
    cfg.MODEL.GRU.EMBEDDING_SIZE = 64
    cfg.MODEL.MOCO.K = 32
    return cfg


def _fixture_model():
    """The model of simple_head.npz: TINY visual spec + small BiGRU + simple head, built from its parts."""
    import types

    import oracle.visual as OV
    from textreid_amd.backbones.gru import GRU
    from textreid_amd.backbones.m_resnet import ModifiedResNet
    from textreid_amd.embeddings import build_embed
    from textreid_amd.model import Model

    ns = types.SimpleNamespace
    spec = OV.TINY
    m = Model.__new__(Model)
    torch.nn.Module.__init__(m)
    m.visual_model = ModifiedResNet(list(spec.layers), spec.output_dim, spec.heads, spec.last_stride, (spec.height, spec.in_width), spec.width)
    m.textual_model = GRU(64, 64, 64, 1, 0.0, True, "clip_vit", "./", vocab_dict=OF.randn("vocab_table_base", (200, 64), 5, 0.5))
    cfg = ns(MODEL=ns(EMBEDDING=ns(EMBED_HEAD="simple", FEATURE_SIZE=32, EPSILON=0.1), NUM_CLASSES=53))
    m.embed_model = build_embed(cfg, m.visual_model.out_channels, m.textual_model.out_channels)
    m.embed_type = "normal"
    m._text_stream = None
    return m


@pytest.mark.parametrize("visual", ["m_resnet50", "m_resnet101"])
def test_build_model_baseline_configs(visual):
    from textreid_amd.embeddings.simple_head.head import SimpleHead
    from textreid_amd.model import build_model

    cfg = _tiny_cfg(visual=visual)
    model = build_model(cfg, vocab_dict=torch.randn(100, 64))
    assert model.embed_type == "normal" and isinstance(model.embed_model, SimpleHead)
    names = list(model.state_dict())
    head = [k for k in names if k.startswith("embed_model.")]
    assert head == ["embed_model.visual_embed_layer.weight", "embed_model.visual_embed_layer.bias", "embed_model.textual_embed_layer.weight",
                    "embed_model.textual_embed_layer.bias", "embed_model.loss_evaluator.projection"]
    assert not any("encoder" in k or "queue" in k for k in names)  # no key encoders, queues or aliases
    assert all(k.split(".")[0] in ("visual_model", "textual_model", "embed_model") for k in names)
    sd = model.state_dict()
    assert tuple(sd["embed_model.loss_evaluator.projection"].shape) == (32, 53)
    assert tuple(sd["embed_model.visual_embed_layer.weight"].shape) == (32, model.visual_model.out_channels)
    assert tuple(sd["embed_model.textual_embed_layer.weight"].shape) == (32, 128)
    assert float(sd["embed_model.visual_embed_layer.bias"].abs().max()) == 0.0  # _init_weight: zero bias on the head's Linears


def test_default_config_head_builds():
    """'simple' is the default EMBED_HEAD of config.py: a config that names no head builds the baseline model."""
    from textreid_amd.config import get_cfg_defaults
    from textreid_amd.model import build_model

    cfg = _tiny_cfg()
    assert get_cfg_defaults().MODEL.EMBEDDING.EMBED_HEAD == cfg.MODEL.EMBEDDING.EMBED_HEAD == "simple"
    assert build_model(cfg, vocab_dict=torch.randn(100, 64)).embed_type == "normal"


def test_state_dict_names_and_shapes_equal_the_reference(golden_dir):
    g = np.load(os.path.join(golden_dir, "simple_head.npz"))
    want = OrderedDict((str(k), tuple(int(d) for d in str(s).split(",")) if str(s) else ()) for k, s in zip(g["state_names"], g["state_shapes"]))
    got = OrderedDict((k, tuple(v.shape)) for k, v in _fixture_model().state_dict().items())
    assert list(got) == list(want)  # same names in the same order
    assert got == want
    assert [k for k, p in _fixture_model().named_parameters() if p.requires_grad] == [str(k) for k in g["trainable_names"]]


def test_unknown_head_raises_and_moco_is_unchanged():
    from textreid_amd.embeddings import build_embed
    from textreid_amd.embeddings.moco_head.head import MoCoHead
    from textreid_amd.model import build_model

    with pytest.raises(NotImplementedError):
        build_model(_tiny_cfg(head="fancy"), vocab_dict=torch.randn(100, 64))
    with pytest.raises(NotImplementedError):
        build_embed(_tiny_cfg(head="moco"), 64, 128)  # the MoCo head is not built through build_embed (embeddings/build.py:4-9)
    moco = build_model(_tiny_cfg(head="moco"), vocab_dict=torch.randn(100, 64))
    assert moco.embed_type == "moco" and isinstance(moco.embed_model, MoCoHead)
    names = list(moco.state_dict())
    for k in ("embed_model.v_encoder_q.conv1.weight", "embed_model.v_encoder_k.conv1.weight", "embed_model.t_encoder_k.gru.weight_ih_l0",
              "embed_model.v_embed_layer.weight", "embed_model.t_queue", "embed_model.id_queue", "embed_model.queue_ptr",
              "embed_model.loss_evaluator.projection", "visual_model.conv1.weight", "textual_model.gru.weight_hh_l0"):
        assert k in names
    base = list(build_model(_tiny_cfg(), vocab_dict=torch.randn(100, 64)).state_dict())
    # MoCo = the baseline's encoders + the head's aliases of them, key copies, queues and its own embed layers
    assert [k for k in names if not k.startswith("embed_model.")] == [k for k in base if not k.startswith("embed_model.")]


def test_make_optimizer_one_group_per_trainable_tensor():
    from textreid_amd.model import build_model
    from textreid_amd.solver import make_optimizer

    cfg = _tiny_cfg()
    model = build_model(cfg, vocab_dict=torch.randn(100, 64))
    opt = make_optimizer(cfg, model, fused=False)
    named = [(k, p) for k, p in model.named_parameters() if p.requires_grad]
    assert len(opt.param_groups) == len(named) == len(list(model.parameters()))  # nothing frozen, nothing aliased
    for (k, p), grp in zip(named, opt.param_groups):
        assert len(grp["params"]) == 1 and grp["params"][0] is p
        if "bias" in k:
            assert grp["lr"] == cfg.SOLVER.BASE_LR * cfg.SOLVER.BIAS_LR_FACTOR and grp["weight_decay"] == cfg.SOLVER.WEIGHT_DECAY_BIAS
        else:
            assert grp["lr"] == cfg.SOLVER.BASE_LR and grp["weight_decay"] == cfg.SOLVER.WEIGHT_DECAY


@pytest.mark.parametrize("prefix", ["", "module."])
def test_reference_baseline_checkpoint_loads(golden_dir, prefix):
    """A state dict with the reference's baseline keys (names from the fixture, optionally `module.`-prefixed, wrapped as a
    best.pth's "model" entry) loads through the suffix aligner: every key lands, strictly, with its own values."""
    from textreid_amd.checkpoint import load_reference_state

    g = np.load(os.path.join(golden_dir, "simple_head.npz"))
    shapes = {str(k): tuple(int(d) for d in str(s).split(",")) if str(s) else () for k, s in zip(g["state_names"], g["state_shapes"])}
    model = _fixture_model()
    own = model.state_dict()
    ckpt = OrderedDict()
    for k, shp in shapes.items():
        ckpt[prefix + k] = OF.fill("ckpt." + k, shp, 3) if own[k].dtype.is_floating_point else torch.full(shp, 4, dtype=own[k].dtype)
    assert set(shapes) == set(own)  # no missing, no unexpected key
    load_reference_state(model, {"model": ckpt, "epoch": 3})
    for k, v in model.state_dict().items():
        assert torch.equal(v, ckpt[prefix + k]), k


def test_new_losses_refuse_cpu_tensors():
    from textreid_amd import losses as L

    v, t, p = torch.randn(4, 8), torch.randn(4, 8), torch.randn(8, 11)
    lab = torch.tensor([0, 1, 1, 2])
    for fn in (lambda: L.cmpm_loss(v, t, lab), lambda: L.cmpm_loss(v, t, lab, verbose=True), lambda: L.cmpc_loss(p, v, t, lab),
               lambda: L.cmpc_loss(p, v, t, lab, verbose=True), lambda: L.global_align_loss_from_sim(v @ t.t(), lab)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn()


def test_data_parallel_refuses_the_simple_head(monkeypatch):
    import textreid_amd.model as M

    monkeypatch.setattr(M, "dp_active", lambda: True)
    with pytest.raises(NotImplementedError, match="data parallelism"):
        M.build_model(_tiny_cfg(), vocab_dict=torch.randn(100, 64))


def test_baseline_model_refuses_cpu_images():
    from textreid_amd.caption import CaptionBatch
    from textreid_amd.model import build_model

    model = build_model(_tiny_cfg(), vocab_dict=torch.randn(100, 64)).eval()
    cb = CaptionBatch(torch.ones(2, 8, dtype=torch.int64), torch.tensor([3, 4]), torch.tensor([0, 1]))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        model(torch.randn(2, 3, 96, 32), cb)
