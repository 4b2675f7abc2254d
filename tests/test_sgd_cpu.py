"""Host side of the fused SGD (textreid_amd.solver.FusedSGD, lib/solver/build.py:19-22): the public surface, the refusals
torch.optim.SGD makes, and state-dict interchange with torch.optim.SGD in both directions.  Nothing here launches a kernel."""

import pytest
import torch


def _tiny_cfg():
    from textreid_amd.config import baseline_cfg

    cfg = baseline_cfg("m_resnet50", height=96, width=32, num_classes=53)
    cfg.MODEL.EMBEDDING.FEATURE_SIZE = 32
    cfg.MODEL.GRU.NUM_UNITS = 64
    cfg.MODEL.GRU.VOCABULARY_SIZE = 64
    cfg.MODEL.GRU.EMBEDDING_SIZE = 64
    cfg.SOLVER.OPTIMIZER = "SGD"
    return cfg


def test_make_optimizer_sgd_returns_the_fused_optimizer():
    from textreid_amd.model import build_model
    from textreid_amd.solver import FusedSGD, make_optimizer

    cfg = _tiny_cfg()
    model = build_model(cfg, vocab_dict=torch.randn(100, 64))
    opt = make_optimizer(cfg, model)
    assert isinstance(opt, FusedSGD) and isinstance(opt, torch.optim.Optimizer)
    named = [(k, p) for k, p in model.named_parameters() if p.requires_grad]
    assert len(opt.param_groups) == len(named)
    assert any("bias" in k for k, _ in named)
    for (k, p), grp in zip(named, opt.param_groups):
        assert len(grp["params"]) == 1 and grp["params"][0] is p
        assert grp["momentum"] == cfg.SOLVER.SGD_MOMENTUM and grp["dampening"] == 0 and grp["nesterov"] is False
        if "bias" in k:
            assert grp["lr"] == cfg.SOLVER.BASE_LR * cfg.SOLVER.BIAS_LR_FACTOR and grp["weight_decay"] == cfg.SOLVER.WEIGHT_DECAY_BIAS
        else:
            assert grp["lr"] == cfg.SOLVER.BASE_LR and grp["weight_decay"] == cfg.SOLVER.WEIGHT_DECAY
    ref = make_optimizer(cfg, model, fused=False)
    assert type(ref) is torch.optim.SGD and len(ref.param_groups) == len(named)
    assert all(g["momentum"] == cfg.SOLVER.SGD_MOMENTUM for g in ref.param_groups)
    for name in ("prepare_capture", "finish_capture", "advance_for_replay"):  # what engine.graph.CapturedTrainStep drives
        assert callable(getattr(opt, name))


def test_fused_adam_keeps_its_surface_on_the_shared_base():
    from textreid_amd.solver import FusedAdam

    opt = FusedAdam([torch.nn.Parameter(torch.zeros(3))], lr=1e-2)
    assert isinstance(opt, torch.optim.Optimizer)
    assert opt.defaults == dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0) and opt.decoupled is False


def test_constructor_refusals():
    from textreid_amd.solver import FusedSGD

    p = lambda: [torch.nn.Parameter(torch.zeros(3))]
    with pytest.raises(ValueError):
        FusedSGD(p(), lr=0.1, momentum=0.0, nesterov=True)
    with pytest.raises(ValueError):
        FusedSGD(p(), lr=0.1, momentum=0.9, dampening=0.1, nesterov=True)
    with pytest.raises(ValueError):
        FusedSGD(p(), lr=-1.0)
    FusedSGD(p(), lr=0.1, momentum=0.9, nesterov=True)
    a, b = torch.nn.Parameter(torch.zeros(3)), torch.nn.Parameter(torch.zeros(3))
    opt = FusedSGD([{"params": [a]}, {"params": [b], "momentum": 0.5}], lr=0.1, momentum=0.9)
    a.grad, b.grad = torch.ones(3), torch.ones(3)
    with pytest.raises(RuntimeError, match="momentum"):
        opt.step()
    for key, val in (("dampening", 0.2), ("nesterov", True)):
        opt = FusedSGD([{"params": [a]}, {"params": [b], key: val}], lr=0.1, momentum=0.9)
        with pytest.raises(RuntimeError, match=key):
            opt.step()


def test_state_dict_interchange_with_torch_sgd():
    from textreid_amd.solver import FusedSGD

    torch.manual_seed(0)
    shapes = [(7, 3), (5,), (2, 2, 3, 3)]
    mk = lambda: [torch.nn.Parameter(torch.randn(s)) for s in shapes]
    groups = lambda ps: [{"params": [p], "lr": 0.1 * (i + 1), "weight_decay": 0.01 * i} for i, p in enumerate(ps)]
    tp = mk()
    topt = torch.optim.SGD(groups(tp), lr=0.1, momentum=0.9)
    for _ in range(2):
        for p in tp[:2]:  # the third parameter never has a gradient ...
            p.grad = torch.randn_like(p)
        topt.step()
    saved = topt.state_dict()
    # ... and gets an entry synthesised by hand: this state_dict() holds none for it.  {"momentum_buffer": None} is a form
    # checkpoints of torch.optim.SGD can carry, and the loader has to take it
    saved["state"][2] = {"momentum_buffer": None}
    fp = mk()
    fopt = FusedSGD(groups(fp), lr=0.5, momentum=0.9)
    fopt._plan = {"stale": True}
    fopt.load_state_dict(saved)
    assert fopt._plan is None  # cached pointer tables do not survive a load
    assert [g["lr"] for g in fopt.param_groups] == [g["lr"] for g in topt.param_groups]
    for a, b in zip(fp[:2], tp[:2]):
        assert torch.equal(fopt.state[a]["momentum_buffer"], topt.state[b]["momentum_buffer"])
    assert "momentum_buffer" not in fopt.state[fp[2]]  # first-update rule still ahead of it
    # ... and back: what FusedSGD writes loads into torch.optim.SGD
    back = fopt.state_dict()
    tp2 = [torch.nn.Parameter(p.detach().clone()) for p in tp]
    topt2 = torch.optim.SGD(groups(tp2), lr=0.1, momentum=0.9)
    topt2.load_state_dict(back)
    for a, b in zip(tp2[:2], tp[:2]):
        assert torch.equal(topt2.state[a]["momentum_buffer"], topt.state[b]["momentum_buffer"])
    for p in tp2 + tp:
        p.grad = torch.ones_like(p)
    topt2.step()
    topt.step()  # the loaded optimizer continues as the original does
    for a, b in zip(tp2[:2], tp[:2]):
        assert torch.equal(topt2.state[a]["momentum_buffer"], topt.state[b]["momentum_buffer"])
    import copy
    import pickle

    again = pickle.loads(pickle.dumps(fopt))
    assert again._plan is None and again._fresh == set()
    assert copy.deepcopy(fopt.state_dict())["param_groups"][0]["momentum"] == 0.9


def test_header_declares_the_sgd_entry_point():
    from textreid_amd import lib

    assert "trid_sgd_multi_f32" in lib.EXPORTS
    ret, sig = lib.DECLS["trid_sgd_multi_f32"]
    assert ret == "int" and sig == "pppppppppp" + "ii" + "f" + "i" + "p"
