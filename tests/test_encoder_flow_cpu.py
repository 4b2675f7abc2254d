"""The two image encoders share ONE fp32 Bottleneck flow, eval plan, Function and base class (textreid_amd/backbones/bottleneck.py).
These checks pin the hooks that such a move can disconnect without any test noticing: the switch globals bench.py and the tests
set on m_resnet, the late-read size limit of resnet.py, the ops wrappers tests replace, and the parameter / state-dict order."""

import hashlib
import importlib
import inspect
import json
import os
import pkgutil
import re
import types

import textreid_amd.backbones as BK
from textreid_amd.backbones import bottleneck as S
from textreid_amd.backbones import m_resnet as M
from textreid_amd.backbones import resnet as R

SWITCHES = {"_SERIAL_WGRAD", "_SERIAL_ATTN_WGRAD", "_EARLY_WPT", "_BATCH_WGRAD", "_MASKED_ACC", "_BN3_FUSE", "_BN3_FUSE_MIN_PLANES"}


def _names(code):
    out = set(code.co_names)
    for c in code.co_consts:
        if isinstance(c, types.CodeType):
            out |= _names(c)
    return out


def _functions():
    """[(name or Class.name, function)] of every function and method reachable in the modules of textreid_amd.backbones."""
    found = []

    def add(obj, owner):
        if isinstance(obj, (staticmethod, classmethod)):
            obj = obj.__func__
        if isinstance(obj, property):
            obj = obj.fget
        if isinstance(obj, types.FunctionType) and obj.__module__.startswith(BK.__name__):
            found.append((owner + obj.__name__, obj))

    for info in pkgutil.iter_modules(BK.__path__):
        mod = importlib.import_module(BK.__name__ + "." + info.name)
        for name, obj in vars(mod).items():
            if inspect.isclass(obj) and obj.__module__.startswith(BK.__name__):
                for attr in vars(obj).values():
                    add(attr, obj.__name__ + ".")
            else:
                add(obj, "")
    return found


def test_switch_readers_live_in_m_resnet():
    """bench.py --full and test_schedule_and_fusion_switches_leave_the_gradients_alone SET the switches on m_resnet: a reader
    defined in another module would read its own copy and the switch would do nothing."""
    readers = [(q, f) for q, f in _functions() if _names(f.__code__) & SWITCHES]
    wrong = [q for q, f in readers if f.__globals__ is not vars(M)]
    assert not wrong, wrong
    found = {q for q, _ in readers}
    for q in ("_WgradStream.run", "_WgradStream.defer", "_WgradStream.flush", "block_backward_p16", "ModifiedResNet._run_forward"):
        assert q in found, (q, sorted(found))


def test_p16_size_limit_is_read_at_call_time(monkeypatch):
    assert R.eval_p16_shape_ok(2, 72, 40)
    monkeypatch.setattr(R, "P16_LIMIT_BYTES", 1 << 16)
    assert not R.eval_p16_shape_ok(2, 72, 40)
    monkeypatch.undo()
    assert R.eval_p16_shape_ok(2, 72, 40)


def test_shared_module_binds_no_ops_wrapper_by_name():
    """Tests replace ops.<wrapper> with counting wrappers: the shared flows must look them up at call time."""
    for name in ("conv_eval_p16", "conv3x3_s2_eval_p16", "subsample2_p16", "bn_apply", "conv1x1", "conv3x3"):
        assert not hasattr(S, name), name
    from textreid_amd import ops

    assert S.ops is ops


def test_parameter_and_state_order_are_the_parents(golden_dir, tmp_path):
    want = json.load(open(os.path.join(golden_dir, "encoder_flow_parent.json")))["names"]
    for tag, m, blk_cls in (("clip", M.ModifiedResNet([3, 4, 6, 3], 1024, 32, 1, (384, 128)), M.Bottleneck),
                            ("imagenet", R.ResNet(R.model_archs["resnet50"], 2, pretrained=None, root=str(tmp_path)), R.Bottleneck)):
        params, state = [k for k, _ in m.named_parameters()], list(m.state_dict())
        assert hashlib.sha256("\n".join(params).encode()).hexdigest() == want[tag + ":parameters"], tag
        assert hashlib.sha256("\n".join(state).encode()).hexdigest() == want[tag + ":state_dict"], tag
        for attr in ("down_conv", "down_bn", "pooled_stride"):
            assert hasattr(blk_cls, attr), (tag, attr)
        blk = m.layer2[0]
        assert isinstance(blk, blk_cls) and blk.downsample is not None
        assert blk.down_conv.weight.dim() == 4 and blk.down_bn.running_mean.dim() == 1 and blk.pooled_stride is (tag == "clip")
        assert list(m.state_dict()) == state and [k for k, _ in m.named_parameters()] == params
    assert M.Bottleneck.pooled_stride is True and R.Bottleneck.pooled_stride is False


def test_one_definition_of_the_shared_flow():
    for name in ("forward", "_eval_plan", "blocks", "_to_channels_last"):
        assert getattr(R.ResNet, name) is getattr(M.ModifiedResNet, name) is getattr(S.BottleneckEncoder, name), name
    # the ImageNet pass calls the module attributes tests/test_blocks_gpu.py reaches as M.block_forward / M.block_backward
    assert "block_forward" in R.ResNet._run_forward.__code__.co_names and "block_backward" in R.ResNet._run_backward.__code__.co_names
    assert R.ResNet._run_forward.__globals__["block_forward"] is M.block_forward is S.block_forward
    assert R.ResNet._run_backward.__globals__["block_backward"] is M.block_backward is S.block_backward
    src = "".join(open(inspect.getsourcefile(mod)).read() for mod in (S, M, R))  # (gru.py has the text encoder's own Functions)
    for pat in (r"def block_forward\(", r"def block_backward\(", r"def _eval_plan\(", r"def blocks\(", r"def _to_channels_last\(",
                r"class \w+\(torch\.autograd\.Function\)"):
        assert len(re.findall(pat, src)) == 1, pat
