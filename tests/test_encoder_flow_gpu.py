"""The two image encoders compute the bits, and make the library calls, of the commit before their fp32 Bottleneck flow, eval plan
and autograd Function were merged into textreid_amd/backbones/bottleneck.py.

tests/golden/encoder_flow_parent.json was written by tests/golden/make_encoder_flow_parent.py at that parent commit (two
processes, identical files).  The same script computes the quantities here: sha256 of the train-mode output, of every parameter
gradient, of every BatchNorm buffer and of the eval-mode outputs, and the number and names of the library calls of every pass.
Nothing on these paths accumulates with atomics (test_imagenet_baseline_step_is_deterministic), so the comparison is equality."""

import importlib.util
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from test_baseline_gpu import stream_state_left_as_found  # noqa: E402,F401  (autouse: every backward pass draws a side stream from torch's pool)


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import textreid_amd  # noqa: F401

    return torch.device("cuda")


@pytest.fixture(scope="module")
def maker(golden_dir):
    spec = importlib.util.spec_from_file_location("make_encoder_flow_parent", os.path.join(golden_dir, "make_encoder_flow_parent.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def parent(golden_dir):
    return json.load(open(os.path.join(golden_dir, "encoder_flow_parent.json")))


# A: CLIP fp32 flow (stride-1 downsample, three stride-2 blocks, an identity block) + both eval passes; B: CLIP, layer4 at stride 1;
# C: ImageNet, RES5_STRIDE 1 / 2, even and odd maps, P16 and unfused eval passes; D: CLIP P16 training flow and P16 eval pass
@pytest.mark.parametrize("case", ["A", "B", "C:96x32:s1", "C:96x32:s2", "C:90x30:s1", "C:90x30:s2", "D"])
def test_encoder_bits_and_call_sequence_are_the_parents(gpu, maker, parent, case):
    assert case in maker.CASES
    got, want = maker.compute(case, gpu), parent[case]
    assert sorted(got) == sorted(want), sorted(set(got) ^ set(want))
    if case == "D":
        assert got["eval_p16_taken"] is True  # the eval pass took ModifiedResNet._run_forward_eval_p16
    differing = sorted(k for k in want if got[k] != want[k])
    print(case, len(want), "quantities,", len(differing), "differ")
    assert not differing, [(k, got[k], want[k]) for k in differing[:8]]
