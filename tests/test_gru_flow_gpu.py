"""The BiGRU text encoder computes the bits, and makes the library calls, of the commit before its two autograd Functions (one
layer / stacked) were merged into one and its four cell kernels into one templated pair (csrc/gru_step.hip).

tests/golden/gru_flow_parent.json was written by tests/golden/make_gru_flow_parent.py at that parent commit (two processes,
identical files).  The same script computes the quantities here: sha256 of the train-mode output, of every parameter gradient,
of every keep mask and layer input, of a no_grad and an eval forward, and per pass the number of library calls and the sha256 of
their ordered (entry point, scalar arguments).  Nothing on these paths accumulates with atomics (the parent's two processes
agreed), so the comparison is equality: no tolerance."""

import importlib.util
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

_MAKER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "make_gru_flow_parent.py")


def _load_maker():
    spec = importlib.util.spec_from_file_location("make_gru_flow_parent", _MAKER)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


maker = _load_maker()


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import textreid_amd  # noqa: F401

    return torch.device("cuda")


@pytest.fixture(scope="module")
def parent(golden_dir):
    return json.load(open(os.path.join(golden_dir, "gru_flow_parent.json")))


def test_every_recorded_case_is_recomputed(parent):
    assert sorted(parent) == sorted(maker.CASES)


# table / embedding / linear: the three input forms, depths 1-3, fused and unfused steps; dropout: two training steps and the
# frozen module; splitk: L*B >= 1024; bound: a bound_only batch two steps longer than its captions; precision: ops.CONV_PRECISION
# 16 and 6; h48: an H the step kernels refuse (the automatic fall-back to the GEMM + cell form)
@pytest.mark.parametrize("case", maker.CASES)
def test_gru_bits_and_call_sequence_are_the_parents(gpu, parent, case):
    got, want = maker.compute(case, gpu), parent[case]
    assert sorted(got) == sorted(want), sorted(set(got) ^ set(want))
    differing = sorted(k for k in want if got[k] != want[k])
    print(case, len(want), "quantities,", len(differing), "differ")
    assert not differing, [(k, got[k], want[k]) for k in differing[:8]]
