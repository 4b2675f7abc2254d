"""The retrieval host paths (similarity_topk, GalleryIndex.search beyond 32 queries, the matrix-free rank passes, their sharded
forms in one process, evaluation) compute the bits, and make the library calls, of the commit before they were reduced to one
launch sequence, one shard merge and one count pass.

tests/golden/retrieval_parent.json was written by tests/golden/make_retrieval_parent.py at that parent commit (two processes,
identical files).  The same script computes the quantities here: sha256 of every returned tensor and the multiset of (entry
point, scalar arguments) of the library calls.  Every result on these paths is an integer count or comes out of a deterministic
merge, so the comparison is equality."""

import importlib.util
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import textreid_amd  # noqa: F401

    return torch.device("cuda")


@pytest.fixture(scope="module")
def maker(golden_dir):
    spec = importlib.util.spec_from_file_location("make_retrieval_parent", os.path.join(golden_dir, "make_retrieval_parent.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def parent(golden_dir):
    return json.load(open(os.path.join(golden_dir, "retrieval_parent.json")))


CASES = ["topk:256:1x8193x3", "topk:256:70x8261x10", "topk:256:33x8255x1", "topk:64:5x8192x10", "topk:64:5x8193x3",
         "topk:overflow:host", "topk:overflow:gated", "index:9001", "index:5000",
         "rank:ties9001", "rank:ties20011", "rank:ties9001:panel", "rank:ties9001:chunk", "rank:rnd256", "rank:rnd64",
         "sharded:ties9001", "sharded:rnd256",
         "evaluation:free:re", "evaluation:free:plain", "evaluation:matrix:re", "evaluation:matrix:plain"]


def test_the_cases_are_the_recorded_ones(maker, parent):
    assert CASES == maker.CASES and sorted(CASES) == sorted(parent)


@pytest.mark.parametrize("case", CASES)
def test_retrieval_bits_and_calls_are_the_parents(gpu, maker, parent, case):
    got, want = maker.compute(case, gpu), parent[case]
    assert sorted(got) == sorted(want), sorted(set(got) ^ set(want))
    differing = sorted(k for k in want if got[k] != want[k])
    print(case, len(want), "quantities,", len(differing), "differ")
    if "calls" in differing:
        print("calls:", sorted(set(got["calls"].items()) ^ set(want["calls"].items())))
    assert not differing, [(k, got[k], want[k]) for k in differing if k != "calls"][:8]
    if case.startswith("sharded:"):  # one process, no process group: the tensors of the unsharded entry points on the same inputs
        one = parent["rank:" + case.split(":", 1)[1]]
        assert [k for k in got if k != "calls" and got[k] != one[k]] == []
