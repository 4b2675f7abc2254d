#!/usr/bin/env python3
"""Step time of the baseline (EMBED_HEAD 'simple') train step: synthetic inputs of bench.py's shape (B=128, RN50,
384x128 images, 64-token captions), eager and captured, 5 warm-up + 20 timed steps, device-sync bracketed.
Prints one JSON line.  Information only: compare with `python bench.py` (the MoCo step) from the same session.

Usage:  python tools/baseline_step_time.py [--visual m_resnet50|m_resnet101|resnet50|resnet101] [--batch 128] [--warmup 5] [--steps 20]
                                           [--optimizer Adam|AdamW|SGD] [--eager]
(--optimizer: SOLVER.OPTIMIZER of the run; --eager: the eager step only)
(resnet50 / resnet101: the ImageNet ResNet of baseline_gru_rn50_ls_bs128.yaml, built from config.imagenet_cfg, 12000-word vocabulary)
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from oracle.cases import synth_batch  # noqa: E402
from textreid_amd.caption import CaptionBatch  # noqa: E402
from textreid_amd.config import baseline_cfg, imagenet_cfg  # noqa: E402
from textreid_amd.engine.graph import CapturedTrainStep  # noqa: E402
from textreid_amd.model import build_model  # noqa: E402
from textreid_amd.solver import make_optimizer  # noqa: E402


def run(mode, args, dev):
    torch.manual_seed(0)
    imagenet = args.visual in ("resnet50", "resnet101")
    cfg = imagenet_cfg(args.visual) if imagenet else baseline_cfg(args.visual)
    model = build_model(cfg, vocab_dict=None if imagenet else torch.randn(49408, 512) * 0.02).to(dev).train()
    vocab = cfg.MODEL.GRU.VOCABULARY_SIZE if imagenet else 49408
    cfg.SOLVER.OPTIMIZER = args.optimizer
    opt = make_optimizer(cfg, model)
    runner = CapturedTrainStep(model, opt, warmup=2, caption_bound=64)
    batches = [tuple(x.to(dev) for x in synth_batch(args.batch, s, 3)) for s in range(4)]

    def step(i):
        images, tokens, lengths, ids = batches[i % len(batches)]
        cb = CaptionBatch(tokens % vocab, lengths, ids % 11003, max_len=64)  # (ids of the nn.Embedding vocabulary)
        return runner._eager(images, cb) if mode == "eager" else runner(images, cb)

    for i in range(args.warmup):
        ld = step(i)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(args.warmup, args.warmup + args.steps):
        ld = step(i)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / args.steps
    if mode == "captured" and runner.graph is None:
        raise RuntimeError("the step was not captured")
    return {"ms_per_step": round(dt * 1e3, 3), "pairs_per_s": round(args.batch / dt, 1), "losses": {k: float(v) for k, v in ld.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--visual", default="m_resnet50", choices=["m_resnet50", "m_resnet101", "resnet50", "resnet101"])
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--optimizer", default="Adam", choices=["Adam", "AdamW", "SGD"])
    ap.add_argument("--eager", action="store_true", help="time the eager step only")
    args = ap.parse_args()
    dev = torch.device("cuda")
    out = {"workload": "baseline_step", "visual": args.visual, "batch": args.batch, "warmup": args.warmup, "steps": args.steps}
    if args.optimizer != "Adam":
        out["optimizer"] = args.optimizer
    for mode in ("eager",) if args.eager else ("eager", "captured"):
        out[mode] = run(mode, args, dev)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
