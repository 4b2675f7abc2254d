"""Worker for tests/test_sgd_gpu.py: the data-parallel train step with the fused SGD, RECORDED (engine.graph.CapturedTrainStep with
the run's GradReducer) and replayed in segments around its collectives, against the eager data-parallel step.  The optimizer
launch sits behind the bucketed all-reduce's cut point, where the Adam launch of tests/dp_gpu_worker.py sits.  Five steps (two
eager warm-ups, the recording, two replays; the learning rate changes between steps 3 and 4) must agree bit for bit: losses,
every parameter, queue and BatchNorm buffer, every momentum buffer."""
import os
import sys
import types

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import oracle.fill as OF  # noqa: E402
import oracle.head as OH  # noqa: E402
import oracle.visual as OV  # noqa: E402


def main():
    dist.init_process_group(os.environ.get("TRID_DIST_BACKEND", "gloo"), init_method="env://")
    W, r = dist.get_world_size(), dist.get_rank()
    dev = torch.device("cuda", r % torch.cuda.device_count())
    torch.cuda.set_device(dev)
    from textreid_amd.backbones.gru import GRU
    from textreid_amd.backbones.m_resnet import ModifiedResNet
    from textreid_amd.caption import CaptionBatch
    from textreid_amd.embeddings.moco_head.head import MoCoHead
    from textreid_amd.engine.graph import CapturedTrainStep
    from textreid_amd.parallel import GradReducer, dp_active
    from textreid_amd.solver import FusedSGD

    assert dp_active(), "the worker checks the data-parallel step (more than one rank, or TRID_DP_FORCE=1)"
    spec, hidden, embed, vocab, C, K, NC, Bl, seed = OV.TINY, 64, 64, 200, 32, 32, 53, 4, 9
    ns = types.SimpleNamespace
    table = OF.randn("vocab_table_dp", (vocab, embed), seed, 0.5)
    vis = ModifiedResNet(list(spec.layers), spec.output_dim, spec.heads, spec.last_stride, (spec.height, spec.in_width), spec.width)
    txt = GRU(hidden, embed, embed, 1, 0.0, True, "clip_vit", "./", vocab_dict=table)
    cfg = ns(MODEL=ns(EMBEDDING=ns(FEATURE_SIZE=C, EPSILON=0.1), MOCO=ns(K=K, M=0.9, FC=False), NUM_CLASSES=NC))
    head = MoCoHead(cfg, vis, txt)
    filled = OF.fill_state(head.state_dict(), seed, "dp.")
    st = {k: v.clone() for k, v in filled.items()}
    OH.init_queues(st, seed)
    for k in ("t_queue", "v_queue", "id_queue", "queue_ptr"):
        filled[k] = st[k].clone()
    head.to(dev).train()
    Bg = Bl * W
    x = OF.randn("img:dp", (Bg, 3, spec.height, spec.in_width), seed)
    tok = OF.randint("tok:dp", 1, vocab, (Bg, 105), seed)
    ln = OF.randint("len:dp", 3, 30, (Bg,), seed)
    for i, n in enumerate(ln.tolist()):
        tok[i, n:] = 0
    ids = torch.arange(Bg) // 2
    sl = slice(r * Bl, (r + 1) * Bl)
    pre = [p for n, p in head.named_parameters() if p.requires_grad and "loss_evaluator" not in n][::-1]
    runs = {}
    for mode in ("eager", "recorded"):
        head.load_state_dict(filled)
        for p_ in head.parameters():
            p_.grad = None
        red = GradReducer(bucket_mb=1)
        head.v_encoder_q.grad_sync = red
        opt = FusedSGD([{"params": [p_], "lr": 2e-2 if n.endswith("bias") else 1e-2, "weight_decay": 0.0 if n.endswith("bias") else 4e-5}
                        for n, p_ in head.named_parameters() if p_.requires_grad], lr=1e-2, momentum=0.9)
        # (caption_bound = the batches' own maximum: the recorded text encoder runs the launch shapes of the eager one)
        runner = CapturedTrainStep(head, opt, warmup=2, caption_bound=int(ln[sl].max()), reducer=red, pre_gather=pre)
        losses = []
        for i in range(5):
            if i == 3:  # an LR scheduler step between steps 3 and 4
                for grp in opt.param_groups:
                    grp["lr"] *= 0.5
            xi = x[sl].roll(i, 0).to(dev)
            cb = CaptionBatch(tok[sl].roll(i, 0).to(dev), ln[sl].roll(i, 0).to(dev), ((ids[sl] + i) % NC).to(dev))
            out = runner._eager(xi, cb) if mode == "eager" else runner(xi, cb)
            losses.append(torch.stack([v.detach().clone() for v in out.values()]))
        torch.cuda.synchronize()
        if mode == "recorded":
            assert runner.graph is not None and not runner.disabled, "the data-parallel SGD step was not recorded"
            assert red.bytes_staged > 0 and red.bytes_post > 0
            assert len(runner.cuts) >= 3 and runner.replayer is not None, "the collectives are cut points of the stream plan"
            n_cuts = len(runner.cuts)
        bufs = [opt.state[p_]["momentum_buffer"].clone() for g_ in opt.param_groups for p_ in g_["params"]]
        runs[mode] = (torch.stack(losses), {k: v.detach().clone() for k, v in head.state_dict().items()}, bufs)
        del runner, opt
    assert bool(torch.isfinite(runs["eager"][0]).all())
    assert torch.equal(runs["eager"][0], runs["recorded"][0]), (runs["eager"][0] - runs["recorded"][0]).abs().max()
    for k, v in runs["eager"][1].items():
        assert torch.equal(v, runs["recorded"][1][k]), k
    assert not torch.equal(runs["eager"][1]["v_embed_layer.weight"], filled["v_embed_layer.weight"].to(dev))  # (the steps moved it)
    assert len(runs["eager"][2]) == len(runs["recorded"][2]) > 0
    for a, b in zip(runs["eager"][2], runs["recorded"][2]):
        assert torch.equal(a, b)
    if r == 0:
        print("DP_SGD_CAPTURED_OK backend=%s world=%d segments=%d momentum_buffers=%d" % (dist.get_backend(), W, n_cuts + 1, len(runs["eager"][2])))
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
