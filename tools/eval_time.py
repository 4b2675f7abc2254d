"""GPU box: eval-mode image encoder (gallery encode, inference.py:14-26) - the P16 kernels with fused eval epilogues against the
round-2 path (BatchNorm-folded filters, on-the-fly split) and the unfolded pass; agreement of the outputs; images / s per batch size.
usage: python tools/eval_time.py [rn50|rn101] [batch sizes ...]
       python tools/eval_time.py --visual resnet50|resnet101 [batch sizes ...] [--json PATH]
--visual: the ImageNet encoder (backbones/resnet.py) - its P16 eval pass against the unfused pass (TRID_EVAL_P16=0: the training data
flow on running-statistics coefficients), alternated twice per batch size, then the event time of every library call of ONE fused
pass grouped by entry point; --json writes the figures."""
import os, sys, time
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def imagenet_main(argv):
    import collections, json
    from textreid_amd import lib, ops
    from textreid_amd.backbones.resnet import ResNet, model_archs

    arch = argv[argv.index("--visual") + 1]
    out_path = argv[argv.index("--json") + 1] if "--json" in argv else None
    sizes = [int(a) for a in argv if a.isdigit()] or [128, 512]
    torch.manual_seed(0)
    m = ResNet(model_archs[arch], 1).cuda()  # RES5_STRIDE 1, as baseline_gru_rn50_ls_bs128.yaml
    res = {"visual": arch, "input": [3, 384, 128], "device": torch.cuda.get_device_name(0), "runs": [], "calls": {}}
    with torch.no_grad():
        m.train()
        for _ in range(3):
            m(torch.randn(32, 3, 384, 128, device="cuda"))  # running statistics away from their initial values
        m.eval()
        for B in sizes:
            x = torch.randn(B, 3, 384, 128, device="cuda")
            outs = {}
            for name, p16 in (("unfused", False), ("P16 eval", True)) * 2:
                ops.USE_EVAL_P16 = p16
                for _ in range(2):
                    outs[name] = m(x)
                torch.cuda.synchronize()
                n = max(5, 2048 // B)
                t0 = time.perf_counter()
                for _ in range(n):
                    m(x)
                th = time.perf_counter() - t0
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                res["runs"].append({"B": B, "path": name, "ms_per_batch": dt * 1e3 / n, "host_enqueue_ms": th * 1e3 / n, "imgs_per_s": n * B / dt})
                print("B %4d %-9s %7.2f ms/batch (host enqueue %6.2f)  %7.0f imgs/s" % (B, name, dt * 1e3 / n, th * 1e3 / n, n * B / dt), flush=True)
            ref = outs["unfused"].double()
            err = float((outs["P16 eval"].double() - ref).abs().max() / ref.abs().max())
            res["runs"].append({"B": B, "fused_vs_unfused_max_rel_err": err})
            print("   P16 eval vs unfused: max rel err %.1e" % err)
        # event time of every library call of one fused pass at the first batch size
        B = sizes[0]
        x = torch.randn(B, 3, 384, 128, device="cuda")
        for name, p16 in (("unfused", False), ("P16 eval", True)):
            ops.USE_EVAL_P16 = p16
            m(x)
            torch.cuda.synchronize()
            lib.TRACE = []
            m(x)
            torch.cuda.synchronize()
            tr, lib.TRACE = lib.TRACE, None
            kinds = collections.defaultdict(lambda: [0, 0.0])
            for fn, scal, e0, e1 in tr:
                kinds[fn][0] += 1
                kinds[fn][1] += e0.elapsed_time(e1) * 1e3
            tot = sum(v[1] for v in kinds.values())
            print("%s, B = %d: %d calls, %.2f ms of event time" % (name, B, len(tr), tot / 1e3))
            for fn, (cnt, us) in sorted(kinds.items(), key=lambda kv: -kv[1][1]):
                print("  %8.1f us  x%-3d %s" % (us, cnt, fn))
            res["calls"][name] = {"B": B, "n_calls": len(tr), "event_ms": tot / 1e3, "by_entry_us": {fn: [cnt, round(us, 1)] for fn, (cnt, us) in kinds.items()}}
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1, sort_keys=True)


if "--visual" in sys.argv:
    imagenet_main(sys.argv[1:])
    sys.exit(0)
import oracle.visual as OV
from textreid_amd import ops
from textreid_amd.backbones.m_resnet import ModifiedResNet
spec = OV.RN101 if (len(sys.argv) > 1 and sys.argv[1] == "rn101") else OV.RN50
sizes = [int(a) for a in sys.argv[2:] if a.isdigit()] or [128]
ONLY_P16 = "--only-p16" in sys.argv  # (profiling runs)
torch.manual_seed(0)
m = ModifiedResNet(list(spec.layers), spec.output_dim, spec.heads, spec.last_stride, (spec.height, spec.in_width), spec.width).cuda()
with torch.no_grad():
    m.train()
    for _ in range(3):
        m(torch.randn(32, 3, 384, 128, device="cuda"))  # running statistics away from their initial values
    m.eval()
    for B in sizes:
        x = torch.randn(B, 3, 384, 128, device="cuda")
        outs = {}
        for name, fold, p16 in ((("P16 eval", True, True),) if ONLY_P16 else (("unfolded", False, False), ("folded (r02)", True, False), ("P16 eval", True, True)) * 2):
            m.fold_eval_bn, ops.USE_EVAL_P16 = fold, p16
            outs[name] = m(x); torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(10): m(x)
            th = time.perf_counter() - t0
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            print("B %4d %-13s %7.2f ms/batch (host enqueue %6.2f)  %7.0f imgs/s" % (B, name, dt * 100, th * 100, 10 * B / dt), flush=True)
        if ONLY_P16:
            continue
        ref = outs["unfolded"].double()
        for k in ("folded (r02)", "P16 eval"):
            print("   %-13s vs unfolded: max rel err %.1e" % (k, float((outs[k].double() - ref).abs().max() / ref.abs().max())))
