"""GPU box: configs[4] match (Q = 1e4 queries x G = 1e6 gallery rows, top-10) - pre-split operands + streaming filter kernel against
the on-the-fly split GEMM; agreement of the results.  usage: python tools/retrieval_time.py [G] [Q] [--map]
--map: times the matrix-free mAP (evaluation.rank_from_embeddings, 3 positives per query on synthetic pids; plain, and the re-ranked
ranks with the gallery's neighbour lists given)
next to the top-10 match at the same Q and G and prints one bench-line JSON with the rows/s figures and their ratios."""
import json, os, sys, time
import torch
MAP = "--map" in sys.argv
sys.argv = [a for a in sys.argv if a != "--map"]
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import textreid_amd.evaluation as E
G = int(sys.argv[1]) if len(sys.argv) > 1 else 1000000
Q = int(sys.argv[2]) if len(sys.argv) > 2 else 10000
gen = torch.Generator(device="cpu").manual_seed(7)
q = torch.nn.functional.normalize(torch.randn(Q, 256, generator=gen), dim=1).cuda()
g = torch.nn.functional.normalize(torch.randn(G, 256, generator=gen), dim=1).cuda()
res = {}
ONLY = os.environ.get("TRID_RETR_ONLY_P16", "0") == "1"  # (profiling runs: 1 warm-up + 3 timed calls of the product path)
for name, flag in ((("pre-split + streaming filter", True),) if ONLY else (("on-the-fly split", False), ("pre-split + streaming filter", True)) * 2):
    E.USE_SIM_P16 = flag
    E.similarity_topk(q, g, 10, normalize=False); torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(3):
        res[name] = E.similarity_topk(q, g, 10, normalize=False)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / 3
    print("%-30s %7.2f ms  %6.1f M gallery rows/s  %5.0f TFLOP/s (fp32-equivalent)" % (name, dt * 1e3, G / dt / 1e6, 2.0 * Q * G * 256 / dt / 1e12), flush=True)
if MAP:
    E.USE_SIM_P16 = True
    qp = torch.arange(Q, device="cuda")
    gp = torch.arange(G, device="cuda") % max(G // 3, 1)  # 3 gallery rows per identity, the first Q identities queried
    line = {"Q": Q, "G": G, "C": 256, "positives_per_query": 3}
    # re-rank leg: the queries' neighbours from the real top-5 match; the gallery's own neighbour lists are GIVEN (row i: i and four
    # rows at fixed strides, every row in five lists) - the G x G match that produces them is a separate, one-off cost per gallery
    gnn = ((torch.arange(G, device="cuda").view(-1, 1) + torch.arange(5, device="cuda").view(1, -1) * 7919) % G).contiguous()

    def rerank_leg():
        return E.positive_ranks(q, g, qp, gp, E._topk_neighbours(q, g, 5), gnn, 0.05)
    legs = (("top10", lambda: E.similarity_topk(q, g, 10, normalize=False)),
            ("map", lambda: E.rank_from_embeddings(q, g, qp, gp, (1, 5, 10), normalize=False)),
            ("map_rerank", rerank_leg))
    for name, fn in legs:
        fn(); torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        line[name + "_rows_per_s"] = G / ((time.perf_counter() - t0) / 3)
    line["map_over_top10"] = line["map_rows_per_s"] / line["top10_rows_per_s"]
    line["map_rerank_over_top10"] = line["map_rerank_rows_per_s"] / line["top10_rows_per_s"]
    print(json.dumps(line), flush=True)
if ONLY or MAP:
    sys.exit(0)
a, b = res["on-the-fly split"], res["pre-split + streaming filter"]
print("indices equal:", bool(torch.equal(a[1], b[1])), " values equal:", bool(torch.equal(a[0], b[0])), " max |dv| %.1e" % float((a[0] - b[0]).abs().max()))
