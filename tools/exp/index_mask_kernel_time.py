"""GPU box: the one-pass GalleryIndex kernels alone (events around trid_index_search_p16 / trid_index_search_masked_p16, merge launch
included), ONE index and the same buffers for every form, alternating, 30 calls each after 3 warm-ups: unmasked, masked with an all-ones
mask, masked with 10 % of the rows disallowed; G = 1e6, Q = 1 and 32, k = 10.  One JSON line.  Separates the kernel's own cost of the
allow bits from the host path and from the placement of a second gallery that tools/retrieval_time.py --index --masked also sees.
usage: python tools/exp/index_mask_kernel_time.py"""
import json, os, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from textreid_amd import GalleryIndex, lib as L, ops
from textreid_amd.ops import _p, stream
G, K = 1000000, 10
gen = torch.Generator(device="cpu").manual_seed(7)
idx = GalleryIndex(capacity=G)
idx.add((torch.randn(G, 256, generator=gen) * 3.0).cuda())
gone = torch.rand(G, generator=gen) < 0.1
nw = (G + 31) // 32
ones = torch.full((nw,), -1, dtype=torch.int32, device="cuda")
w10 = torch.zeros(nw, dtype=torch.int32, device="cuda")
L.call("trid_index_pack_mask_u32", None, _p((~gone).cuda()), G, _p(w10), nw, stream())
out = {"lib": os.environ.get("TRID_LIB_PATH", "product")}
for Q in (1, 32):
    q = ops.l2norm_rows((torch.randn(Q, 256, generator=gen)).cuda())[0]
    q16 = torch.zeros(32, 256, device="cuda")
    q16[:Q] = ops.p16_pack(q, amax_=idx.unit_amax).data
    ws = torch.empty(L.load().trid_index_search_ws_bytes(G, 32, 16, 0), dtype=torch.uint8, device="cuda")
    v = torch.empty(Q, K, device="cuda"); r = torch.empty(Q, K, dtype=torch.int64, device="cuda")
    forms = {"unmasked": lambda: L.call("trid_index_search_p16", _p(q16), _p(idx.rows_p16), _p(idx.unit_amax), Q, G, K, 0, _p(v), _p(r), _p(ws), 0, stream()),
             "masked_ones": lambda: L.call("trid_index_search_masked_p16", _p(q16), _p(idx.rows_p16), _p(idx.unit_amax), _p(ones), Q, G, K, 0, _p(v), _p(r), _p(ws), 0, stream()),
             "masked_10pct": lambda: L.call("trid_index_search_masked_p16", _p(q16), _p(idx.rows_p16), _p(idx.unit_amax), _p(w10), Q, G, K, 0, _p(v), _p(r), _p(ws), 0, stream())}
    for f in forms.values():
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    t = {n: [] for n in forms}
    for _ in range(30):
        for n, f in forms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); f(); e1.record(); torch.cuda.synchronize()
            t[n].append(e0.elapsed_time(e1) * 1e3)
    out["Q%d" % Q] = {n: {"median_us": sorted(x)[15], "min_us": min(x), "max_us": max(x)} for n, x in t.items()}
print(json.dumps(out), flush=True)
