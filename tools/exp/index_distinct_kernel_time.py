"""GPU box: the one-pass GalleryIndex kernels alone (events around trid_index_search_p16 / _masked_p16 / _distinct_p16, merge launch
included), ONE index of 1e6 rows with 4 rows per pid and the same buffers for every form, Q = 1 and 32, k = 10, medians of 30 calls in us;
pids_tail = the three torch kernels that turn the rows of search_pids into pids.  usage: python tools/exp/index_distinct_kernel_time.py"""
import json, os, sys, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from textreid_amd import GalleryIndex, lib as L
from textreid_amd.ops import _p, stream
G, K = 1000000, 10
gen = torch.Generator().manual_seed(7)
idx = GalleryIndex(capacity=G)
idx.add((torch.randn(G, 256, generator=gen) * 3).cuda(), pids=torch.randperm(G, generator=gen) // 4)
gids = idx._group_ids()
ones = torch.full(((G + 31) // 32,), -1, dtype=torch.int32, device="cuda")
out = {}
for Q in (1, 32):
    q16 = torch.zeros(32, 256, device="cuda")
    from textreid_amd import ops
    qu = ops.l2norm_rows((torch.randn(Q, 256, generator=gen)).cuda())[0]
    q16[:Q] = ops.p16_pack(qu, amax_=idx.unit_amax).data
    v = torch.empty(Q, K, device="cuda"); r = torch.empty(Q, K, dtype=torch.int64, device="cuda")
    ws = torch.empty(L.load().trid_index_search_ws_bytes(G, 32, 16, 0), dtype=torch.uint8, device="cuda")
    forms = {"unmasked": lambda: L.call("trid_index_search_p16", _p(q16), _p(idx.rows_p16), _p(idx.unit_amax), Q, G, K, 0, _p(v), _p(r), _p(ws), 0, stream()),
             "masked_ones": lambda: L.call("trid_index_search_masked_p16", _p(q16), _p(idx.rows_p16), _p(idx.unit_amax), _p(ones), Q, G, K, 0, _p(v), _p(r), _p(ws), 0, stream()),
             "distinct": lambda: L.call("trid_index_search_distinct_p16", _p(q16), _p(idx.rows_p16), _p(idx.unit_amax), _p(gids), None, Q, G, K, 0, _p(v), _p(r), _p(ws), 0, stream()),
             "pids_tail": lambda: idx._pids[:G][r].masked_fill_(r < 0, -1)}
    for n, fn in forms.items():
        for _ in range(5): fn()
        ts = []
        for _ in range(30):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); fn(); b.record(); torch.cuda.synchronize(); ts.append(a.elapsed_time(b) * 1e3)
        ts.sort(); out["Q%d_%s_us" % (Q, n)] = round(ts[len(ts) // 2], 1)
print(json.dumps(out))
