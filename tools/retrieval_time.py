"""GPU box: configs[4] match (Q = 1e4 queries x G = 1e6 gallery rows, top-10) - pre-split operands + streaming filter kernel against
the on-the-fly split GEMM; agreement of the results.  usage: python tools/retrieval_time.py [G] [Q] [--map]
--map: times the matrix-free mAP (evaluation.rank_from_embeddings, 3 positives per query on synthetic pids; plain, and the re-ranked
ranks with the gallery's neighbour lists given)
next to the top-10 match at the same Q and G and prints one bench-line JSON with the rows/s figures and their ratios.
Under torch.distributed.run with more than one rank --map times the SHARDED form instead (evaluation.rank_from_embeddings_sharded /
positive_ranks_sharded: the same synthetic gallery split evenly over the ranks, queries replicated, one rank per device when the box has
them) and rank 0 prints one JSON line with world, map_rows_per_s and map_rerank_rows_per_s (GLOBAL gallery rows per second).
usage: python -m torch.distributed.run --nproc_per_node W tools/retrieval_time.py [G] [Q] --map
usage: python tools/retrieval_time.py --index [G] [Q ...] [--wg N] [--masked [F]] [--distinct [M]] [--deep K [K ...]] [--rerank K [K ...]] [--expanded M [M ...]]
                                       [--deep-distinct ROWS_PER_PID K [K ...]] [--shards S [--shards-rerank] [--shards-refresh M [M ...]]]
--index: small-batch serving.  For each Q (default 1 8 32 64 256; G default 1e6) three forms are timed in one process, alternating,
after 3 warm-up calls each, over 20 calls that each end in a synchronise: GalleryIndex.search, similarity_topk(q, g, 10) on raw
embeddings and similarity_topk(..., normalize=False) on unit rows (the two forms a caller without the index has).  One JSON line: the
median and the spread (min, max) of each in ms, the bytes the index search needs, the HBM floor they give at 6.3 TB/s, the one-off
add time.  --wg N forces the number of workers of the one-pass kernel (tuning).
--masked [F]: a fourth form, index_masked, timed in the same process alternating with the others: the same search on a second index
over the same gallery from which the fraction F (default 0.1) of the rows was removed (the masked one-pass kernel; panels of 32 queries
for Q > 32).  Each Q entry gains index_masked_ms and masked_over_index = its median over the unmasked index search's median.
--distinct [M]: a further form, index_distinct, timed in the same process alternating with the others: GalleryIndex.search_pids on an
index over the same gallery with M rows per pid (default 4; pid = a fixed random permutation of the rows // M: the distinct one-pass
kernel, panels of 32 queries for Q > 32).  Each Q entry gains index_distinct_ms and distinct_over_index.
--deep K [K ...]: GalleryIndex.shortlist(k=K) for each K (17 .. 1024 is the point; any 1 .. 1024 runs) and the k = 16 search of the same
index, timed in the same process alternating with the others.  Each Q entry gains index_k16_ms, shortlist_ms {K: median, min, max},
shortlist_over_index {K: its median over the k = 16 search's median} and shortlist_split_ms {K: {entry point: ms}}: one more call
with an event pair around every library call (the dense product, the deep select, the query packing), summed per entry point.
--deep-distinct M K [K ...]: GalleryIndex.shortlist_pids(k=K) for each K on an index over the same gallery with M rows per pid (pid = a
fixed random permutation of the rows // M) next to shortlist(k=K) of the plain index - the yardstick - timed in the same process
alternating with the others.  Each Q entry gains shortlist_pids_ms and shortlist_pids_yardstick_ms {K: median, min, max},
shortlist_pids_over_shortlist {K: ratio of the medians}, shortlist_pids_split_ms {K: {entry point: ms}} (the dense product, trid_index_
group_best_f32, trid_topk_rows_deep_pairs_f32, the query packing) and, for Q <= 32, shortlist_pids_bytes / shortlist_pids_floor_ms: the
P16 gallery read, the score buffer written and read, the order read, the best-pair buffers written and read, at 6.3 TB/s.  The line
gains deep_distinct_one_pid: the documented worst case, ONE pid holding a gallery of 1e5 rows (one wave walks it), k = 100, per Q the
median of shortlist_pids and the time of the group-best pass alone.
--rerank K [K ...]: GalleryIndex.build_neighbours(5) timed once (build_neighbours_ms), then search_reranked(k=K) and shortlist(k=K) of the
same index for each K, timed in the same process alternating with the others.  Each Q entry gains reranked_ms and reranked_shortlist_ms
{K: median, min, max}, reranked_over_shortlist {K: ratio of the medians}, reranked_split_ms {K: {entry point: ms}} (the bonus pass is
trid_index_rerank_add_f32) and bonus_floor_ms: the graph's G * n * 4 bytes read once per panel of 32 queries, at 6.3 TB/s.
--expanded M [M ...]: GalleryIndex.search_expanded(k = 100, m = M, power = 1) for each M next to shortlist(k = 100) of the same index - the
yardstick - timed in the same process alternating with the others.  Each Q entry gains expanded_ms {M: median, min, max},
expanded_shortlist_ms, expanded_over_shortlist {M: ratio of the medians}, expanded_split_ms {M: {entry point: ms}} (the blend is
trid_index_blend_rows_f32), blend_floor_ms {M: Q * (M + 2) KB at 6.3 TB/s} and expanded_equals_composition {M: search_expanded ==
shortlist(expand_queries(...)) bit for bit}.
--refresh M [M ...]: after the Q loop and a timed build_neighbours(5) (the one of --rerank if given), per M: M rows are appended and
GalleryIndex.refresh_neighbours() is timed (add_refresh_ms, add_counts = what it returned), then M random live rows are removed and it is
timed again (remove_refresh_ms, remove_counts) - each one call after one untimed warm-up refresh of either kind; each change is then made
a second time with an event pair around every library call of the refresh (add_split_ms / remove_split_ms per entry point).  Next to them
build_over_add_refresh / build_over_remove_refresh (build_neighbours_ms over each) and add_floor_ms: the bytes a refresh after the add
needs (per group of 32 new rows: the old P16 rows for the product and the gallery for the search pass, the candidate buffer written and
read, lists and values read and written) at 6.3 TB/s.
--shards S: the same searches through GalleryShards (textreid_amd/index_shards.py, the in-process form) with S equal parts over the same
gallery, 4 rows per pid, next to one plain GalleryIndex with the same pids, timed in the same process alternating with the others:
search(k = 10), shortlist(k = 100) and shortlist_pids(k = 100).  Each Q entry gains shards_ms and shards_plain_ms {method: median, min,
max}, shards_over_plain {method: ratio of the medians}, shards_split_ms {method: {entry point: ms}} (the merge is
trid_index_merge_lists_f32) and shards_equal_plain {method: the values bit for bit and the mapped rows equal}.
--shards-rerank (with --shards): build_neighbours(5) of the shards and of the plain index, each timed once (shards_build_neighbours_ms,
shards_plain_build_neighbours_ms; shards_graph_equal_plain: lists after the id mapping and values bit for bit), and search_reranked(k = 10)
as a fourth method of every entry above - the plain index over the same rows is the yardstick.
--shards-refresh M [M ...] (with --shards; after the Q loop, it changes the shards): per M, M rows are appended and
GalleryShards.refresh_neighbours() is timed (refresh_ms, counts), then build_neighbours(5) on the same contents (build_ms; refresh_equals_
build: lists and values bit for bit), then M more rows and one refresh with an event pair around every library call (split_ms per entry
point, and merge_launches / merge_ms_per_launch of trid_index_nn_merge_sharded_f32 alone) - each after one untimed warm-up refresh."""
import json, os, sys, time
import torch


def index_main(argv):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import textreid_amd.evaluation as E
    from textreid_amd import GalleryIndex

    wg = 0
    if "--wg" in argv:
        i = argv.index("--wg")
        wg = int(argv[i + 1])
        argv = argv[:i] + argv[i + 2:]
    distinct = None
    if "--distinct" in argv:  # (--distinct M comes last or before another option: a bare number after it is M)
        i = argv.index("--distinct")
        given = i + 1 < len(argv) and not argv[i + 1].startswith("--")
        distinct = int(argv[i + 1]) if given else 4
        argv = argv[:i] + argv[i + (2 if given else 1):]
    deep_distinct, dd_rows = [], 0
    if "--deep-distinct" in argv:  # (the first bare number after it is the rows per pid, every further one a K)
        i = argv.index("--deep-distinct")
        j = i + 1
        while j < len(argv) and not argv[j].startswith("--"):
            deep_distinct.append(int(argv[j]))
            j += 1
        dd_rows, deep_distinct = deep_distinct[0], deep_distinct[1:]
        argv = argv[:i] + argv[j:]
    deep = []
    if "--deep" in argv:  # (every bare number after --deep is a K, up to the next option)
        i = argv.index("--deep")
        j = i + 1
        while j < len(argv) and not argv[j].startswith("--"):
            deep.append(int(argv[j]))
            j += 1
        argv = argv[:i] + argv[j:]
    rerank = []
    if "--rerank" in argv:  # (as --deep: every bare number after it is a K)
        i = argv.index("--rerank")
        j = i + 1
        while j < len(argv) and not argv[j].startswith("--"):
            rerank.append(int(argv[j]))
            j += 1
        argv = argv[:i] + argv[j:]
    expanded = []
    if "--expanded" in argv:  # (as --deep: every bare number after it is an M)
        i = argv.index("--expanded")
        j = i + 1
        while j < len(argv) and not argv[j].startswith("--"):
            expanded.append(int(argv[j]))
            j += 1
        argv = argv[:i] + argv[j:]
    refresh = []
    if "--refresh" in argv:  # (as --deep: every bare number after it is an M)
        i = argv.index("--refresh")
        j = i + 1
        while j < len(argv) and not argv[j].startswith("--"):
            refresh.append(int(argv[j]))
            j += 1
        argv = argv[:i] + argv[j:]
    shards_rerank = "--shards-rerank" in argv
    argv = [a for a in argv if a != "--shards-rerank"]
    shards_refresh = []
    if "--shards-refresh" in argv:  # (as --deep: every bare number after it is an M)
        i = argv.index("--shards-refresh")
        j = i + 1
        while j < len(argv) and not argv[j].startswith("--"):
            shards_refresh.append(int(argv[j]))
            j += 1
        argv = argv[:i] + argv[j:]
    shards = 0
    if "--shards" in argv:
        i = argv.index("--shards")
        shards = int(argv[i + 1])
        argv = argv[:i] + argv[i + 2:]
    masked = None
    if "--masked" in argv:
        i = argv.index("--masked")
        given = i + 1 < len(argv) and 0.0 < float(argv[i + 1]) < 1.0  # (a fraction; an integer that follows is G or a Q)
        masked = float(argv[i + 1]) if given else 0.1
        argv = argv[:i] + argv[i + (2 if given else 1):]
    nums = [int(float(a)) for a in argv]
    G = nums[0] if nums else 1000000
    Qs = nums[1:] if len(nums) > 1 else [1, 8, 32, 64, 256]
    CALLS, WARM, K, HBM = 20, 3, 10, 6.3e12
    KE = 100  # the depth --expanded times search_expanded and its yardstick shortlist at
    gen = torch.Generator(device="cpu").manual_seed(7)
    g_raw = (torch.randn(G, 256, generator=gen) * 3.0).cuda()
    idx = GalleryIndex(capacity=G + 2 * sum(refresh) + (1 if refresh else 0))  # (--refresh appends 2 M rows per M: no growth inside the measurement)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    idx.add(g_raw)
    torch.cuda.synchronize()
    line = {"G": G, "C": 256, "k": K, "calls": CALLS, "warmup": WARM, "forced_workgroups": wg, "add_ms": (time.perf_counter() - t0) * 1e3, "Q": {}}
    g_unit = idx.rows
    if rerank:  # the neighbour graph, built once: ceil(G / 32) one-pass searches of the whole gallery
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        idx.build_neighbours(5)
        torch.cuda.synchronize()
        line["build_neighbours_ms"], line["neighbours_n"], line["build_panels"] = (time.perf_counter() - t0) * 1e3, 5, (G + 31) // 32
    idx_m = None
    if masked is not None:
        idx_m = GalleryIndex(capacity=G)
        idx_m.add(g_raw)
        gone = torch.nonzero(torch.rand(G, generator=gen) < masked).reshape(-1)
        line["masked_fraction"], line["masked_removed"] = masked, idx_m.remove(rows=gone)
        torch.cuda.synchronize()
    idx_d = None
    if distinct is not None:
        idx_d = GalleryIndex(capacity=G)
        idx_d.add(g_raw, pids=torch.randperm(G, generator=gen) // distinct)
        line["distinct_rows_per_pid"] = distinct
        torch.cuda.synchronize()
    idx_dd = None
    if deep_distinct:
        idx_dd = GalleryIndex(capacity=G)
        idx_dd.add(g_raw, pids=torch.randperm(G, generator=gen) // dd_rows)
        line["deep_distinct_rows_per_pid"] = dd_rows
        torch.cuda.synchronize()
    idx_s = sh = None
    SHARD_FORMS = (("search", K), ("shortlist", 100), ("shortlist_pids", 100)) + ((("search_reranked", K),) if shards_rerank else ())
    if shards:
        from textreid_amd import GalleryShards
        from textreid_amd.index_shards import SHARD_STRIDE

        shard_rows = (G + shards - 1) // shards
        pids_s = torch.randperm(G, generator=gen) // 4
        idx_s = GalleryIndex(capacity=G)
        idx_s.add(g_raw, pids=pids_s)
        sh = GalleryShards(shard_rows=shard_rows)
        sh.add(g_raw, pids=pids_s)
        line["shards"], line["shard_rows"], line["shards_rows_per_pid"] = sh.n_shards, shard_rows, 4
        torch.cuda.synchronize()
        if shards_rerank:  # the graph over the shards and the plain index's: S one-pass searches and one merge per panel of 32 rows
            t0 = time.perf_counter()
            sh.build_neighbours(5)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            idx_s.build_neighbours(5)
            torch.cuda.synchronize()
            line["shards_build_neighbours_ms"], line["shards_plain_build_neighbours_ms"] = (t1 - t0) * 1e3, (time.perf_counter() - t1) * 1e3
            want = idx_s.neighbours.long()
            want = torch.where(want < 0, want, (want // shard_rows) * SHARD_STRIDE + want % shard_rows)
            line["shards_graph_equal_plain"] = bool(torch.equal(torch.cat(sh.neighbours).long(), want) and
                                                    torch.equal(torch.cat(sh.neighbour_values).view(torch.int32), idx_s.neighbour_values.view(torch.int32)))

    def timed(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3

    def split_of(fn):
        """one more call with an event pair around every library call, summed per entry point"""
        from textreid_amd import lib as LIB

        torch.cuda.synchronize()
        LIB.TRACE = []
        fn()
        torch.cuda.synchronize()
        trace, LIB.TRACE = LIB.TRACE, None
        split = {}
        for name, _, e0, e1 in trace:
            split[name] = split.get(name, 0.0) + e0.elapsed_time(e1)
        return split

    for Q in Qs:
        q_raw = (torch.randn(Q, 256, generator=gen) * 3.0).cuda()
        q_unit = E.l2_normalize_rows(q_raw)
        out_v = torch.empty(Q, K, device="cuda")
        out_r = torch.empty(Q, K, dtype=torch.int64, device="cuda")
        forms = {"index": (lambda: idx.search(q_raw, K)) if (wg == 0 or Q > 32) else (lambda: idx._search_small(q_raw, K, True, out_v, out_r, wg)),
                 "topk_raw": lambda: E.similarity_topk(q_raw, g_raw, K),
                 "topk_unit": lambda: E.similarity_topk(q_unit, g_unit, K, normalize=False)}
        if idx_m is not None:
            forms["index_masked"] = (lambda: idx_m.search(q_raw, K)) if (wg == 0 or Q > 32) else (lambda: idx_m._search_small(q_raw, K, True, out_v, out_r, wg, idx_m._mask_words(None)))
        if idx_d is not None:
            forms["index_distinct"] = (lambda: idx_d.search_pids(q_raw, K)) if (wg == 0 or Q > 32) else (lambda: idx_d._search_small(q_raw, K, True, out_v, out_r, wg, None, idx_d._group_ids()))
        if deep:
            forms["index_k16"] = lambda: idx.search(q_raw, 16)
        for kd in deep:
            forms["shortlist_k%d" % kd] = lambda kd=kd: idx.shortlist(q_raw, kd)
        for kp in deep_distinct:
            forms["shortlist_k%d" % kp] = lambda kp=kp: idx.shortlist(q_raw, kp)
            forms["shortlist_pids_k%d" % kp] = lambda kp=kp: idx_dd.shortlist_pids(q_raw, kp)
        for kr in rerank:
            forms["shortlist_k%d" % kr] = lambda kr=kr: idx.shortlist(q_raw, kr)
            forms["reranked_k%d" % kr] = lambda kr=kr: idx.search_reranked(q_raw, kr)
        if expanded:
            forms["expanded_shortlist"] = lambda: idx.shortlist(q_raw, KE)
        for me in expanded:
            forms["expanded_m%d" % me] = lambda me=me: idx.search_expanded(q_raw, KE, m=me)
        for name, ks in (SHARD_FORMS if shards else ()):
            forms["shards_plain_%s" % name] = lambda name=name, ks=ks: getattr(idx_s, name)(q_raw, ks)
            forms["shards_%s" % name] = lambda name=name, ks=ks: getattr(sh, name)(q_raw, ks)
        for fn in forms.values():
            for _ in range(WARM):
                fn()
        torch.cuda.synchronize()
        times = {n: [] for n in forms}
        for _ in range(CALLS):
            for n, fn in forms.items():
                times[n].append(timed(fn))
        ent = {}
        for n, ts in times.items():
            ts = sorted(ts)
            ent[n + "_ms"] = {"median": ts[len(ts) // 2], "min": ts[0], "max": ts[-1]}
        if Q <= 32:
            lists = 2 * int(E.ops.L.load().trid_index_search_ws_bytes(G, Q, K, wg))  # written by the pass, read by the merge
            ent["index_bytes"] = G * 1024 + 32 * 1024 + lists
            ent["hbm_floor_ms"] = ent["index_bytes"] / HBM * 1e3
            ent["index_over_floor"] = ent["index_ms"]["median"] / ent["hbm_floor_ms"]
        ent["raw_over_index"] = ent["topk_raw_ms"]["median"] / ent["index_ms"]["median"]
        ent["unit_over_index"] = ent["topk_unit_ms"]["median"] / ent["index_ms"]["median"]
        if shards:
            ent["shards_plain_ms"] = {name: ent.pop("shards_plain_%s_ms" % name) for name, _ in SHARD_FORMS}
            ent["shards_ms"] = {name: ent.pop("shards_%s_ms" % name) for name, _ in SHARD_FORMS}
            ent["shards_over_plain"] = {name: ent["shards_ms"][name]["median"] / ent["shards_plain_ms"][name]["median"] for name, _ in SHARD_FORMS}
            ent["shards_split_ms"] = {name: split_of(lambda name=name, ks=ks: getattr(sh, name)(q_raw, ks)) for name, ks in SHARD_FORMS}
            ent["shards_equal_plain"] = {}
            for name, ks in SHARD_FORMS:  # (more than 32 queries: the plain search takes the streaming route, whose values differ in the last bits)
                a, b = getattr(sh, name)(q_raw, ks), getattr(idx_s, name if Q <= 32 or name != "search" else "shortlist")(q_raw, ks)
                rows = (b[1] // shard_rows) * SHARD_STRIDE + b[1] % shard_rows
                ent["shards_equal_plain"][name] = bool(torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1], rows))
        if expanded:  # the blend reads Q * (m + 1) KB and writes Q KB
            ent["expanded_k"] = KE
            ent["expanded_shortlist_ms"] = ent.pop("expanded_shortlist_ms")
            ent["expanded_ms"] = {str(me): ent.pop("expanded_m%d_ms" % me) for me in expanded}
            ent["expanded_over_shortlist"] = {str(me): ent["expanded_ms"][str(me)]["median"] / ent["expanded_shortlist_ms"]["median"] for me in expanded}
            ent["expanded_split_ms"] = {str(me): split_of(lambda me=me: idx.search_expanded(q_raw, KE, m=me)) for me in expanded}
            ent["blend_floor_ms"] = {str(me): Q * (me + 2) * 1024 / HBM * 1e3 for me in expanded}
            ent["expanded_equals_composition"] = {}
            for me in expanded:
                a, b = idx.search_expanded(q_raw, KE, m=me), idx.shortlist(idx.expand_queries(q_raw, m=me), KE, normalize=False)
                ent["expanded_equals_composition"][str(me)] = bool(torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1], b[1]))
        if idx_m is not None:
            ent["masked_over_index"] = ent["index_masked_ms"]["median"] / ent["index_ms"]["median"]
            ent["masked_within_index_spread"] = bool(ent["index_ms"]["min"] <= ent["index_masked_ms"]["median"] <= ent["index_ms"]["max"])
        if idx_d is not None:
            ent["distinct_over_index"] = ent["index_distinct_ms"]["median"] / ent["index_ms"]["median"]
        if deep_distinct:
            later = set(deep) | set(rerank)  # (their blocks below take the shortlist entry out)
            ent["shortlist_pids_ms"] = {str(kp): ent.pop("shortlist_pids_k%d_ms" % kp) for kp in deep_distinct}
            ent["shortlist_pids_yardstick_ms"] = {str(kp): ent["shortlist_k%d_ms" % kp] if kp in later else ent.pop("shortlist_k%d_ms" % kp) for kp in deep_distinct}
            ent["shortlist_pids_over_shortlist"] = {str(kp): ent["shortlist_pids_ms"][str(kp)]["median"] / ent["shortlist_pids_yardstick_ms"][str(kp)]["median"]
                                                    for kp in deep_distinct}
            ent["shortlist_pids_split_ms"] = {str(kp): split_of(lambda kp=kp: idx_dd.shortlist_pids(q_raw, kp)) for kp in deep_distinct}
            if Q <= 32:  # the P16 gallery read, the score buffer written and read, the order read, the best pairs written and read
                cols, n_pids = idx_dd._ws["scores"].shape[1], idx_dd._ws["gtable"][2]
                ent["shortlist_pids_bytes"] = G * 1024 + 2 * G * cols * 4 + G * 4 + 2 * 2 * n_pids * 32 * 4
                ent["shortlist_pids_floor_ms"] = ent["shortlist_pids_bytes"] / HBM * 1e3
        if rerank:
            from textreid_amd import lib as LIB

            ent["reranked_ms"] = {str(kr): ent.pop("reranked_k%d_ms" % kr) for kr in rerank}
            ent["reranked_shortlist_ms"] = {str(kr): ent["shortlist_k%d_ms" % kr] if kr in deep else ent.pop("shortlist_k%d_ms" % kr) for kr in rerank}
            ent["reranked_over_shortlist"] = {str(kr): ent["reranked_ms"][str(kr)]["median"] / ent["reranked_shortlist_ms"][str(kr)]["median"] for kr in rerank}
            ent["reranked_split_ms"] = {}
            for kr in rerank:  # one more call with an event pair around every library call, summed per entry point
                torch.cuda.synchronize()
                LIB.TRACE = []
                idx.search_reranked(q_raw, kr)
                torch.cuda.synchronize()
                trace, LIB.TRACE = LIB.TRACE, None
                split = {}
                for name, _, e0, e1 in trace:
                    split[name] = split.get(name, 0.0) + e0.elapsed_time(e1)
                ent["reranked_split_ms"][str(kr)] = split
            ent["bonus_bytes"] = G * line["neighbours_n"] * 4  # the pass's floor: the graph read once per panel of 32 queries
            ent["bonus_floor_ms"] = ((Q + 31) // 32) * ent["bonus_bytes"] / HBM * 1e3
        if deep:
            from textreid_amd import lib as LIB

            ent["shortlist_ms"] = {str(kd): ent.pop("shortlist_k%d_ms" % kd) for kd in deep}
            ent["shortlist_over_index"] = {str(kd): ent["shortlist_ms"][str(kd)]["median"] / ent["index_k16_ms"]["median"] for kd in deep}
            ent["shortlist_split_ms"] = {}
            for kd in deep:
                torch.cuda.synchronize()
                LIB.TRACE = []
                idx.shortlist(q_raw, kd)
                torch.cuda.synchronize()
                trace, LIB.TRACE = LIB.TRACE, None
                split = {}
                for name, _, e0, e1 in trace:
                    split[name] = split.get(name, 0.0) + e0.elapsed_time(e1)
                ent["shortlist_split_ms"][str(kd)] = split
            if Q <= 32:  # the P16 gallery read once, the score buffer written once and read once
                cols = idx._ws["scores"].shape[1]
                ent["shortlist_bytes"] = G * 1024 + 2 * G * cols * 4
                ent["shortlist_floor_ms"] = ent["shortlist_bytes"] / HBM * 1e3
            a16, s16 = idx.search(q_raw, 16), idx.shortlist(q_raw, 16)
            ent["shortlist16_equals_search"] = bool(torch.equal(a16[1], s16[1]) and torch.equal(a16[0].view(torch.int32), s16[0].view(torch.int32))) if Q <= 32 else None
        a, b = idx.search(q_raw, K), E.similarity_topk(q_raw, g_raw, K)
        ent["rows_equal_parent"] = bool(torch.equal(a[1], b[1]))
        ent["max_dv_parent"] = float((a[0] - b[0]).abs().max())
        line["Q"][str(Q)] = ent
    if deep_distinct:  # the documented worst case of the group-best pass: one pid holds the whole gallery, one wave walks it
        rows_1 = 100000
        one = GalleryIndex(capacity=rows_1)
        one.add(g_raw[:rows_1], pids=torch.zeros(rows_1, dtype=torch.int64))
        worst = {"rows": rows_1, "k": 100, "Q": {}}
        for Q in Qs:
            q_raw = (torch.randn(Q, 256, generator=gen) * 3.0).cuda()
            fn = lambda: one.shortlist_pids(q_raw, 100)  # noqa: E731 (one real result, then 99 (-inf, -1, -1) slots)
            for _ in range(WARM):
                fn()
            ts = sorted(timed(fn) for _ in range(CALLS))
            worst["Q"][str(Q)] = {"shortlist_pids_ms": {"median": ts[len(ts) // 2], "min": ts[0], "max": ts[-1]},
                                  "group_best_ms": split_of(fn).get("trid_index_group_best_f32")}
        line["deep_distinct_one_pid"] = worst
    if shards and shards_refresh:  # it changes the shards (rows appended: they open a part)
        from textreid_amd import lib as LIB

        def new_rows(M):
            return (torch.randn(M, 256, generator=gen) * 3.0).cuda(), torch.arange(len(sh), len(sh) + M) // 4 + G

        if not sh.neighbours_current:
            line["shards_build_neighbours_ms"] = timed(lambda: sh.build_neighbours(5))
        sh.add(*new_rows(1))  # warm-up: every kernel of a refresh has run once
        sh.refresh_neighbours()
        line["shards_refresh"] = {}
        for M in shards_refresh:
            rows_before = len(sh)
            sh.add(*new_rows(M))
            counts = []
            ms = timed(lambda: counts.append(sh.refresh_neighbours()))
            nn, val = [t.clone() for t in sh.neighbours], [t.clone() for t in sh.neighbour_values]
            build_ms = timed(lambda: sh.build_neighbours(5))
            same = all(torch.equal(a, b) for a, b in zip(nn, sh.neighbours)) and all(
                torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(val, sh.neighbour_values))
            sh.add(*new_rows(M))
            torch.cuda.synchronize()
            LIB.TRACE = []
            sh.refresh_neighbours()
            torch.cuda.synchronize()
            trace, LIB.TRACE = LIB.TRACE, None
            split, merges = {}, []
            for name, _, e0, e1 in trace:
                split[name] = split.get(name, 0.0) + e0.elapsed_time(e1)
                if name == "trid_index_nn_merge_sharded_f32":
                    merges.append(e0.elapsed_time(e1))
            line["shards_refresh"][str(M)] = {"rows_before": rows_before, "shards_after": sh.n_shards, "refresh_ms": ms, "counts": list(counts[0]),
                                              "build_ms": build_ms, "build_over_refresh": build_ms / ms, "refresh_equals_build": bool(same),
                                              "split_ms": split, "merge_launches": len(merges),
                                              "merge_ms_per_launch": sum(merges) / max(len(merges), 1)}
    if refresh:  # last: it changes the index (rows appended, rows removed)
        from textreid_amd import lib as LIB

        if "build_neighbours_ms" not in line:
            line["build_neighbours_ms"], line["neighbours_n"], line["build_panels"] = timed(lambda: idx.build_neighbours(5)), 5, (G + 31) // 32
        n = line["neighbours_n"]

        def one_refresh(change):
            """change() makes the graph stale -> (wall ms of refresh_neighbours, its counts); then the same change again with an event
            pair around every library call of the refresh, summed per entry point"""
            change()
            counts = []
            ms = timed(lambda: counts.append(idx.refresh_neighbours()))
            change()
            torch.cuda.synchronize()
            LIB.TRACE = []
            idx.refresh_neighbours()
            torch.cuda.synchronize()
            trace, LIB.TRACE = LIB.TRACE, None
            split = {}
            for name, _, e0, e1 in trace:
                split[name] = split.get(name, 0.0) + e0.elapsed_time(e1)
            return ms, list(counts[0]), split

        idx.add((torch.randn(1, 256, generator=gen) * 3.0).cuda())  # warm-up: every kernel of a refresh has run once
        idx.refresh_neighbours()
        idx.remove(rows=[0])
        idx.refresh_neighbours()
        line["refresh"] = {}
        for M in refresh:
            def add_rows():
                idx.add((torch.randn(M, 256, generator=gen) * 3.0).cuda())

            def remove_rows():
                live = torch.nonzero(idx.live).reshape(-1)
                idx.remove(rows=live[torch.randperm(live.numel(), generator=gen)[:M].to(live.device)])

            rows_before = len(idx)
            a_ms, a_counts, a_split = one_refresh(add_rows)
            r_ms, r_counts, r_split = one_refresh(remove_rows)
            groups = (M + 31) // 32
            # the bytes one refresh after an add needs: per group of 32 new rows the old P16 rows read by the product, the candidate
            # buffer written and read once, the lists and values read and written, and one search pass over the P16 gallery
            add_bytes = groups * (2 * rows_before * 1024 + 2 * min(M, 32) * rows_before * 4 + 2 * rows_before * n * 8)
            line["refresh"][str(M)] = {"rows_before": rows_before, "add_refresh_ms": a_ms, "add_counts": a_counts, "add_split_ms": a_split,
                                       "add_bytes": add_bytes, "add_floor_ms": add_bytes / HBM * 1e3,
                                       "remove_refresh_ms": r_ms, "remove_counts": r_counts, "remove_split_ms": r_split,
                                       "build_over_add_refresh": line["build_neighbours_ms"] / a_ms,
                                       "build_over_remove_refresh": line["build_neighbours_ms"] / r_ms}
    print(json.dumps(line), flush=True)


def map_sharded_main(argv):
    import torch.distributed as dist

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import textreid_amd.evaluation as E

    nums = [int(float(a)) for a in argv]
    G = nums[0] if nums else 1000000
    Q = nums[1] if len(nums) > 1 else 10000
    r, W = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    ndev = torch.cuda.device_count()
    torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", r)) % ndev)
    dist.init_process_group(os.environ.get("TRID_DIST_BACKEND", "nccl" if ndev >= W else "gloo"), init_method="env://")
    gen = torch.Generator(device="cpu").manual_seed(7)  # (the inputs of the one-rank run, cut by rows)
    q = torch.nn.functional.normalize(torch.randn(Q, 256, generator=gen), dim=1).cuda()
    lo, hi = r * G // W, (r + 1) * G // W
    g = torch.nn.functional.normalize(torch.randn(G, 256, generator=gen), dim=1)[lo:hi].cuda()
    qp = torch.arange(Q, device="cuda")
    gp = (torch.arange(G, device="cuda") % max(G // 3, 1))[lo:hi].contiguous()
    gnn = ((torch.arange(lo, hi, device="cuda").view(-1, 1) + torch.arange(5, device="cuda").view(1, -1) * 7919) % G).contiguous()
    line = {"world": W, "backend": dist.get_backend(), "devices": ndev, "Q": Q, "G": G, "C": 256, "positives_per_query": 3}

    def rerank_leg():
        return E.positive_ranks_sharded(q, g, qp, gp, E.similarity_topk(q, g, 5, normalize=False)[1], gnn, 0.05)
    for name, fn in (("map", lambda: E.rank_from_embeddings_sharded(q, g, qp, gp, (1, 5, 10), normalize=False)), ("map_rerank", rerank_leg)):
        fn(); torch.cuda.synchronize(); dist.barrier()
        t0 = time.perf_counter()
        for _ in range(3):
            fn()
        torch.cuda.synchronize(); dist.barrier()
        line[name + "_rows_per_s"] = G / ((time.perf_counter() - t0) / 3)
    if r == 0:
        print(json.dumps(line), flush=True)
    dist.destroy_process_group()


if "--index" in sys.argv:
    index_main([a for a in sys.argv[1:] if a != "--index"])
    sys.exit(0)
if "--map" in sys.argv and int(os.environ.get("WORLD_SIZE", "1")) > 1:
    map_sharded_main([a for a in sys.argv[1:] if a != "--map"])
    sys.exit(0)
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
