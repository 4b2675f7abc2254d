// Matrix-free rank metrics (evaluation.py:11-37 rank / mAP, :40-65 k-reciprocal re-rank, :144-163 the four tables):
// CMC and mAP from per-positive RANKS instead of a sorted [Q,G] matrix.  For a query q and a relevant gallery row j
//     r(q,j) = 1 + #{ i : s(q,i) > s(q,j)  or  s(q,i) == s(q,j) and i < j }        (descending, ties lower index first)
// and with a query's P ranks in ascending order AP = (1/P) sum_k k / r_(k), first hit = r_(1) - 1.
//   1. pair values: s(q,j) of the pairs a CSR list names (the positives; with the re-rank also the few pairs whose
//      neighbour sets intersect), by the SAME tile code that counts - a row compares equal to its own duplicate;
//   2. count: the gallery streams past the resident queries once per RANK_PC positives of the longest list and the
//      epilogue counts (gemm_stream.hip FUSE 5; any C % 4 == 0 / precision: the [Q, 8192] panel GEMM, one panel at a time);
//   3. re-rank: s' = s + alpha J(nn(q), nn(i)) differs from s on the pairs with intersecting neighbour sets only, so the
//      streamed pass counts against the re-ranked thresholds and a correction over those pairs moves the few counts;
//   4. finalise (retrieval.hip, beside cmc_kernel): one wave per query orders its ranks by enumeration and sums the precision terms.
// Sharded gallery: g is rows offset .. offset + G - 1 of the global one and the lists name GLOBAL rows; a shard counts its own rows
// against the thresholds of all pairs with the tie rule on offset + i, and the shards' counts are summed by the caller.

#include "gemm_common.h"

namespace trid {

namespace {

__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
// (value, row) precedes (t, j) in the descending order with ties to the lower row
__device__ __forceinline__ int precedes(float v, int row, float t, int j) { return (v > t || (v == t && row < j)) ? 1 : 0; }
// query of entry e of a CSR list: the last q with ptr[q] <= e
__device__ __forceinline__ int csr_row(const long long* __restrict__ ptr, int Q, long long e) {
    int lo = 0, hi = Q;  // ptr[lo] <= e < ptr[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (ptr[mid] <= e) lo = mid;
        else hi = mid;
    }
    return lo;
}
// alpha * |A n B| / |A u B| of two rows of n unique neighbour indices: the expression of jaccard_add_kernel (retrieval.hip)
__device__ __forceinline__ float jaccard_term(const long long* __restrict__ a, const long long* __restrict__ b, int n, float alpha) {
    int inter = 0;
    for (int u = 0; u < n; ++u) {
        const long long bu = b[u];
        for (int t = 0; t < n; ++t) inter += (a[t] == bu) ? 1 : 0;
    }
    return alpha * (float)inter / (float)(2 * n - inter);
}

}  // namespace

// generic path, pair values: the listed pairs whose (global) row lies in the panel's columns [c0, c0 + n) - c0 = the shard's
// offset + the panel's first local row - take their value from it; the others are left as they are
__global__ __launch_bounds__(256) void rank_pick_panel_kernel(const float* __restrict__ panel, int ld, int n, long long c0,
                                                              const long long* __restrict__ ptr, const long long* __restrict__ idx,
                                                              float* __restrict__ val, int Q, long long NP) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= NP) return;
    const long long j = idx[e] - c0;
    if (j < 0 || j >= n) return;
    val[e] = panel[(long long)csr_row(ptr, Q, e) * ld + j];
}

// generic path, count: one workgroup per query walks its panel row once per RANK_PC listed positives
__global__ __launch_bounds__(256) void rank_count_panel_kernel(const float* __restrict__ panel, int ld, int n, int c0,
                                                               const long long* __restrict__ ptr, const long long* __restrict__ idx,
                                                               const float* __restrict__ thr, int* __restrict__ counts, long long offset) {
    const int q = blockIdx.x, lane = threadIdx.x & 63;
    const int b = (int)ptr[q], e = (int)ptr[q + 1];
    const float* r = panel + (long long)q * ld;
    for (int p0 = b; p0 < e; p0 += RANK_PC) {
        float t[RANK_PC], tmin = INFINITY;
        int j[RANK_PC], c[RANK_PC];
#pragma unroll
        for (int u = 0; u < RANK_PC; ++u) {
            const bool ok = p0 + u < e;
            t[u] = ok ? thr[p0 + u] : INFINITY;
            // (the listed row, GLOBAL, as a column of this panel: one below it never wins a tie, one beyond it always does)
            long long jl = ok ? idx[p0 + u] - offset - c0 : -1ll;
            jl = jl < -1ll ? -1ll : jl > (long long)n ? (long long)n : jl;
            j[u] = (int)jl;
            c[u] = 0;
            tmin = fminf(tmin, t[u]);
        }
        for (int i = threadIdx.x; i < n; i += 256) {
            const float v = r[i];
            if (v >= tmin) {
#pragma unroll
                for (int u = 0; u < RANK_PC; ++u) c[u] += precedes(v, i, t[u], j[u]);
            }
        }
#pragma unroll
        for (int u = 0; u < RANK_PC; ++u) {
            const int s = wave_sum_i(c[u]);
            if (lane == 0 && s != 0 && p0 + u < e) atomicAdd(counts + p0 + u, s);
        }
    }
}

// val[e] += alpha * J(qnn[q(e)], gnn[idx[e]]) for every listed pair
__global__ __launch_bounds__(256) void rank_pairs_jaccard_kernel(const long long* __restrict__ ptr, const long long* __restrict__ idx,
                                                                 float* __restrict__ val, const long long* __restrict__ qnn,
                                                                 const long long* __restrict__ gnn, int n, float alpha, int Q, long long NP) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= NP) return;
    const int q = csr_row(ptr, Q, e);
    val[e] = __fadd_rn(val[e], jaccard_term(qnn + (long long)q * n, gnn + idx[e] * n, n, alpha));
}

// Re-rank correction.  counts came from the PLAIN similarities against the re-ranked thresholds; the pairs (q, i) of the
// second list are the only ones whose value the Jaccard term moves: each takes its plain vote back and casts the moved one.
// Over one shard of the gallery: nb_idx and gnn are LOCAL rows of the shard whose row 0 is global row `offset` (the whole gallery:
// offset 0), pos_idx are GLOBAL rows (any shard's); counts are this shard's share, summed over the shards afterwards
__global__ __launch_bounds__(256) void rank_rerank_fix_shard_kernel(const long long* __restrict__ pos_ptr, const long long* __restrict__ pos_idx,
                                                                    const float* __restrict__ thr, int* __restrict__ counts,
                                                                    const long long* __restrict__ nb_ptr, const long long* __restrict__ nb_idx,
                                                                    const float* __restrict__ nb_val, const long long* __restrict__ qnn,
                                                                    const long long* __restrict__ gnn, int n, float alpha, int Q, long long NB,
                                                                    long long offset) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= NB) return;
    const int q = csr_row(nb_ptr, Q, e);
    const long long i = nb_idx[e];
    const float v = nb_val[e];
    const float v2 = __fadd_rn(v, jaccard_term(qnn + (long long)q * n, gnn + i * n, n, alpha));
    if (v2 == v) return;
    const long long gi = offset + i;
    for (long long p = pos_ptr[q]; p < pos_ptr[q + 1]; ++p) {
        const float t = thr[p];
        const bool first = gi < pos_idx[p];
        const int d = ((v2 > t || (v2 == t && first)) ? 1 : 0) - ((v > t || (v == t && first)) ? 1 : 0);
        if (d != 0) atomicAdd(counts + p, d);
    }
}

}  // namespace trid

using namespace trid;

extern "C" long long trid_rank_ws_floats(int Q, int G) { return (long long)Q * chunk_cols(G); }

#define RANK_LIST_OK(name)                                                                                                        \
    TRID_REQUIRE(ptr && idx && val && Q > 0 && G > 0 && NP >= 0 && NP < (1ll << 31), name ": null list or bad sizes (Q=%d G=%d NP=%lld)", Q, G, NP); \
    TRID_REQUIRE(mode == 0 || mode == 1, name ": mode must be 0 (pair values) or 1 (count)");                                    \
    TRID_REQUIRE(mode == 0 || (counts && max_list >= 0), name ": the count pass needs counts and the longest list's length");   \
    /* (offset: the global row of the streamed g's row 0; idx holds global rows - see the header) */                              \
    TRID_REQUIRE(offset >= 0, name ": negative row offset")

extern "C" int trid_rank_stream_p16(const void* q16, const void* a16, const float* q_amax, const float* g_amax, const int64_t* ptr,
                                    const int64_t* idx, float* val, int32_t* counts, int Q, int G, long long NP, int max_list,
                                    long long offset, int mode, void* stream) {
    RANK_LIST_OK("trid_rank_stream_p16");
    TRID_REQUIRE(q16 && a16 && q_amax && g_amax && aligned16(q16) && aligned16(a16), "trid_rank_stream_p16: the pre-split operands and their amax scalars are needed");
    TRID_REQUIRE((long long)G * 1024 < (1ll << 31), "trid_rank_stream_p16: the streamed rows must stay below 2 GB (G <= 2097151 rows of 256)");
    TRID_REQUIRE(mode == 1 || G == NP, "trid_rank_stream_p16: pair values stream the gathered rows of the list (G == NP)");
    if (NP == 0) return TRID_OK;
    RankCount rk;
    rk.ptr = (const long long*)ptr; rk.idx = (const long long*)idx; rk.val = val; rk.counts = counts;
    rk.p0 = 0; rk.pair_mode = mode == 0; rk.offset = offset;
    if (mode == 0) return stream_rank_count(a16, g_amax, q16, q_amax, G, Q, rk, (hipStream_t)stream);
    for (int p0 = 0; p0 < max_list; p0 += RANK_PC) {  // (queries whose list ends before p0 drop out at the first comparison)
        rk.p0 = p0;
        const int rc = stream_rank_count(a16, g_amax, q16, q_amax, G, Q, rk, (hipStream_t)stream);
        if (rc) return rc;
    }
    return TRID_OK;
}

extern "C" int trid_rank_stream_f32(const float* q, const float* g, const int64_t* ptr, const int64_t* idx, float* val, int32_t* counts,
                                    int Q, int G, int C, long long NP, int max_list, long long offset, int precision, const float* q_amax,
                                    const float* g_amax, float* ws, int mode, void* stream_) {
    RANK_LIST_OK("trid_rank_stream_f32");
    TRID_REQUIRE(q && g && ws && C > 0 && C % 4 == 0, "trid_rank_stream_f32: null operand or bad shape (C%%4)");
    if (NP == 0) return TRID_OK;
    hipStream_t stream = (hipStream_t)stream_;
    if (precision == 16 && !(q_amax && g_amax)) precision = 6;  // the fp16 split needs the operands' magnitudes
    const int Gc = chunk_cols(G);
    for (int c0 = 0; c0 < G; c0 += Gc) {  // one [Q, Gc] panel at a time
        const int n = (G - c0) < Gc ? (G - c0) : Gc;
        trid_gemm_desc d;
        memset(&d, 0, sizeof(d));
        d.A = q; d.B = g + (long long)c0 * C; d.C = ws;
        d.M = Q; d.N = n; d.K = C;
        d.lda = C; d.ldb = C; d.ldc = Gc;
        d.batch = 1; d.splits = 1; d.alpha = 1.f;
        d.a_mode = TRID_A_KC; d.b_mode = TRID_B_KC;
        d.precision = precision;
        d.a_amax = q_amax; d.b_amax = g_amax;
        int rc = trid_gemm_launch(&d, nullptr, nullptr, stream);
        if (rc) return rc;
        if (mode == 0)
            hipLaunchKernelGGL(rank_pick_panel_kernel, dim3((unsigned)((NP + 255) / 256)), dim3(256), 0, stream, (const float*)ws, Gc, n, offset + c0,
                               (const long long*)ptr, (const long long*)idx, val, Q, NP);
        else
            hipLaunchKernelGGL(rank_count_panel_kernel, dim3(Q), dim3(256), 0, stream, (const float*)ws, Gc, n, c0, (const long long*)ptr,
                               (const long long*)idx, (const float*)val, counts, offset);
        rc = check_launch("trid_rank_stream_f32");
        if (rc) return rc;
    }
    return TRID_OK;
}

extern "C" int trid_rank_pairs_jaccard_f32(const int64_t* ptr, const int64_t* idx, float* val, const int64_t* qnn, const int64_t* gnn,
                                           int n, float alpha, int Q, long long NP, void* stream) {
    TRID_REQUIRE(ptr && idx && val && qnn && gnn && Q > 0 && NP >= 0 && NP < (1ll << 31), "trid_rank_pairs_jaccard_f32: null operand or bad sizes");
    TRID_REQUIRE(n >= 1 && n <= 8 && alpha >= 0.f, "trid_rank_pairs_jaccard_f32: 1 <= n <= 8 neighbours, alpha >= 0");
    if (NP == 0) return TRID_OK;
    hipLaunchKernelGGL(rank_pairs_jaccard_kernel, dim3((unsigned)((NP + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const long long*)ptr,
                       (const long long*)idx, val, (const long long*)qnn, (const long long*)gnn, n, alpha, Q, NP);
    return check_launch("trid_rank_pairs_jaccard_f32");
}

extern "C" int trid_rank_rerank_fix(const int64_t* pos_ptr, const int64_t* pos_idx, const float* thr, int32_t* counts, const int64_t* nb_ptr,
                                    const int64_t* nb_idx, const float* nb_val, const int64_t* qnn, const int64_t* gnn, int n, float alpha,
                                    int Q, long long NB, void* stream) {
    TRID_REQUIRE(pos_ptr && pos_idx && thr && counts && nb_ptr && nb_idx && nb_val && qnn && gnn && Q > 0 && NB >= 0 && NB < (1ll << 31),
                 "trid_rank_rerank_fix: null operand or bad sizes");
    TRID_REQUIRE(n >= 1 && n <= 8 && alpha >= 0.f, "trid_rank_rerank_fix: 1 <= n <= 8 neighbours, alpha >= 0");
    if (NB == 0) return TRID_OK;
    hipLaunchKernelGGL(rank_rerank_fix_shard_kernel, dim3((unsigned)((NB + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       (const long long*)pos_ptr, (const long long*)pos_idx, thr, counts, (const long long*)nb_ptr, (const long long*)nb_idx,
                       nb_val, (const long long*)qnn, (const long long*)gnn, n, alpha, Q, NB, 0ll);
    return check_launch("trid_rank_rerank_fix");
}

extern "C" int trid_rank_rerank_fix_shard(const int64_t* pos_ptr, const int64_t* pos_idx, const float* thr, int32_t* counts,
                                          const int64_t* nb_ptr, const int64_t* nb_idx, const float* nb_val, const int64_t* qnn,
                                          const int64_t* gnn, int n, float alpha, int Q, long long NB, long long offset, void* stream) {
    TRID_REQUIRE(pos_ptr && pos_idx && thr && counts && nb_ptr && nb_idx && nb_val && qnn && gnn && Q > 0 && NB >= 0 && NB < (1ll << 31),
                 "trid_rank_rerank_fix_shard: null operand or bad sizes");
    TRID_REQUIRE(n >= 1 && n <= 8 && alpha >= 0.f && offset >= 0, "trid_rank_rerank_fix_shard: 1 <= n <= 8 neighbours, alpha >= 0, offset >= 0");
    if (NB == 0) return TRID_OK;
    hipLaunchKernelGGL(rank_rerank_fix_shard_kernel, dim3((unsigned)((NB + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       (const long long*)pos_ptr, (const long long*)pos_idx, thr, counts, (const long long*)nb_ptr, (const long long*)nb_idx,
                       nb_val, (const long long*)qnn, (const long long*)gnn, n, alpha, Q, NB, offset);
    return check_launch("trid_rank_rerank_fix_shard");
}
