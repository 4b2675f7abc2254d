// The k-reciprocal bonus of GalleryIndex.search_reranked (include/textreid_hip.h "trid_index_rerank_add_f32"): in place on the dense
// score buffer of a query panel, scores[q, g] += bonus(nq(q), c(q, g)) wherever the query's neighbour list qnn[q] and the gallery
// row's stored list gnn[g] share c > 0 rows and row g is allowed.  Everything else keeps its bits and is never written.
//
// One gallery row per lane, grid (ceil(G / 256), ceil(Q / 32)).  A workgroup narrows the qnn of its 32 queries to int32 in LDS (an
// absent slot and a row no int32 holds become -1); every lane of a wave reads the same LDS word, so the read is a broadcast and no
// bank is asked twice.  The row's n graph entries sit in registers (an entry below 0 becomes -2: it equals no slot, absent ones
// included).  At most 32 n^2 compares per row; a hit is rare and is one read-modify-write.
// Arithmetic: the host entry forms the (n + 1) x (n + 1) table bonus(nq, c) = (alpha * (float)c) / (float)(nq + n - c) in plain
// C++ float arithmetic and hands it over by value; the device does ONE fp32 add, so nothing depends on how the device divides.

#include "common.h"

namespace trid {

constexpr int RERANK_N_MAX = 8;
constexpr int RERANK_PANEL = 32;      // queries per workgroup: grid.y runs over groups of 32
constexpr int RERANK_GROUPS_MAX = 65535;  // grid.y

struct RerankTable {
    float b[(RERANK_N_MAX + 1) * (RERANK_N_MAX + 1)];  // bonus(nq, c) at [nq * (n + 1) + c]
};

template <int N>
__global__ __launch_bounds__(256) void index_rerank_add_kernel(float* scores, long long ld_q, long long ld_g, int Q, int G,
                                                                const long long* __restrict__ qnn, const int* __restrict__ gnn,
                                                                const RerankTable tab, const uint32_t* __restrict__ mask) {
    __shared__ int sq[RERANK_PANEL * N];
    __shared__ float sb[(N + 1) * (N + 1)];
    const int tid = threadIdx.x;
    const int q0 = blockIdx.y * RERANK_PANEL;
    const int nq_here = Q - q0 < RERANK_PANEL ? Q - q0 : RERANK_PANEL;
    for (int i = tid; i < RERANK_PANEL * N; i += 256) {
        long long v = -1;
        if (i < nq_here * N) v = qnn[(long long)q0 * N + i];
        sq[i] = (v < 0 || v > 0x7fffffffll) ? -1 : (int)v;
    }
    for (int i = tid; i < (N + 1) * (N + 1); i += 256) sb[i] = tab.b[i];
    __syncthreads();

    const long long g = (long long)blockIdx.x * 256 + tid;
    if (g >= G) return;
    if (mask != nullptr && ((mask[g >> 5] >> (g & 31)) & 1u) == 0) return;
    int b[N];
#pragma unroll
    for (int u = 0; u < N; ++u) {
        const int v = gnn[g * N + u];
        b[u] = v < 0 ? -2 : v;
    }
    float* col = scores + g * ld_g + (long long)q0 * ld_q;
    for (int qi = 0; qi < nq_here; ++qi) {
        int c = 0;
#pragma unroll
        for (int t = 0; t < N; ++t) {
            const int a = sq[qi * N + t];
#pragma unroll
            for (int u = 0; u < N; ++u) c += (a == b[u]) ? 1 : 0;
        }
        if (c > 0) {
            int nq = 0;
#pragma unroll
            for (int t = 0; t < N; ++t) nq += sq[qi * N + t] >= 0 ? 1 : 0;
            c = c > nq ? nq : c;  // (distinct rows by contract: c <= nq; a list that breaks it still stays inside the table)
            float* p = col + (long long)qi * ld_q;
            *p = __fadd_rn(*p, sb[nq * (N + 1) + c]);
        }
    }
}

template <int N>
static void rerank_launch(float* scores, long long ld_q, long long ld_g, int Q, int G, const int64_t* qnn, const int32_t* gnn,
                          const RerankTable& tab, const uint32_t* mask, hipStream_t stream) {
    const dim3 grid((unsigned)(((long long)G + 255) / 256), (unsigned)((Q + RERANK_PANEL - 1) / RERANK_PANEL));
    hipLaunchKernelGGL(index_rerank_add_kernel<N>, grid, dim3(256), 0, stream, scores, ld_q, ld_g, Q, G, (const long long*)qnn,
                       (const int*)gnn, tab, mask);
}

}  // namespace trid

using namespace trid;

extern "C" int trid_index_rerank_add_f32(float* scores, long long ld_q, long long ld_g, int Q, int G, const int64_t* qnn,
                                         const int32_t* gnn, int n, float alpha, const uint32_t* mask_words, void* stream_) {
    TRID_REQUIRE(scores && qnn && gnn, "trid_index_rerank_add_f32: null pointer");
    TRID_REQUIRE(Q >= 1 && G >= 1, "trid_index_rerank_add_f32: Q and G must be >= 1; got Q = %d, G = %d", Q, G);
    TRID_REQUIRE(n >= 1 && n <= RERANK_N_MAX && n <= G, "trid_index_rerank_add_f32: n must be in [1,%d] and <= G = %d; got %d", RERANK_N_MAX, G, n);
    TRID_REQUIRE((Q + RERANK_PANEL - 1) / RERANK_PANEL <= RERANK_GROUPS_MAX,
                 "trid_index_rerank_add_f32: ceil(Q / %d) = %d groups of queries exceed the grid of %d", RERANK_PANEL,
                 (Q + RERANK_PANEL - 1) / RERANK_PANEL, RERANK_GROUPS_MAX);
    // two elements must not alias: one of the strides spans the whole extent of the other (as trid_topk_rows_deep_f32)
    TRID_REQUIRE(ld_q >= 1 && ld_g >= 1 && (ld_q >= (long long)(G - 1) * ld_g + 1 || ld_g >= (long long)(Q - 1) * ld_q + 1),
                 "trid_index_rerank_add_f32: ld_q = %lld, ld_g = %lld make two elements of a [%d, %d] matrix alias", ld_q, ld_g, Q, G);
    TRID_REQUIRE((reinterpret_cast<uintptr_t>(scores) & 3u) == 0 && (reinterpret_cast<uintptr_t>(gnn) & 3u) == 0 &&
                     (reinterpret_cast<uintptr_t>(mask_words) & 3u) == 0 && (reinterpret_cast<uintptr_t>(qnn) & 7u) == 0,
                 "trid_index_rerank_add_f32: scores / gnn / mask_words must be 4-byte, qnn 8-byte aligned");
    RerankTable tab;
    memset(&tab, 0, sizeof(tab));
    for (int nq = 1; nq <= n; ++nq)
        for (int c = 1; c <= nq; ++c) {
            const float num = alpha * (float)c;
            const float den = (float)(nq + n - c);
            tab.b[nq * (n + 1) + c] = num / den;
        }
    hipStream_t stream = (hipStream_t)stream_;
    switch (n) {
        case 1: rerank_launch<1>(scores, ld_q, ld_g, Q, G, qnn, gnn, tab, mask_words, stream); break;
        case 2: rerank_launch<2>(scores, ld_q, ld_g, Q, G, qnn, gnn, tab, mask_words, stream); break;
        case 3: rerank_launch<3>(scores, ld_q, ld_g, Q, G, qnn, gnn, tab, mask_words, stream); break;
        case 4: rerank_launch<4>(scores, ld_q, ld_g, Q, G, qnn, gnn, tab, mask_words, stream); break;
        case 5: rerank_launch<5>(scores, ld_q, ld_g, Q, G, qnn, gnn, tab, mask_words, stream); break;
        case 6: rerank_launch<6>(scores, ld_q, ld_g, Q, G, qnn, gnn, tab, mask_words, stream); break;
        case 7: rerank_launch<7>(scores, ld_q, ld_g, Q, G, qnn, gnn, tab, mask_words, stream); break;
        default: rerank_launch<8>(scores, ld_q, ld_g, Q, G, qnn, gnn, tab, mask_words, stream); break;
    }
    return check_launch("trid_index_rerank_add_f32");
}
