// The merge step of GalleryIndex.refresh_neighbours (include/textreid_hip.h "trid_index_nn_merge_f32"): the stored neighbour lists of
// the rows [0, rows) - nn [*, n] int32 with their values nn_val [*, n] fp32, value descending then row ascending - take in up to m
// candidate rows numbered cand_first .. cand_first + m - 1, all ABOVE every merged row, whose similarities to old row i stand at
// cand[j * ld_cand + i].  Per row i:
//   live[i] == 0                                   -> every slot (-1, -inf), redo[i] = 0
//   nn[i, 0] < 0 or an entry e >= 0 with !live[e]  -> redo[i] = 1, list and values NOT written (the caller recomputes the row)
//   else                                           -> redo[i] = 0; every live candidate, j ascending, goes in front of the first entry
//                                                     it beats by value (float compare: an equal value stays behind the older, lower
//                                                     row - candidates are numbered above every entry and above earlier candidates),
//                                                     the last entry falls off.  Values move with their rows and keep their bits.
//
// One row per lane, 256 threads.  The list and its values sit in 2 N registers; an insert is 2 N compares' worth of selects, no
// branch: slot u becomes the old slot u - 1 if the candidate beats that one, else the candidate if it beats slot u, else itself.
// Lane i reads cand[j * ld_cand + i]: consecutive lanes, consecutive floats.  live[cand_first + j] is the same byte for every lane
// (a uniform branch skips a dead candidate's row of cand).  An entry outside [0, cand_first + m) cannot be looked up in live: it
// counts as a dead entry (redo), nothing is read through it.

#include <climits>

#include "common.h"

namespace trid {

constexpr int NN_MERGE_N_MAX = 8;

template <int N>
__global__ __launch_bounds__(256) void index_nn_merge_kernel(const float* __restrict__ cand, long long ld_cand, int m, int cand_first, int rows,
                                                              const uint8_t* __restrict__ live, int* __restrict__ nn, float* __restrict__ nn_val,
                                                              uint8_t* __restrict__ redo) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= rows) return;
    int* li = nn + (long long)i * N;
    float* lv = nn_val + (long long)i * N;
    if (live[i] == 0) {
#pragma unroll
        for (int u = 0; u < N; ++u) {
            li[u] = -1;
            lv[u] = -INFINITY;
        }
        redo[i] = 0;
        return;
    }
    int e[N];
#pragma unroll
    for (int u = 0; u < N; ++u) e[u] = li[u];
    const unsigned total = (unsigned)cand_first + (unsigned)m;  // (entries of live; the entry checked it against INT_MAX)
    bool again = e[0] < 0;
#pragma unroll
    for (int u = 0; u < N; ++u) {
        if (e[u] >= 0) again |= (unsigned)e[u] >= total || live[(unsigned)e[u] < total ? e[u] : 0] == 0;
    }
    redo[i] = again ? 1 : 0;
    if (again) return;
    float v[N];
#pragma unroll
    for (int u = 0; u < N; ++u) v[u] = lv[u];
    const float* col = cand + i;
#pragma unroll 4
    for (int j = 0; j < m; ++j) {
        if (live[cand_first + j] == 0) continue;  // (uniform)
        const float c = col[(long long)j * ld_cand];
        const int r = cand_first + j;
#pragma unroll
        for (int u = N - 1; u >= 0; --u) {
            const int w = u > 0 ? u - 1 : 0;  // (slot u - 1 still holds its old entry: the slots are rewritten from the last one up)
            const bool here = c > v[u];
            const bool above = u > 0 && c > v[w];
            const float nv = above ? v[w] : (here ? c : v[u]);
            const int ne = above ? e[w] : (here ? r : e[u]);
            v[u] = nv;
            e[u] = ne;
        }
    }
#pragma unroll
    for (int u = 0; u < N; ++u) {
        li[u] = e[u];
        lv[u] = v[u];
    }
}

template <int N>
static void nn_merge_launch(const float* cand, long long ld_cand, int m, int cand_first, int rows, const uint8_t* live, int32_t* nn, float* nn_val,
                            uint8_t* redo, hipStream_t stream) {
    hipLaunchKernelGGL(index_nn_merge_kernel<N>, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, stream, cand, ld_cand, m, cand_first, rows, live,
                       (int*)nn, nn_val, redo);
}

}  // namespace trid

using namespace trid;

extern "C" int trid_index_nn_merge_f32(const float* cand, long long ld_cand, int m, int cand_first, int rows, const uint8_t* live, int32_t* nn,
                                       float* nn_val, int n, uint8_t* redo, void* stream_) {
    TRID_REQUIRE(live && nn && nn_val && redo, "trid_index_nn_merge_f32: null pointer");
    TRID_REQUIRE(n >= 1 && n <= NN_MERGE_N_MAX, "trid_index_nn_merge_f32: n must be in [1,%d]; got %d", NN_MERGE_N_MAX, n);
    TRID_REQUIRE(m >= 0, "trid_index_nn_merge_f32: m must be >= 0; got %d", m);
    TRID_REQUIRE(cand != nullptr || m == 0, "trid_index_nn_merge_f32: null pointer (cand with m = %d candidates)", m);
    TRID_REQUIRE(rows >= 1 && rows <= cand_first, "trid_index_nn_merge_f32: rows must be in [1, cand_first = %d] (candidates are numbered above every merged row); got %d",
                 cand_first, rows);
    TRID_REQUIRE((long long)cand_first + m <= (long long)INT_MAX, "trid_index_nn_merge_f32: cand_first + m = %lld exceeds the int32 row numbers",
                 (long long)cand_first + m);
    TRID_REQUIRE(m == 0 || ld_cand >= rows, "trid_index_nn_merge_f32: ld_cand = %lld is below rows = %d", ld_cand, rows);
    TRID_REQUIRE((reinterpret_cast<uintptr_t>(cand) & 3u) == 0 && (reinterpret_cast<uintptr_t>(nn) & 3u) == 0 && (reinterpret_cast<uintptr_t>(nn_val) & 3u) == 0,
                 "trid_index_nn_merge_f32: cand / nn / nn_val must be 4-byte aligned");
    hipStream_t stream = (hipStream_t)stream_;
    switch (n) {
        case 1: nn_merge_launch<1>(cand, ld_cand, m, cand_first, rows, live, nn, nn_val, redo, stream); break;
        case 2: nn_merge_launch<2>(cand, ld_cand, m, cand_first, rows, live, nn, nn_val, redo, stream); break;
        case 3: nn_merge_launch<3>(cand, ld_cand, m, cand_first, rows, live, nn, nn_val, redo, stream); break;
        case 4: nn_merge_launch<4>(cand, ld_cand, m, cand_first, rows, live, nn, nn_val, redo, stream); break;
        case 5: nn_merge_launch<5>(cand, ld_cand, m, cand_first, rows, live, nn, nn_val, redo, stream); break;
        case 6: nn_merge_launch<6>(cand, ld_cand, m, cand_first, rows, live, nn, nn_val, redo, stream); break;
        case 7: nn_merge_launch<7>(cand, ld_cand, m, cand_first, rows, live, nn, nn_val, redo, stream); break;
        default: nn_merge_launch<8>(cand, ld_cand, m, cand_first, rows, live, nn, nn_val, redo, stream); break;
    }
    return check_launch("trid_index_nn_merge_f32");
}
