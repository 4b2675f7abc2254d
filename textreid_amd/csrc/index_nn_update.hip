// The merge step of refresh_neighbours, for GalleryIndex ("trid_index_nn_merge_f32") and for GalleryShards
// ("trid_index_nn_merge_sharded_f32"; both in include/textreid_hip.h): the stored neighbour lists of the rows [0, rows) - nn [*, n]
// int32 with their values nn_val [*, n] fp32, in the order of the index - take in up to m candidate rows numbered cand_first ..
// cand_first + m - 1, whose similarities to old row i stand at cand[j * ld_cand + i].  The contract: a candidate is in no list yet.
// Per row i:
//   own row removed                                  -> every slot (-1, -inf), redo[i] = 0
//   nn[i, 0] < 0, or an entry e >= 0 that is removed -> redo[i] = 1, list and values NOT written (the caller recomputes the row)
//   else                                             -> redo[i] = 0; every live candidate, j ascending, goes in front of the first entry
//                                                       it is in front of by the order, the last entry falls off.  Values move with
//                                                       their rows and keep their bits.
//
// ONE kernel body; what "removed" means (own row, entry, candidate) and which order rule holds (FULL_ORDER: the predicate itself is
// written out in the kernel, where the compiler keeps its short-circuit form) is the policy's, the Live parameter:
//   FlatLive   one index: ids are rows, live[id] for id < cand_first + m.  An entry outside that range cannot be looked up: it counts
//              as removed (redo), nothing is read through it.  Candidates are numbered ABOVE every merged row and above earlier
//              candidates, so in front = greater by float comparison: an equal value stays behind the older, lower row.
//   ShardedLive a sharded gallery: ids are GLOBAL, id = shard * 2^21 + local row.  live_all holds the parts' liveness bytes one part
//              after the other, part s at live_all[live_off[s] .. live_off[s] + live_len[s]).  An id e decodes as s = e >> 21, l = e &
//              (2^21 - 1) and counts as REMOVED when s >= n_shards, l >= live_len[s], the byte lies outside [0, live_bytes) or the byte
//              is 0; nothing is read through an id that fails a range check, so device contents cannot fault.  Own row i is
//              (self_shard, i); candidate j is the id cand_first + j (consecutive rows of one part).  The order is the full one: in
//              front = greater by float comparison, or equal and the lower global id - candidates may be numbered below stored rows
//              (a new row of part 1 against the lists of part 2).  An absent entry (< 0) is behind every candidate.
//
// One row per lane, 256 threads.  The list and its values sit in 2 N registers; an insert is N branch-free select steps from the last
// slot up: slot u becomes the old slot u - 1 if the candidate goes in front of that one, else the candidate if it goes in front of
// slot u, else itself.  Lane i reads cand[j * ld_cand + i]: consecutive lanes, consecutive floats.  A candidate's liveness is the same
// bytes for every lane: a uniform branch skips a removed candidate's row of cand.

#include <climits>

#include "common.h"

namespace trid {

constexpr int NN_MERGE_N_MAX = 8;
constexpr int SHARD_MERGE_BITS = 21;                          // global id = shard << 21 | local row (index_shards.SHARD_BITS)
constexpr int SHARD_MERGE_LOCAL = (1 << SHARD_MERGE_BITS) - 1;
constexpr int SHARD_MERGE_SHARDS_MAX = 1023;                  // ids of 1023 shards fit int32

struct FlatLive {
    static constexpr int CAND_UNROLL = 4;       // the candidate loop's unroll factor
    static constexpr bool FULL_ORDER = false;   // in front = greater by value alone
    const uint8_t* __restrict__ live;  // one byte per row, [0, cand_first + m)

    __device__ __forceinline__ bool own(int i, unsigned) const { return live[i] != 0; }
    __device__ __forceinline__ bool entry(int e, unsigned total) const { return !((unsigned)e >= total || live[(unsigned)e < total ? e : 0] == 0); }
    __device__ __forceinline__ bool candidate(int r) const { return live[r] != 0; }
};

struct ShardLive {
    const uint8_t* all;
    const long long* off;
    const int* len;
    long long bytes;
    int n_shards;
};

struct ShardedLive {
    static constexpr int CAND_UNROLL = 1;
    static constexpr bool FULL_ORDER = true;    // in front = greater by value, or equal and the lower id; an absent entry is behind
    ShardLive t;
    int self_shard;

    // e >= 0.  Every read is behind the range check that makes it safe.
    __device__ __forceinline__ bool entry(int e, unsigned = 0) const {
        const int s = e >> SHARD_MERGE_BITS;
        const int l = e & SHARD_MERGE_LOCAL;
        if (s >= t.n_shards) return false;
        if (l >= t.len[s]) return false;
        const long long o = t.off[s];
        if (o < 0 || o > t.bytes - 1 - (long long)l) return false;
        return t.all[o + l] != 0;
    }
    __device__ __forceinline__ bool own(int i, unsigned) const { return entry((self_shard << SHARD_MERGE_BITS) | i); }
    __device__ __forceinline__ bool candidate(int r) const { return entry(r); }
};

template <int N, class Live>
__global__ __launch_bounds__(256) void index_nn_merge_kernel(const float* __restrict__ cand, long long ld_cand, int m, int cand_first, int rows,
                                                              const Live lv, int* __restrict__ nn, float* __restrict__ nn_val,
                                                              uint8_t* __restrict__ redo) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= rows) return;
    int* li = nn + (long long)i * N;
    float* lval = nn_val + (long long)i * N;
    const unsigned total = (unsigned)cand_first + (unsigned)m;  // (the ids FlatLive can look up; the entry checked it against INT_MAX)
    if (!lv.own(i, total)) {
#pragma unroll
        for (int u = 0; u < N; ++u) {
            li[u] = -1;
            lval[u] = -INFINITY;
        }
        redo[i] = 0;
        return;
    }
    int e[N];
#pragma unroll
    for (int u = 0; u < N; ++u) e[u] = li[u];
    bool again = e[0] < 0;
#pragma unroll
    for (int u = 0; u < N; ++u) {
        if (e[u] >= 0) again |= !lv.entry(e[u], total);
    }
    redo[i] = again ? 1 : 0;
    if (again) return;
    float v[N];
#pragma unroll
    for (int u = 0; u < N; ++u) v[u] = lval[u];
    const float* col = cand + i;
#pragma unroll Live::CAND_UNROLL
    for (int j = 0; j < m; ++j) {
        const int r = cand_first + j;
        if (!lv.candidate(r)) continue;  // (uniform)
        const float c = col[(long long)j * ld_cand];
        bool front[N];  // the candidate goes in front of the OLD slot u
#pragma unroll
        for (int u = 0; u < N; ++u) front[u] = Live::FULL_ORDER ? (e[u] < 0 || c > v[u] || (c == v[u] && r < e[u])) : c > v[u];
#pragma unroll
        for (int u = N - 1; u >= 0; --u) {
            const int w = u > 0 ? u - 1 : 0;  // (slot u - 1 still holds its old entry: the slots are rewritten from the last one up)
            const bool above = u > 0 && front[w];
            const float nv = above ? v[w] : (front[u] ? c : v[u]);
            const int ne = above ? e[w] : (front[u] ? r : e[u]);
            v[u] = nv;
            e[u] = ne;
        }
    }
#pragma unroll
    for (int u = 0; u < N; ++u) {
        li[u] = e[u];
        lval[u] = v[u];
    }
}

template <int N, class Live>
static void nn_merge_launch_n(const float* cand, long long ld_cand, int m, int cand_first, int rows, const Live& lv, int32_t* nn, float* nn_val,
                              uint8_t* redo, hipStream_t stream) {
    hipLaunchKernelGGL((index_nn_merge_kernel<N, Live>), dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, stream, cand, ld_cand, m, cand_first, rows,
                       lv, (int*)nn, nn_val, redo);
}

template <class Live>
static void nn_merge_launch(int n, const float* cand, long long ld_cand, int m, int cand_first, int rows, const Live& lv, int32_t* nn, float* nn_val,
                            uint8_t* redo, hipStream_t stream) {
    switch (n) {
        case 1: nn_merge_launch_n<1>(cand, ld_cand, m, cand_first, rows, lv, nn, nn_val, redo, stream); break;
        case 2: nn_merge_launch_n<2>(cand, ld_cand, m, cand_first, rows, lv, nn, nn_val, redo, stream); break;
        case 3: nn_merge_launch_n<3>(cand, ld_cand, m, cand_first, rows, lv, nn, nn_val, redo, stream); break;
        case 4: nn_merge_launch_n<4>(cand, ld_cand, m, cand_first, rows, lv, nn, nn_val, redo, stream); break;
        case 5: nn_merge_launch_n<5>(cand, ld_cand, m, cand_first, rows, lv, nn, nn_val, redo, stream); break;
        case 6: nn_merge_launch_n<6>(cand, ld_cand, m, cand_first, rows, lv, nn, nn_val, redo, stream); break;
        case 7: nn_merge_launch_n<7>(cand, ld_cand, m, cand_first, rows, lv, nn, nn_val, redo, stream); break;
        default: nn_merge_launch_n<8>(cand, ld_cand, m, cand_first, rows, lv, nn, nn_val, redo, stream); break;
    }
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
    const FlatLive lv = {live};
    nn_merge_launch(n, cand, ld_cand, m, cand_first, rows, lv, nn, nn_val, redo, (hipStream_t)stream_);
    return check_launch("trid_index_nn_merge_f32");
}

extern "C" int trid_index_nn_merge_sharded_f32(const float* cand, long long ld_cand, int m, int cand_first, int rows, const uint8_t* live_all,
                                               const int64_t* live_off, const int32_t* live_len, long long live_bytes, int n_shards,
                                               int self_shard, int32_t* nn, float* nn_val, int n, uint8_t* redo, void* stream_) {
    const char* who = "trid_index_nn_merge_sharded_f32";
    TRID_REQUIRE(live_all && live_off && live_len && nn && nn_val && redo, "%s: null pointer", who);
    TRID_REQUIRE(n >= 1 && n <= NN_MERGE_N_MAX, "%s: n must be in [1,%d]; got %d", who, NN_MERGE_N_MAX, n);
    TRID_REQUIRE(m >= 0, "%s: m must be >= 0; got %d", who, m);
    TRID_REQUIRE(cand != nullptr || m == 0, "%s: null pointer (cand with m = %d candidates)", who, m);
    TRID_REQUIRE(n_shards >= 1 && n_shards <= SHARD_MERGE_SHARDS_MAX, "%s: n_shards must be in [1,%d] (global ids are int32); got %d", who,
                 SHARD_MERGE_SHARDS_MAX, n_shards);
    TRID_REQUIRE(self_shard >= 0 && self_shard < n_shards, "%s: self_shard must be in [0, n_shards = %d); got %d", who, n_shards, self_shard);
    TRID_REQUIRE(rows >= 1 && rows <= SHARD_MERGE_LOCAL, "%s: rows must be in [1, %d] (the local rows of one shard); got %d", who, SHARD_MERGE_LOCAL,
                 rows);
    TRID_REQUIRE(live_bytes >= 1, "%s: live_bytes must be >= 1; got %lld", who, live_bytes);
    TRID_REQUIRE(cand_first >= 0 && (long long)(cand_first & SHARD_MERGE_LOCAL) + m <= (long long)SHARD_MERGE_LOCAL,
                 "%s: the candidates cand_first = %d .. + m = %d must be >= 0 and local rows of ONE shard (local row + m <= %d)", who, cand_first, m,
                 SHARD_MERGE_LOCAL);
    TRID_REQUIRE(m == 0 || ld_cand >= rows, "%s: ld_cand = %lld is below rows = %d", who, ld_cand, rows);
    TRID_REQUIRE((reinterpret_cast<uintptr_t>(cand) & 3u) == 0 && (reinterpret_cast<uintptr_t>(nn) & 3u) == 0 &&
                     (reinterpret_cast<uintptr_t>(nn_val) & 3u) == 0 && (reinterpret_cast<uintptr_t>(live_len) & 3u) == 0 &&
                     (reinterpret_cast<uintptr_t>(live_off) & 7u) == 0,
                 "%s: cand / nn / nn_val / live_len must be 4-byte, live_off 8-byte aligned", who);
    const ShardedLive lv = {{live_all, (const long long*)live_off, (const int*)live_len, live_bytes, n_shards}, self_shard};
    nn_merge_launch(n, cand, ld_cand, m, cand_first, rows, lv, nn, nn_val, redo, (hipStream_t)stream_);
    return check_launch(who);
}
