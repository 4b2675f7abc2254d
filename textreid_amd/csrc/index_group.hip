// Group best (include/textreid_hip.h "trid_index_group_best_f32"): step 1 of the deep DISTINCT select of GalleryIndex.shortlist_pids.
// For every (group s, query q) of a score matrix the group's first allowed row in the library's one order - value descending by
// float comparison, then row ascending - as a (value, row) pair; (-inf, INT_MAX) where the group has no allowed row and in the padding
// slots behind the last group.  The pass MOVES values and never computes one: the outputs carry the input's bit patterns.
//
// One wave walks a group.  Lane = (query = lane & 31, half = lane >> 5): the halves take alternate rows of the group, so with
// ld_q == 1 (the [G, cols] product of the index) every load is one 128-byte line of the score buffer shared by 32 lanes.  The row
// number comes from `order`, so every score load is a dependent load, and a gallery of a few rows per pid gives a wave one or two
// of them per group.  A wave therefore takes FOUR consecutive slots at a time: the first two rows per half of all four groups are
// loaded together (eight order entries, then eight scores in flight per lane), and only a group with more than four rows goes on
// into its own loop, eight rows per half at a time (1e6 rows, 4 rows per pid, 32 queries on one MI355X: 0.070 ms for the pass
// against 0.094 ms with one slot per wave).  The halves meet in one cross-lane exchange per slot.  Queries beyond 32 go on the grid's second dimension (as
// index_rerank_add_kernel); the waves stride over the slots, so the grid never outgrows the runtime's 2^32 threads.  A group is NOT
// split over waves: one group holding the whole gallery is walked by one wave per 32 queries, serially - correct, and the documented
// worst case.
// "No allowed row" is carried by the ROW (INT_MAX), never by the value: a group whose only allowed score is a real -inf is a result.
// The comparison is the full order (value, then row), so the first allowed row replaces the (-inf, INT_MAX) start whatever its value.
// Device contents cannot be validated by the entry: an order entry outside [0, G) is skipped and never dereferenced, a starts pair is
// clamped to [0, G].

#include "common.h"

namespace trid {

constexpr int GROUP_PANEL = 32;         // queries per wave: grid.y runs over groups of 32
constexpr int GROUP_PANELS_MAX = 65535;  // grid.y
constexpr int GROUP_ABSENT = 0x7fffffff;
constexpr int GROUP_SLOTS = 4;          // consecutive slots a wave takes together
constexpr int GROUP_HEAD = 2;           // rows per half of each of them loaded together
constexpr int GROUP_UNROLL = 8;         // rows per half in flight in the loop over the rest of a long group
constexpr long long GROUP_BLOCKS_MAX = (1ll << 24) - 1;  // workgroups of 256 threads in one launch: fewer than 2^32 threads

// "a comes before b" in the result (topk_deep.hip deep_before)
__device__ __forceinline__ bool group_before(float a, int ia, float b, int ib) { return a > b || (a == b && ia < ib); }

// (value v, row r >= 0) replaces the best pair if it comes before it; r < 0 never does.  Selects, not a branch around two
// assignments: hipcc (ROCm 7) turned the branch form of the unrolled four-slot head into code that dropped the equal-value case.
__device__ __forceinline__ void group_take(float v, int r, float& bv, int& br) {
    const bool t = r >= 0 && group_before(v, r, bv, br);
    bv = t ? v : bv;
    br = t ? r : br;
}

// the order entry at position i of a group that ends at hi -> the row, -1: past the end, outside [0, G), or not allowed
__device__ __forceinline__ int group_row(const int* __restrict__ order, const uint32_t* __restrict__ mask, int i, int hi, int G) {
    int r = i < hi ? order[i] : -1;
    if (r >= G) r = -1;
    if (r >= 0 && mask != nullptr && ((mask[r >> 5] >> (r & 31)) & 1u) == 0) r = -1;
    return r;
}

__global__ __launch_bounds__(256) void index_group_best_kernel(const float* __restrict__ scores, long long ld_q, long long ld_g, int Q, int G,
                                                                const int* __restrict__ order, const int* __restrict__ starts, int n_groups,
                                                                int n_slots, const uint32_t* __restrict__ mask, float* __restrict__ out_val,
                                                                int* __restrict__ out_row, long long out_ld_q, long long out_ld_g) {
    const int lane = threadIdx.x & 63;
    const int half = lane >> 5;
    const int q = blockIdx.y * GROUP_PANEL + (lane & 31);
    const bool live = q < Q;
    const float* col = scores + (long long)(live ? q : 0) * ld_q;
    const long long wave0 = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const long long waves = (long long)gridDim.x * 4;

    for (long long s0 = wave0 * GROUP_SLOTS; s0 < n_slots; s0 += waves * GROUP_SLOTS) {
        int lo[GROUP_SLOTS], hi[GROUP_SLOTS], br[GROUP_SLOTS];
        float bv[GROUP_SLOTS];
#pragma unroll
        for (int j = 0; j < GROUP_SLOTS; ++j) {
            int a = 0, b = 0;
            if (s0 + j < n_groups) { a = starts[s0 + j]; b = starts[s0 + j + 1]; }  // (a padding slot, and one past n_slots, is an empty group)
            lo[j] = a < 0 ? 0 : a > G ? G : a;
            hi[j] = b < 0 ? 0 : b > G ? G : b;
        }
        // the first GROUP_HEAD rows per half of every slot, together
        int r[GROUP_SLOTS][GROUP_HEAD];
        float v[GROUP_SLOTS][GROUP_HEAD];
#pragma unroll
        for (int j = 0; j < GROUP_SLOTS; ++j)
#pragma unroll
            for (int u = 0; u < GROUP_HEAD; ++u) r[j][u] = group_row(order, mask, lo[j] + half + 2 * u, hi[j], G);
#pragma unroll
        for (int j = 0; j < GROUP_SLOTS; ++j)
#pragma unroll
            for (int u = 0; u < GROUP_HEAD; ++u) v[j][u] = (r[j][u] >= 0 && live) ? col[(long long)r[j][u] * ld_g] : -INFINITY;
        // (the first pair STARTS the slot - no comparison against the (-inf, INT_MAX) constants: v is -inf wherever r is -1)
#pragma unroll
        for (int j = 0; j < GROUP_SLOTS; ++j) {
            bv[j] = v[j][0];
            br[j] = r[j][0] >= 0 ? r[j][0] : GROUP_ABSENT;
#pragma unroll
            for (int u = 1; u < GROUP_HEAD; ++u) group_take(v[j][u], r[j][u], bv[j], br[j]);
        }
        // the rest of a long group
#pragma unroll
        for (int j = 0; j < GROUP_SLOTS; ++j) {
            for (int i0 = lo[j] + half + 2 * GROUP_HEAD; i0 < hi[j]; i0 += 2 * GROUP_UNROLL) {
                int rr[GROUP_UNROLL];
                float vv[GROUP_UNROLL];
#pragma unroll
                for (int u = 0; u < GROUP_UNROLL; ++u) rr[u] = group_row(order, mask, i0 + 2 * u, hi[j], G);
#pragma unroll
                for (int u = 0; u < GROUP_UNROLL; ++u) vv[u] = (rr[u] >= 0 && live) ? col[(long long)rr[u] * ld_g] : -INFINITY;
#pragma unroll
                for (int u = 0; u < GROUP_UNROLL; ++u) group_take(vv[u], rr[u], bv[j], br[j]);
            }
        }
        // the halves meet: every lane learns the other half's pair of the same query
#pragma unroll
        for (int j = 0; j < GROUP_SLOTS; ++j) {
            if (s0 + j >= n_slots) break;
            const float ov = __shfl_xor(bv[j], 32, 64);
            const int orow = __shfl_xor(br[j], 32, 64);
            group_take(ov, orow, bv[j], br[j]);  // (an absent pair's INT_MAX is >= 0 and comes before nothing)
            if (half == 0 && live) {
                const long long at = (long long)q * out_ld_q + (s0 + j) * out_ld_g;
                out_val[at] = bv[j];
                out_row[at] = br[j];
            }
        }
    }
}

}  // namespace trid

using namespace trid;

extern "C" int trid_index_group_best_f32(const float* scores, long long ld_q, long long ld_g, int Q, int G, const int32_t* order,
                                         const int32_t* starts, int n_groups, int n_slots, const uint32_t* mask_words, float* out_val,
                                         int32_t* out_row, long long out_ld_q, long long out_ld_g, void* stream_) {
    TRID_REQUIRE(scores && order && starts && out_val && out_row, "trid_index_group_best_f32: null pointer");
    TRID_REQUIRE(Q >= 1 && G >= 1, "trid_index_group_best_f32: Q and G must be >= 1; got Q = %d, G = %d", Q, G);
    TRID_REQUIRE(n_slots >= 1 && n_groups >= 0 && n_groups <= n_slots,
                 "trid_index_group_best_f32: n_slots must be >= 1 and 0 <= n_groups <= n_slots; got n_groups = %d, n_slots = %d", n_groups, n_slots);
    TRID_REQUIRE((Q + GROUP_PANEL - 1) / GROUP_PANEL <= GROUP_PANELS_MAX,
                 "trid_index_group_best_f32: ceil(Q / %d) = %d groups of queries exceed the grid of %d", GROUP_PANEL,
                 (Q + GROUP_PANEL - 1) / GROUP_PANEL, GROUP_PANELS_MAX);
    // two elements must not alias: one of the strides spans the whole extent of the other (as trid_topk_rows_deep_f32)
    TRID_REQUIRE(ld_q >= 1 && ld_g >= 1 && (ld_q >= (long long)(G - 1) * ld_g + 1 || ld_g >= (long long)(Q - 1) * ld_q + 1),
                 "trid_index_group_best_f32: ld_q = %lld, ld_g = %lld make two elements of a [%d, %d] matrix alias", ld_q, ld_g, Q, G);
    TRID_REQUIRE(out_ld_q >= 1 && out_ld_g >= 1 &&
                     (out_ld_q >= (long long)(n_slots - 1) * out_ld_g + 1 || out_ld_g >= (long long)(Q - 1) * out_ld_q + 1),
                 "trid_index_group_best_f32: out_ld_q = %lld, out_ld_g = %lld make two elements of a [%d, %d] output alias", out_ld_q, out_ld_g, Q,
                 n_slots);
    TRID_REQUIRE((reinterpret_cast<uintptr_t>(scores) & 3u) == 0 && (reinterpret_cast<uintptr_t>(order) & 3u) == 0 &&
                     (reinterpret_cast<uintptr_t>(starts) & 3u) == 0 && (reinterpret_cast<uintptr_t>(mask_words) & 3u) == 0 &&
                     (reinterpret_cast<uintptr_t>(out_val) & 3u) == 0 && (reinterpret_cast<uintptr_t>(out_row) & 3u) == 0,
                 "trid_index_group_best_f32: scores / order / starts / mask_words / out_val / out_row must be 4-byte aligned");
    const long long panels = (Q + GROUP_PANEL - 1) / GROUP_PANEL;
    long long blocks = ((long long)n_slots + 4 * GROUP_SLOTS - 1) / (4 * GROUP_SLOTS);  // four waves of GROUP_SLOTS slots each; the waves stride over what is left
    if (blocks > GROUP_BLOCKS_MAX / panels) blocks = GROUP_BLOCKS_MAX / panels;
    const dim3 grid((unsigned)blocks, (unsigned)panels);
    hipLaunchKernelGGL(index_group_best_kernel, grid, dim3(256), 0, (hipStream_t)stream_, scores, ld_q, ld_g, Q, G, (const int*)order,
                       (const int*)starts, n_groups, n_slots, mask_words, out_val, (int*)out_row, out_ld_q, out_ld_g);
    return check_launch("trid_index_group_best_f32");
}
