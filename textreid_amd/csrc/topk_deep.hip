// Deep per-row top-k (include/textreid_hip.h "trid_topk_rows_deep_f32"): the exact k best (value, column) pairs of every row of a
// given fp32 score matrix for k up to 1024 - past the 16 that a wave's register list (topk_wave.h) holds.  The select MOVES values
// and never computes one: the outputs carry the input's bit patterns.
//
// One ordering step, used by every level: a workgroup holds P pairs in LDS (P a power of two), orders runs of K2 = next_pow2(k)
// with the bitonic network of argsort_rows_desc_kernel (retrieval.hip), then halves the number of runs until one is left: the
// pairwise better of a descending run and its ascending neighbour is a bitonic sequence that holds the K2 best of both, and
// log2(K2) merge stages order it again.  A full sort of 8192 pairs is 91 stages over all of them; k = 100 takes 28 + ~7.  The
// stages whose distance is below RB = min(16, P / 256, K2) run on blocks of RB consecutive pairs in a thread's registers: one
// pass over LDS for all of them (P = 8192, k = 100: 10 + ~5 passes and barriers instead of 28 + ~8).  Blocks of 32 pairs would
// save three more passes but the unrolled network then takes 256 VGPRs + 56 AGPRs, one workgroup per CU: measured slower
// (DESIGN.md section 7h).
//   level 1: grid (query fastest, chunk): a workgroup loads `chunk` columns of one row; disallowed columns and padding become the
//            sentinel (-inf, INT_MAX), which sorts behind every real pair (a real -inf has a lower column);
//   merges : a workgroup loads chunk / k lists of the level before.  The number of levels depends on (G, k, chunk) only.
// Order: value descending by float comparison (+0 == -0), then column ascending.  NaN: undefined.
// "trid_topk_rows_deep_pairs_f32" is the same select with another level 1 (template parameter PAIRS): the column of every element is
// GIVEN (int32, addressed like the values) instead of numbered, a given column of INT_MAX is the sentinel whatever its value, and
// there are no mask words.  The merge levels are shared: they only ever saw (value, column) pairs.

#include "common.h"

namespace trid {

constexpr int TOPK_DEEP_MAX = 1024;
constexpr int DEEP_CHUNK_MAX = 8192;  // 66 KB of padded pairs: two workgroups fit a CU's 160 KB of LDS (and, at <= 58 VGPRs, its registers)
constexpr int DEEP_SENTINEL = 0x7fffffff;
constexpr long long DEEP_GROUPS_MAX = (1ll << 24) - 1;  // workgroups of 256 threads in one launch: the runtime takes fewer than 2^32 threads

struct __attribute__((aligned(8))) DeepPair {
    float v;
    int c;
};

struct DeepArgs {
    // level 1
    const float* sim;
    const int* col;  // PAIRS: the given column of every element, addressed like sim (DEEP_SENTINEL = absent)
    long long ld_q, ld_g;
    const uint32_t* mask;
    int G, chunk;
    // merge levels
    const DeepPair* in;
    int nin, fan;
    // both
    int Q, k, K2, P, nout;
    DeepPair* out;  // the next level's lists [Q][nout][k]; null: this is the last level
    float* out_val;
    long long* out_idx;
    long long idx_offset;
};

// "a comes before b" in the result
__device__ __forceinline__ bool deep_before(float a, int ia, float b, int ib) { return a > b || (a == b && ia < ib); }

// pair i lives at word deep_at(i): one pad word per 32, so that the blocks of RB consecutive pairs that neighbouring threads
// hold in registers start in different banks (RB = 16: threads 2u, 2u + 1 read from words 33 u, 33 u + 16), and consecutive
// pairs stay consecutive
__device__ __forceinline__ int deep_at(int i) { return i + (i >> 5); }

// compare-exchange: up = the pair belongs to a run in the final order
__device__ __forceinline__ void deep_cex(float& x, int& ix, float& y, int& iy, bool up) {
    const bool sw = up != deep_before(x, ix, y, iy);
    const float tx = sw ? y : x, ty = sw ? x : y;
    const int tix = sw ? iy : ix, tiy = sw ? ix : iy;
    x = tx; y = ty; ix = tix; iy = tiy;
}

// A block of RB consecutive pairs (base a multiple of RB, RB divides 32: inside one padded group) in a thread's registers.
template <int RB>
struct DeepBlock {
    float v[RB];
    int c[RB];
    __device__ __forceinline__ void load(const float* sv, const int* si, int base) {
        const int o = deep_at(base);
#pragma unroll
        for (int r = 0; r < RB; ++r) { v[r] = sv[o + r]; c[r] = si[o + r]; }
    }
    __device__ __forceinline__ void store(float* sv, int* si, int base) const {
        const int o = deep_at(base);
#pragma unroll
        for (int r = 0; r < RB; ++r) { sv[o + r] = v[r]; si[o + r] = c[r]; }
    }
    // the network's phases k2 = 2 .. RB: the block ordered, final order when (base & RB) == 0
    __device__ __forceinline__ void sort(int base) {
#pragma unroll
        for (int k2 = 2; k2 <= RB; k2 <<= 1) {
#pragma unroll
            for (int j = k2 >> 1; j > 0; j >>= 1) {
#pragma unroll
                for (int x = 0; x < RB / 2; ++x) {
                    const int i = ((x & ~(j - 1)) << 1) | (x & (j - 1));
                    deep_cex(v[i], c[i], v[i | j], c[i | j], ((base | i) & k2) == 0);
                }
            }
        }
    }
    // the stages j = RB / 2 .. 1 of a merge whose direction the block shares
    __device__ __forceinline__ void merge(bool up) {
#pragma unroll
        for (int j = RB >> 1; j > 0; j >>= 1) {
#pragma unroll
            for (int x = 0; x < RB / 2; ++x) {
                const int i = ((x & ~(j - 1)) << 1) | (x & (j - 1));
                deep_cex(v[i], c[i], v[i | j], c[i | j], up);
            }
        }
    }
};

// RB = min(16, P / 256, K2), at least 2: every stage of distance < RB runs on blocks in registers - one LDS pass for all of them
// instead of one pass and one barrier each.  K2 == 1 has no stages at all (RB = 2 is never used then).
// PAIRS (level 1 only): the columns are GIVEN (a.col, addressed like a.sim) instead of numbered - trid_topk_rows_deep_pairs_f32.
template <bool FIRST, int RB, bool PAIRS = false>
__global__ __launch_bounds__(256) void topk_deep_kernel(const DeepArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const int P = a.P, K2 = a.K2, k = a.k;
    float* sv = reinterpret_cast<float*>(smem_raw);
    int* si = reinterpret_cast<int*>(sv + deep_at(P));
    const int tid = threadIdx.x;
    const unsigned q = blockIdx.x % (unsigned)a.Q;  // (the query is the fastest coordinate: with ld_q == 1 the workgroups that run
    const unsigned w = blockIdx.x / (unsigned)a.Q;  //  together share the 128-byte lines of one chunk)

    if (FIRST) {
        const long long g0 = (long long)w * a.chunk;
        const float* r = a.sim + (long long)q * a.ld_q;
        const int* rc = PAIRS ? a.col + (long long)q * a.ld_q : nullptr;
        // eight independent loads in flight per thread: with ld_q == 1 every element is a 128-byte line of its own
        for (int i0 = tid; i0 < P; i0 += 8 * 256) {
            float x[8];
            int c[8];
            bool ok[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int i = i0 + u * 256;
                const long long g = g0 + i;
                ok[u] = i < P && g < a.G;
                if (!PAIRS && ok[u] && a.mask != nullptr) ok[u] = (a.mask[g >> 5] >> (g & 31)) & 1u;
                x[u] = ok[u] ? r[g * a.ld_g] : -INFINITY;
                if (PAIRS) {  // a given column of DEEP_SENTINEL is absent whatever its value: it takes the sentinel's -inf
                    c[u] = ok[u] ? rc[g * a.ld_g] : DEEP_SENTINEL;
                    if (c[u] == DEEP_SENTINEL) x[u] = -INFINITY;
                } else {
                    c[u] = ok[u] ? (int)(g0 + i) : DEEP_SENTINEL;
                }
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int i = i0 + u * 256;
                if (i < P) {
                    sv[deep_at(i)] = x[u];
                    si[deep_at(i)] = c[u];
                }
            }
        }
    } else {
        const int l0 = (int)w * a.fan;
        const int cnt = a.nin - l0 < a.fan ? a.nin - l0 : a.fan;
        const int n = cnt * k;
        const DeepPair* src = a.in + ((long long)q * a.nin + l0) * k;
        for (int i = tid; i < P; i += 256) {
            DeepPair p;
            p.v = -INFINITY;
            p.c = DEEP_SENTINEL;
            if (i < n) p = src[i];
            sv[deep_at(i)] = p.v;
            si[deep_at(i)] = p.c;
        }
    }
    __syncthreads();

    const bool staged = K2 >= RB;  // (false only for K2 == 1)
    constexpr int LG_RB = RB == 2 ? 1 : RB == 4 ? 2 : RB == 8 ? 3 : 4;
    DeepBlock<RB> blk;

    // runs of K2: run r in the final order when r is even, reversed when it is odd
    if (staged) {
        for (int b = tid; b < (P >> LG_RB); b += 256) {
            blk.load(sv, si, b << LG_RB);
            blk.sort(b << LG_RB);
            blk.store(sv, si, b << LG_RB);
        }
        __syncthreads();
        for (int k2 = 2 * RB; k2 <= K2; k2 <<= 1) {
            for (int j = k2 >> 1; j >= RB; j >>= 1) {
                for (int e = tid; e < (P >> 1); e += 256) {
                    const int i = ((e & ~(j - 1)) << 1) | (e & (j - 1));
                    const int pi = deep_at(i), pl = deep_at(i | j);
                    float x = sv[pi], y = sv[pl];
                    int ix = si[pi], iy = si[pl];
                    if (((i & k2) == 0) != deep_before(x, ix, y, iy)) {
                        sv[pi] = y; sv[pl] = x;
                        si[pi] = iy; si[pl] = ix;
                    }
                }
                __syncthreads();
            }
            for (int b = tid; b < (P >> LG_RB); b += 256) {
                blk.load(sv, si, b << LG_RB);
                blk.merge(((b << LG_RB) & k2) == 0);
                blk.store(sv, si, b << LG_RB);
            }
            __syncthreads();
        }
    }

    // halve the runs: run r of the new set starts at r * 2 * stride and keeps the K2 best of old runs 2r (final order) and 2r + 1
    // (reversed), then is ordered again - final order for even r, reversed for odd r
    const int lg = __ffs(K2) - 1;
    for (int nr = P >> lg, stride = K2; nr > 1; nr >>= 1, stride <<= 1) {
        const int half = nr >> 1;
        for (int e = tid; e < (half << lg); e += 256) {
            const int i = (e >> lg) * 2 * stride + (e & (K2 - 1));
            const int pi = deep_at(i), pl = deep_at(i + stride);
            const float x = sv[pi], y = sv[pl];
            const int ix = si[pi], iy = si[pl];
            if (!deep_before(x, ix, y, iy)) {
                sv[pi] = y;
                si[pi] = iy;
            }
        }
        __syncthreads();
        if (!staged) continue;
        for (int j = K2 >> 1; j >= RB; j >>= 1) {
            for (int e = tid; e < (half << lg >> 1); e += 256) {
                const int r = e >> (lg - 1);
                const int p = e & ((K2 >> 1) - 1);
                const int i = r * 2 * stride + (((p & ~(j - 1)) << 1) | (p & (j - 1)));
                const int pi = deep_at(i), pl = deep_at(i | j);  // (the run's base is a multiple of 2 K2: the bit is free)
                const float x = sv[pi], y = sv[pl];
                const int ix = si[pi], iy = si[pl];
                if (((r & 1) == 0) != deep_before(x, ix, y, iy)) {
                    sv[pi] = y; sv[pl] = x;
                    si[pi] = iy; si[pl] = ix;
                }
            }
            __syncthreads();
        }
        const int bl = lg - LG_RB;  // a run is 2^bl blocks
        for (int b = tid; b < (half << bl); b += 256) {
            const int r = b >> bl;
            const int base = r * 2 * stride + ((b & ((1 << bl) - 1)) << LG_RB);
            blk.load(sv, si, base);
            blk.merge((r & 1) == 0);
            blk.store(sv, si, base);
        }
        __syncthreads();
    }

    if (a.out != nullptr) {
        DeepPair* dst = a.out + ((long long)q * a.nout + w) * k;
        for (int t = tid; t < k; t += 256) {
            DeepPair p;
            p.v = sv[deep_at(t)];
            p.c = si[deep_at(t)];
            dst[t] = p;
        }
    } else {
        for (int t = tid; t < k; t += 256) {
            const int c = si[deep_at(t)];
            a.out_val[(long long)q * k + t] = sv[deep_at(t)];
            a.out_idx[(long long)q * k + t] = c == DEEP_SENTINEL ? -1ll : a.idx_offset + c;
        }
    }
}

static int next_pow2(long long x) {
    int p = 1;
    while (p < x) p <<= 1;
    return p;
}

static int deep_default_chunk(int k) { return k <= 512 ? DEEP_CHUNK_MAX : 2048; }

// the chunk in force, 0: not a legal one for this k
static int deep_chunk(int k, int chunk) {
    if (chunk == 0) return deep_default_chunk(k);
    const int lo = 2 * next_pow2(k) > 64 ? 2 * next_pow2(k) : 64;
    if (chunk < lo || chunk > DEEP_CHUNK_MAX || (chunk & (chunk - 1)) != 0) return 0;
    return chunk;
}

// lists a level leaves per query: n1 after level 1, n2 after the first merge (0: level 1 is the last level)
static void deep_lists(int G, int k, int chunk, long long* n1, long long* n2) {
    *n1 = ((long long)G + chunk - 1) / chunk;
    const int fan = chunk / k;
    *n2 = *n1 > 1 ? (*n1 + fan - 1) / fan : 0;
}

static bool deep_shape_ok(int Q, int G, int k) { return Q >= 1 && G >= 1 && k >= 1 && k <= TOPK_DEEP_MAX && k <= G; }

constexpr int DEEP_RB_MAX = 16;  // pairs per register block at most (see the kernel's comment)
constexpr int DEEP_LDS_MAX = (DEEP_CHUNK_MAX + (DEEP_CHUNK_MAX >> 5)) * (int)sizeof(DeepPair);

// A chunk of 8192 pairs needs more dynamic LDS than the 48 KB a kernel gets unasked.  The FIRST call on a device raises the limit
// of EVERY instantiation, so that a later call - a recorded one, whose k may pick another instantiation than the eager call
// before it - makes nothing but launches.  (The flags are written without synchronisation: two first calls at once both set the
// same values.)
static int deep_raise_lds(const char* who) {
    static bool raised[64] = {};
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e == hipSuccess && dev >= 0 && dev < 64 && raised[dev]) return TRID_OK;
    const void* fns[] = {(const void*)topk_deep_kernel<true, 2>,  (const void*)topk_deep_kernel<true, 4>,  (const void*)topk_deep_kernel<true, 8>,
                         (const void*)topk_deep_kernel<true, 16>, (const void*)topk_deep_kernel<false, 2>, (const void*)topk_deep_kernel<false, 4>,
                         (const void*)topk_deep_kernel<false, 8>, (const void*)topk_deep_kernel<false, 16>,
                         (const void*)topk_deep_kernel<true, 2, true>, (const void*)topk_deep_kernel<true, 4, true>,
                         (const void*)topk_deep_kernel<true, 8, true>, (const void*)topk_deep_kernel<true, 16, true>};
    for (const void* fn : fns)
        if (e == hipSuccess) e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, DEEP_LDS_MAX);
    if (e != hipSuccess) { set_error("%s: cannot reserve %d B of LDS: %s", who, DEEP_LDS_MAX, hipGetErrorString(e)); return (int)e; }
    if (dev >= 0 && dev < 64) raised[dev] = true;
    return TRID_OK;
}

template <bool FIRST, int RB, bool PAIRS>
static int deep_launch_rb(const char* who, const DeepArgs& a, long long groups, hipStream_t stream) {
    const size_t lds = (size_t)(a.P + (a.P >> 5)) * sizeof(DeepPair);
    hipLaunchKernelGGL((topk_deep_kernel<FIRST, RB, PAIRS>), dim3((unsigned)groups), dim3(256), lds, stream, a);
    return check_launch(who);
}

template <bool FIRST, bool PAIRS = false>
static int deep_launch(const char* who, const DeepArgs& a, long long groups, hipStream_t stream) {
    int rb = a.P / 256 < a.K2 ? a.P / 256 : a.K2;  // pairs per register block: a thread's share of P, no longer than a run
    rb = rb > DEEP_RB_MAX ? DEEP_RB_MAX : rb < 2 ? 2 : rb;
    switch (rb) {
        case 2: return deep_launch_rb<FIRST, 2, PAIRS>(who, a, groups, stream);
        case 4: return deep_launch_rb<FIRST, 4, PAIRS>(who, a, groups, stream);
        case 8: return deep_launch_rb<FIRST, 8, PAIRS>(who, a, groups, stream);
        default: return deep_launch_rb<FIRST, 16, PAIRS>(who, a, groups, stream);
    }
}

}  // namespace trid

using namespace trid;

extern "C" int trid_topk_rows_deep_chunk(int k) { return k >= 1 && k <= TOPK_DEEP_MAX ? deep_default_chunk(k) : 0; }

extern "C" long long trid_topk_rows_deep_ws_bytes(int Q, int G, int k, int chunk) {
    if (!deep_shape_ok(Q, G, k)) return 0;
    const int c = deep_chunk(k, chunk);
    if (c == 0) return 0;
    long long n1, n2;
    deep_lists(G, k, c, &n1, &n2);
    if (n1 * Q > DEEP_GROUPS_MAX) return 0;
    if (n1 == 1) return 16;  // (nothing is staged; a workspace is still handed over)
    return (n1 + n2) * Q * k * (long long)sizeof(DeepPair);
}

// Both entries: the argument rules, level 1 (numbered columns with mask words, or the GIVEN columns `col`), then the merge levels.
// who: the entry's name in every message; gname: what it calls its column count.
static int deep_select(const char* who, const char* gname, const float* sim, const int32_t* col, bool pairs, long long ld_q, long long ld_g, int Q,
                       int G, int k, const uint32_t* mask_words, long long idx_offset, float* out_val, int64_t* out_idx, void* ws,
                       long long ws_bytes, int chunk, void* stream_) {
    TRID_REQUIRE(sim && out_val && out_idx && ws && (col || !pairs), "%s: null pointer", who);
    TRID_REQUIRE(Q >= 1 && G >= 1, "%s: Q and %s must be >= 1; got Q = %d, %s = %d", who, gname, Q, gname, G);
    TRID_REQUIRE(k >= 1 && k <= TOPK_DEEP_MAX && k <= G, "%s: k must be in [1,%d] and <= %s = %d; got %d", who, TOPK_DEEP_MAX, gname, G, k);
    const int c = deep_chunk(k, chunk);
    TRID_REQUIRE(c != 0, "%s: chunk must be 0 or a power of two in [max(64, 2 * next_pow2(k)) = %d, %d]; got %d", who,
                 2 * next_pow2(k) > 64 ? 2 * next_pow2(k) : 64, DEEP_CHUNK_MAX, chunk);
    // two elements must not alias: one of the strides spans the whole extent of the other
    TRID_REQUIRE(ld_q >= 1 && ld_g >= 1 && (ld_q >= (long long)(G - 1) * ld_g + 1 || ld_g >= (long long)(Q - 1) * ld_q + 1),
                 "%s: ld_q = %lld, ld_g = %lld make two elements of a [%d, %d] matrix alias", who, ld_q, ld_g, Q, G);
    TRID_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 7u) == 0 && (reinterpret_cast<uintptr_t>(sim) & 3u) == 0 &&
                     (reinterpret_cast<uintptr_t>(mask_words) & 3u) == 0 && (reinterpret_cast<uintptr_t>(col) & 3u) == 0 &&
                     (reinterpret_cast<uintptr_t>(out_idx) & 7u) == 0,
                 "%s: %s must be 4-byte, out_idx / ws 8-byte aligned", who, pairs ? "val / col" : "sim / mask_words");
    long long n1, n2;
    deep_lists(G, k, c, &n1, &n2);
    TRID_REQUIRE(n1 * Q <= DEEP_GROUPS_MAX, "%s: Q * ceil(%s / chunk) = %lld workgroups exceed the grid of %lld (2^32 threads)", who, gname, n1 * Q,
                 DEEP_GROUPS_MAX);
    const long long need = trid_topk_rows_deep_ws_bytes(Q, G, k, chunk);
    TRID_REQUIRE(ws_bytes >= need, "%s: ws_bytes = %lld, trid_topk_rows_deep_ws_bytes asks for %lld", who, ws_bytes, need);
    hipStream_t stream = (hipStream_t)stream_;
    int rc = deep_raise_lds(who);
    if (rc) return rc;

    DeepPair* buf[2] = {reinterpret_cast<DeepPair*>(ws), reinterpret_cast<DeepPair*>(ws) + n1 * Q * k};
    DeepArgs a;
    memset(&a, 0, sizeof(a));
    a.Q = Q; a.k = k; a.K2 = next_pow2(k);
    a.out_val = out_val; a.out_idx = (long long*)out_idx; a.idx_offset = idx_offset;
    a.sim = sim; a.col = (const int*)col; a.ld_q = ld_q; a.ld_g = ld_g; a.mask = mask_words; a.G = G; a.chunk = c;
    a.P = G < c ? (next_pow2(G) > 64 ? next_pow2(G) : 64) : c;  // (one short chunk: no more pairs than the row has; >= K2 as k <= G)
    a.nout = (int)n1;
    a.out = n1 > 1 ? buf[0] : nullptr;
    rc = pairs ? deep_launch<true, true>(who, a, n1 * Q, stream) : deep_launch<true>(who, a, n1 * Q, stream);
    if (rc) return rc;
    const int fan = c / k;
    int src = 0;
    for (long long nin = n1; nin > 1; src ^= 1) {
        const long long nout = (nin + fan - 1) / fan;
        a.in = buf[src]; a.nin = (int)nin; a.fan = fan; a.nout = (int)nout;
        a.out = nout > 1 ? buf[src ^ 1] : nullptr;
        a.P = next_pow2((nin < fan ? nin : fan) * k);  // (>= 2 K2: at least two lists of k)
        rc = deep_launch<false>(who, a, nout * Q, stream);
        if (rc) return rc;
        nin = nout;
    }
    return TRID_OK;
}

extern "C" int trid_topk_rows_deep_f32(const float* sim, long long ld_q, long long ld_g, int Q, int G, int k, const uint32_t* mask_words,
                                       long long idx_offset, float* out_val, int64_t* out_idx, void* ws, long long ws_bytes, int chunk,
                                       void* stream_) {
    return deep_select("trid_topk_rows_deep_f32", "G", sim, nullptr, false, ld_q, ld_g, Q, G, k, mask_words, idx_offset, out_val, out_idx, ws,
                       ws_bytes, chunk, stream_);
}

extern "C" int trid_topk_rows_deep_pairs_f32(const float* val, const int32_t* col, long long ld_q, long long ld_g, int Q, int n_slots, int k,
                                             long long idx_offset, float* out_val, int64_t* out_idx, void* ws, long long ws_bytes, int chunk,
                                             void* stream_) {
    return deep_select("trid_topk_rows_deep_pairs_f32", "n_slots", val, col, true, ld_q, ld_g, Q, n_slots, k, nullptr, idx_offset, out_val, out_idx,
                       ws, ws_bytes, chunk, stream_);
}
