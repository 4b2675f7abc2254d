// GalleryIndex search (textreid_amd/index.py): the top-k of at most 32 queries against a persistent P16 gallery in ONE pass.
//
// The retrieval filter of gemm_stream.hip (FUSE 4) is built for Q = 1e4: 256 resident queries per workgroup on 8 column waves, a
// threshold taken from a first panel, candidate lists in global memory and merges between growing segments.  For a handful of
// queries seven of its eight column waves multiply zero padding.  Here
//   * the whole query panel (32 queries x K = 256, 32 KB) is ONE set of MFMA B fragments, 128 VGPRs, resident in EVERY wave;
//   * the waves of a workgroup split the gallery ROWS: a step tile is IX_NW x 32 rows, each wave brings its own 32 rows in by
//     LDS-DMA into a private two-slot ring (16-byte units XOR-swizzled by the row, as gemm_stream.hip) - no barrier in the loop;
//   * persistent workgroups own contiguous ranges of step tiles: every gallery row is read from HBM exactly once;
//   * selection needs no earlier pass: a lane keeps a running threshold of its query (from -inf), appends the rare elements above
//     it to a lane-private staging list in LDS and folds the list into a sorted list of 16 in registers when it fills;
//   * a workgroup leaves one sorted list of k per query; a second launch merges the workgroups' lists.
// index_search_kernel<true> (trid_index_search_masked_p16) also honours a per-row ALLOW bit: a wave's 32 rows of a step tile are one
// 32-bit mask word, read on the scalar path; a row whose bit is clear becomes -inf BEFORE the selection sees it, so it is never
// staged and never tightens the threshold.  trid_index_pack_mask_u32 derives the words from byte arrays (liveness, caller's mask).
// Arithmetic and product order are those of gemm_p16_kernel<A_KC> (hi*lo + lo*hi + hi*hi per 16-deep k step, k ascending, gallery
// = A, queries = B): the similarities are bit-identical to trid_gemm_p16 on the same operands.
// ONE order everywhere: value descending, then gallery row ascending - the result does not depend on the partition.
// index_search_kernel<true, true> (trid_index_search_distinct_p16) answers "the k best PEOPLE": every row carries an int32 group id
// (equal ids = one person) and every list - lane, workgroup, final - holds at most one entry per group, the group's first row in the
// order above.  The wave's 32 ids of a step tile come in by LDS-DMA beside its rows, a staging entry is (value, row, group), and the
// insert de-duplicates (ix_insert_distinct).  The k-th entry of a de-duplicated list over SOME rows bounds the k-th distinct value
// over ALL rows from below, so the running threshold and the strict comparison against it hold as they are; the top-k-distinct of
// a union is the top-k-distinct of the parts' lists, so every merge is the same insert (index_merge_distinct_kernel in pass 2).

#include <algorithm>
#include <cstdio>
#include <mutex>

#include "split_common.h"
#include "topk_wave.h"

namespace trid {

namespace {

constexpr int IX_NW = 2;                  // waves per workgroup (two private rings of 2 x 32 KB fill the LDS)
constexpr int IX_RB = IX_NW * 32;         // gallery rows per step tile
constexpr int IX_ROWB = 1024;             // bytes of one P16 row (K = 256)
constexpr int IX_SLOT = 32 * IX_ROWB;     // one wave's tile
constexpr int IX_MAX_WORKERS = 4096;
constexpr int IX_CUS = 256;

// The staging lists of one instantiation.  Rows: entries of (value, row), fold at 8, 24 entries per lane, 2 x 12 KB beside the 128 KB
// of rings.  Distinct: entries of (value, row, group) - a fold can come tiles after the staging, so the id travels with the entry -
// and 2 x 2 x 256 B of id slots; at 24 entries that would be 165 KB, so the fold is due at 4 and a lane holds 19: 157.5 KB.
template <bool DISTINCT>
struct IxCfg {
    static constexpr int FOLD = DISTINCT ? 4 : 8;     // a fold is due at FOLD staged entries; one tile adds at most 16
    static constexpr int SCAP = DISTINCT ? 19 : 24;   // staging entries per lane
    static constexpr int ENT = DISTINCT ? 12 : 8;     // bytes of an entry
    static constexpr int ESTEP = 64 * ENT;            // [entry][lane] x ENT: bytes between a lane's entries
    static constexpr int STG = SCAP * ESTEP;          // bytes of one wave's staging lists
    static constexpr int IDSLOT = 256;                // one LDS-DMA of 4 bytes per lane: the ids of a wave's 32 rows, then zeros
    static constexpr int IDS = DISTINCT ? IX_NW * 2 * IDSLOT : 0;
    static constexpr int LDS = IX_NW * 2 * IX_SLOT + IDS + IX_NW * STG;
    static_assert(SCAP >= FOLD - 1 + 16 && SCAP >= TOPK_MAX, "staging list: one tile beyond the fold mark, and the final lists");
    static_assert(LDS <= 160 * 1024, "LDS of one CU");
};
static_assert(IxCfg<false>::LDS == 128 * 1024 + 24 * 1024 && IxCfg<true>::LDS == 128 * 1024 + 1024 + 2 * 14592, "the two LDS totals");

struct IxParams {
    const char* q16;    // P16 [32][256], rows >= Q zero
    const char* g16;    // P16 [G][256]
    const float* unit;  // the amax both were packed with
    float* wval;        // [Q][W][k]
    int* wrow;          // [Q][W][k]
    int Q, G, k, W, tiles;
};

__device__ __forceinline__ void ix_dma16(const __amdgpu_buffer_rsrc_t& rs, void* lds_base, unsigned voffset) {
    typedef __attribute__((address_space(3))) void* lds_ptr;
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (lds_ptr)lds_base, 16, voffset, 0, 0, 0);
}
__device__ __forceinline__ void ix_dma4(const __amdgpu_buffer_rsrc_t& rs, void* lds_base, unsigned voffset) {
    typedef __attribute__((address_space(3))) void* lds_ptr;
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (lds_ptr)lds_base, 4, voffset, 0, 0, 0);
}
// (inline asm: beside an LDS-DMA in flight hipcc orders a visible LDS access behind s_waitcnt vmcnt(0))
__device__ __forceinline__ void ix_lds_store(unsigned addr, unsigned v) { asm volatile("ds_write_b32 %0, %1" ::"v"(addr), "v"(v) : "memory"); }
__device__ __forceinline__ unsigned ix_lds_load(unsigned addr) {
    unsigned r;
    asm volatile("ds_read_b32 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(r) : "v"(addr) : "memory");
    return r;
}

// "a comes before b": value descending, then row ascending (empty slots are -inf / -1: behind every real pair)
__device__ __forceinline__ bool ix_before(float av, int ar, float bv, int br) { return av > bv || (av == bv && (unsigned)ar < (unsigned)br); }

// The de-duplicating insert of (cv, cr, cg) into a sorted list with at most one entry per group, branch-free over the 16 slots.  The
// candidate bubbles down as in the plain insert; the slot that holds its group ends the pass: a candidate that has not found its
// place by then is dropped (an equal or better row of the group is there), otherwise the slot takes the entry shifted into it and
// the group's old entry is discarded.  Without such a slot the last entry falls off.  Empty slots are (-inf, -1, -1); ids may be
// any int32 (a real group -1 meets its own entry before it meets an empty slot, and an empty slot ends the shift anyway).
__device__ __forceinline__ void ix_insert_distinct(float (&lv)[TOPK_MAX], int (&lr)[TOPK_MAX], int (&lg)[TOPK_MAX], float cv, int cr, int cg) {
    const int g0 = cg;
#pragma unroll
    for (int i = 0; i < TOPK_MAX; ++i) {
        const bool b = ix_before(cv, cr, lv[i], lr[i]);
        const bool m = lg[i] == g0;
        const float tv = lv[i];
        const int tr = lr[i], tg = lg[i];
        lv[i] = b ? cv : tv;
        lr[i] = b ? cr : tr;
        lg[i] = b ? cg : tg;
        cv = m ? -INFINITY : (b ? tv : cv);
        cr = m ? -1 : (b ? tr : cr);
        cg = b ? tg : cg;
    }
}

}  // namespace

// MASKED: mask = uint32[ceil(G / 32)], bit (r & 31) of word (r >> 5) set = row r may be returned (unused and NULL otherwise)
// DISTINCT: gid = int32[G], the group of every row; at most one row per group is returned; mask may be NULL (every row allowed)
template <bool MASKED, bool DISTINCT>
__global__ __launch_bounds__(IX_NW * 64) void index_search_kernel(IxParams p, const unsigned* __restrict__ mask, const int* __restrict__ gid) {
    static_assert(MASKED || !DISTINCT, "the distinct form is built on the masked one");
    using Cfg = IxCfg<DISTINCT>;
    constexpr int KG = 8;
    extern __shared__ __attribute__((aligned(16))) uint4 ix_smem[];
    char* const lds = reinterpret_cast<char*>(ix_smem);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int khalf = lane >> 5;
    char* const ring = lds + wave * (2 * IX_SLOT);
    char* const ids = lds + IX_NW * 2 * IX_SLOT + wave * (2 * Cfg::IDSLOT);  // (DISTINCT) this wave's two id slots
    char* const stg_all = lds + IX_NW * 2 * IX_SLOT + Cfg::IDS;
    // this lane's staging entry 0; entries are Cfg::ESTEP bytes apart (one VGPR: see gemm_stream.hip f_wbuf)
    unsigned stg = (unsigned)(uintptr_t)(stg_all + wave * Cfg::STG) + (unsigned)lane * (unsigned)Cfg::ENT;
    asm volatile("" : "+v"(stg));

    // this worker's contiguous range of step tiles
    const int w = blockIdx.x;
    const int t0 = (int)((long long)w * p.tiles / p.W), t1 = (int)((long long)(w + 1) * p.tiles / p.W);

    const float s = f16_scale_of(*p.unit);
    const float unscale = 1.f / (s * s);

    // the query panel: [k group][k step][plane] fragments, 128 VGPRs
    f16x8 bf[KG][2][2];
    {
        const char* br = p.q16 + (size_t)(lane & 31) * IX_ROWB;
#pragma unroll
        for (int g = 0; g < KG; ++g)
#pragma unroll
            for (int ks = 0; ks < 2; ++ks)
#pragma unroll
                for (int pl = 0; pl < 2; ++pl)
                    bf[g][ks][pl] = __builtin_bit_cast(f16x8, *reinterpret_cast<const uint4*>(br + g * 128 + (4 * pl + 2 * ks + khalf) * 16));
    }
    const __amdgpu_buffer_rsrc_t rsG = __builtin_amdgcn_make_buffer_rsrc((void*)p.g16, 0, (unsigned)((size_t)p.G * IX_ROWB), 0x00020000);
    constexpr unsigned OOB = 0x80000000u;
    __amdgpu_buffer_rsrc_t rsI = rsG;
    if constexpr (DISTINCT) rsI = __builtin_amdgcn_make_buffer_rsrc((void*)gid, 0, (unsigned)((size_t)p.G * 4), 0x00020000);

    // running threshold of this lane's query: -inf admits everything; the zero padding columns of the panel admit nothing
    const bool q_live = (lane & 31) < p.Q;
    float f_thr = q_live ? -INFINITY : INFINITY;
    // this lane's sorted list: the best 16 pairs among the rows IT saw (its query, the rows of its k half); the first k count
    float lv[TOPK_MAX];
    int lr[TOPK_MAX];
    int lg[DISTINCT ? TOPK_MAX : 1];  // (DISTINCT) the groups of the pairs: all different but for the empty slots' -1
#pragma unroll
    for (int i = 0; i < TOPK_MAX; ++i) {
        lv[i] = -INFINITY;
        lr[i] = -1;
        if constexpr (DISTINCT) lg[i] = -1;
    }
    int cnt = 0;  // staged entries of this lane

    // one DMA instruction = one gallery row (64 units of 16 bytes); lane = stored unit, source unit = lane ^ (row & 15).  Rows
    // beyond G lie beyond the descriptor's range: the slot reads zeros there
    auto issue = [&](int tile, int slot, int zero) {
        const int ln = lane + zero;
        const int row0 = tile * IX_RB + wave * 32;
        char* dst = ring + slot * IX_SLOT;
#pragma unroll
        for (int d = 0; d < 32; ++d) {
            const int row = row0 + d;
            ix_dma16(rsG, dst + d * IX_ROWB, row < p.G ? (unsigned)row * (unsigned)IX_ROWB + (unsigned)((ln ^ (d & 15)) << 4) : OOB);
        }
        // the ids of the same 32 rows, lane = row: issued beside the rows, so the wait that orders the tile orders them too (the
        // upper 32 lanes and rows beyond G lie beyond the range: zeros)
        if constexpr (DISTINCT) ix_dma4(rsI, ids + slot * Cfg::IDSLOT, (ln < 32 && row0 + ln < p.G) ? (unsigned)(row0 + ln) * 4u : OOB);
    };

    // staged pairs -> the sorted list (one pair per lane and round, every lane its own), then the tightened threshold
    auto fold = [&]() {
        const int nmax = __builtin_amdgcn_readfirstlane((int)wave_max((float)cnt));
        for (int e = 0; e < nmax; ++e) {
            const bool has = e < cnt;
            float cv = -INFINITY;
            int cr = -1, cg = -1;
            if (has) {
                cv = __uint_as_float(ix_lds_load(stg + (unsigned)Cfg::ESTEP * (unsigned)e));
                cr = (int)ix_lds_load(stg + (unsigned)Cfg::ESTEP * (unsigned)e + 4u);
                if constexpr (DISTINCT) cg = (int)ix_lds_load(stg + (unsigned)Cfg::ESTEP * (unsigned)e + 8u);
            }
            if constexpr (DISTINCT) {
                ix_insert_distinct(lv, lr, lg, cv, cr, cg);
            } else {
#pragma unroll
                for (int i = 0; i < TOPK_MAX; ++i) {
                    const bool b = ix_before(cv, cr, lv[i], lr[i]);
                    const float tv = lv[i];
                    const int tr = lr[i];
                    lv[i] = b ? cv : tv;
                    lr[i] = b ? cr : tr;
                    cv = b ? tv : cv;
                    cr = b ? tr : cr;
                }
            }
        }
        cnt = 0;
        float kth = lv[0];
#pragma unroll
        for (int i = 1; i < TOPK_MAX; ++i) kth = (i == p.k - 1) ? lv[i] : kth;
        // the k-th best of EITHER half of the query's rows bounds the k-th best of all of them from below
        kth = fmaxf(kth, __shfl_xor(kth, 32, 64));
        if (q_live) f_thr = kth;
    };

    const int a_off = (lane & 31) * IX_ROWB;
    const int rsw = lane & 15;
    const unsigned id_at = (unsigned)(uintptr_t)ids + 16u * (unsigned)khalf;  // (DISTINCT) the id of this lane's element 0 in slot 0

    // the panel's loads are waited for HERE, by an instruction the compiler accounts for (gemm_stream.hip, same place)
#pragma unroll
    for (int g = 0; g < KG; ++g)
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
#pragma unroll
            for (int pl = 0; pl < 2; ++pl) asm volatile("" : "+v"(bf[g][ks][pl]));
    asm volatile("" : "+v"(f_thr));
    __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0)

    if (t0 < t1) issue(t0, 0, 0);
    int slot = 0;
    for (int t = t0; t < t1; ++t, slot ^= 1) {
        // this wave's own DMA of tile t: its covering vmcnt orders it for this wave's reads
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        int zero = 0;
        asm volatile("" : "+v"(zero));
        // this wave's 32 rows are ONE mask word, the same for every lane: a scalar load (it counts on lgkmcnt, not on the vmcnt that
        // orders the ring), issued BEFORE the DMA of tile t + 1 so that it neither queues behind those 32 KB nor is waited for
        // before they are under way (a wave without rows in a ragged last tile has no word)
        unsigned mw = 0xFFFFFFFFu;
        if constexpr (DISTINCT) {
            const int word = t * IX_NW + wave;
            if (mask != nullptr) mw = word * 32 < p.G ? mask[word] : 0u;
        } else if constexpr (MASKED) {
            const int word = t * IX_NW + wave;
            mw = word * 32 < p.G ? mask[word] : 0u;
        }
        // the other slot was last read by the MFMAs of tile t - 1, all issued: free
        if (t + 1 < t1) issue(t + 1, slot ^ 1, zero);

        v16f acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
        const char* sA = ring + slot * IX_SLOT;
        f16x8 af[2][2];
        auto fetch = [&](int q, f16x8(&dst)[2]) {  // q = k group * 2 + k step
            const int g = q >> 1, ks = q & 1;
            const int u0 = g * 8 + 2 * ks + khalf;
            dst[0] = __builtin_bit_cast(f16x8, *reinterpret_cast<const uint4*>(sA + a_off + ((u0 ^ rsw) << 4)));
            dst[1] = __builtin_bit_cast(f16x8, *reinterpret_cast<const uint4*>(sA + a_off + (((u0 + 4) ^ rsw) << 4)));
        };
        fetch(0, af[0]);
#pragma unroll
        for (int q = 0; q < 2 * KG; ++q) {
            if (q + 1 < 2 * KG) fetch(q + 1, af[(q + 1) & 1]);
            const int g = q >> 1, ks = q & 1;
            acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[q & 1][0], bf[g][ks][1], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[q & 1][1], bf[g][ks][0], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[q & 1][0], bf[g][ks][0], acc, 0, 0, 0);
        }

        // ---- selection: element r of the accumulator = (gallery row rb + (r & 3) + 8 (r >> 2), query lane & 31)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] *= unscale;
        const int rb = t * IX_RB + wave * 32 + 4 * khalf;
        if ((t + 1) * IX_RB > p.G) {  // (a ragged last tile read zeros: never candidates)
#pragma unroll
            for (int r = 0; r < 16; ++r)
                if (rb + (r & 3) + 8 * (r >> 2) >= p.G) acc[r] = -INFINITY;
        }
        if constexpr (MASKED) {
            // The allow bits come BEFORE the maximum and the threshold: a disallowed row becomes -inf, so it is never staged and never
            // moves f_thr.  Element r is row 4 khalf + (r & 3) + 8 (r >> 2) of the wave's 32: the lanes of k half 0 look at bit
            // b = (r & 3) + 8 (r >> 2) of the word, those of k half 1 at bit b + 4 - a 64-bit LANE mask formed on the scalar unit
            // (two sign-extended 1-bit fields), one v_cndmask per element (the compiler's own form tests the bit per lane: 3 VALU)
            if (mw != 0xFFFFFFFFu) {
                const float ninf = -INFINITY;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int b = (r & 3) + 8 * (r >> 2);
                    const unsigned lo = (unsigned)((int)(mw << (31 - b)) >> 31), hi = (unsigned)((int)(mw << (27 - b)) >> 31);
                    const unsigned long long keep = ((unsigned long long)hi << 32) | lo;
                    float a = acc[r];
                    asm("v_cndmask_b32_e64 %0, %1, %0, %2" : "+v"(a) : "v"(ninf), "s"(keep));
                    acc[r] = a;
                }
            }
        }
        float mx = acc[0];
#pragma unroll
        for (int r = 1; r < 16; ++r) mx = fmaxf(mx, acc[r]);
        // rows ascend with time: a later element that only EQUALS the k-th best loses the tie - strictly above the threshold
        if (__ballot(mx > f_thr) != 0ull) {
            if (mx > f_thr) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    if (acc[r] > f_thr) {
                        const unsigned a = stg + (unsigned)Cfg::ESTEP * (unsigned)cnt;
                        ix_lds_store(a, __float_as_uint(acc[r]));
                        ix_lds_store(a + 4u, (unsigned)(rb + (r & 3) + 8 * (r >> 2)));
                        // the row's id is read only here, for an element that is staged: row 4 khalf + (r & 3) + 8 (r >> 2) of the slot
                        if constexpr (DISTINCT) ix_lds_store(a + 8u, ix_lds_load(id_at + (unsigned)(slot * Cfg::IDSLOT + 4 * ((r & 3) + 8 * (r >> 2)))));
                        ++cnt;
                    }
                }
            }
            if (__ballot(cnt >= Cfg::FOLD) != 0ull) fold();
        }
    }
    fold();

    // ---- the workgroup's list of k per query: the 2 x IX_NW sorted lane lists of the query, merged by lane `query` of wave 0
#pragma unroll
    for (int i = 0; i < TOPK_MAX; ++i) {
        ix_lds_store(stg + (unsigned)Cfg::ESTEP * (unsigned)i, __float_as_uint(lv[i]));
        ix_lds_store(stg + (unsigned)Cfg::ESTEP * (unsigned)i + 4u, (unsigned)lr[i]);
        if constexpr (DISTINCT) ix_lds_store(stg + (unsigned)Cfg::ESTEP * (unsigned)i + 8u, (unsigned)lg[i]);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __syncthreads();
    if constexpr (DISTINCT) {
        // lane `query` of wave 0 holds the list of its own rows: the other 2 x IX_NW - 1 lists of the query go through the same insert
        if (wave == 0 && lane < p.Q) {
            for (int l = 1; l < 2 * IX_NW; ++l) {
                const char* src = stg_all + (l >> 1) * Cfg::STG + (lane + 32 * (l & 1)) * Cfg::ENT;
                for (int e = 0; e < TOPK_MAX; ++e) {
                    const int* f = reinterpret_cast<const int*>(src + e * Cfg::ESTEP);
                    ix_insert_distinct(lv, lr, lg, __int_as_float(f[0]), f[1], f[2]);
                }
            }
            float* ov = p.wval + ((long long)lane * p.W + w) * p.k;
            int* orow = p.wrow + ((long long)lane * p.W + w) * p.k;
#pragma unroll
            for (int j = 0; j < TOPK_MAX; ++j) {
                if (j < p.k) {
                    ov[j] = lv[j];
                    orow[j] = lr[j];
                }
            }
        }
    } else if (wave == 0 && lane < p.Q) {
        constexpr int NL = 2 * IX_NW;
        int head[NL];
        const float2* src[NL];
#pragma unroll
        for (int l = 0; l < NL; ++l) {
            head[l] = 0;
            src[l] = reinterpret_cast<const float2*>(stg_all + (l >> 1) * Cfg::STG) + lane + 32 * (l & 1);  // entry e at src[l][64 e]
        }
        float* ov = p.wval + ((long long)lane * p.W + w) * p.k;
        int* orow = p.wrow + ((long long)lane * p.W + w) * p.k;
        for (int j = 0; j < p.k; ++j) {
            float bv = -INFINITY;
            int br = -1, bl = 0;
#pragma unroll
            for (int l = 0; l < NL; ++l) {
                if (head[l] < TOPK_MAX) {
                    const float2 e = src[l][64 * head[l]];
                    const int er = __float_as_int(e.y);
                    if (ix_before(e.x, er, bv, br)) {
                        bv = e.x;
                        br = er;
                        bl = l;
                    }
                }
            }
#pragma unroll
            for (int l = 0; l < NL; ++l) head[l] += (l == bl && br >= 0) ? 1 : 0;
            ov[j] = bv;
            orow[j] = br;
        }
    }
}

// pass 2: one wave per query folds the W x k pairs the workers left (empty slots -inf / -1 are skipped) into the final list
__global__ __launch_bounds__(256) void index_merge_kernel(const float* __restrict__ wval, const int* __restrict__ wrow, int Q, int n, int k,
                                                          long long idx_offset, float* __restrict__ out_val, long long* __restrict__ out_idx) {
    const int lane = threadIdx.x & 63;
    const int q = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= Q) return;
    WaveTopk<TOPK_MAX> L;
    L.init(lane, nullptr, nullptr);
    const float* v = wval + (long long)q * n;
    const int* r = wrow + (long long)q * n;
    for (int base = 0; base < n; base += 64) {
        const bool in = base + lane < n;
        const int row = in ? r[base + lane] : -1;
        const float x = in ? v[base + lane] : -INFINITY;
        L.offer_lanes(row >= 0, x, idx_offset + row);
    }
    if (lane < k) {
        out_val[(long long)q * k + lane] = L.lv;
        out_idx[(long long)q * k + lane] = L.li;
    }
}

// pass 2 of the distinct search: the same fold with at most one pair per group.  The wave holds the list one pair per lane (lane i =
// i-th best); a pair whose group is in the list ahead of its place is dropped, otherwise the lanes from its place down to the group's
// old pair (or to the end of the list) shift by one.  The groups are read here, by row: an ordinary load in a launch of its own.
__global__ __launch_bounds__(256) void index_merge_distinct_kernel(const float* __restrict__ wval, const int* __restrict__ wrow,
                                                                   const int* __restrict__ gid, int Q, int n, int k, long long idx_offset,
                                                                   float* __restrict__ out_val, long long* __restrict__ out_idx) {
    const int lane = threadIdx.x & 63;
    const int q = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= Q) return;
    float lv = -INFINITY;  // lanes >= TOPK_MAX stay empty
    int lr = -1, lg = -1;
    float t = -INFINITY;   // the pair of lane TOPK_MAX - 1: what a candidate must come before
    int tr = -1;
    const float* v = wval + (long long)q * n;
    const int* r = wrow + (long long)q * n;
    // U x 64 pairs per round: the loads of a round are independent, and so are the gathers of the groups that follow them (one
    // dependent chain of two memory latencies per round, not per 64 pairs)
    constexpr int U = 8;
    for (int base = 0; base < n; base += 64 * U) {
        int row[U], grp[U];
        float x[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int i = base + 64 * u + lane;
            row[u] = i < n ? r[i] : -1;
            x[u] = i < n ? v[i] : -INFINITY;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) grp[u] = row[u] >= 0 ? gid[row[u]] : -1;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            unsigned long long bal = __ballot(row[u] >= 0 && x[u] >= t);
            while (bal) {
                const int src = __ffsll((long long)bal) - 1;
                bal &= bal - 1;
                const float cv = __shfl(x[u], src, 64);
                const int cr = __shfl(row[u], src, 64), cg = __shfl(grp[u], src, 64);
                if (!ix_before(cv, cr, t, tr)) continue;
                const int pos = __popcll(__ballot(lane < TOPK_MAX && ix_before(lv, lr, cv, cr)));
                const unsigned long long same = __ballot(lane < TOPK_MAX && lr >= 0 && lg == cg);
                const int dup = same ? __ffsll((long long)same) - 1 : TOPK_MAX - 1;  // (no such pair: the last one falls off)
                if (dup < pos) continue;
                const float uv = __shfl_up(lv, 1, 64);
                const int ur = __shfl_up(lr, 1, 64), ug = __shfl_up(lg, 1, 64);
                if (lane > pos && lane <= dup) { lv = uv; lr = ur; lg = ug; }
                if (lane == pos) { lv = cv; lr = cr; lg = cg; }
                t = __shfl(lv, TOPK_MAX - 1, 64);
                tr = __shfl(lr, TOPK_MAX - 1, 64);
            }
        }
    }
    if (lane < k) {
        out_val[(long long)q * k + lane] = lv;
        out_idx[(long long)q * k + lane] = lr >= 0 ? idx_offset + lr : -1;
    }
}

// words[w] bit b = live[32 w + b] && allow[32 w + b] for rows < n (a NULL array counts as all ones), 0 beyond: one ballot per 64 rows
__global__ __launch_bounds__(256) void index_pack_mask_kernel(const uint8_t* __restrict__ live, const uint8_t* __restrict__ allow, int n,
                                                              unsigned* __restrict__ words, int n_words) {
    const long long row = (long long)blockIdx.x * 256 + threadIdx.x;
    bool on = row < n;
    if (on && live != nullptr) on = live[row] != 0;
    if (on && allow != nullptr) on = allow[row] != 0;
    const unsigned long long b = __ballot(on);
    const int lane = threadIdx.x & 63;
    const long long w = (row >> 6) * 2 + (lane >> 5);
    if ((lane & 31) == 0 && w < n_words) words[w] = lane ? (unsigned)(b >> 32) : (unsigned)b;
}

static int ix_workers(int G, int workgroups) {
    if (workgroups > 0) return workgroups;
    const int tiles = (G + IX_RB - 1) / IX_RB;
    return std::max(1, std::min(IX_CUS, tiles));  // one persistent workgroup per CU (its rings fill the LDS), no more than tiles
}

}  // namespace trid

using namespace trid;

extern "C" long long trid_index_search_ws_bytes(int G, int Q, int k, int workgroups) {
    if (G <= 0 || Q <= 0 || k <= 0 || workgroups < 0 || workgroups > IX_MAX_WORKERS) return 0;
    return (long long)ix_workers(G, workgroups) * Q * k * 8;
}

// DISTINCT (with MASKED): group_ids is required, mask_words may be NULL
template <bool MASKED, bool DISTINCT>
static int ix_search(const char* fn, const void* q16, const void* g16, const float* unit_amax, const int32_t* group_ids,
                     const uint32_t* mask_words, int Q, int G, int k, long long idx_offset, float* out_val, int64_t* out_idx, void* ws,
                     int workgroups, void* stream) {
    TRID_REQUIRE(q16 && g16 && unit_amax && out_val && out_idx && ws, "%s: null operand", fn);
    if (MASKED && !DISTINCT) TRID_REQUIRE(mask_words != nullptr, "%s: null mask_words (the unmasked search is trid_index_search_p16)", fn);
    if (DISTINCT) TRID_REQUIRE(group_ids != nullptr, "%s: null group_ids", fn);
    TRID_REQUIRE(Q >= 1 && Q <= 32, "%s: 1 <= Q <= 32 (Q=%d): larger batches go through trid_sim_topk_p16", fn, Q);
    TRID_REQUIRE(G >= 1 && (long long)G * IX_ROWB < (1ll << 31), "%s: 1 <= G and G * 1024 < 2^31 (G=%d)", fn, G);
    TRID_REQUIRE(k >= 1 && k <= TOPK_MAX && k <= G, "%s: k must be in [1,%d] and <= G (k=%d G=%d)", fn, TOPK_MAX, k, G);
    TRID_REQUIRE(workgroups >= 0 && workgroups <= IX_MAX_WORKERS, "%s: 0 <= workgroups <= %d (workgroups=%d)", fn, IX_MAX_WORKERS, workgroups);
    TRID_REQUIRE(aligned16(q16) && aligned16(g16) && aligned16(ws), "%s: operands must be 16-byte aligned", fn);
    if (MASKED) TRID_REQUIRE((reinterpret_cast<uintptr_t>(mask_words) & 3u) == 0, "%s: mask_words must be 4-byte aligned", fn);
    if (DISTINCT) TRID_REQUIRE((reinterpret_cast<uintptr_t>(group_ids) & 3u) == 0, "%s: group_ids must be 4-byte aligned", fn);
    static std::once_flag once;  // (one per instantiation)
    static hipError_t attr_err = hipSuccess;
    std::call_once(once, [] {
        attr_err = hipFuncSetAttribute((const void*)index_search_kernel<MASKED, DISTINCT>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    });
    if (attr_err != hipSuccess) {
        set_error("%s: cannot reserve LDS: %s", fn, hipGetErrorString(attr_err));
        return (int)attr_err;
    }
    IxParams p;
    p.q16 = (const char*)q16; p.g16 = (const char*)g16; p.unit = unit_amax;
    p.Q = Q; p.G = G; p.k = k;
    p.W = ix_workers(G, workgroups);
    p.tiles = (G + IX_RB - 1) / IX_RB;
    p.wval = reinterpret_cast<float*>(ws);
    p.wrow = reinterpret_cast<int*>(p.wval + (long long)p.W * Q * k);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL((index_search_kernel<MASKED, DISTINCT>), dim3(p.W), dim3(IX_NW * 64), IxCfg<DISTINCT>::LDS, s, p,
                       reinterpret_cast<const unsigned*>(mask_words), reinterpret_cast<const int*>(group_ids));
    char what[80];
    int rc = check_launch(fn);
    if (rc != TRID_OK) return rc;
    if (DISTINCT)
        hipLaunchKernelGGL(index_merge_distinct_kernel, dim3((Q + 3) / 4), dim3(256), 0, s, p.wval, p.wrow, reinterpret_cast<const int*>(group_ids), Q,
                           p.W * k, k, idx_offset, out_val, reinterpret_cast<long long*>(out_idx));
    else
        hipLaunchKernelGGL(index_merge_kernel, dim3((Q + 3) / 4), dim3(256), 0, s, p.wval, p.wrow, Q, p.W * k, k, idx_offset, out_val, reinterpret_cast<long long*>(out_idx));
    snprintf(what, sizeof what, "%s (merge)", fn);
    return check_launch(what);
}

extern "C" int trid_index_search_p16(const void* q16, const void* g16, const float* unit_amax, int Q, int G, int k, long long idx_offset,
                                     float* out_val, int64_t* out_idx, void* ws, int workgroups, void* stream) {
    return ix_search<false, false>("trid_index_search_p16", q16, g16, unit_amax, nullptr, nullptr, Q, G, k, idx_offset, out_val, out_idx, ws, workgroups, stream);
}

extern "C" int trid_index_search_masked_p16(const void* q16, const void* g16, const float* unit_amax, const uint32_t* mask_words, int Q, int G,
                                            int k, long long idx_offset, float* out_val, int64_t* out_idx, void* ws, int workgroups,
                                            void* stream) {
    return ix_search<true, false>("trid_index_search_masked_p16", q16, g16, unit_amax, nullptr, mask_words, Q, G, k, idx_offset, out_val, out_idx, ws,
                                  workgroups, stream);
}

extern "C" int trid_index_search_distinct_p16(const void* q16, const void* g16, const float* unit_amax, const int32_t* group_ids,
                                              const uint32_t* mask_words, int Q, int G, int k, long long idx_offset, float* out_val,
                                              int64_t* out_idx, void* ws, int workgroups, void* stream) {
    return ix_search<true, true>("trid_index_search_distinct_p16", q16, g16, unit_amax, group_ids, mask_words, Q, G, k, idx_offset, out_val, out_idx,
                                 ws, workgroups, stream);
}

extern "C" int trid_index_pack_mask_u32(const uint8_t* live, const uint8_t* allow, int n, uint32_t* words, int n_words, void* stream) {
    TRID_REQUIRE(live || allow, "trid_index_pack_mask_u32: live and allow are both NULL (one may be: it counts as all ones)");
    TRID_REQUIRE(words != nullptr, "trid_index_pack_mask_u32: null words");
    TRID_REQUIRE((reinterpret_cast<uintptr_t>(words) & 3u) == 0, "trid_index_pack_mask_u32: words must be 4-byte aligned");
    TRID_REQUIRE(n >= 1, "trid_index_pack_mask_u32: n >= 1 (n=%d)", n);
    TRID_REQUIRE((long long)n_words * 32 >= n && n_words <= (1 << 26), "trid_index_pack_mask_u32: ceil(n / 32) <= n_words <= 2^26 (n=%d n_words=%d)", n, n_words);
    const int blocks = (int)(((long long)n_words * 32 + 255) / 256);
    hipLaunchKernelGGL(index_pack_mask_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, live, allow, n, reinterpret_cast<unsigned*>(words), n_words);
    return check_launch("trid_index_pack_mask_u32");
}
