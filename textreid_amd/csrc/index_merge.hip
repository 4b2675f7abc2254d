// List merge (include/textreid_hip.h "trid_index_merge_lists_f32"): the merge step of GalleryShards (textreid_amd/index_shards.py).
// Per query, n_lists candidate lists of k_in (value, local row[, pid]) entries - the answers of the gallery's shards - become the
// first k of their union in the library's one order: value descending by float comparison, then GLOBAL row ascending (global row =
// list_base[list] + local row).  With pids (the distinct form) a candidate counts only if no earlier candidate in that order has
// its pid.  The pass MOVES values and never computes one: the outputs carry the input's bit patterns.
//
// One workgroup per query, everything in LDS, P = max(64, next_pow2(n_lists * k_in)) slots, min(1024, max(64, P / 2)) threads:
//   1. load: slot i = candidate i: its value, its number i and - in a table that is indexed by the candidate NUMBER and does not
//      move - its global row.  A slot with row < 0, and the padding behind the last candidate, is ABSENT: (-inf, row INT64_MAX), which
//      sorts behind every present candidate (a real -inf has a lower row).  The present candidates are counted.
//   2. one full bitonic sort of the (value, number) pairs by (value, table[number]): the lists need not be sorted.  Afterwards the
//      present candidates are the slots [0, present) in the result order.  The rows form writes the first k of them and is done.
//   3. distinct form: the table is reloaded with the candidates' PIDS (the rows are read again at the output), and a second bitonic
//      sort orders the slot POSITIONS of step 2 by (present first, pid, position): the first position of every run of equal pids is
//      that pid's first candidate in the result order.  Those positions are flagged (a bit on the slot's candidate number), a
//      workgroup-wide prefix count over the positions gives every flagged slot its place, and the first k are written.
// Nothing read from `row` or `pid` is ever used as an address: they are compared and copied.  Every LDS index is one of the kernel's
// own numbers in [0, P); the global re-reads of step 3 go through a candidate number that is checked against n_lists * k_in.
// Duplicate global rows among one query's present candidates break the caller's contract: the order between them is then
// unspecified, nothing else is.  NaN: undefined order, as elsewhere.
// LDS: 16 bytes per slot (8 table + 4 value + 4 number) + 128: 128 KB at 8192 candidates - more than the 64 KB a kernel gets
// unasked, so the first call on a device raises the limit of both instantiations (index_merge_raise_lds).

#include "common.h"

namespace trid {

constexpr int MERGE_K_MAX = 1024;
constexpr int MERGE_CAND_MAX = 8192;
constexpr int MERGE_THREADS_MAX = 1024;
constexpr int MERGE_SLOTS_MIN = 64;
constexpr long long MERGE_Q_MAX = (1ll << 22) - 1;  // workgroups of up to 1024 threads in one launch: the runtime takes fewer than 2^32 threads
constexpr long long MERGE_ABSENT = 0x7fffffffffffffffll;
constexpr int MERGE_FIRST = 0x40000000;  // on a slot's candidate number: the first candidate of its pid in the result order
constexpr int MERGE_MISC_BYTES = 128;    // 16 wave counts, the present count, the result count
constexpr int MERGE_LDS_MAX = MERGE_CAND_MAX * 16 + MERGE_MISC_BYTES;

// the global row of candidate i of the query whose lists start at `at` (two's-complement wrap: device contents are not validated)
__device__ __forceinline__ long long merge_global_row(const long long* __restrict__ row, const long long* __restrict__ base, long long at, int i,
                                                      int k_in) {
    const unsigned long long b = base != nullptr ? (unsigned long long)base[i / k_in] : 0ull;
    return (long long)((unsigned long long)row[at + i] + b);
}

template <bool DISTINCT>
__global__ __launch_bounds__(MERGE_THREADS_MAX) void index_merge_kernel(const float* __restrict__ val, const long long* __restrict__ row,
                                                                        const long long* __restrict__ base, const long long* __restrict__ pid,
                                                                        int n, int k_in, int k, int P, float* __restrict__ out_val,
                                                                        long long* __restrict__ out_row, long long* __restrict__ out_pid) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    long long* key = reinterpret_cast<long long*>(smem_raw);  // by candidate number: the global row, then (distinct form) the pid
    float* sv = reinterpret_cast<float*>(key + P);            // by slot: the value; step 3: the positions being ordered
    int* si = reinterpret_cast<int*>(sv + P);                 // by slot: the candidate number
    int* misc = si + P;
    const int tid = threadIdx.x, nt = blockDim.x;
    const long long at = (long long)blockIdx.x * n;
    const long long out_at = (long long)blockIdx.x * k;

    if (tid == 0) misc[16] = 0;
    __syncthreads();
    int mine = 0;
    for (int i = tid; i < P; i += nt) {
        float v = -INFINITY;
        long long g = MERGE_ABSENT;
        if (i < n && row[at + i] >= 0) {
            v = val[at + i];
            g = merge_global_row(row, base, at, i, k_in);
            ++mine;
        }
        key[i] = g;
        sv[i] = v;
        si[i] = i;
    }
    if (mine) atomicAdd(&misc[16], mine);
    __syncthreads();
    const int present = misc[16];

    // step 2: slots in the result order
    for (int k2 = 2; k2 <= P; k2 <<= 1) {
        for (int j = k2 >> 1; j > 0; j >>= 1) {
            for (int e = tid; e < (P >> 1); e += nt) {
                const int i = ((e & ~(j - 1)) << 1) | (e & (j - 1)), l = i | j;
                const float x = sv[i], y = sv[l];
                const int cx = si[i], cy = si[l];
                const bool before = x > y || (x == y && key[cx] < key[cy]);
                if (((i & k2) == 0) != before) {
                    sv[i] = y; sv[l] = x;
                    si[i] = cy; si[l] = cx;
                }
            }
            __syncthreads();
        }
    }

    if (!DISTINCT) {
        for (int t = tid; t < k; t += nt) {
            const bool have = t < present;
            out_val[out_at + t] = have ? sv[t] : -INFINITY;
            out_row[out_at + t] = have ? key[si[t]] : -1ll;
        }
        return;
    }

    // step 3: the positions [0, P) ordered by (present first, pid, position)
    int* ord = reinterpret_cast<int*>(sv);
    for (int i = tid; i < P; i += nt) {
        key[i] = i < n ? pid[at + i] : 0ll;
        ord[i] = i;
    }
    __syncthreads();
    for (int k2 = 2; k2 <= P; k2 <<= 1) {
        for (int j = k2 >> 1; j > 0; j >>= 1) {
            for (int e = tid; e < (P >> 1); e += nt) {
                const int i = ((e & ~(j - 1)) << 1) | (e & (j - 1)), l = i | j;
                const int a = ord[i], b = ord[l];
                const bool pa = a < present, pb = b < present;
                bool before;
                if (pa && pb) {
                    const long long ga = key[si[a]], gb = key[si[b]];
                    before = ga < gb || (ga == gb && a < b);
                } else {
                    before = pa != pb ? pa : a < b;
                }
                if (((i & k2) == 0) != before) {
                    ord[i] = b;
                    ord[l] = a;
                }
            }
            __syncthreads();
        }
    }
    // the first position of every run of equal pids: decided for all of them, then flagged
    unsigned firsts = 0;
    int it = 0;
    for (int t = tid; t < P; t += nt, ++it) {
        const int a = ord[t];
        if (a < present && (t == 0 || key[si[ord[t - 1]]] != key[si[a]])) firsts |= 1u << it;
    }
    __syncthreads();
    it = 0;
    for (int t = tid; t < P; t += nt, ++it)
        if ((firsts >> it) & 1u) si[ord[t]] |= MERGE_FIRST;
    __syncthreads();

    // a thread owns P / nt consecutive positions: its flagged slots follow those of the threads before it
    const int per = P / nt, p0 = tid * per;
    int cnt = 0;
    for (int u = 0; u < per; ++u) cnt += (si[p0 + u] & MERGE_FIRST) != 0;
    int incl = cnt;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int up = __shfl_up(incl, o, 64);
        if ((tid & 63) >= o) incl += up;
    }
    if ((tid & 63) == 63) misc[tid >> 6] = incl;
    __syncthreads();
    int slot = incl - cnt, total = 0;
    for (int w = 0; w < (nt >> 6); ++w) {
        const int c = misc[w];
        if (w < (tid >> 6)) slot += c;
        total += c;
    }
    for (int u = 0; u < per && slot < k; ++u) {
        const int c = si[p0 + u];
        if ((c & MERGE_FIRST) == 0) continue;
        const int cand = c & ~MERGE_FIRST;
        const bool ok = cand < n;  // (always, unless the device contents broke the contract: then a fill slot, never a read outside the lists)
        out_val[out_at + slot] = ok ? val[at + cand] : -INFINITY;
        out_row[out_at + slot] = ok ? merge_global_row(row, base, at, cand, k_in) : -1ll;
        out_pid[out_at + slot] = ok ? key[cand] : -1ll;
        ++slot;
    }
    for (int t = total + tid; t < k; t += nt) {
        out_val[out_at + t] = -INFINITY;
        out_row[out_at + t] = -1ll;
        out_pid[out_at + t] = -1ll;
    }
}

static int merge_next_pow2(long long x) {
    int p = 1;
    while (p < x) p <<= 1;
    return p;
}

// 8192 candidates need more dynamic LDS than the 64 KB a kernel gets unasked.  The FIRST call on a device raises the limit of
// EVERY instantiation, so that a later call - a recorded one, whose arguments may pick another instantiation than the eager call
// before it - makes nothing but launches.  (The flags are written without synchronisation: two first calls at once both set the
// same values.)
static int index_merge_raise_lds(const char* who) {
    static bool raised[64] = {};
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e == hipSuccess && dev >= 0 && dev < 64 && raised[dev]) return TRID_OK;
    const void* fns[] = {(const void*)index_merge_kernel<false>, (const void*)index_merge_kernel<true>};
    for (const void* fn : fns)
        if (e == hipSuccess) e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, MERGE_LDS_MAX);
    if (e != hipSuccess) { set_error("%s: cannot reserve %d B of LDS: %s", who, MERGE_LDS_MAX, hipGetErrorString(e)); return (int)e; }
    if (dev >= 0 && dev < 64) raised[dev] = true;
    return TRID_OK;
}

}  // namespace trid

using namespace trid;

extern "C" int trid_index_merge_max_candidates(void) { return MERGE_CAND_MAX; }

extern "C" int trid_index_merge_lists_f32(const float* val, const int64_t* row, const int64_t* list_base, const int64_t* pid, int Q, int n_lists,
                                          int k_in, int k, float* out_val, int64_t* out_row, int64_t* out_pid, void* stream_) {
    const char* who = "trid_index_merge_lists_f32";
    TRID_REQUIRE(val && row && out_val && out_row && (out_pid || !pid), "%s: null pointer", who);
    TRID_REQUIRE(k >= 1 && k <= MERGE_K_MAX, "%s: k must be in [1,%d]; got %d", who, MERGE_K_MAX, k);
    TRID_REQUIRE(n_lists >= 1 && k_in >= 1 && (long long)n_lists * k_in <= MERGE_CAND_MAX,
                 "%s: n_lists and k_in must be >= 1 and n_lists * k_in <= %d candidates (trid_index_merge_max_candidates); got %d * %d", who,
                 MERGE_CAND_MAX, n_lists, k_in);
    const int n = n_lists * k_in;
    TRID_REQUIRE(k <= n, "%s: k must be <= n_lists * k_in = %d; got %d", who, n, k);
    TRID_REQUIRE(Q >= 1 && Q <= MERGE_Q_MAX, "%s: Q must be in [1,%lld] (one workgroup per query, 2^32 threads); got %d", who, MERGE_Q_MAX, Q);
    TRID_REQUIRE((reinterpret_cast<uintptr_t>(val) & 3u) == 0 && (reinterpret_cast<uintptr_t>(out_val) & 3u) == 0 &&
                     (reinterpret_cast<uintptr_t>(row) & 7u) == 0 && (reinterpret_cast<uintptr_t>(list_base) & 7u) == 0 &&
                     (reinterpret_cast<uintptr_t>(pid) & 7u) == 0 && (reinterpret_cast<uintptr_t>(out_row) & 7u) == 0 &&
                     (reinterpret_cast<uintptr_t>(out_pid) & 7u) == 0,
                 "%s: val / out_val must be 4-byte, row / list_base / pid / out_row / out_pid 8-byte aligned", who);
    int rc = index_merge_raise_lds(who);
    if (rc) return rc;
    const int P = merge_next_pow2(n) > MERGE_SLOTS_MIN ? merge_next_pow2(n) : MERGE_SLOTS_MIN;
    const int threads = P / 2 > MERGE_THREADS_MAX ? MERGE_THREADS_MAX : P / 2 < 64 ? 64 : P / 2;
    const size_t lds = (size_t)P * 16 + MERGE_MISC_BYTES;
    hipStream_t stream = (hipStream_t)stream_;
    if (pid != nullptr)
        hipLaunchKernelGGL(index_merge_kernel<true>, dim3((unsigned)Q), dim3(threads), lds, stream, val, (const long long*)row,
                           (const long long*)list_base, (const long long*)pid, n, k_in, k, P, out_val, (long long*)out_row, (long long*)out_pid);
    else
        hipLaunchKernelGGL(index_merge_kernel<false>, dim3((unsigned)Q), dim3(threads), lds, stream, val, (const long long*)row,
                           (const long long*)list_base, (const long long*)nullptr, n, k_in, k, P, out_val, (long long*)out_row, (long long*)nullptr);
    return check_launch(who);
}
