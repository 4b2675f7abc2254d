// The blend of GalleryIndex.expand_queries / search_expanded / augmented (include/textreid_hip.h "trid_index_blend_rows_f32"): a
// weighted gather-sum of stored unit fp32 rows, out[i] = base[i] + sum_j w(vals[i, j]) * rows[ids[i, j]], every multiply and every
// add rounded to fp32 on its own and taken in list order, so that a numpy float32 loop gives the same bits.
//
// One wave per output row, 4 rows per 256-thread workgroup.  A lane owns 4 consecutive columns: a gathered row is one 16-byte load
// per lane, 1 KB coalesced per wave.  The list entry (id, value), the part's base address and its length are the same for every
// lane of the wave: the wave number goes through readfirstlane, so they are scalar loads and the skip of an absent or out-of-extent
// entry is a uniform branch.  Nothing is read through an id before it passed the range checks.  out is written with plain 16-byte
// stores.  No LDS, no atomics, nothing that waits on another workgroup.  Memory: M * (m + 1) KB read (M * m without a base), M KB
// written.
// This file is built with -ffp-contract=off (csrc/Makefile) AND spells the two operations as __fmul_rn / __fadd_rn: no FMA.

#include "common.h"

namespace trid {

constexpr int BLEND_DIM = 256;     // the row width: 64 lanes x 4 columns
constexpr int BLEND_M_MAX = 32;    // list entries per output row
constexpr int BLEND_POWER_MAX = 4;
constexpr int BLEND_ROWS_PER_WG = 4;

template <typename IdT>
__global__ __launch_bounds__(256) void index_blend_rows_kernel(const long long* __restrict__ part_rows, const long long* __restrict__ part_len,
                                                                int n_parts, int shift, const IdT* __restrict__ ids,
                                                                const float* __restrict__ vals, long long ld_list, int M, int m, int power,
                                                                const float* __restrict__ base, long long ld_base, float* __restrict__ out) {
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int lane = threadIdx.x & 63;
    const long long i = (long long)blockIdx.x * BLEND_ROWS_PER_WG + wave;
    if (i >= M) return;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    if (base != nullptr) acc = *reinterpret_cast<const float4*>(base + i * ld_base + lane * 4);
    const IdT* idr = ids + i * ld_list;
    const float* valr = vals + i * ld_list;
    const long long low = shift == 0 ? ~0ll : (1ll << shift) - 1;
    for (int j = 0; j < m; ++j) {
        const long long id = (long long)idr[j];
        if (id < 0) continue;
        const long long part = shift == 0 ? 0 : id >> shift;
        const long long row = id & low;
        if (part >= n_parts) continue;
        if (row >= part_len[part]) continue;
        const float t = fmaxf(valr[j], 0.0f);
        float w = power == 0 ? 1.0f : t;
        for (int p = 1; p < power; ++p) w = __fmul_rn(w, t);
        const float* src = reinterpret_cast<const float*>(part_rows[part]) + row * BLEND_DIM + lane * 4;
        const float4 r = *reinterpret_cast<const float4*>(src);
        acc.x = __fadd_rn(acc.x, __fmul_rn(w, r.x));
        acc.y = __fadd_rn(acc.y, __fmul_rn(w, r.y));
        acc.z = __fadd_rn(acc.z, __fmul_rn(w, r.z));
        acc.w = __fadd_rn(acc.w, __fmul_rn(w, r.w));
    }
    *reinterpret_cast<float4*>(out + i * BLEND_DIM + lane * 4) = acc;
}

}  // namespace trid

using namespace trid;

extern "C" int trid_index_blend_rows_f32(const long long* part_rows, const long long* part_len, int n_parts, int shift, const void* ids,
                                         int id_bytes, const float* vals, long long ld_list, int M, int m, int power, const float* base,
                                         long long ld_base, float* out, void* stream_) {
    TRID_REQUIRE(part_rows && part_len && ids && vals && out, "trid_index_blend_rows_f32: null pointer (part_rows / part_len / ids / vals / out)");
    TRID_REQUIRE(m >= 1 && m <= BLEND_M_MAX, "trid_index_blend_rows_f32: m must be in [1,%d]; got %d", BLEND_M_MAX, m);
    TRID_REQUIRE(power >= 0 && power <= BLEND_POWER_MAX, "trid_index_blend_rows_f32: power must be in [0,%d]; got %d", BLEND_POWER_MAX, power);
    TRID_REQUIRE(ld_list >= m, "trid_index_blend_rows_f32: ld_list = %lld must be >= m = %d", ld_list, m);
    TRID_REQUIRE(id_bytes == 4 || id_bytes == 8, "trid_index_blend_rows_f32: id_bytes must be 4 (int32) or 8 (int64); got %d", id_bytes);
    TRID_REQUIRE(M >= 1, "trid_index_blend_rows_f32: M must be >= 1; got %d", M);
    TRID_REQUIRE(shift >= 0 && shift < 31, "trid_index_blend_rows_f32: shift must be in [0,31); got %d", shift);
    TRID_REQUIRE(n_parts >= 1 && (shift != 0 || n_parts == 1),
                 "trid_index_blend_rows_f32: n_parts must be >= 1, and 1 when shift == 0 (id = local row); got %d with shift = %d", n_parts, shift);
    TRID_REQUIRE(aligned16(out) && aligned16(base) && (base == nullptr || (ld_base >= BLEND_DIM && (ld_base & 3) == 0)),
                 "trid_index_blend_rows_f32: out and base must be 16-byte aligned, ld_base a multiple of 4 and >= %d; got ld_base = %lld", BLEND_DIM,
                 ld_base);
    TRID_REQUIRE((reinterpret_cast<uintptr_t>(ids) & (uintptr_t)(id_bytes - 1)) == 0 && (reinterpret_cast<uintptr_t>(vals) & 3u) == 0 &&
                     (reinterpret_cast<uintptr_t>(part_rows) & 7u) == 0 && (reinterpret_cast<uintptr_t>(part_len) & 7u) == 0,
                 "trid_index_blend_rows_f32: ids must be id_bytes-aligned, vals 4-byte, the two tables 8-byte aligned");
    const dim3 grid((unsigned)(((long long)M + BLEND_ROWS_PER_WG - 1) / BLEND_ROWS_PER_WG));
    hipStream_t stream = (hipStream_t)stream_;
    if (id_bytes == 4)
        hipLaunchKernelGGL(index_blend_rows_kernel<int>, grid, dim3(256), 0, stream, part_rows, part_len, n_parts, shift, (const int*)ids, vals,
                           ld_list, M, m, power, base, ld_base, out);
    else
        hipLaunchKernelGGL(index_blend_rows_kernel<long long>, grid, dim3(256), 0, stream, part_rows, part_len, n_parts, shift,
                           (const long long*)ids, vals, ld_list, M, m, power, base, ld_base, out);
    return check_launch("trid_index_blend_rows_f32");
}
