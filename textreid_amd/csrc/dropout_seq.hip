// Dropout between the layers of a stacked GRU (nn.GRU(dropout=p), gru.py:36-43: applied to the output sequence of every
// layer but the last, in training mode only): x_next = yseq * keep / (1 - p), one elementwise pass over yseq
// [B*L, 2H], 16 bytes per lane.
//
// The keep decisions come from a counter-based generator, Philox4x32-10 (Salmon et al., "Parallel random numbers: as
// easy as 1, 2, 3", SC'11): the group of four consecutive elements 4g .. 4g+3 takes the four output words of
//   philox(counter = (g.lo, g.hi, offset.lo, offset.hi), key = (seed.lo, seed.hi)),
// element 4g + k keeps iff word k >= floor(p * 2^32).  (seed, offset) is a pair of int64 in DEVICE memory that the
// kernel reads at run time: a recorded step (hipGraph or stream replay) re-executes the very same launches, and a
// one-thread launch behind the masks of a forward advances the offset - so every replay draws a fresh mask with no
// host involvement and nothing re-recorded.  The keep bytes are written out for the backward pass, which applies the
// same scale to the upper layer's dX.

#include "common.h"

namespace trid {

__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                              uint32_t out[4]) {
    constexpr uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(M0, c0), lo0 = M0 * c0;
        const uint32_t hi1 = __umulhi(M1, c2), lo1 = M1 * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += W0;
        k1 += W1;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// one thread per group of four elements (the last group may be partial); x may alias y (in place)
__global__ void dropout_seq_fwd_kernel(const float* y, float* x, uint8_t* __restrict__ keep, long long n, uint32_t threshold,
                                       float scale, const int64_t* __restrict__ state, long long draw) {
    const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (4 * g >= n) return;
    const unsigned long long seed = (unsigned long long)state[0];
    const unsigned long long off = (unsigned long long)state[1] + (unsigned long long)draw;
    uint32_t r[4];
    philox4x32_10((uint32_t)g, (uint32_t)((unsigned long long)g >> 32), (uint32_t)off, (uint32_t)(off >> 32), (uint32_t)seed,
                  (uint32_t)(seed >> 32), r);
    if (4 * g + 4 <= n) {
        const float4 v = reinterpret_cast<const float4*>(y)[g];
        const uint32_t k0 = r[0] >= threshold, k1 = r[1] >= threshold, k2 = r[2] >= threshold, k3 = r[3] >= threshold;
        reinterpret_cast<float4*>(x)[g] = make_float4(k0 ? v.x * scale : 0.f, k1 ? v.y * scale : 0.f, k2 ? v.z * scale : 0.f,
                                                      k3 ? v.w * scale : 0.f);
        reinterpret_cast<uint32_t*>(keep)[g] = k0 | (k1 << 8) | (k2 << 16) | (k3 << 24);
    } else {
        for (int k = 0; 4 * g + k < n; ++k) {
            const bool kp = r[k] >= threshold;
            x[4 * g + k] = kp ? y[4 * g + k] * scale : 0.f;
            keep[4 * g + k] = kp ? 1 : 0;
        }
    }
}

__global__ void dropout_seq_bwd_kernel(float* __restrict__ dx, const uint8_t* __restrict__ keep, long long n, float scale) {
    const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (4 * g >= n) return;
    if (4 * g + 4 <= n) {
        const float4 v = reinterpret_cast<const float4*>(dx)[g];
        const uint32_t k = reinterpret_cast<const uint32_t*>(keep)[g];
        reinterpret_cast<float4*>(dx)[g] = make_float4((k & 0xffu) ? v.x * scale : 0.f, (k & 0xff00u) ? v.y * scale : 0.f,
                                                       (k & 0xff0000u) ? v.z * scale : 0.f, (k & 0xff000000u) ? v.w * scale : 0.f);
    } else {
        for (int e = 0; 4 * g + e < n; ++e) dx[4 * g + e] = keep[4 * g + e] ? dx[4 * g + e] * scale : 0.f;
    }
}

__global__ void dropout_advance_kernel(int64_t* __restrict__ state, long long draws) {
    if (blockIdx.x == 0 && threadIdx.x == 0) state[1] += draws;
}

static bool dropout_p_ok(float p) { return p > 0.f && p < 1.f; }

}  // namespace trid

using namespace trid;

extern "C" int trid_dropout_seq_fwd_f32(const float* y, float* x, uint8_t* keep, long long n, float p, const int64_t* state,
                                        long long draw, void* stream) {
    TRID_REQUIRE(y && x && keep && state && n > 0 && draw >= 0, "trid_dropout_seq_fwd_f32: bad arguments");
    TRID_REQUIRE(dropout_p_ok(p), "trid_dropout_seq_fwd_f32: 0 < p < 1 (got %g)", (double)p);
    TRID_REQUIRE(aligned16(y) && aligned16(x) && (reinterpret_cast<uintptr_t>(keep) & 3u) == 0 && (reinterpret_cast<uintptr_t>(state) & 7u) == 0,
                 "trid_dropout_seq_fwd_f32: y / x must be 16-byte, keep 4-byte, state 8-byte aligned");
    const uint32_t threshold = (uint32_t)((double)p * 4294967296.0);
    const long long groups = (n + 3) / 4;
    hipLaunchKernelGGL(dropout_seq_fwd_kernel, dim3((unsigned)((groups + 255) / 256)), dim3(256), 0, (hipStream_t)stream, y, x, keep, n,
                       threshold, 1.f / (1.f - p), state, draw);
    return check_launch("trid_dropout_seq_fwd_f32");
}

extern "C" int trid_dropout_seq_bwd_f32(float* dx, const uint8_t* keep, long long n, float p, void* stream) {
    TRID_REQUIRE(dx && keep && n > 0, "trid_dropout_seq_bwd_f32: bad arguments");
    TRID_REQUIRE(dropout_p_ok(p), "trid_dropout_seq_bwd_f32: 0 < p < 1 (got %g)", (double)p);
    TRID_REQUIRE(aligned16(dx) && (reinterpret_cast<uintptr_t>(keep) & 3u) == 0, "trid_dropout_seq_bwd_f32: dx must be 16-byte, keep 4-byte aligned");
    const long long groups = (n + 3) / 4;
    hipLaunchKernelGGL(dropout_seq_bwd_kernel, dim3((unsigned)((groups + 255) / 256)), dim3(256), 0, (hipStream_t)stream, dx, keep, n,
                       1.f / (1.f - p));
    return check_launch("trid_dropout_seq_bwd_f32");
}

extern "C" int trid_dropout_advance(int64_t* state, long long draws, void* stream) {
    TRID_REQUIRE(state && draws > 0 && (reinterpret_cast<uintptr_t>(state) & 7u) == 0, "trid_dropout_advance: bad arguments");
    hipLaunchKernelGGL(dropout_advance_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, state, draws);
    return check_launch("trid_dropout_advance");
}
