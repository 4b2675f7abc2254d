// The pieces of the ImageNet ResNet-50/101 image encoder (reference lib/models/backbones/resnet.py:101-167) that CLIP's
// ModifiedResNet has no use for: the 7x7 stride-2 stem convolution and its weight gradient, BatchNorm + ReLU + 3x3 stride-2
// max pool and the pool's backward, the even-pixel subsample behind the stride-2 1x1 downsample convolutions and the
// global average pool.  (The stride-2 3x3 convolutions are loader modes of trid_gemm_f32: gemm.hip / gemm_bf16.hip, CS.)
// Nothing here synchronises the host or accumulates a result with atomics: sums run in a fixed order, so a step is
// bitwise repeatable (the amax side outputs fold a maximum, which has no order).

#include "gemm_common.h"

namespace trid {

// ---------------------------------------------------------------------------------------------------- helpers
__device__ __forceinline__ float4 rn_affine4(float4 v, float4 s, float4 t) {  // the arithmetic of bn_pool.hip's affine4
    return make_float4(fmaf(v.x, s.x, t.x), fmaf(v.y, s.y, t.y), fmaf(v.z, s.z, t.z), fmaf(v.w, s.w, t.w));
}
__device__ __forceinline__ float4 rn_relu4(float4 v) { return make_float4(fmaxf(v.x, 0.f), fmaxf(v.y, 0.f), fmaxf(v.z, 0.f), fmaxf(v.w, 0.f)); }
__device__ __forceinline__ unsigned rn_amax4(unsigned m, float4 v) {
    const unsigned a = __builtin_bit_cast(unsigned, v.x) & 0x7fffffffu, b = __builtin_bit_cast(unsigned, v.y) & 0x7fffffffu;
    const unsigned c = __builtin_bit_cast(unsigned, v.z) & 0x7fffffffu, d = __builtin_bit_cast(unsigned, v.w) & 0x7fffffffu;
    const unsigned ab = a > b ? a : b, cd = c > d ? c : d;
    const unsigned q = ab > cd ? ab : cd;
    return q > m ? q : m;
}
// max|out| into a device scalar that starts at 0 (the precision-16 operand scale of the consumer): wave fold, block fold, one
// integer atomicMax on the bit pattern per block
__device__ __forceinline__ void rn_amax_commit(unsigned m, float* amax) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned t = __shfl_xor(m, o, 64);
        m = t > m ? t : m;
    }
    __shared__ unsigned amax_red[8];
    const int w = threadIdx.x >> 6, nw = blockDim.x >> 6;
    if ((threadIdx.x & 63) == 0) amax_red[w] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned r = 0;
        for (int i = 0; i < nw; ++i) r = amax_red[i] > r ? amax_red[i] : r;
        if (r != 0) atomicMax(reinterpret_cast<unsigned*>(amax), r);
    }
}

// ---------------------------------------------------------------------------------------------------- 7x7 stem convolution
// y[b, yo, xo, n] = sum_{c, ky, kx} img[b, c, 2 yo - 3 + ky, 2 xo - 3 + kx] * w[n, c, ky, kx]   (7x7, stride 2, pad 3)
// on v_mfma_f32_32x32x2_f32 (exact fp32), the pattern of stem_conv.hip's conv1: a wave = 32 consecutive output pixels x all
// 64 output channels (two accumulators), K = 147 (+1 zero) in 74 steps; A[pixel][k] gathered straight from the NCHW image
// (taps outside the image, k = 147 and pixels beyond M read as zero through the buffer descriptor), B[k][n] = the filter as
// stored ([64][3][7][7]), transposed once per workgroup into LDS.  A workgroup = 4 waves = one 128-row BatchNorm slab:
// per-channel (mean, M2), Chan-merged over its four 32-row wave partials in wave order.
constexpr int S7_K = 147;
constexpr int S7_STEPS = 74;

struct Stem7Params {
    const float* img;   // [B][3][Hi][Wi]
    const float* w;     // [64][147]
    float* y;           // [B][Ho][Wo][64]
    float* stats;       // [ceil(M / 128)][64][2] or null
    int B, Hi, Wi, Ho, Wo;
    long long M;        // B * Ho * Wo
    int nslabs;
    FastDiv fdWo, fdHo;
};

__global__ __launch_bounds__(256) void stem7_conv_kernel(Stem7Params p) {
    __shared__ float wl[2 * S7_STEPS * 64];  // [k][n]
    __shared__ float2 sstat[2][4][64];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int kh = lane >> 5, n = lane & 31;
    for (int e = tid; e < 2 * S7_STEPS * 64; e += 256) {
        const int nn = e / (2 * S7_STEPS), j = e - nn * (2 * S7_STEPS);
        wl[j * 64 + nn] = j < S7_K ? p.w[nn * S7_K + j] : 0.f;
    }
    __syncthreads();
    const size_t img_bytes = (size_t)p.B * 3 * p.Hi * p.Wi * 4;
    const __amdgpu_buffer_rsrc_t rsI = __builtin_amdgcn_make_buffer_rsrc((void*)p.img, 0, (unsigned)img_bytes, 0x00020000);
    constexpr unsigned OOB = 0x80000000u;
    int it = 0;
    for (int slab = blockIdx.x; slab < p.nslabs; slab += gridDim.x, ++it) {
        const long long m = (long long)slab * 128 + wave * 32 + (lane & 31);
        const bool live = m < p.M;
        const uint32_t mm = live ? (uint32_t)m : 0u;
        const uint32_t q = fdiv(mm, p.fdWo);
        const int xo = (int)(mm - q * p.Wo);
        const uint32_t b = fdiv(q, p.fdHo);
        const int yo = (int)(q - b * p.Ho);
        const unsigned img0 = (unsigned)b * 3u * (unsigned)(p.Hi * p.Wi);
        float a[S7_STEPS];
#pragma unroll
        for (int kk = 0; kk < S7_STEPS; ++kk) {
            const int j0 = 2 * kk, j1 = 2 * kk + 1;  // this lane's k index is j0 (lower half-wave) or j1 (upper)
            const int c = kh ? j1 / 49 : j0 / 49;
            const int ky = kh ? (j1 % 49) / 7 : (j0 % 49) / 7, kx = kh ? (j1 % 49) % 7 : (j0 % 49) % 7;
            const int yy = 2 * yo - 3 + ky, xx = 2 * xo - 3 + kx;
            const bool ok = live & ((2 * kk + kh) < S7_K) & (yy >= 0) & (yy < p.Hi) & (xx >= 0) & (xx < p.Wi);
            const unsigned off = (img0 + (unsigned)((c * p.Hi + yy) * p.Wi + xx)) * 4u;
            a[kk] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsI, ok ? off : OOB, 0, 0));
        }
        v16f acc0, acc1;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc0[r] = acc1[r] = 0.f;
#pragma unroll
        for (int kk = 0; kk < S7_STEPS; ++kk) {
            const float b0 = wl[(2 * kk + kh) * 64 + n], b1 = wl[(2 * kk + kh) * 64 + 32 + n];
            acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[kk], b0, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[kk], b1, acc1, 0, 0, 0);
        }
        const long long row0 = (long long)slab * 128 + wave * 32;
        const int cnt_w = (int)(p.M - row0 < 32 ? (p.M - row0 > 0 ? p.M - row0 : 0) : 32);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = (r & 3) + 8 * (r >> 2) + 4 * kh;
            if (row < cnt_w) {
                float* dst = p.y + (row0 + row) * 64 + n;
                dst[0] = acc0[r];
                dst[32] = acc1[r];
            }
        }
        if (p.stats != nullptr) {
#pragma unroll
            for (int jb = 0; jb < 2; ++jb) {
                const v16f& acc = jb ? acc1 : acc0;
                float sum = 0.f;
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    if ((r & 3) + 8 * (r >> 2) + 4 * kh < cnt_w) sum += acc[r];
                sum += __shfl_xor(sum, 32, 64);
                const float mean = cnt_w > 0 ? sum / (float)cnt_w : 0.f;
                float m2 = 0.f;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float d = acc[r] - mean;
                    if ((r & 3) + 8 * (r >> 2) + 4 * kh < cnt_w) m2 += d * d;
                }
                m2 += __shfl_xor(m2, 32, 64);
                if (kh == 0) sstat[it & 1][wave][jb * 32 + n] = make_float2(mean, m2);
            }
            __syncthreads();  // (double-buffered: the next slab's partials go to the other half)
            if (tid < 64) {
                float cnt = 0.f, mean = 0.f, m2 = 0.f;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const long long r0 = (long long)slab * 128 + k * 32;
                    const float nb = (float)(p.M - r0 < 32 ? (p.M - r0 > 0 ? p.M - r0 : 0) : 32);
                    if (nb > 0.f) {
                        const float2 v = sstat[it & 1][k][tid];
                        const float nt = cnt + nb, d = v.x - mean;
                        mean += d * (nb / nt);
                        m2 += v.y + d * d * (cnt * nb / nt);
                        cnt = nt;
                    }
                }
                reinterpret_cast<float2*>(p.stats)[(long long)slab * 64 + tid] = make_float2(mean, m2);
            }
        }
    }
}

// The stem's weight gradient, dW[n][j] = sum over output pixels m of dy[m][n] * patch[m][j] (j = c * 49 + ky * 7 + kx), again
// straight from the NCHW image (stem_conv.hip's conv1 weight gradient with a 64 x 147 output): the OUTPUT of the MFMAs is the
// gradient itself - 2 x 5 tiles of 32 x 32 (160 columns, 147 used) in the accumulators for the whole launch - and the reduction
// runs over pixels, two per MFMA.  Every wave owns a contiguous run of pixels; the four waves of a workgroup fold into LDS one
// after the other, the workgroups' [64][147] slabs are folded by trid_slab_reduce_f32: a fixed assignment and order.
struct Stem7WgradParams {
    const float* img;   // [B][3][Hi][Wi]
    const float* dy;    // [B][Ho][Wo][64]
    float* slabs;       // [gridDim.x][64 * 147]
    int B, Hi, Wi, Ho, Wo;
    long long M;
    int per_wave;       // pixels per wave (a multiple of 2 * S7W_U)
    FastDiv fdWo, fdHo;
};

constexpr int S7W_SLABS = 256;
constexpr int S7W_U = 4;
constexpr int S7W_PITCH = 161;

__global__ __launch_bounds__(256) void stem7_conv_wgrad_kernel(Stem7WgradParams p) {
    __shared__ float red[64 * S7W_PITCH];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int kh = lane >> 5, j = lane & 31;
    int t_ky[5], t_kx[5], t_off[5];
    bool t_live[5];
#pragma unroll
    for (int jb = 0; jb < 5; ++jb) {
        const int jj = j + 32 * jb;
        const int c = jj / 49;
        t_ky[jb] = (jj % 49) / 7;
        t_kx[jb] = jj % 7;
        t_live[jb] = jj < S7_K;
        t_off[jb] = (c * p.Hi + t_ky[jb] - 3) * p.Wi + (t_kx[jb] - 3);  // relative to pixel (2 yo, 2 xo) of plane 0
    }
    const __amdgpu_buffer_rsrc_t rsI = __builtin_amdgcn_make_buffer_rsrc((void*)p.img, 0, (unsigned)((size_t)p.B * 3 * p.Hi * p.Wi * 4), 0x00020000);
    const __amdgpu_buffer_rsrc_t rsD = __builtin_amdgcn_make_buffer_rsrc((void*)p.dy, 0, (unsigned)(p.M * 256), 0x00020000);
    constexpr unsigned OOB = 0x80000000u;
    const long long first = ((long long)blockIdx.x * 4 + wave) * p.per_wave;
    long long last = first + p.per_wave;
    last = last < p.M ? last : p.M;
    v16f acc[2][5];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int jb = 0; jb < 5; ++jb)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][jb][r] = 0.f;
    for (long long t = first; t < last; t += 2 * S7W_U) {
        float a[S7W_U][2], b[S7W_U][5];
#pragma unroll
        for (int u = 0; u < S7W_U; ++u) {
            const long long m = t + 2 * u + kh;
            const bool live = m < last;
            const uint32_t mm = live ? (uint32_t)m : 0u;
            a[u][0] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsD, live ? mm * 256u + (unsigned)j * 4u : OOB, 0, 0));
            a[u][1] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsD, live ? mm * 256u + 128u + (unsigned)j * 4u : OOB, 0, 0));
            const uint32_t q = fdiv(mm, p.fdWo);
            const int xo = (int)(mm - q * p.Wo);
            const uint32_t bi = fdiv(q, p.fdHo);
            const int yo = (int)(q - bi * p.Ho);
            const unsigned base = bi * 3u * (unsigned)(p.Hi * p.Wi) + (unsigned)(2 * yo * p.Wi + 2 * xo);
#pragma unroll
            for (int jb = 0; jb < 5; ++jb) {
                const int yy = 2 * yo - 3 + t_ky[jb], xx = 2 * xo - 3 + t_kx[jb];
                const bool ok = live & t_live[jb] & (yy >= 0) & (yy < p.Hi) & (xx >= 0) & (xx < p.Wi);
                const unsigned off = (base + (unsigned)t_off[jb]) * 4u;
                b[u][jb] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsI, ok ? off : OOB, 0, 0));
            }
        }
#pragma unroll
        for (int u = 0; u < S7W_U; ++u)
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int jb = 0; jb < 5; ++jb) acc[i][jb] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u][i], b[u][jb], acc[i][jb], 0, 0, 0);
    }
    // the four waves fold into LDS in wave order
    for (int w = 0; w < 4; ++w) {
        if (wave == w) {
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int jb = 0; jb < 5; ++jb)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        float* dst = red + (32 * i + (r & 3) + 8 * (r >> 2) + 4 * kh) * S7W_PITCH + 32 * jb + j;
                        *dst = (w == 0) ? acc[i][jb][r] : *dst + acc[i][jb][r];
                    }
        }
        __syncthreads();
    }
    float* out = p.slabs + (size_t)blockIdx.x * (64 * S7_K);
    for (int e = tid; e < 64 * S7_K; e += 256) {
        const int nn = e / S7_K, jj = e - nn * S7_K;
        out[e] = red[nn * S7W_PITCH + jj];
    }
}

// ---------------------------------------------------------------------------------------------------- BatchNorm + ReLU + max pool
// out[b][hp][wp][c] = max over the 3x3 / stride 2 / pad 1 window of relu(scale_c * y + shift_c)   (resnet.py:115-117).  The window
// always holds its centre (2 hp, 2 wp) and ReLU outputs are >= 0, so starting the maximum at 0 never lets the padding win.
__global__ __launch_bounds__(256) void bn_relu_maxpool_kernel(const float4* __restrict__ y, const float4* __restrict__ scale, const float4* __restrict__ shift,
                                                              float4* __restrict__ out, int H, int W, int CQ, int Hp, int Wp, long long total4,
                                                              float* __restrict__ amax) {
    unsigned am = 0;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total4; i += (long long)gridDim.x * 256) {
        const int cq = (int)(i % CQ);
        long long t = i / CQ;
        const int wp = (int)(t % Wp);
        t /= Wp;
        const int hp = (int)(t % Hp);
        const long long b = t / Hp;
        const float4 s = scale[cq], sh = shift[cq];
        float4 best = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
            const int h = 2 * hp - 1 + ky;
            if (h < 0 || h >= H) continue;
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const int w = 2 * wp - 1 + kx;
                if (w < 0 || w >= W) continue;
                const float4 v = rn_relu4(rn_affine4(y[((b * H + h) * W + w) * CQ + cq], s, sh));
                best = make_float4(fmaxf(best.x, v.x), fmaxf(best.y, v.y), fmaxf(best.z, v.z), fmaxf(best.w, v.w));
            }
        }
        out[i] = best;
        am = rn_amax4(am, best);
    }
    if (amax != nullptr) rn_amax_commit(am, amax);
}

// The pool's backward as a gather: input position (h, w) lies in at most four windows; each window's winner is recomputed from
// y, scale and shift (PyTorch's rule: the FIRST maximum in row-major window order) and the gradients of the windows this
// position wins are summed in window order.  No atomics, no index tensor.  dx is the gradient with respect to the ReLU OUTPUT:
// where a window is all <= 0 its gradient lands on the window's first position and trid_bn_bwd's ReLU mask removes it.
__device__ __forceinline__ void rn_take(float v, int idx, float& best, int& bidx) {
    if (v > best) {
        best = v;
        bidx = idx;
    }
}

__global__ __launch_bounds__(256) void bn_relu_maxpool_bwd_kernel(const float4* __restrict__ g, const float4* __restrict__ y, const float4* __restrict__ scale,
                                                                  const float4* __restrict__ shift, float4* __restrict__ dx, int H, int W, int CQ,
                                                                  int Hp, int Wp, long long total4) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total4; i += (long long)gridDim.x * 256) {
        const int cq = (int)(i % CQ);
        long long t = i / CQ;
        const int w = (int)(t % W);
        t /= W;
        const int h = (int)(t % H);
        const long long b = t / H;
        const float4 s = scale[cq], sh = shift[cq];
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        // even rows / columns lie in one window (hp = h / 2), odd ones in two (h / 2 and h / 2 + 1)
        const int hp1 = (h + 1) / 2 < Hp ? (h + 1) / 2 : Hp - 1, wp1 = (w + 1) / 2 < Wp ? (w + 1) / 2 : Wp - 1;
        for (int hp = h / 2; hp <= hp1; ++hp)
            for (int wp = w / 2; wp <= wp1; ++wp) {
                float4 best = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
                int bx = -1, by = -1, bz = -1, bw = -1;
#pragma unroll
                for (int ky = 0; ky < 3; ++ky) {
                    const int hh = 2 * hp - 1 + ky;
                    if (hh < 0 || hh >= H) continue;
#pragma unroll
                    for (int kx = 0; kx < 3; ++kx) {
                        const int ww = 2 * wp - 1 + kx;
                        if (ww < 0 || ww >= W) continue;
                        const float4 v = rn_relu4(rn_affine4(y[((b * H + hh) * W + ww) * CQ + cq], s, sh));
                        const int idx = ky * 3 + kx;
                        rn_take(v.x, idx, best.x, bx);
                        rn_take(v.y, idx, best.y, by);
                        rn_take(v.z, idx, best.z, bz);
                        rn_take(v.w, idx, best.w, bw);
                    }
                }
                const int mine = (h - (2 * hp - 1)) * 3 + (w - (2 * wp - 1));
                const float4 gv = g[((b * Hp + hp) * Wp + wp) * CQ + cq];
                acc.x += bx == mine ? gv.x : 0.f;
                acc.y += by == mine ? gv.y : 0.f;
                acc.z += bz == mine ? gv.z : 0.f;
                acc.w += bw == mine ? gv.w : 0.f;
            }
        dx[i] = acc;
    }
}

// ---------------------------------------------------------------------------------------------------- stride-2 subsample
// The input of a stride-2 1x1 convolution (the downsample branch, resnet.py:137-143): out[b][ho][wo] = x[b][2 ho][2 wo].
__global__ __launch_bounds__(256) void subsample2_kernel(const float4* __restrict__ x, float4* __restrict__ out, int H, int W, int CQ, int Ho, int Wo,
                                                         long long total4, float* __restrict__ amax) {
    unsigned am = 0;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total4; i += (long long)gridDim.x * 256) {
        const int cq = (int)(i % CQ);
        long long t = i / CQ;
        const int wo = (int)(t % Wo);
        t /= Wo;
        const int ho = (int)(t % Ho);
        const long long b = t / Ho;
        const float4 v = x[((b * H + 2 * ho) * W + 2 * wo) * CQ + cq];
        out[i] = v;
        am = rn_amax4(am, v);
    }
    if (amax != nullptr) rn_amax_commit(am, amax);
}

__global__ __launch_bounds__(256) void subsample2_bwd_kernel(const float4* __restrict__ g, float4* __restrict__ dx, int H, int W, int CQ, int Ho, int Wo,
                                                             long long total4) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total4; i += (long long)gridDim.x * 256) {
        const int cq = (int)(i % CQ);
        long long t = i / CQ;
        const int w = (int)(t % W);
        t /= W;
        const int h = (int)(t % H);
        const long long b = t / H;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (((h | w) & 1) == 0) v = g[((b * Ho + h / 2) * Wo + w / 2) * CQ + cq];
        dx[i] = v;
    }
}

// ---------------------------------------------------------------------------------------------------- global average pool
// out[b][c] = (sum over the HW pixels, in pixel order) / HW   (nn.AdaptiveAvgPool2d((1, 1)), resnet.py:130,165)
__global__ __launch_bounds__(256) void global_avgpool_kernel(const float4* __restrict__ x, float4* __restrict__ out, int HW, int CQ, long long total4) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total4; i += (long long)gridDim.x * 256) {
        const int cq = (int)(i % CQ);
        const long long b = i / CQ;
        const float4* src = x + b * HW * CQ + cq;
        float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int px = 0; px < HW; ++px) {
            const float4 v = src[(long long)px * CQ];
            s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
        }
        const float n = (float)HW;
        out[i] = make_float4(s.x / n, s.y / n, s.z / n, s.w / n);
    }
}

__global__ __launch_bounds__(256) void global_avgpool_bwd_kernel(const float4* __restrict__ g, float4* __restrict__ dx, int HW, int CQ, long long total4) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total4; i += (long long)gridDim.x * 256) {
        const int cq = (int)(i % CQ);
        const long long b = i / ((long long)HW * CQ);
        const float4 v = g[b * CQ + cq];
        const float n = (float)HW;
        dx[i] = make_float4(v.x / n, v.y / n, v.z / n, v.w / n);
    }
}

}  // namespace trid

using namespace trid;

static int stem7_geometry(int B, int Hi, int Wi, int* Ho, int* Wo, long long* M, const char* who) {
    TRID_REQUIRE(B > 0 && Hi > 0 && Wi > 0, "%s: bad arguments", who);
    TRID_REQUIRE((long long)B * 3 * Hi * Wi * 4 < (1ll << 31), "%s: the image batch must stay below 2 GB", who);
    *Ho = (Hi - 1) / 2 + 1;
    *Wo = (Wi - 1) / 2 + 1;
    *M = (long long)B * *Ho * *Wo;
    TRID_REQUIRE(*M * 256 < (1ll << 31), "%s: the output must stay below 2 GB (31-bit offsets)", who);
    return TRID_OK;
}

extern "C" int trid_stem7_conv_f32(const float* img, const float* w, float* y, float* stats, int B, int Hi, int Wi, void* stream) {
    TRID_REQUIRE(img && w && y, "trid_stem7_conv_f32: null pointer");
    Stem7Params p;
    memset(&p, 0, sizeof(p));
    int rc = stem7_geometry(B, Hi, Wi, &p.Ho, &p.Wo, &p.M, "trid_stem7_conv_f32");
    if (rc) return rc;
    p.img = img; p.w = w; p.y = y; p.stats = stats;
    p.B = B; p.Hi = Hi; p.Wi = Wi;
    p.nslabs = (int)((p.M + 127) / 128);
    p.fdWo = make_fastdiv((uint32_t)p.Wo);
    p.fdHo = make_fastdiv((uint32_t)p.Ho);
    const int grid = p.nslabs < 256 * 8 ? p.nslabs : 256 * 8;
    hipLaunchKernelGGL(stem7_conv_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, p);
    return check_launch("trid_stem7_conv_f32");
}

extern "C" int trid_stem7_conv_wgrad_slabs(void) { return S7W_SLABS; }

extern "C" int trid_stem7_conv_wgrad_f32(const float* img, const float* dy, float* dw, float* slabs, int B, int Hi, int Wi, void* stream) {
    TRID_REQUIRE(img && dy && dw && slabs, "trid_stem7_conv_wgrad_f32: null pointer");
    TRID_REQUIRE(aligned16(dw) && aligned16(slabs), "trid_stem7_conv_wgrad_f32: dw / slabs must be 16-byte aligned");
    Stem7WgradParams p;
    memset(&p, 0, sizeof(p));
    int rc = stem7_geometry(B, Hi, Wi, &p.Ho, &p.Wo, &p.M, "trid_stem7_conv_wgrad_f32");
    if (rc) return rc;
    p.img = img; p.dy = dy; p.slabs = slabs;
    p.B = B; p.Hi = Hi; p.Wi = Wi;
    const long long waves = (long long)S7W_SLABS * 4;
    p.per_wave = (int)(((p.M + waves - 1) / waves + 2 * S7W_U - 1) / (2 * S7W_U) * (2 * S7W_U));
    p.fdWo = make_fastdiv((uint32_t)p.Wo);
    p.fdHo = make_fastdiv((uint32_t)p.Ho);
    hipLaunchKernelGGL(stem7_conv_wgrad_kernel, dim3(S7W_SLABS), dim3(256), 0, (hipStream_t)stream, p);
    rc = check_launch("trid_stem7_conv_wgrad_f32");
    if (rc) return rc;
    return trid_slab_reduce_f32(slabs, dw, 64 * S7_K, S7W_SLABS, 64 * S7_K, 0, stream);
}

extern "C" int trid_bn_relu_maxpool_f32(const float* y, const float* scale, const float* shift, float* out, int B, int H, int W, int C,
                                        float* amax, void* stream) {
    TRID_REQUIRE(y && scale && shift && out && B > 0 && H > 0 && W > 0 && C > 0 && C % 4 == 0, "trid_bn_relu_maxpool_f32: bad arguments");
    TRID_REQUIRE(aligned16(y) && aligned16(scale) && aligned16(shift) && aligned16(out), "trid_bn_relu_maxpool_f32: operands must be 16-byte aligned");
    const int Hp = (H - 1) / 2 + 1, Wp = (W - 1) / 2 + 1;
    const long long total4 = (long long)B * Hp * Wp * (C / 4);
    hipLaunchKernelGGL(bn_relu_maxpool_kernel, dim3(grid_for(total4, 256, 8192)), dim3(256), 0, (hipStream_t)stream, (const float4*)y, (const float4*)scale,
                       (const float4*)shift, (float4*)out, H, W, C / 4, Hp, Wp, total4, amax);
    return check_launch("trid_bn_relu_maxpool_f32");
}

extern "C" int trid_bn_relu_maxpool_bwd_f32(const float* g, const float* y, const float* scale, const float* shift, float* dx, int B, int H, int W,
                                            int C, void* stream) {
    TRID_REQUIRE(g && y && scale && shift && dx && B > 0 && H > 0 && W > 0 && C > 0 && C % 4 == 0, "trid_bn_relu_maxpool_bwd_f32: bad arguments");
    TRID_REQUIRE(aligned16(g) && aligned16(y) && aligned16(scale) && aligned16(shift) && aligned16(dx), "trid_bn_relu_maxpool_bwd_f32: operands must be 16-byte aligned");
    const int Hp = (H - 1) / 2 + 1, Wp = (W - 1) / 2 + 1;
    const long long total4 = (long long)B * H * W * (C / 4);
    hipLaunchKernelGGL(bn_relu_maxpool_bwd_kernel, dim3(grid_for(total4, 256, 16384)), dim3(256), 0, (hipStream_t)stream, (const float4*)g, (const float4*)y,
                       (const float4*)scale, (const float4*)shift, (float4*)dx, H, W, C / 4, Hp, Wp, total4);
    return check_launch("trid_bn_relu_maxpool_bwd_f32");
}

extern "C" int trid_subsample2_f32(const float* x, float* out, int B, int H, int W, int C, float* amax, void* stream) {
    TRID_REQUIRE(x && out && B > 0 && H > 0 && W > 0 && C > 0 && C % 4 == 0 && aligned16(x) && aligned16(out), "trid_subsample2_f32: bad arguments");
    const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
    const long long total4 = (long long)B * Ho * Wo * (C / 4);
    hipLaunchKernelGGL(subsample2_kernel, dim3(grid_for(total4, 256, 8192)), dim3(256), 0, (hipStream_t)stream, (const float4*)x, (float4*)out, H, W, C / 4,
                       Ho, Wo, total4, amax);
    return check_launch("trid_subsample2_f32");
}

extern "C" int trid_subsample2_bwd_f32(const float* g, float* dx, int B, int H, int W, int C, void* stream) {
    TRID_REQUIRE(g && dx && B > 0 && H > 0 && W > 0 && C > 0 && C % 4 == 0 && aligned16(g) && aligned16(dx), "trid_subsample2_bwd_f32: bad arguments");
    const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
    const long long total4 = (long long)B * H * W * (C / 4);
    hipLaunchKernelGGL(subsample2_bwd_kernel, dim3(grid_for(total4, 256, 8192)), dim3(256), 0, (hipStream_t)stream, (const float4*)g, (float4*)dx, H, W, C / 4,
                       Ho, Wo, total4);
    return check_launch("trid_subsample2_bwd_f32");
}

extern "C" int trid_global_avgpool_f32(const float* x, float* out, int B, int HW, int C, void* stream) {
    TRID_REQUIRE(x && out && B > 0 && HW > 0 && C > 0 && C % 4 == 0 && aligned16(x) && aligned16(out), "trid_global_avgpool_f32: bad arguments");
    const long long total4 = (long long)B * (C / 4);
    hipLaunchKernelGGL(global_avgpool_kernel, dim3(grid_for(total4, 256, 8192)), dim3(256), 0, (hipStream_t)stream, (const float4*)x, (float4*)out, HW, C / 4,
                       total4);
    return check_launch("trid_global_avgpool_f32");
}

extern "C" int trid_global_avgpool_bwd_f32(const float* g, float* dx, int B, int HW, int C, void* stream) {
    TRID_REQUIRE(g && dx && B > 0 && HW > 0 && C > 0 && C % 4 == 0 && aligned16(g) && aligned16(dx), "trid_global_avgpool_bwd_f32: bad arguments");
    const long long total4 = (long long)B * HW * (C / 4);
    hipLaunchKernelGGL(global_avgpool_bwd_kernel, dim3(grid_for(total4, 256, 8192)), dim3(256), 0, (hipStream_t)stream, (const float4*)g, (float4*)dx, HW,
                       C / 4, total4);
    return check_launch("trid_global_avgpool_bwd_f32");
}
