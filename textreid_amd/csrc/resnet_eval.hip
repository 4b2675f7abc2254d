// Eval-mode (model.eval(), running-statistics BatchNorm) pieces of the ImageNet ResNet-50/101 image encoder on pre-split (P16)
// activations - what the CLIP encoder's eval flow (gemm_p16.hip c_fmt 1, gemm_stream.hip, stem_conv.hip) has no counterpart for:
// the 7x7 stride-2 stem with the fused BatchNorm + ReLU + P16 epilogue, the 3x3 stride-2 max pool of a P16 tensor, the even-pixel
// subsample in front of the stride-2 1x1 downsample convolutions and the global average pool that unpacks the last P16 tensor.
// (The stride-2 3x3 convolution is the A_CONV_S2 loader of gemm_p16.hip.)  Reference: lib/models/backbones/resnet.py:154-167.
// Nothing here accumulates a result with atomics (the tmax side outputs fold a maximum, which has no order).

#include "split_common.h"

namespace trid {

// ---------------------------------------------------------------------------------------------------- 7x7 stem, eval epilogue
// The gather and the MFMA loop of resnet_ops.hip's stem7_conv_kernel (exact fp32, K = 147 (+1) straight from the NCHW batch, a wave =
// 32 output pixels x 64 channels in two accumulators); the epilogue is stem_conv.hip's conv1 eval epilogue: v = act(acc * scale_n +
// shift_n) split into its two fp16 planes in the lane that holds channel n, neighbouring lanes exchange one plane each and every
// lane stores ONE dword per pixel and 32-channel group - even lanes the high parts of channels (n, n + 1), odd lanes the low parts
// of (n - 1, n).  The output's scale comes from the bound of gemm_common.h EvalBound, its true maximum goes to *ev.out_tmax.
constexpr int S7E_K = 147;
constexpr int S7E_STEPS = 74;

struct Stem7EvalParams {
    const float* img;   // [B][3][Hi][Wi]
    const float* w;     // [64][147]
    char* out16;        // P16 [B][Ho][Wo][64]
    const float* bn_scale;
    const float* bn_shift;
    int relu;
    EvalBound ev;
    int B, Hi, Wi, Ho, Wo;
    long long M;        // B * Ho * Wo
    int nslabs;
    FastDiv fdWo, fdHo;
};

__global__ __launch_bounds__(256) void stem7_eval_p16_kernel(Stem7EvalParams p) {
    __shared__ float wl[2 * S7E_STEPS * 64];  // [k][n]
    __shared__ unsigned redu[4];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int kh = lane >> 5, n = lane & 31;
    for (int e = tid; e < 2 * S7E_STEPS * 64; e += 256) {
        const int nn = e / (2 * S7E_STEPS), j = e - nn * (2 * S7E_STEPS);
        wl[j * 64 + nn] = j < S7E_K ? p.w[nn * S7E_K + j] : 0.f;
    }
    const float sc[2] = {p.bn_scale[n], p.bn_scale[32 + n]}, sh[2] = {p.bn_shift[n], p.bn_shift[32 + n]};
    const float bound = eval_out_bound(p.ev);
    if (p.ev.out_bound != nullptr && blockIdx.x == 0 && tid == 0) *p.ev.out_bound = bound;
    const float oscale = f16_scale_of(bound);
    unsigned tmax = 0;
    __syncthreads();
    const size_t img_bytes = (size_t)p.B * 3 * p.Hi * p.Wi * 4;
    const __amdgpu_buffer_rsrc_t rsI = __builtin_amdgcn_make_buffer_rsrc((void*)p.img, 0, (unsigned)img_bytes, 0x00020000);
    constexpr unsigned OOB = 0x80000000u;
    const bool even = (n & 1) == 0;
    const int lane_off = even ? 2 * n : 64 + 2 * (n - 1);  // byte offset of this lane's dword inside a 128-byte group
    for (int slab = blockIdx.x; slab < p.nslabs; slab += gridDim.x) {
        const long long m = (long long)slab * 128 + wave * 32 + (lane & 31);
        const bool live = m < p.M;
        const uint32_t mm = live ? (uint32_t)m : 0u;
        const uint32_t q = fdiv(mm, p.fdWo);
        const int xo = (int)(mm - q * p.Wo);
        const uint32_t b = fdiv(q, p.fdHo);
        const int yo = (int)(q - b * p.Ho);
        const unsigned img0 = (unsigned)b * 3u * (unsigned)(p.Hi * p.Wi);
        float a[S7E_STEPS];
#pragma unroll
        for (int kk = 0; kk < S7E_STEPS; ++kk) {
            const int j0 = 2 * kk, j1 = 2 * kk + 1;  // this lane's k index is j0 (lower half-wave) or j1 (upper)
            const int c = kh ? j1 / 49 : j0 / 49;
            const int ky = kh ? (j1 % 49) / 7 : (j0 % 49) / 7, kx = kh ? (j1 % 49) % 7 : (j0 % 49) % 7;
            const int yy = 2 * yo - 3 + ky, xx = 2 * xo - 3 + kx;
            const bool ok = live & ((2 * kk + kh) < S7E_K) & (yy >= 0) & (yy < p.Hi) & (xx >= 0) & (xx < p.Wi);
            const unsigned off = (img0 + (unsigned)((c * p.Hi + yy) * p.Wi + xx)) * 4u;
            a[kk] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsI, ok ? off : OOB, 0, 0));
        }
        v16f acc[2];
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[0][r] = acc[1][r] = 0.f;
#pragma unroll
        for (int kk = 0; kk < S7E_STEPS; ++kk) {
            const float b0 = wl[(2 * kk + kh) * 64 + n], b1 = wl[(2 * kk + kh) * 64 + 32 + n];
            acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[kk], b0, acc[0], 0, 0, 0);
            acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[kk], b1, acc[1], 0, 0, 0);
        }
        const long long row0 = (long long)slab * 128 + wave * 32;
        const int cnt_w = (int)(p.M - row0 < 32 ? (p.M - row0 > 0 ? p.M - row0 : 0) : 32);
#pragma unroll
        for (int g = 0; g < 2; ++g) {
#pragma unroll
            for (int r = 0; r < 16; r += 2) {
                float v0 = fmaf(acc[g][r], sc[g], sh[g]), v1 = fmaf(acc[g][r + 1], sc[g], sh[g]);
                if (p.relu) { v0 = fmaxf(v0, 0.f); v1 = fmaxf(v1, 0.f); }
                unsigned h2, l2;  // (hi_r | hi_r+1 << 16), (lo_r | lo_r+1 << 16)
                f16_split2(v0 * oscale, v1 * oscale, h2, l2);
#pragma unroll
                for (int k = 0; k < 2; ++k) {
                    const int row = ((r + k) & 3) + 8 * ((r + k) >> 2) + 4 * kh;  // rows beyond M: no store, kept out of the maximum
                    const unsigned av = __builtin_bit_cast(unsigned, k == 0 ? v0 : v1) & 0x7fffffffu;
                    if (row < cnt_w) tmax = av > tmax ? av : tmax;
                    const unsigned mine = k == 0 ? ((h2 & 0xffffu) | (l2 << 16)) : ((h2 >> 16) | (l2 & 0xffff0000u));  // (hi | lo << 16) of this row
                    const unsigned nbr = (unsigned)__shfl_xor((int)mine, 1, 64);
                    const unsigned outw = even ? ((mine & 0xffffu) | (nbr << 16)) : ((nbr >> 16) | (mine & 0xffff0000u));
                    if (row < cnt_w) *reinterpret_cast<unsigned*>(p.out16 + (row0 + row) * 256 + g * 128 + lane_off) = outw;
                }
            }
        }
    }
    if (p.ev.out_tmax != nullptr) {  // one atomic per (persistent) workgroup
        tmax = wave_umax(tmax);
        if (lane == 0) redu[wave] = tmax;
        __syncthreads();
        if (tid == 0) {
            const unsigned a = redu[0] > redu[1] ? redu[0] : redu[1], b = redu[2] > redu[3] ? redu[2] : redu[3];
            const unsigned r = a > b ? a : b;
            if (r != 0) atomicMax(reinterpret_cast<unsigned*>(p.ev.out_tmax), r);
        }
    }
}

// ---------------------------------------------------------------------------------------------------- 3x3 stride-2 max pool on P16
// out[b][hp][wp][c] = max over the in-range taps of the 3x3 / stride 2 / pad 1 window (nn.MaxPool2d(3, 2, 1), resnet.py:159; the
// padding is -inf: the window always holds its centre (2 hp, 2 wp)).  Input and output share ONE scale, so nothing is re-split:
// the candidates are compared by hi + lo in the scaled domain (what trid_p16_unpack_f32 multiplies by 2^-s, a monotone map) and
// the winner's two fp16 parts are copied through - unpack(out) == max_pool2d(unpack(x)) exactly.  A thread owns a channel quad.
__global__ __launch_bounds__(256) void maxpool3s2_p16_kernel(const uint2* __restrict__ x, uint2* __restrict__ out, int H, int W, int CQ, int Hp, int Wp,
                                                             long long total4, const float* __restrict__ amax, float* __restrict__ out_tmax) {
    __shared__ unsigned redu[4];
    float am = 0.f;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total4; i += (long long)gridDim.x * 256) {
        const int cq = (int)(i % CQ);
        long long t = i / CQ;
        const int wp = (int)(t % Wp);
        t /= Wp;
        const int hp = (int)(t % Hp);
        const long long b = t / Hp;
        float best[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
        unsigned bh[4] = {0, 0, 0, 0}, bl[4] = {0, 0, 0, 0};
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
            const int h = 2 * hp - 1 + ky;
            if (h < 0 || h >= H) continue;
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const int w = 2 * wp - 1 + kx;
                if (w < 0 || w >= W) continue;
                const uint2* src = x + ((b * H + h) * W + w) * (2 * CQ) + (cq >> 3) * 16 + (cq & 7);
                const uint2 hh = src[0], ll = src[8];
                const unsigned hv[4] = {hh.x & 0xffffu, hh.x >> 16, hh.y & 0xffffu, hh.y >> 16};
                const unsigned lv[4] = {ll.x & 0xffffu, ll.x >> 16, ll.y & 0xffffu, ll.y >> 16};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float v = (float)__builtin_bit_cast(_Float16, (unsigned short)hv[e]) + (float)__builtin_bit_cast(_Float16, (unsigned short)lv[e]);
                    if (v > best[e]) {
                        best[e] = v;
                        bh[e] = hv[e];
                        bl[e] = lv[e];
                    }
                }
            }
        }
        uint2* dst = out + (i / CQ) * (2 * CQ) + (cq >> 3) * 16 + (cq & 7);
        dst[0] = make_uint2(bh[0] | (bh[1] << 16), bh[2] | (bh[3] << 16));
        dst[8] = make_uint2(bl[0] | (bl[1] << 16), bl[2] | (bl[3] << 16));
#pragma unroll
        for (int e = 0; e < 4; ++e) am = fmaxf(am, fabsf(best[e]));
    }
    if (out_tmax != nullptr) {  // true max|out| in the tensor's own units: one atomic per workgroup
        const float inv = 1.f / f16_scale_of(*amax);
        unsigned m = wave_umax(__builtin_bit_cast(unsigned, am * inv));
        if ((threadIdx.x & 63) == 0) redu[threadIdx.x >> 6] = m;
        __syncthreads();
        if (threadIdx.x == 0) {
            const unsigned a = redu[0] > redu[1] ? redu[0] : redu[1], c = redu[2] > redu[3] ? redu[2] : redu[3];
            const unsigned r = a > c ? a : c;
            if (r != 0) atomicMax(reinterpret_cast<unsigned*>(out_tmax), r);
        }
    }
}

// ---------------------------------------------------------------------------------------------------- stride-2 subsample of P16
// The input of a stride-2 1x1 convolution (the downsample branch, resnet.py:137-143): out[b][ho][wo] = x[b][2 ho][2 wo], whole
// C * 4-byte rows copied in 16-byte pieces; the output keeps the source's scale scalar.
__global__ __launch_bounds__(256) void subsample2_p16_kernel(const uint4* __restrict__ x, uint4* __restrict__ out, int H, int W, int U, int Ho, int Wo,
                                                             long long total) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int u = (int)(i % U);
        long long t = i / U;
        const int wo = (int)(t % Wo);
        t /= Wo;
        const int ho = (int)(t % Ho);
        const long long b = t / Ho;
        out[i] = x[((b * H + 2 * ho) * W + 2 * wo) * U + u];
    }
}

// ---------------------------------------------------------------------------------------------------- global average pool of P16
// out[b][c] = (sum over the HW pixels, in pixel order, of the unpacked values) / HW   (nn.AdaptiveAvgPool2d((1, 1)), resnet.py:165):
// the arithmetic of resnet_ops.hip's global_avgpool_kernel on trid_p16_unpack_f32's values, without the fp32 tensor.
__global__ __launch_bounds__(256) void global_avgpool_p16_kernel(const uint2* __restrict__ x, float4* __restrict__ out, int HW, int CQ, long long total4,
                                                                 const float* __restrict__ amax) {
    const float inv = 1.f / f16_scale_of(*amax);
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total4; i += (long long)gridDim.x * 256) {
        const int cq = (int)(i % CQ);
        const long long b = i / CQ;
        float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int px = 0; px < HW; ++px) {
            const float4 v = p16_load4_rc(x, b * HW + px, cq, CQ, inv);
            s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
        }
        const float n = (float)HW;
        out[i] = make_float4(s.x / n, s.y / n, s.z / n, s.w / n);
    }
}

}  // namespace trid

using namespace trid;

extern "C" int trid_stem7_eval_p16(const float* img, const float* w, const float* bn_scale, const float* bn_shift, void* out, const float* eval_coef,
                                   const float* eval_tin, float* out_bound, float* out_tmax, int B, int Hi, int Wi, int relu, void* stream) {
    TRID_REQUIRE(img && w && bn_scale && bn_shift && out && eval_coef && eval_tin && B > 0 && Hi > 0 && Wi > 0, "trid_stem7_eval_p16: bad arguments");
    TRID_REQUIRE((long long)B * 3 * Hi * Wi * 4 < (1ll << 31), "trid_stem7_eval_p16: the image batch must stay below 2 GB");
    TRID_REQUIRE((reinterpret_cast<uintptr_t>(out) & 3u) == 0, "trid_stem7_eval_p16: out must be 4-byte aligned");
    Stem7EvalParams p;
    memset(&p, 0, sizeof(p));
    p.Ho = (Hi - 1) / 2 + 1;
    p.Wo = (Wi - 1) / 2 + 1;
    p.M = (long long)B * p.Ho * p.Wo;
    TRID_REQUIRE(p.M * 256 < (1ll << 31), "trid_stem7_eval_p16: the output must stay below 2 GB (31-bit offsets)");
    p.img = img; p.w = w; p.out16 = reinterpret_cast<char*>(out);
    p.bn_scale = bn_scale; p.bn_shift = bn_shift; p.relu = relu;
    p.ev.coef = eval_coef; p.ev.tin = eval_tin; p.ev.out_bound = out_bound; p.ev.out_tmax = out_tmax;
    p.B = B; p.Hi = Hi; p.Wi = Wi;
    p.nslabs = (int)((p.M + 127) / 128);
    p.fdWo = make_fastdiv((uint32_t)p.Wo);
    p.fdHo = make_fastdiv((uint32_t)p.Ho);
    const int grid = p.nslabs < 256 * 8 ? p.nslabs : 256 * 8;
    hipLaunchKernelGGL(stem7_eval_p16_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, p);
    return check_launch("trid_stem7_eval_p16");
}

extern "C" int trid_maxpool3s2_p16(const void* x, const float* x_amax, void* out, float* out_tmax, int B, int H, int W, int C, void* stream) {
    TRID_REQUIRE(x && x_amax && out && B > 0 && H > 0 && W > 0 && C > 0 && C % 32 == 0 && aligned16(x) && aligned16(out), "trid_maxpool3s2_p16: bad arguments (C %% 32 == 0)");
    const int Hp = (H - 1) / 2 + 1, Wp = (W - 1) / 2 + 1;
    const long long total4 = (long long)B * Hp * Wp * (C / 4);
    hipLaunchKernelGGL(maxpool3s2_p16_kernel, dim3(grid_for(total4, 256, 8192)), dim3(256), 0, (hipStream_t)stream, (const uint2*)x, (uint2*)out, H, W, C / 4, Hp,
                       Wp, total4, x_amax, out_tmax);
    return check_launch("trid_maxpool3s2_p16");
}

extern "C" int trid_subsample2_p16(const void* x, void* out, int B, int H, int W, int C, void* stream) {
    TRID_REQUIRE(x && out && B > 0 && H > 0 && W > 0 && C > 0 && C % 32 == 0 && aligned16(x) && aligned16(out), "trid_subsample2_p16: bad arguments (C %% 32 == 0)");
    const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
    const long long total = (long long)B * Ho * Wo * (C / 4);
    hipLaunchKernelGGL(subsample2_p16_kernel, dim3(grid_for(total, 256, 8192)), dim3(256), 0, (hipStream_t)stream, (const uint4*)x, (uint4*)out, H, W, C / 4, Ho, Wo,
                       total);
    return check_launch("trid_subsample2_p16");
}

extern "C" int trid_global_avgpool_p16(const void* x, const float* x_amax, float* out, int B, int HW, int C, void* stream) {
    TRID_REQUIRE(x && x_amax && out && B > 0 && HW > 0 && C > 0 && C % 32 == 0 && aligned16(x) && aligned16(out), "trid_global_avgpool_p16: bad arguments (C %% 32 == 0)");
    const long long total4 = (long long)B * (C / 4);
    hipLaunchKernelGGL(global_avgpool_p16_kernel, dim3(grid_for(total4, 256, 8192)), dim3(256), 0, (hipStream_t)stream, (const uint2*)x, (float4*)out, HW, C / 4,
                       total4, x_amax);
    return check_launch("trid_global_avgpool_p16");
}
