// Embedding head and loss kernels: L2 row normalisation, the batch-wide queue
// hit mask, masked InfoNCE rows, label-smoothed cross-entropy rows, projection
// column normalisation, global-align softplus terms, CMPM rows, the CMPC cross
// projection, small reductions.
// Reference: head.py:126-175, losses.py:6-217, moco_head/loss.py.
// The [rows, K] similarity / logit matrices are produced by trid_gemm_f32; the
// kernels here turn them into per-row losses and, in place, into dL/dlogits, so
// that the backward pass is two more GEMMs and no second softmax.

#include "common.h"

namespace trid {

__device__ __forceinline__ float block_sum(float v, float* red) {
    v = wave_sum(v);
    const int w = threadIdx.x >> 6, nw = blockDim.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[w] = v;
    __syncthreads();
    float s = 0.f;
    for (int i = 0; i < nw; ++i) s += red[i];
    return s;
}
__device__ __forceinline__ float block_max(float v, float* red) {
    v = wave_max(v);
    const int w = threadIdx.x >> 6, nw = blockDim.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[w] = v;
    __syncthreads();
    float s = -INFINITY;
    for (int i = 0; i < nw; ++i) s = fmaxf(s, red[i]);
    return s;
}

// one wave per row
__global__ void l2norm_rows_kernel(const float* __restrict__ x, float* __restrict__ y, float* __restrict__ inv_norm,
                                   long long rows, int C, float eps) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float* xr = x + row * C;
    float s = 0.f;
    for (int j = lane; j < C; j += 64) s = fmaf(xr[j], xr[j], s);
    s = wave_sum(s);
    const float inv = 1.f / fmaxf(sqrtf(s), eps);
    for (int j = lane; j < C; j += 64) y[row * C + j] = xr[j] * inv;
    if (lane == 0 && inv_norm != nullptr) inv_norm[row] = inv;
}

__global__ void l2norm_rows_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ y,
                                       const float* __restrict__ inv_norm, float* __restrict__ dx, long long rows, int C,
                                       int accumulate) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float* dr = dy + row * C;
    const float* yr = y + row * C;
    float d = 0.f;
    for (int j = lane; j < C; j += 64) d = fmaf(dr[j], yr[j], d);
    d = wave_sum(d);
    const float inv = inv_norm[row];
    for (int j = lane; j < C; j += 64) {
        const float v = (dr[j] - yr[j] * d) * inv;
        dx[row * C + j] = accumulate ? dx[row * C + j] + v : v;
    }
}

__global__ void queue_hit_mask_kernel(const int64_t* __restrict__ id_queue, const int64_t* __restrict__ ids,
                                      uint8_t* __restrict__ flag, int K, int B) {
    extern __shared__ int64_t sid[];
    for (int i = threadIdx.x; i < B; i += blockDim.x) sid[i] = ids[i];
    __syncthreads();
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= K) return;
    const int64_t v = id_queue[k];
    bool hit = false;
    for (int i = 0; i < B; ++i) hit |= (sid[i] == v);
    flag[k] = hit ? 1 : 0;
}

// InfoNCE over one query row's masked queue logits, split over the row so that long queues fill the chip:
// a row of K logits is cut into segments of INFONCE_SEG columns, one workgroup each.
//   pass 1 (infonce_partial_kernel): per segment, max and sum of exp over the unmasked columns;
//   pass 2 (infonce_finish_kernel) : every workgroup folds the row's segment partials (fixed order, so the
//          result does not depend on scheduling) with the positive logit into the row's log-sum-exp,
//          then rewrites its segment in place as dL/dS; segment 0 also emits the row loss and dL/dpos.
// float4 accesses throughout (K and ldS multiples of 4 take the vector path).
constexpr int INFONCE_SEG = 4096;

__global__ __launch_bounds__(256) void infonce_partial_kernel(const float* __restrict__ S, const uint8_t* __restrict__ hit,
                                                              float2* __restrict__ part, int K, int ldS, float invT) {
    __shared__ float red[8];
    const int b = blockIdx.x, seg = blockIdx.y, nseg = gridDim.y;
    const float* r = S + (long long)b * ldS;
    const int k0 = seg * INFONCE_SEG, k1 = min(K, k0 + INFONCE_SEG);
    const bool vec = ((ldS & 3) == 0) && ((reinterpret_cast<uintptr_t>(S) & 15) == 0);
    float m = -INFINITY;
    if (vec) {
        for (int k = k0 + 4 * threadIdx.x; k < k1; k += 1024) {
            const float4 v = *reinterpret_cast<const float4*>(r + k);
            if (k + 3 < k1) {
                const uchar4 h = *reinterpret_cast<const uchar4*>(hit + k);  // k % 4 == 0; the tail reads hit byte-wise
                if (!h.x) m = fmaxf(m, v.x * invT);
                if (!h.y) m = fmaxf(m, v.y * invT);
                if (!h.z) m = fmaxf(m, v.z * invT);
                if (!h.w) m = fmaxf(m, v.w * invT);
            } else {
                for (int t = k; t < k1; ++t) if (!hit[t]) m = fmaxf(m, r[t] * invT);
            }
        }
    } else {
        for (int k = k0 + threadIdx.x; k < k1; k += 256) if (!hit[k]) m = fmaxf(m, r[k] * invT);
    }
    m = block_max(m, red);
    float l = 0.f;
    if (m > -INFINITY) {
        if (vec) {
            for (int k = k0 + 4 * threadIdx.x; k < k1; k += 1024) {
                const float4 v = *reinterpret_cast<const float4*>(r + k);
                if (k + 3 < k1) {
                    const uchar4 h = *reinterpret_cast<const uchar4*>(hit + k);
                    if (!h.x) l += expf(v.x * invT - m);
                    if (!h.y) l += expf(v.y * invT - m);
                    if (!h.z) l += expf(v.z * invT - m);
                    if (!h.w) l += expf(v.w * invT - m);
                } else {
                    for (int t = k; t < k1; ++t) if (!hit[t]) l += expf(r[t] * invT - m);
                }
            }
        } else {
            for (int k = k0 + threadIdx.x; k < k1; k += 256) if (!hit[k]) l += expf(r[k] * invT - m);
        }
    }
    l = block_sum(l, red);
    if (threadIdx.x == 0) part[(long long)b * nseg + seg] = make_float2(m, l);
}

// `pos` may be null: then the positive logit <q_b, key_b> is computed here from q / key [B, C] (saves a
// launch), and segment 0 also writes dq0[b, :] = dL/dpos * key_b, the positive-pair term of dL/dq that the
// gradient GEMM then accumulates onto.
__global__ __launch_bounds__(256) void infonce_finish_kernel(float* __restrict__ S, const float* __restrict__ pos,
                                                             const uint8_t* __restrict__ hit,
                                                             const float2* __restrict__ part,
                                                             float* __restrict__ loss_rows, float* __restrict__ dpos,
                                                             int K, int ldS, float invT, float gs,
                                                             const float* __restrict__ q, const float* __restrict__ key,
                                                             float* __restrict__ dq0, int C) {
    __shared__ float red[8];
    const int b = blockIdx.x, seg = blockIdx.y, nseg = gridDim.y;
    float* r = S + (long long)b * ldS;
    float praw;
    if (pos != nullptr) {
        praw = pos[b];
    } else {
        float d = 0.f;
        for (int c = threadIdx.x; c < C; c += 256) d = fmaf(q[(long long)b * C + c], key[(long long)b * C + c], d);
        praw = block_sum(d, red);
    }
    const float p = praw * invT;
    float m = p;
    for (int s2 = 0; s2 < nseg; ++s2) m = fmaxf(m, part[(long long)b * nseg + s2].x);
    float l = expf(p - m);
    for (int s2 = 0; s2 < nseg; ++s2) {
        const float2 q = part[(long long)b * nseg + s2];
        if (q.x > -INFINITY) l += q.y * expf(q.x - m);
    }
    const float lse = m + logf(l);
    const int k0 = seg * INFONCE_SEG, k1 = min(K, k0 + INFONCE_SEG);
    const bool vec = ((ldS & 3) == 0) && ((reinterpret_cast<uintptr_t>(S) & 15) == 0);
    if (vec) {
        for (int k = k0 + 4 * threadIdx.x; k < k1; k += 1024) {
            if (k + 3 < k1) {
                float4 v = *reinterpret_cast<const float4*>(r + k);
                const uchar4 h = *reinterpret_cast<const uchar4*>(hit + k);
                v.x = h.x ? 0.f : expf(v.x * invT - lse) * gs;
                v.y = h.y ? 0.f : expf(v.y * invT - lse) * gs;
                v.z = h.z ? 0.f : expf(v.z * invT - lse) * gs;
                v.w = h.w ? 0.f : expf(v.w * invT - lse) * gs;
                *reinterpret_cast<float4*>(r + k) = v;
            } else {
                for (int t = k; t < k1; ++t) r[t] = hit[t] ? 0.f : expf(r[t] * invT - lse) * gs;
            }
        }
    } else {
        for (int k = k0 + threadIdx.x; k < k1; k += 256) r[k] = hit[k] ? 0.f : expf(r[k] * invT - lse) * gs;
    }
    if (seg == 0) {
        const float dp = (expf(p - lse) - 1.f) * gs;
        if (threadIdx.x == 0) {
            loss_rows[b] = lse - p;
            if (dpos != nullptr) dpos[b] = dp;
        }
        if (dq0 != nullptr)
            for (int c = threadIdx.x; c < C; c += 256) dq0[(long long)b * C + c] = dp * key[(long long)b * C + c];
    }
}

__global__ void rowdot_kernel(const float* __restrict__ x, const float* __restrict__ y, float* __restrict__ out,
                              long long rows, int C) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (row >= rows) return;
    float d = 0.f;
    for (int j = lane; j < C; j += 64) d = fmaf(x[row * C + j], y[row * C + j], d);
    d = wave_sum(d);
    if (lane == 0) out[row] = d;
}

__global__ void rowscale_add_kernel(const float* __restrict__ s, const float* __restrict__ y, float* __restrict__ dx,
                                    long long rows, int C, int accumulate) {
    const long long total = rows * C;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += (long long)gridDim.x * blockDim.x) {
        const float v = s[i / C] * y[i];
        dx[i] = accumulate ? dx[i] + v : v;
    }
}

// one workgroup per row; in place logits -> dlogits
__global__ __launch_bounds__(256) void smooth_ce_rows_kernel(float* __restrict__ logits,
                                                             const int64_t* __restrict__ labels,
                                                             float* __restrict__ loss_rows, int n, int ld, float eps,
                                                             float gs) {
    __shared__ float red[8];
    const long long row = blockIdx.x;
    float* r = logits + row * ld;
    const int y = (int)labels[row];
    float m = -INFINITY, sum = 0.f;
    for (int j = threadIdx.x; j < n; j += 256) {
        const float v = r[j];
        m = fmaxf(m, v);
        sum += v;
    }
    m = block_max(m, red);
    sum = block_sum(sum, red);
    float l = 0.f;
    for (int j = threadIdx.x; j < n; j += 256) l += expf(r[j] - m);
    l = block_sum(l, red);
    const float lse = m + logf(l);
    const float sy = r[y];
    __syncthreads();
    const float un = eps / (float)n;
    for (int j = threadIdx.x; j < ld; j += 256) {
        float g = 0.f;
        if (j < n) g = (expf(r[j] - lse) - un - (j == y ? (1.f - eps) : 0.f)) * gs;
        r[j] = g;
    }
    if (threadIdx.x == 0) loss_rows[row] = -(1.f - eps) * (sy - lse) - un * (sum - (float)n * lse);
}

// projection [C,N] -> pn [C,ldn] (optional) and pnt [ldn,C]: one workgroup per 64 columns.
// Reads are coalesced along N, the transposed write goes through an LDS tile.
__global__ __launch_bounds__(256) void colnorm_kernel(const float* __restrict__ proj, float* __restrict__ pn,
                                                      float* __restrict__ pnt, float* __restrict__ inv_norm, int C, int N,
                                                      int ldn) {
    __shared__ float tile[64][65];
    __shared__ float part[4][64];
    __shared__ float invs[64];
    const int cl = threadIdx.x & 63, rl = threadIdx.x >> 6;
    const int j0 = blockIdx.x * 64;
    const int j = j0 + cl;
    float s = 0.f;
    if (j < N)
        for (int c = rl; c < C; c += 4) {
            const float v = proj[(long long)c * N + j];
            s = fmaf(v, v, s);
        }
    part[rl][cl] = s;
    __syncthreads();
    if (rl == 0) {
        const float t = part[0][cl] + part[1][cl] + part[2][cl] + part[3][cl];
        const float inv = j < N ? 1.f / fmaxf(sqrtf(t), 1e-12f) : 0.f;
        invs[cl] = inv;
        if (j < N) inv_norm[j] = inv;
    }
    __syncthreads();
    const float inv = invs[cl];
    for (int c0 = 0; c0 < C; c0 += 64) {
        for (int c = c0 + rl; c < c0 + 64 && c < C; c += 4) {
            const float v = j < N ? proj[(long long)c * N + j] * inv : 0.f;
            if (pn != nullptr && j < ldn) pn[(long long)c * ldn + j] = v;
            tile[c - c0][cl] = v;
        }
        __syncthreads();
        // write pnt rows j0..j0+63, columns c0..c0+63: lanes along c
        for (int jj = rl; jj < 64; jj += 4) {
            const int c = c0 + cl;
            if (j0 + jj < ldn && c < C) pnt[(long long)(j0 + jj) * C + c] = tile[cl][jj];
        }
        __syncthreads();
    }
}

// one wave per column j: dproj[c,j] = (dpnt[j,c] - pnt[j,c]*<dpnt_j,pnt_j>)*inv_j
__global__ void colnorm_bwd_kernel(const float* __restrict__ dpnt, const float* __restrict__ pnt,
                                   const float* __restrict__ inv_norm, float* __restrict__ dproj, int C, int N) {
    const int lane = threadIdx.x & 63;
    const int j = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (j >= N) return;
    const float* dr = dpnt + (long long)j * C;
    const float* pr = pnt + (long long)j * C;
    float d = 0.f;
    for (int c = lane; c < C; c += 64) d = fmaf(dr[c], pr[c], d);
    d = wave_sum(d);
    const float inv = inv_norm[j];
    for (int c = lane; c < C; c += 64) dproj[(long long)c * N + j] = (dr[c] - pr[c] * d) * inv;
}

// one workgroup per row of the cosine matrix
__global__ __launch_bounds__(256) void global_align_rows_kernel(float* __restrict__ S, const int64_t* __restrict__ ids,
                                                                float* __restrict__ loss_rows, int B, int ldS,
                                                                float alpha, float beta, float sp, float sn, float gs) {
    __shared__ float red[8];
    const int i = blockIdx.x;
    float* r = S + (long long)i * ldS;
    const int64_t idi = ids[i];
    float acc = 0.f;
    for (int j = threadIdx.x; j < B; j += 256) {
        const float s = r[j];
        float l, g;
        if (ids[j] == idi) {
            const float e = expf(-sp * (s - alpha));
            l = logf(1.f + e);
            g = -sp * e / (1.f + e);
        } else {
            const float e = expf(sn * (s - beta));
            l = logf(1.f + e);
            g = sn * e / (1.f + e);
        }
        acc += l;
        r[j] = g * gs;
    }
    acc = block_sum(acc, red);
    if (threadIdx.x == 0) loss_rows[i] = acc * 2.f / (float)B;
}

// CMPM rows (losses.py:156-203): one wavefront per row of the projection matrix S [B, ldS] (only the first B columns
// enter the softmax: the zero padding of the GEMM operands stays out).  p = softmax(row), target q_ij = [id_i == id_j] /
// sqrt(n_i) with n_i the number of row i's same-id columns.  (The reference divides element [i,j] by the norm of mask
// row j, a [B] vector broadcast along the last axis; the mask is non-zero only where id_i == id_j, and equal ids have
// equal counts, so that is the per-row form computed here.)  loss_i = sum_j p_ij (log p_ij - log(q_ij + eps));
// in place S_ij <- gs * p_ij ((log p_ij - log(q_ij + eps)) - loss_i) = gs * dloss_i/dS_ij.
// B <= 256: the row lives in four registers per lane; longer rows are re-read (L2-resident) in each pass.
__global__ __launch_bounds__(256) void cmpm_rows_kernel(float* __restrict__ S, const int64_t* __restrict__ ids,
                                                        float* __restrict__ loss_rows, int B, int ldS, float eps,
                                                        float gs) {
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (i >= B) return;  // (whole wavefronts leave: no partial-wave shuffles below)
    float* r = S + (long long)i * ldS;
    const int64_t idi = ids[i];
    const bool inreg = B <= 256;
    float v[4];
    unsigned same = 0;  // bit k: column lane + 64 k carries row i's id (register path)
    float m = -INFINITY, cnt = 0.f;
    if (inreg) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int j = lane + 64 * k;
            v[k] = j < B ? r[j] : -INFINITY;
            if (j < B && ids[j] == idi) same |= 1u << k;
            m = fmaxf(m, v[k]);
        }
        cnt = (float)__popc(same);
    } else {
        for (int j = lane; j < B; j += 64) {
            m = fmaxf(m, r[j]);
            cnt += ids[j] == idi ? 1.f : 0.f;
        }
    }
    m = wave_max(m);
    cnt = wave_sum(cnt);
    float l = 0.f;
    if (inreg) {
#pragma unroll
        for (int k = 0; k < 4; ++k) l += expf(v[k] - m);  // exp(-inf) = 0 for the columns past B
    } else {
        for (int j = lane; j < B; j += 64) l += expf(r[j] - m);
    }
    l = wave_sum(l);
    const float lse = m + logf(l);
    const float lq_same = logf(1.f / sqrtf(cnt) + eps), lq_diff = logf(eps);
    float acc = 0.f;
    if (inreg) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (lane + 64 * k < B) {
                const float lp = v[k] - lse;
                acc += expf(lp) * (lp - ((same >> k) & 1u ? lq_same : lq_diff));
            }
        }
    } else {
        for (int j = lane; j < B; j += 64) {
            const float lp = r[j] - lse;
            acc += expf(lp) * (lp - (ids[j] == idi ? lq_same : lq_diff));
        }
    }
    const float loss = wave_sum(acc);
    if (inreg) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int j = lane + 64 * k;
            if (j < B) {
                const float lp = v[k] - lse;
                r[j] = gs * expf(lp) * ((lp - ((same >> k) & 1u ? lq_same : lq_diff)) - loss);
            }
        }
    } else {
        for (int j = lane; j < B; j += 64) {
            const float lp = r[j] - lse;
            r[j] = gs * expf(lp) * ((lp - (ids[j] == idi ? lq_same : lq_diff)) - loss);
        }
    }
    if (lane == 0) loss_rows[i] = loss;
}

// mean of row_scale[i] * S[i,j] over the same-id pairs and over the different-id pairs (cmpm_loss's `verbose` figures,
// losses.py:196-200): one workgroup, fixed summation order.  An empty set gives 0/0 = NaN, as torch.mean of nothing.
__global__ __launch_bounds__(256) void pair_sim_means_kernel(const float* __restrict__ S, const float* __restrict__ row_scale,
                                                             const int64_t* __restrict__ ids, float* __restrict__ out2,
                                                             int B, int ldS) {
    __shared__ float red[8];
    float sp = 0.f, sn = 0.f, np = 0.f;
    for (int e = threadIdx.x; e < B * B; e += 256) {
        const int i = e / B, j = e - i * B;
        const float s = S[(long long)i * ldS + j] * (row_scale != nullptr ? row_scale[i] : 1.f);
        if (ids[i] == ids[j]) {
            sp += s;
            np += 1.f;
        } else {
            sn += s;
        }
    }
    sp = block_sum(sp, red);
    sn = block_sum(sn, red);
    np = block_sum(np, red);
    if (threadIdx.x == 0) {
        out2[0] = sp / np;
        out2[1] = sn / ((float)B * (float)B - np);
    }
}

// CMPC operand (losses.py:73-82): one wavefront per pair i.  With d = <v_i, t_i>, iv = 1/max(|v_i|, 1e-12) and it
// likewise: ipt_i = (v_i . t^_i) t^_i = (d it) it t_i -> X[i], tpi_i = (t_i . v^_i) v^_i = (d iv) iv v_i -> X[B + i];
// dots[i] = v_i . t^_i, dots[B + i] = t_i . v^_i, inv[i] = iv, inv[B + i] = it.  VEC: 128-bit accesses (C % 4 == 0).
template <bool VEC>
__global__ __launch_bounds__(256) void cross_project_rows_kernel(const float* __restrict__ v, const float* __restrict__ t,
                                                                 float* __restrict__ X, float* __restrict__ dots,
                                                                 float* __restrict__ inv, int B, int C) {
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (i >= B) return;
    const float* vr = v + (long long)i * C;
    const float* tr = t + (long long)i * C;
    float vv = 0.f, tt = 0.f, vt = 0.f;
    if (VEC) {
        for (int c = 4 * lane; c < C; c += 256) {
            const float4 a = *reinterpret_cast<const float4*>(vr + c), b = *reinterpret_cast<const float4*>(tr + c);
            vv += a.x * a.x + a.y * a.y + a.z * a.z + a.w * a.w;
            tt += b.x * b.x + b.y * b.y + b.z * b.z + b.w * b.w;
            vt += a.x * b.x + a.y * b.y + a.z * b.z + a.w * b.w;
        }
    } else {
        for (int c = lane; c < C; c += 64) {
            vv = fmaf(vr[c], vr[c], vv);
            tt = fmaf(tr[c], tr[c], tt);
            vt = fmaf(vr[c], tr[c], vt);
        }
    }
    vv = wave_sum(vv);
    tt = wave_sum(tt);
    vt = wave_sum(vt);
    const float iv = 1.f / fmaxf(sqrtf(vv), 1e-12f), it = 1.f / fmaxf(sqrtf(tt), 1e-12f);
    const float a = vt * it, b = vt * iv;
    float* x1 = X + (long long)i * C;
    float* x2 = X + (long long)(B + i) * C;
    if (VEC) {
        const float s1 = a * it, s2 = b * iv;
        for (int c = 4 * lane; c < C; c += 256) {
            const float4 p = *reinterpret_cast<const float4*>(vr + c), q = *reinterpret_cast<const float4*>(tr + c);
            *reinterpret_cast<float4*>(x1 + c) = make_float4(s1 * q.x, s1 * q.y, s1 * q.z, s1 * q.w);
            *reinterpret_cast<float4*>(x2 + c) = make_float4(s2 * p.x, s2 * p.y, s2 * p.z, s2 * p.w);
        }
    } else {
        for (int c = lane; c < C; c += 64) {
            x1[c] = a * it * tr[c];
            x2[c] = b * iv * vr[c];
        }
    }
    if (lane == 0) {
        dots[i] = a;
        dots[B + i] = b;
        inv[i] = iv;
        inv[B + i] = it;
    }
}

// Backward of the above.  G [2B, C] = dL/dX.  With g1 = G[i], g2 = G[B + i], a = dots[i], b = dots[B + i],
// p1 = g1 . t^, p2 = g2 . v^:
//   through ipt:  dv  = p1 t^;   dt^ = a g1 + p1 v, and the normalisation's Jacobian (dt^ - t^ <dt^, t^>) it with
//                 <dt^, t^> = a p1 + p1 (v . t^) = 2 a p1;
//   through tpi:  dt  = p2 v^;   dv^ = b g2 + p2 t, <dv^, v^> = 2 b p2, Jacobian likewise.
// Each modality receives two contributions, summed in that fixed order (ipt's first).
__global__ __launch_bounds__(256) void cross_project_rows_bwd_kernel(const float* __restrict__ G, const float* __restrict__ v,
                                                                     const float* __restrict__ t,
                                                                     const float* __restrict__ dots,
                                                                     const float* __restrict__ inv, float* __restrict__ dv,
                                                                     float* __restrict__ dt, int B, int C) {
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (i >= B) return;
    const float* vr = v + (long long)i * C;
    const float* tr = t + (long long)i * C;
    const float* g1 = G + (long long)i * C;
    const float* g2 = G + (long long)(B + i) * C;
    const float a = dots[i], b = dots[B + i], iv = inv[i], it = inv[B + i];
    float p1 = 0.f, p2 = 0.f;
    for (int c = lane; c < C; c += 64) {
        p1 = fmaf(g1[c], tr[c], p1);
        p2 = fmaf(g2[c], vr[c], p2);
    }
    p1 = wave_sum(p1) * it;
    p2 = wave_sum(p2) * iv;
    for (int c = lane; c < C; c += 64) {
        const float vn = vr[c] * iv, tn = tr[c] * it;
        const float dv1 = p1 * tn;
        const float dt1 = (a * g1[c] + p1 * vr[c] - 2.f * a * p1 * tn) * it;
        const float dt2 = p2 * vn;
        const float dv2 = (b * g2[c] + p2 * tr[c] - 2.f * b * p2 * vn) * iv;
        dv[(long long)i * C + c] = dv1 + dv2;
        dt[(long long)i * C + c] = dt1 + dt2;
    }
}

// one workgroup per row: index of the row maximum (ties: the lowest index, as torch.argmax); hit[r] = 1 if it equals
// labels[r] (both outputs optional)
__global__ __launch_bounds__(256) void argmax_rows_kernel(const float* __restrict__ x, const int64_t* __restrict__ labels,
                                                          int64_t* __restrict__ idx, float* __restrict__ hit, int n,
                                                          int ld) {
    __shared__ float bv[4];
    __shared__ int bi[4];
    const long long row = blockIdx.x;
    const float* r = x + row * ld;
    float best = -INFINITY;
    int at = n;  // (every index beats n: an all -inf row answers 0 through the scan below)
    for (int j = threadIdx.x; j < n; j += 256) {
        const float s = r[j];
        if (s > best || (s == best && j < at)) {
            best = s;
            at = j;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ob = __shfl_xor(best, o, 64);
        const int oa = __shfl_xor(at, o, 64);
        if (ob > best || (ob == best && oa < at)) {
            best = ob;
            at = oa;
        }
    }
    if ((threadIdx.x & 63) == 0) {
        bv[threadIdx.x >> 6] = best;
        bi[threadIdx.x >> 6] = at;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w)
            if (bv[w] > best || (bv[w] == best && bi[w] < at)) {
                best = bv[w];
                at = bi[w];
            }
        if (at >= n) at = 0;
        if (idx != nullptr) idx[row] = at;
        if (hit != nullptr) hit[row] = (int64_t)at == labels[row] ? 1.f : 0.f;
    }
}

__global__ __launch_bounds__(256) void sum_kernel(const float* __restrict__ x, float* __restrict__ out, long long n,
                                                  float scale, int accumulate) {
    __shared__ float red[8];
    float s = 0.f;
    for (long long i = threadIdx.x; i < n; i += 256) s += x[i];
    s = block_sum(s, red);
    if (threadIdx.x == 0) out[0] = accumulate ? out[0] + s * scale : s * scale;
}

// dx = act > 0 ? dy : 0   (ReLU backward of the MoCo head's fc branches, head.py:33-42)
__global__ void relu_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ act, float* __restrict__ dx, long long n) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
        dx[i] = act[i] > 0.f ? dy[i] : 0.f;
}

// out = g[0]*a + g[1]*b + g[2]*c with device-resident scalars (b, c optional)
__global__ void axpby3_kernel(float* __restrict__ out, const float* __restrict__ a, const float* __restrict__ b,
                              const float* __restrict__ c, const float* __restrict__ g, long long n) {
    const float g0 = g[0], g1 = b ? g[1] : 0.f, g2 = c ? g[2] : 0.f;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        float v = g0 * a[i];
        if (b) v = fmaf(g1, b[i], v);
        if (c) v = fmaf(g2, c[i], v);
        out[i] = v;
    }
}

}  // namespace trid

using namespace trid;

extern "C" int trid_relu_bwd_f32(const float* dy, const float* act, float* dx, long long n, void* stream) {
    TRID_REQUIRE(dy && act && dx && n > 0, "trid_relu_bwd_f32: bad arguments");
    hipLaunchKernelGGL(relu_bwd_kernel, dim3(grid_for(n, 256 * 4, 2048)), dim3(256), 0, (hipStream_t)stream, dy, act, dx, n);
    return check_launch("trid_relu_bwd_f32");
}

extern "C" int trid_axpby3_f32(float* out, const float* a, const float* b, const float* c, const float* g3,
                               long long n, void* stream) {
    TRID_REQUIRE(out && a && g3 && n > 0, "trid_axpby3_f32: bad arguments");
    hipLaunchKernelGGL(axpby3_kernel, dim3(grid_for(n, 256 * 4, 2048)), dim3(256), 0, (hipStream_t)stream, out, a, b, c, g3,
                       n);
    return check_launch("trid_axpby3_f32");
}

extern "C" int trid_l2norm_rows_f32(const float* x, float* y, float* inv_norm, long long rows, int C, float eps,
                                    void* stream) {
    TRID_REQUIRE(x && y && rows > 0 && C > 0, "trid_l2norm_rows_f32: bad arguments");
    hipLaunchKernelGGL(l2norm_rows_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, x, y,
                       inv_norm, rows, C, eps);
    return check_launch("trid_l2norm_rows_f32");
}

extern "C" int trid_l2norm_rows_bwd_f32(const float* dy, const float* y, const float* inv_norm, float* dx,
                                        long long rows, int C, int accumulate, void* stream) {
    TRID_REQUIRE(dy && y && inv_norm && dx && rows > 0 && C > 0, "trid_l2norm_rows_bwd_f32: bad arguments");
    hipLaunchKernelGGL(l2norm_rows_bwd_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, dy, y,
                       inv_norm, dx, rows, C, accumulate);
    return check_launch("trid_l2norm_rows_bwd_f32");
}

extern "C" int trid_queue_hit_mask(const int64_t* id_queue, const int64_t* ids, uint8_t* flag, int K, int B,
                                   void* stream) {
    TRID_REQUIRE(id_queue && ids && flag && K > 0 && B > 0 && B <= 8192, "trid_queue_hit_mask: bad arguments");
    hipLaunchKernelGGL(queue_hit_mask_kernel, dim3((K + 255) / 256), dim3(256), (size_t)B * sizeof(int64_t),
                       (hipStream_t)stream, id_queue, ids, flag, K, B);
    return check_launch("trid_queue_hit_mask");
}

extern "C" long long trid_infonce_ws_floats(int B, int K) { return 2LL * B * ((K + INFONCE_SEG - 1) / INFONCE_SEG); }

extern "C" int trid_infonce_rows_f32(float* S, const float* pos, const uint8_t* hit, float* loss_rows, float* dpos,
                                     int B, int K, int ldS, float invT, float gscale, float* ws, void* stream) {
    TRID_REQUIRE(S && pos && hit && loss_rows && dpos && ws && B > 0 && K > 0 && ldS >= K, "trid_infonce_rows_f32: bad arguments");
    TRID_REQUIRE((reinterpret_cast<uintptr_t>(hit) & 3) == 0 && (reinterpret_cast<uintptr_t>(ws) & 7) == 0, "trid_infonce_rows_f32: hit must be 4-byte and ws 8-byte aligned");
    const int nseg = (K + INFONCE_SEG - 1) / INFONCE_SEG;
    hipLaunchKernelGGL(infonce_partial_kernel, dim3(B, nseg), dim3(256), 0, (hipStream_t)stream, S, hit, (float2*)ws, K, ldS, invT);
    hipLaunchKernelGGL(infonce_finish_kernel, dim3(B, nseg), dim3(256), 0, (hipStream_t)stream, S, pos, hit, (const float2*)ws,
                       loss_rows, dpos, K, ldS, invT, gscale * invT / (float)B, (const float*)nullptr, (const float*)nullptr,
                       (float*)nullptr, 0);
    return check_launch("trid_infonce_rows_f32");
}

extern "C" int trid_infonce_queue_rows_f32(float* S, const float* q, const float* key, const uint8_t* hit, float* loss_rows,
                                           float* dq0, int B, int K, int ldS, int C, float invT, float gscale, float* ws,
                                           void* stream) {
    TRID_REQUIRE(S && q && key && hit && loss_rows && dq0 && ws && B > 0 && K > 0 && C > 0 && ldS >= K,
                 "trid_infonce_queue_rows_f32: bad arguments");
    TRID_REQUIRE((reinterpret_cast<uintptr_t>(hit) & 3) == 0 && (reinterpret_cast<uintptr_t>(ws) & 7) == 0,
                 "trid_infonce_queue_rows_f32: hit must be 4-byte and ws 8-byte aligned");
    const int nseg = (K + INFONCE_SEG - 1) / INFONCE_SEG;
    hipLaunchKernelGGL(infonce_partial_kernel, dim3(B, nseg), dim3(256), 0, (hipStream_t)stream, S, hit, (float2*)ws, K, ldS, invT);
    hipLaunchKernelGGL(infonce_finish_kernel, dim3(B, nseg), dim3(256), 0, (hipStream_t)stream, S, (const float*)nullptr, hit,
                       (const float2*)ws, loss_rows, (float*)nullptr, K, ldS, invT, gscale * invT / (float)B, q, key, dq0, C);
    return check_launch("trid_infonce_queue_rows_f32");
}

extern "C" int trid_rowdot_f32(const float* x, const float* y, float* out, long long rows, int C, void* stream) {
    TRID_REQUIRE(x && y && out && rows > 0 && C > 0, "trid_rowdot_f32: bad arguments");
    hipLaunchKernelGGL(rowdot_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, x, y, out,
                       rows, C);
    return check_launch("trid_rowdot_f32");
}

extern "C" int trid_rowscale_add_f32(const float* s, const float* y, float* dx, long long rows, int C, int accumulate,
                                     void* stream) {
    TRID_REQUIRE(s && y && dx && rows > 0 && C > 0, "trid_rowscale_add_f32: bad arguments");
    hipLaunchKernelGGL(rowscale_add_kernel, dim3(grid_for(rows * C, 256)), dim3(256), 0, (hipStream_t)stream, s, y, dx,
                       rows, C, accumulate);
    return check_launch("trid_rowscale_add_f32");
}

extern "C" int trid_smooth_ce_rows_f32(float* logits, const int64_t* labels, float* loss_rows, long long rows, int n,
                                       int ld, float epsilon, float gscale, void* stream) {
    TRID_REQUIRE(logits && labels && loss_rows && rows > 0 && n > 0 && ld >= n, "trid_smooth_ce_rows_f32: bad arguments");
    hipLaunchKernelGGL(smooth_ce_rows_kernel, dim3((unsigned)rows), dim3(256), 0, (hipStream_t)stream, logits, labels,
                       loss_rows, n, ld, epsilon, gscale);
    return check_launch("trid_smooth_ce_rows_f32");
}

extern "C" int trid_colnorm_f32(const float* proj, float* pn, float* pnt, float* inv_norm, int C, int N, int ldn,
                                void* stream) {
    TRID_REQUIRE(proj && pnt && inv_norm && C > 0 && N > 0 && ldn >= N, "trid_colnorm_f32: bad arguments");
    hipLaunchKernelGGL(colnorm_kernel, dim3((ldn + 63) / 64), dim3(256), 0, (hipStream_t)stream, proj, pn, pnt, inv_norm, C,
                       N, ldn);
    return check_launch("trid_colnorm_f32");
}

extern "C" int trid_colnorm_bwd_f32(const float* dpnt, const float* pnt, const float* inv_norm, float* dproj, int C,
                                    int N, int ldn, void* stream) {
    TRID_REQUIRE(dpnt && pnt && inv_norm && dproj && C > 0 && N > 0 && ldn >= N, "trid_colnorm_bwd_f32: bad arguments");
    hipLaunchKernelGGL(colnorm_bwd_kernel, dim3((N + 3) / 4), dim3(256), 0, (hipStream_t)stream, dpnt, pnt, inv_norm,
                       dproj, C, N);
    return check_launch("trid_colnorm_bwd_f32");
}

extern "C" int trid_global_align_rows_f32(float* S, const int64_t* ids, float* loss_rows, int B, int ldS, float alpha,
                                          float beta, float scale_pos, float scale_neg, float gscale, void* stream) {
    TRID_REQUIRE(S && ids && loss_rows && B > 0 && ldS >= B, "trid_global_align_rows_f32: bad arguments");
    hipLaunchKernelGGL(global_align_rows_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, S, ids, loss_rows, B, ldS,
                       alpha, beta, scale_pos, scale_neg, gscale * 2.f / (float)B);
    return check_launch("trid_global_align_rows_f32");
}

extern "C" int trid_cmpm_rows_f32(float* S, const int64_t* ids, float* loss_rows, int B, int ldS, float epsilon,
                                  float gscale, void* stream) {
    TRID_REQUIRE(S && ids && loss_rows && B > 0 && ldS >= B && epsilon > 0.f, "trid_cmpm_rows_f32: bad arguments");
    hipLaunchKernelGGL(cmpm_rows_kernel, dim3((B + 3) / 4), dim3(256), 0, (hipStream_t)stream, S, ids, loss_rows, B, ldS,
                       epsilon, gscale);
    return check_launch("trid_cmpm_rows_f32");
}

extern "C" int trid_pair_sim_means_f32(const float* S, const float* row_scale, const int64_t* ids, float* out2, int B,
                                       int ldS, void* stream) {
    TRID_REQUIRE(S && ids && out2 && B > 0 && B <= 16384 && ldS >= B, "trid_pair_sim_means_f32: bad arguments");
    hipLaunchKernelGGL(pair_sim_means_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, S, row_scale, ids, out2, B, ldS);
    return check_launch("trid_pair_sim_means_f32");
}

extern "C" int trid_cross_project_rows_f32(const float* v, const float* t, float* X, float* dots, float* inv, int B, int C,
                                           void* stream) {
    TRID_REQUIRE(v && t && X && dots && inv && B > 0 && C > 0, "trid_cross_project_rows_f32: bad arguments");
    const bool vec = (C & 3) == 0 && aligned16(v) && aligned16(t) && aligned16(X);
    if (vec)
        hipLaunchKernelGGL(cross_project_rows_kernel<true>, dim3((B + 3) / 4), dim3(256), 0, (hipStream_t)stream, v, t, X,
                           dots, inv, B, C);
    else
        hipLaunchKernelGGL(cross_project_rows_kernel<false>, dim3((B + 3) / 4), dim3(256), 0, (hipStream_t)stream, v, t, X,
                           dots, inv, B, C);
    return check_launch("trid_cross_project_rows_f32");
}

extern "C" int trid_cross_project_rows_bwd_f32(const float* G, const float* v, const float* t, const float* dots,
                                               const float* inv, float* dv, float* dt, int B, int C, void* stream) {
    TRID_REQUIRE(G && v && t && dots && inv && dv && dt && B > 0 && C > 0, "trid_cross_project_rows_bwd_f32: bad arguments");
    hipLaunchKernelGGL(cross_project_rows_bwd_kernel, dim3((B + 3) / 4), dim3(256), 0, (hipStream_t)stream, G, v, t, dots,
                       inv, dv, dt, B, C);
    return check_launch("trid_cross_project_rows_bwd_f32");
}

extern "C" int trid_argmax_rows_f32(const float* x, const int64_t* labels, int64_t* idx, float* hit, long long rows, int n,
                                    int ld, void* stream) {
    TRID_REQUIRE(x && (idx || hit) && (labels || !hit) && rows > 0 && n > 0 && ld >= n, "trid_argmax_rows_f32: bad arguments");
    hipLaunchKernelGGL(argmax_rows_kernel, dim3((unsigned)rows), dim3(256), 0, (hipStream_t)stream, x, labels, idx, hit, n,
                       ld);
    return check_launch("trid_argmax_rows_f32");
}

extern "C" int trid_sum_f32(const float* x, float* out, long long n, float scale, int accumulate, void* stream) {
    TRID_REQUIRE(x && out && n > 0, "trid_sum_f32: bad arguments");
    hipLaunchKernelGGL(sum_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, x, out, n, scale, accumulate);
    return check_launch("trid_sum_f32");
}
