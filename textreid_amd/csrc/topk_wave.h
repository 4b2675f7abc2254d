// Running per-row top-k held by one wave: shared by the retrieval merges (retrieval.hip) and the gallery index (gallery_index.hip).
#pragma once
#include "common.h"

namespace trid {

constexpr int TOPK_MAX = 16;

// Running top-k of one similarity row, held by one wave.  The k best (value, index) pairs live one per
// lane (lane i = i-th best, sorted by value descending, ties lower index first); the k-th value is the
// wave-uniform admission threshold.  Survivors are inserted one at a time with a ballot-popcount
// position and a one-lane shuffle shift.
template <int KK>
struct WaveTopk {
    float lv, t;
    long long li, ti;
    int lane;
    __device__ __forceinline__ void init(int lane_, const float* __restrict__ val, const long long* __restrict__ idx) {
        lane = lane_;
        lv = -INFINITY;
        li = -1;
        if (val != nullptr && lane < KK) { lv = val[lane]; li = idx[lane]; }
        t = __shfl(lv, KK - 1, 64);
        ti = __shfl(li, KK - 1, 64);
    }
    __device__ __forceinline__ void offer(float cv, long long ci) {  // wave-uniform candidate
        if (!(cv > t || (cv == t && (ti < 0 || ci < ti)))) return;
        const bool ahead = lane < KK && (lv > cv || (lv == cv && li >= 0 && li < ci));
        const int pos = __popcll(__ballot(ahead));
        const float uv = __shfl_up(lv, 1, 64);
        const long long ui = __shfl_up(li, 1, 64);
        if (lane > pos) { lv = uv; li = ui; }
        if (lane == pos) { lv = cv; li = ci; }
        if (lane >= KK) { lv = -INFINITY; li = -1; }
        t = __shfl(lv, KK - 1, 64);
        ti = __shfl(li, KK - 1, 64);
    }
    // every lane's candidate (xc, ci) with ok set is offered, in lane order
    __device__ __forceinline__ void offer_lanes(bool ok, float xc, long long ci) {
        unsigned long long bal = __ballot(ok && xc >= t);
        while (bal) {
            const int src = __ffsll((long long)bal) - 1;
            bal &= bal - 1;
            offer(__shfl(xc, src, 64), __shfl(ci, src, 64));
        }
    }
    __device__ __forceinline__ void store(float* __restrict__ val, long long* __restrict__ idx) const {
        if (lane < KK) { val[lane] = lv; idx[lane] = li; }
    }
};

}  // namespace trid
