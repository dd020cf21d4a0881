// Device helpers shared by the set criteria's kernel files (msda_criterion.hip, msda_criterion_dino.hip): the focal loss
// element and its derivative, the slot -> frame map of the reference's valid-frame pairing, the fixed-order block sum,
// torch's argmax rule, the hand-label test and a frame's target range.  Plain fp32 / fp64 with contraction off in both
// files, so either file gives the same bits.
#pragma once
#include <math.h>

#include "msda_common.h"
#include "msda_set_args.h"

#pragma clang fp contract(off)   // from here to the end of the including file: every product and sum rounds on its own

namespace msda {

// slot -> frame for every slot (every thread of the block calls it); wcnt holds one int per wave
static __device__ void cr_slot_frames(const int32_t *is_valid, int bs, int *frame_of, int *wcnt)
{
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, nw = blockDim.x >> 6;
    for (int k = tid; k < bs; k += blockDim.x) frame_of[k] = is_valid ? -1 : k;
    __syncthreads();
    if (!is_valid) return;
    int base = 0;
    for (int f0 = 0; f0 < bs; f0 += blockDim.x) {
        const int f = f0 + tid;
        const bool valid = f < bs && is_valid[f] != 0;
        const unsigned long long b = __ballot(valid);
        const int rank = __popcll(b & ((1ull << lane) - 1ull));
        if (lane == 0) wcnt[w] = __popcll(b);
        __syncthreads();
        int before = 0, total = 0;
        for (int x = 0; x < nw; ++x) {
            before += x < w ? wcnt[x] : 0;
            total += wcnt[x];
        }
        if (valid) frame_of[base + before + rank] = f;   // base + before + rank < bs
        base += total;
        __syncthreads();
    }
}

// a label whose keypoints are the hand head's (bit `label` of hand_mask)
__device__ __forceinline__ bool cr_hand(unsigned long long hand_mask, int label)
{
    return label < 64 && ((hand_mask >> label) & 1ull);
}

// The targets of frame f: true and [lo, hi) when the offsets describe them.
__device__ __forceinline__ bool cr_frame_targets(const SetTargets &tg, int f, long long &lo, long long &hi)
{
    lo = tg.offsets[f];
    hi = tg.offsets[f + 1];
    return !(lo < 0 || hi < lo || hi > tg.n_targets);
}

// torch's sigmoid_focal_loss element (binary_cross_entropy_with_logits via log_sigmoid), t in {0, 1}
__device__ __forceinline__ float cr_focal(float x, float t, float alpha)
{
    const float p = 1.f / (1.f + expf(-x));
    const float ls = fminf(x, 0.f) - log1pf(expf(-fabsf(x)));
    const float ce = (1.f - t) * x - ls;
    const float pt = p * t + (1.f - p) * (1.f - t);
    const float om = 1.f - pt;
    const float at = alpha * t + (1.f - alpha) * (1.f - t);
    return at * (ce * (om * om));
}

// its derivative in x
__device__ __forceinline__ float cr_focal_grad(float x, bool pos, float alpha)
{
    const float p = 1.f / (1.f + expf(-x));
    const float l1p = log1pf(expf(-fabsf(x)));
    if (pos) {   // d/dx of alpha (1-p)^2 softplus(-x)
        const float q = 1.f - p;
        return -alpha * (q * q) * (q + 2.f * p * (fmaxf(-x, 0.f) + l1p));
    }
    return (1.f - alpha) * (p * p) * (p + 2.f * (fmaxf(x, 0.f) + l1p) * (1.f - p));   // (1-alpha) p^2 softplus(x)
}

// torch's argmax over a row
__device__ __forceinline__ int cr_argmax(const float *x, int K)
{
    int best = 0;
    float bv = x[0];
    for (int c = 1; c < K; ++c) {
        const float v = x[c];
        if (v > bv || (v != v && bv == bv)) { bv = v; best = c; }   // torch: NaN is the maximum; ties keep the first
    }
    return best;
}

// Block sum in a fixed order (every thread gets it); `red` holds one value per wave and is not reused.
static __device__ double cr_block_sum(double x, double *red)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
    x = wave_sum(x);
    if (lane == 0) red[w] = x;
    __syncthreads();
    double t = 0.0;
    for (int i = 0; i < nw; ++i) t += red[i];   // in order: every thread gets the same value
    return t;
}

}  // namespace msda
