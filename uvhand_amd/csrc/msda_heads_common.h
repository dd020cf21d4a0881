// Device helpers the two forms of the DETR prediction heads share (msda_heads.hip, msda_heads_bf16.hip): which problem and which
// column group of the launch's table a workgroup or a column belongs to, and the fp32 reference offsets of the keypoint
// epilogues.  The problem tables themselves are msda_launch.h's.
#pragma once
#include "msda_launch.h"

namespace msda {

// the reference's inverse_sigmoid (util/misc.py:614-618)
__device__ __forceinline__ float inv_sigmoid(float x)
{
    x = fminf(fmaxf(x, 0.f), 1.f);
    const float x1 = fmaxf(x, 1e-5f), x2 = fmaxf(1.f - x, 1e-5f);
    return logf(x1 / x2);
}

// the problem of table P that owns this workgroup: the last one whose first workgroup (tile0) is not behind blockIdx.x
template <class Args>
__device__ __forceinline__ int heads_problem(const Args &P)
{
    int pi = 0;
    while (pi + 1 < P.nprob && (int)blockIdx.x >= P.p[pi + 1].tile0) ++pi;
    return pi;
}

// the column group of forward problem p that owns its column j
__device__ __forceinline__ int heads_group(const HeadsFwdArgs &P, const HeadsFwdProb &p, int j)
{
    int gi = p.g0;
    while (gi + 1 < p.g0 + p.ng && j >= P.g[gi + 1].off) ++gi;
    return gi;
}

// AssemblyHands keypoints: the x / y offsets of each row of the tile at row m0 (models/assembly_detr.py:172-199): the reference
// point (2-d) or the means of the 21 x and 21 y values (42-d), after inverse_sigmoid; levels >= 1 map r -> (r + 0.5) / 2 first.
// fp32 in both forms.  Every thread of the workgroup calls it; refoff is complete when it returns.
__device__ __forceinline__ void heads_refoff(const HeadsFwdArgs &P, const HeadsFwdProb &p, int m0, float (*refoff)[2])
{
    const int tid = threadIdx.x;
    if (tid < 2 * kHeadsTile) {
        const int row = tid >> 1, coord = tid & 1, gr = p.row0 + m0 + row;
        float v = 0.f;
        if (m0 + row < p.rows) {
            const bool first = gr < P.M;
            const float *ref = first ? P.init_ref + (long long)gr * P.R : P.inter_ref + (long long)(gr - P.M) * P.R;
            if (P.R == 2) {
                const float r = ref[coord];
                v = inv_sigmoid(first ? r : (r + 0.5f) / 2.f);
            } else {
                float sum = 0.f;
                for (int q = 0; q < P.R / 2; ++q) {
                    const float r = ref[2 * q + coord];
                    sum += inv_sigmoid(first ? r : (r + 0.5f) / 2.f);
                }
                v = sum / (float)(P.R / 2);
            }
        }
        refoff[row][coord] = v;
    }
    __syncthreads();
}

}  // namespace msda
