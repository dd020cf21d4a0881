// The grouped fp32-MFMA tile shared by the grouped-GEMM kernels (msda_heads.hip, msda_smoother.hip): a 64 x 64 output tile per
// 256-thread workgroup, 2 x 2 wavefronts of 32 x 32 (v_mfma_f32_32x32x2_f32, the lane / register layout of msda_gemm.hip), the
// reduction in stages of 32 through double-buffered LDS (one barrier per stage, next stage's global loads in flight during the
// MFMAs).  An operand is staged K-major ([64][32 + 4]) or MN-major ([32][64 + 4]) as it lies in memory, from 16-byte loads
// (VEC: rows whose length is a multiple of 4 floats) or 4-byte loads (any width).  Included inside an anonymous namespace.
#pragma once

constexpr int kHBlock = 256, kHT = 64, kHS = 32, kRowK = kHS + 4, kRowN = kHT + 4;
constexpr int kLdsK = kHT * kRowK, kLdsN = kHS * kRowN;
constexpr int kLds = kLdsK > kLdsN ? kLdsK : kLdsN;
using f32x16 = __attribute__((ext_vector_type(16))) float;

__device__ __forceinline__ int acc_row(int r, int g) { return (r & 3) + 8 * (r >> 2) + 4 * g; }

// ---- staging: 8 floats per thread and operand per stage ----------------------------------------------------------------
// K-major, 16-byte: row t/8 + 32u, k (t%8)*4 + 0..3.   K-major, 4-byte: row t/32 + 8u, k t%32.
// MN-major, 16-byte: k t/16 + 16u, col (t%16)*4 + 0..3. MN-major, 4-byte: k t/64 + 4u, col t%64.
template <bool KM, bool VEC>
__device__ __forceinline__ void stage_store(float *S, int t, const float (&r)[8])
{
#pragma unroll
    for (int u = 0; u < (VEC ? 2 : 8); ++u) {
        if (KM && VEC) *reinterpret_cast<float4 *>(&S[(t / 8 + 32 * u) * kRowK + (t % 8) * 4]) = make_float4(r[4 * u], r[4 * u + 1], r[4 * u + 2], r[4 * u + 3]);
        if (KM && !VEC) S[(t / 32 + 8 * u) * kRowK + t % 32] = r[u];
        if (!KM && VEC) *reinterpret_cast<float4 *>(&S[(t / 16 + 16 * u) * kRowN + (t % 16) * 4]) = make_float4(r[4 * u], r[4 * u + 1], r[4 * u + 2], r[4 * u + 3]);
        if (!KM && !VEC) S[(t / 64 + 4 * u) * kRowN + t % 64] = r[u];
    }
}

// lane (c, g) owns reduction indices 8i + 4g + t of the stage, t = 0..3 feeding 4 MFMAs (msda_gemm.hip)
template <bool KM>
__device__ __forceinline__ float4 frag(const float *S, int rc, int i, int g)
{
    if (KM) return *reinterpret_cast<const float4 *>(&S[rc * kRowK + 8 * i + 4 * g]);
    const float *p = &S[(8 * i + 4 * g) * kRowN + rc];
    return make_float4(p[0], p[kRowN], p[2 * kRowN], p[3 * kRowN]);
}

// The stage loop shared by the three GEMM kernels: `load(s, r_a, r_b)` fills the registers of stage s; `per_stage(buf)` runs
// after the MFMAs of a stage with that stage's LDS buffer still intact (the wgrad bias sums).
// BLOCKED: each stage's 32 reduction indices are summed on their own and added to the running total once (a long reduction
// of terms that cancel then loses about sqrt(stages) less than one running sum does; the weight gradients reduce over rows).
template <bool AKM, bool AVEC, bool BKM, bool BVEC, bool BLOCKED, class Load, class PerStage>
__device__ __forceinline__ f32x16 tile_loop_impl(float (*As)[kLds], float (*Bs)[kLds], int nstages, Load load, PerStage per_stage)
{
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int i0 = (wave >> 1) * 32, j0 = (wave & 1) * 32, g = lane >> 5, c = lane & 31;
    f32x16 acc, total;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = total[r] = 0.f;
    float ra[8], rb[8];
    load(0, ra, rb);
    stage_store<AKM, AVEC>(As[0], tid, ra);
    stage_store<BKM, BVEC>(Bs[0], tid, rb);
    __syncthreads();
    int cur = 0;
    for (int s = 0; s < nstages; ++s) {
        const bool more = s + 1 < nstages;                          // uniform
        if (more) load(s + 1, ra, rb);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float4 a = frag<AKM>(As[cur], i0 + c, i, g), b = frag<BKM>(Bs[cur], j0 + c, i, g);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b.x, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b.y, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b.z, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b.w, acc, 0, 0, 0);
        }
        if (BLOCKED) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                total[r] += acc[r];
                acc[r] = 0.f;
            }
        }
        per_stage(As[cur]);
        if (more) {
            stage_store<AKM, AVEC>(As[cur ^ 1], tid, ra);
            stage_store<BKM, BVEC>(Bs[cur ^ 1], tid, rb);
        }
        __syncthreads();
        cur ^= 1;
    }
    return BLOCKED ? total : acc;
}

template <bool AKM, bool AVEC, bool BKM, bool BVEC, class Load, class PerStage>
__device__ __forceinline__ f32x16 tile_loop(float (*As)[kLds], float (*Bs)[kLds], int nstages, Load load, PerStage per_stage)
{
    return tile_loop_impl<AKM, AVEC, BKM, BVEC, false>(As, Bs, nstages, load, per_stage);
}

struct NoStage {
    __device__ void operator()(const float *) const {}
};
