// The 64 x 64 staged bf16-MFMA tile loop the bf16-autocast GEMM kernels share (msda_heads_bf16.hip: the DETR prediction heads;
// msda_ffn_bf16.hip: the layers' FFN).  Every product runs on v_mfma_f32_16x16x32_bf16 with fp32 accumulation.
//
// 64 x 64 output tile per 256-thread workgroup, 2 x 2 wavefronts of 32 x 32 = 2 x 2 MFMA tiles of 16 x 16, reduction in stages
// of 32 (one MFMA step) through double-buffered LDS, one barrier per stage, the next stage's global loads in flight during the
// MFMAs.  An operand is staged as it lies in memory, 8 consecutive elements of one row per thread and stage, rounded to bf16
// (nearest even) on the way:
//   K-major (x, W of a forward, dy of a dgrad): LDS rows [64][kAbRow = 40], the fragment layout of msda_attn_tile.h: lane
//     (c, r) reads k = 8 r .. 8 r + 7 of row c with one ds_read_b128;
//   MN-major (W of a dgrad, dy and x of a wgrad): LDS rows [32][kTrRow = 72], read transposed with ds_read_b64_tr_b16 (ab_tr's
//     addressing on a 64-column row): lane (c, r) supplies 4 columns of row 8 r + c / 4 and receives rows 8 r .. 8 r + 3 of
//     column c; two reads give the 8 k of an MFMA operand.  The transposed read needs all 64 lanes: the stage loop is uniform.
#pragma once
#include "msda_attn_tile.h"

namespace msda {

constexpr int kBBlock = 256, kBT = 64, kBS = 32, kTrRow = kBT + 8;
constexpr int kBLds = kBT * kAbRow > kBS * kTrRow ? kBT * kAbRow : kBS * kTrRow;

__device__ __forceinline__ float bf_f(uint16_t x) { return __uint_as_float((unsigned)x << 16); }
__device__ __forceinline__ uint16_t f_bf(float x) { return __builtin_bit_cast(uint16_t, (__bf16)x); }    // nearest even
__device__ __forceinline__ float bf_round(float x) { return (float)(__bf16)x; }
__device__ __forceinline__ float ld_elem(const void *p, long long e, int bf16)
{
    return bf16 ? bf_f(static_cast<const uint16_t *>(p)[e]) : static_cast<const float *>(p)[e];
}
__device__ __forceinline__ uint4 pack8(const float (&v)[8])
{
    uint4 u;
    u.x = f_bf(v[0]) | ((unsigned)f_bf(v[1]) << 16);
    u.y = f_bf(v[2]) | ((unsigned)f_bf(v[3]) << 16);
    u.z = f_bf(v[4]) | ((unsigned)f_bf(v[5]) << 16);
    u.w = f_bf(v[6]) | ((unsigned)f_bf(v[7]) << 16);
    return u;
}
// 8 consecutive values of a row whose start is 16-byte (bf16) / 32-byte-per-8 (fp32: two 16-byte loads) aligned
__device__ __forceinline__ uint4 ld_row8(const void *p, long long e, int bf16)
{
    if (bf16) return *reinterpret_cast<const uint4 *>(static_cast<const uint16_t *>(p) + e);
    const float4 lo = ld4(static_cast<const float *>(p) + e), hi = ld4(static_cast<const float *>(p) + e + 4);
    const float v[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    return pack8(v);
}

// 8 packed bf16 of dy under the ReLU mask of 8 packed bf16 activations (`act > 0`: bit patterns 0x0001 .. 0x7f80)
__device__ __forceinline__ unsigned relu_mask2(unsigned a, unsigned act)
{
    const unsigned lo = act & 0xffffu, hi = act >> 16;
    return a & ((lo - 1u < 0x7f80u ? 0xffffu : 0u) | (hi - 1u < 0x7f80u ? 0xffff0000u : 0u));
}
__device__ __forceinline__ uint4 relu_mask8(const uint4 &a, const uint4 &act)
{
    return make_uint4(relu_mask2(a.x, act.x), relu_mask2(a.y, act.y), relu_mask2(a.z, act.z), relu_mask2(a.w, act.w));
}

// Staging slots.  K-major source: thread t holds row t / 4 (of 64), k 8 (t % 4) ..; MN-major source: k t / 8 (of 32), columns
// 8 (t % 8) ...  slot_row / slot_k name the (row of the source, first of the 8 elements along it).
template <bool KM>
__device__ __forceinline__ int slot_row(int t) { return KM ? t >> 2 : t >> 3; }
template <bool KM>
__device__ __forceinline__ int slot_k(int t) { return KM ? (t & 3) * 8 : (t & 7) * 8; }
template <bool KM>
__device__ __forceinline__ void stage_store(uint16_t *S, int t, const uint4 &v)
{
    *reinterpret_cast<uint4 *>(S + slot_row<KM>(t) * (KM ? kAbRow : kTrRow) + slot_k<KM>(t)) = v;
}

// the MFMA operand of lane (c, r) for the tile's rows / columns x0 .. x0 + 15: 8 k of row x0 + c (K-major), or the
// transposed read of column x0 + c (MN-major)
template <bool KM>
__device__ __forceinline__ at_bf8 operand(const uint16_t *S, int x0, int r, int c)
{
    if (KM) return ab_ld8(S + (x0 + c) * kAbRow + 8 * r);
    const uint16_t *p = S + (8 * r + (c >> 2)) * kTrRow + x0 + 4 * (c & 3);
    const at_bf4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((at_lds_bf4 *)p);
    const at_bf4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((at_lds_bf4 *)(p + 4 * kTrRow));
    return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}

// The stage loop: `load(s, a, b)` fills this thread's 8 bf16 of each operand for stage s; `per_stage(buf)` runs after the
// MFMAs of a stage with that stage's A buffer intact.  acc[ti][tj]: rows i0 + 16 ti + 4 r + v, column j0 + 16 tj + c.
template <bool AKM, bool BKM, class Load, class PerStage>
__device__ __forceinline__ void tile_loop(uint16_t (*As)[kBLds], uint16_t (*Bs)[kBLds], int nstages, Load load, PerStage per_stage,
                                          at_f4 (&acc)[2][2])
{
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int i0 = (wave >> 1) * 32, j0 = (wave & 1) * 32, r = lane >> 4, c = lane & 15;
#pragma unroll
    for (int ti = 0; ti < 2; ++ti)
#pragma unroll
        for (int tj = 0; tj < 2; ++tj) acc[ti][tj] = at_f4{0.f, 0.f, 0.f, 0.f};
    uint4 ra, rb;
    load(0, ra, rb);
    stage_store<AKM>(As[0], tid, ra);
    stage_store<BKM>(Bs[0], tid, rb);
    __syncthreads();
    int cur = 0;
    for (int s = 0; s < nstages; ++s) {
        const bool more = s + 1 < nstages;                          // uniform
        if (more) load(s + 1, ra, rb);
        const at_bf8 a0 = operand<AKM>(As[cur], i0, r, c), a1 = operand<AKM>(As[cur], i0 + 16, r, c);
        const at_bf8 b0 = operand<BKM>(Bs[cur], j0, r, c), b1 = operand<BKM>(Bs[cur], j0 + 16, r, c);
        acc[0][0] = ab_mfma(a0, b0, acc[0][0]);
        acc[0][1] = ab_mfma(a0, b1, acc[0][1]);
        acc[1][0] = ab_mfma(a1, b0, acc[1][0]);
        acc[1][1] = ab_mfma(a1, b1, acc[1][1]);
        per_stage(As[cur]);
        if (more) {
            stage_store<AKM>(As[cur ^ 1], tid, ra);
            stage_store<BKM>(Bs[cur ^ 1], tid, rb);
        }
        __syncthreads();
        cur ^= 1;
    }
}

struct NoStage {
    __device__ void operator()(const uint16_t *) const {}
};

}  // namespace msda
