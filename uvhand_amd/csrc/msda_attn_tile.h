// MFMA fragment helpers of the head_dim-32 attention cores (msda_attn.hip: the decoder's self-attention; msda_swin.hip: Swin
// window attention): 16 x 16 score tiles of one (batch, head) pair whose operands sit in LDS, a lane being (c = lane & 15,
// r = lane >> 4).  The score tile never changes layout between the two products it takes part in.
//
// fp32 (at_*): operands in LDS row-major as [rows][kAtRow = 36 floats] (16-byte aligned rows, the 16 lanes of a ds_read_b128 on
// different bank groups), every product on v_mfma_f32_16x16x4_f32 (fp32 in, fp32 accumulate: the arithmetic of an fmaf chain).
//   * forward and dQ work on S^T tiles (rows = keys, columns = queries).  The accumulator of a 16 x 16 tile gives lane
//     (c = lane & 15, r = lane >> 4) the entries [4r .. 4r+3][c]; the following product sums over KEYS, and a sum does not care
//     in which order its terms arrive: MFMA step v of a tile takes "k index r" to mean key 4r + v, so the B operand is the
//     accumulator register v as it stands and the A operand is row 4r + v of V (or K) in LDS.  No transposition through LDS,
//     no shuffles.
//   * dK / dV work on S tiles (rows = queries, columns = keys) and sum over QUERIES the same way.
//   * the head dimension is relabelled likewise (step (half, v): k index r = channel 16 half + 4r + v), so the operand whose
//     row index is the lane's column reads four steps with one ds_read_b128 / one float4 global load.
//
// bf16 (ab_*): operands in LDS as bf16 rows [rows][kAbRow = 40] (80-byte rows, 16-byte aligned), every product on
// v_mfma_f32_16x16x32_bf16 (fp32 accumulate): one instruction covers a score tile's whole head dimension.  The rows are read two
// ways: a row (8 channels of one key / query) with one ds_read_b128 as the operand of the products over channels, and transposed
// (4 keys / queries of one channel) with ds_read_b64_tr_b16 as the operand of the products over keys / queries.  The transposed
// read needs all 64 lanes active: every loop around ab_tr is wave-uniform.
// Relabelling.  A bf16 operand holds 8 consecutive k per lane (k = 8 (lane >> 4) + j), an accumulator 4 rows per lane (4 (lane >> 4)
// + v).  The score tiles come in pairs b = 0, 1 covering 32 keys (or queries) 32T .. 32T + 31, and tile b's row i is taken to
// be key 32T + 8 (i >> 2) + 4b + (i & 3): the row operand of the first product is read for that key, so the accumulators of the
// pair give lane (c, r) keys 32T + 8r + j in natural order (j = 4b + v) — exactly the 8 k of the next product's operand.
// Rows up to a multiple of 32 are zero in LDS.
#pragma once
#include <math.h>

#include "msda_common.h"

namespace msda {

constexpr int kAtRow = 36, kAbRow = 40;
using at_f4 = __attribute__((ext_vector_type(4))) float;
using at_bf8 = __attribute__((ext_vector_type(8))) __bf16;
using at_bf4 = __attribute__((ext_vector_type(4))) __bf16;
typedef __attribute__((address_space(3))) at_bf4 at_lds_bf4;

__device__ __forceinline__ at_f4 at_mfma(float a, float b, at_f4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
__device__ __forceinline__ at_f4 ab_mfma(at_bf8 a, at_bf8 b, at_f4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }

// ---- the dropout hash (msda_attn.hip: attention dropout; msda_ffn_bf16.hip: the FFN's) -------------------------------------
// 32 bits per element: a counter + mix — mix = seed and pair, uniform — through the two multiply-xorshift rounds of the usual
// 32-bit finalizer; its last xor-shift is left out (it only folds high bits into low ones, and the result is compared with a
// threshold).  v_mul_lo_u32 is a quarter-rate instruction and the vector unit is as busy as the matrix pipe in these kernels:
// a lane adds its part of the counter once per tile, an element one constant.
__device__ __forceinline__ unsigned at_mix(unsigned long long seed, unsigned pair)
{
    return (unsigned)seed + pair * 0x9E3779B1u + (unsigned)(seed >> 32) * 0x85EBCA6Bu;
}
__device__ __forceinline__ unsigned at_hash(unsigned counter)
{
    unsigned x = counter;
    x ^= x >> 16; x *= 0x85EBCA6Bu;
    x ^= x >> 13; x *= 0xC2B2AE35u;
    return x;
}

// ---- fp32 ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float4 at_zero4() { return make_float4(0.f, 0.f, 0.f, 0.f); }

// acc += A-rows(tile) . breg over the 32 channels: `arow` = LDS row of this lane's A row (channels 4r.. of each half at +0, +16)
__device__ __forceinline__ at_f4 at_dot32(const float *arow, const float4 &b0, const float4 &b1)
{
    const float4 a0 = ld4(arow), a1 = ld4(arow + 16);
    at_f4 acc = {0.f, 0.f, 0.f, 0.f};
    acc = at_mfma(a0.x, b0.x, acc); acc = at_mfma(a0.y, b0.y, acc); acc = at_mfma(a0.z, b0.z, acc); acc = at_mfma(a0.w, b0.w, acc);
    acc = at_mfma(a1.x, b1.x, acc); acc = at_mfma(a1.y, b1.y, acc); acc = at_mfma(a1.z, b1.z, acc); acc = at_mfma(a1.w, b1.w, acc);
    return acc;                                      // (one chain: the sum's association is the channel order)
}

// the same for this tile and the next one (16 rows further), the two accumulators' chains interleaved
__device__ __forceinline__ void at_dot32x2(const float *arow, const float4 &b0, const float4 &b1, at_f4 &acc0, at_f4 &acc1)
{
    const float4 a0 = ld4(arow), a1 = ld4(arow + 16), c0 = ld4(arow + 16 * kAtRow), c1 = ld4(arow + 16 * kAtRow + 16);
    at_f4 x = {0.f, 0.f, 0.f, 0.f}, y = x;
    x = at_mfma(a0.x, b0.x, x); y = at_mfma(c0.x, b0.x, y); x = at_mfma(a0.y, b0.y, x); y = at_mfma(c0.y, b0.y, y);
    x = at_mfma(a0.z, b0.z, x); y = at_mfma(c0.z, b0.z, y); x = at_mfma(a0.w, b0.w, x); y = at_mfma(c0.w, b0.w, y);
    x = at_mfma(a1.x, b1.x, x); y = at_mfma(c1.x, b1.x, y); x = at_mfma(a1.y, b1.y, x); y = at_mfma(c1.y, b1.y, y);
    x = at_mfma(a1.z, b1.z, x); y = at_mfma(c1.z, b1.z, y); x = at_mfma(a1.w, b1.w, x); y = at_mfma(c1.w, b1.w, y);
    acc0 = x; acc1 = y;
}

// o[half] += X^T-rows . w over the tile's 16 rows: X = LDS tile base (row 16t), w = accumulator-layout weights of this lane
__device__ __forceinline__ void at_accum_t(const float *xt, int r, int c, const at_f4 &w, at_f4 &o0, at_f4 &o1)
{
#pragma unroll
    for (int v = 0; v < 4; ++v) {
        const float *row = xt + (4 * r + v) * kAtRow + c;
        o0 = at_mfma(row[0], w[v], o0);
        o1 = at_mfma(row[16], w[v], o1);
    }
}

__device__ __forceinline__ float at_rsum(float x)               // over the four lanes c, c + 16, c + 32, c + 48
{
    x += __shfl_xor(x, 16);
    x += __shfl_xor(x, 32);
    return x;
}
__device__ __forceinline__ float at_rmax(float x)
{
    x = fmaxf(x, __shfl_xor(x, 16));
    x = fmaxf(x, __shfl_xor(x, 32));
    return x;
}

// ---- the log-sum-exp across the ABI (resident fp32 and streaming cores) ----------------------------------------------------------
// The log-sum-exp crosses the ABI as an fp32 natural logarithm and the kernels work in base 2.  A plain product on each side
// would add a rounding of ulp(lse) / 2 twice to EVERY exponent of a row — a common factor of about 2e-7 on the row's
// probabilities and gradients; both conversions therefore carry the product's low part.
// forward: (m + l) * ln 2 rounded once (m + l by a two-sum, the constant as hi + lo)
__device__ __forceinline__ float at_lse_natural(float m, float l)
{
    const float t = m + l;
    if (!(fabsf(t) < INFINITY)) return t;               // (-inf: every key hidden)
    const float bb = t - m, e = (m - (t - bb)) + (l - bb);
    return fmaf(t, 0.693147182464599609375f, fmaf(t, -1.904654299957e-9f, e * 0.693147182464599609375f));
}
// backward: lse * log2 e as hi + lo; a score's exponent is (s - hi) - lo.  +inf (rows past Lq) stays (+inf, 0).
__device__ __forceinline__ void at_lse_base2(float lse, float &hi, float &lo)
{
    hi = lse * 1.44269502162933349609375f;
    lo = fabsf(hi) < INFINITY ? fmaf(lse, 1.44269502162933349609375f, -hi) + lse * 1.925963033500e-8f : 0.f;
}

// ---- bf16 ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ at_bf8 ab_ld8(const uint16_t *p) { return *reinterpret_cast<const at_bf8 *>(p); }
__device__ __forceinline__ at_bf8 ab_zero8() { return at_bf8{}; }
__device__ __forceinline__ float ab_f(__bf16 x) { return (float)x; }

// the score-tile pair T: acc[b] = rows(X) . bop over the 32 channels, X = LDS slice, rows relabelled as above
__device__ __forceinline__ void ab_pair(const uint16_t *xs, int T, int r, int c, const at_bf8 &bop, at_f4 &acc0, at_f4 &acc1)
{
    const uint16_t *row = xs + (32 * T + 8 * (c >> 2) + (c & 3)) * kAbRow + 8 * r;
    const at_bf8 a0 = ab_ld8(row), a1 = ab_ld8(row + 4 * kAbRow);
    const at_f4 z = {0.f, 0.f, 0.f, 0.f};
    acc0 = ab_mfma(a0, bop, z);
    acc1 = ab_mfma(a1, bop, z);
}

// the transposed operand: lane (c, r) gets X[32T + 8r + j][16 half + c], j = 0..7 (X = LDS slice, rows = keys / queries)
__device__ __forceinline__ at_bf8 ab_tr(const uint16_t *xs, int T, int half, int r, int c)
{
    const uint16_t *p = xs + (32 * T + 8 * r + (c >> 2)) * kAbRow + 16 * half + 4 * (c & 3);
    const at_bf4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((at_lds_bf4 *)p);
    const at_bf4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((at_lds_bf4 *)(p + 4 * kAbRow));
    return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}

__device__ __forceinline__ at_bf8 ab_pack(const at_f4 &x0, const at_f4 &x1)
{
    return at_bf8{(__bf16)x0[0], (__bf16)x0[1], (__bf16)x0[2], (__bf16)x0[3], (__bf16)x1[0], (__bf16)x1[1], (__bf16)x1[2], (__bf16)x1[3]};
}

// 4 accumulator values (scaled) -> 4 bf16 at p (8 bytes)
__device__ __forceinline__ void ab_st4(uint16_t *p, const at_f4 &x, float s)
{
    *reinterpret_cast<at_bf4 *>(p) = at_bf4{(__bf16)(x[0] * s), (__bf16)(x[1] * s), (__bf16)(x[2] * s), (__bf16)(x[3] * s)};
}

}  // namespace msda
