// Masked, long-sequence form of the decoder self-attention core (msda_attn32x_*_f32, include/msda.h):
//     out = dropout(softmax(q k^T * scale + M), p) v,   head_dim 32, fp32, 1 <= Lq, Lk <= 2048, M = -inf where mask != 0.
// The DINO decoder (models/dino/deformable_transformer.py:966) runs nn.MultiheadAttention over pad_size + num_queries rows
// (about 200 + 900) under the contrastive-denoising mask of models/dino/dn_components.py:125-137.  One (batch, head) pair's K
// and V in msda_attn.hip's resident [rows][36 floats] layout would take 317 KB of LDS at 1100 rows; a CU has 160 KB.  So these
// kernels STREAM the other operand through LDS in chunks of kAxChunk = 64 rows, and several workgroups share a pair:
//   * forward and dQ: a workgroup of 8 wavefronts owns kAxRows = 128 queries (16 per wavefront) and walks the key chunks.
//     The forward keeps an online softmax per query (running maximum m, running sum, O rescaled by 2^(m_old - m_new) at each
//     chunk) and normalises once at the end; dQ recomputes the probabilities from the forward's log-sum-exp.
//   * dK / dV: a workgroup owns 128 keys and walks the query chunks; delta = rowsum(dO * O) and the log-sum-exp of a chunk's
//     queries are formed while the chunk is loaded.
// LDS: two [64][36] fp32 slices = 18 KB (dK / dV: + 768 B) — under the 64 KB that need no opt-in, eight workgroups to a CU.
// Every product runs on v_mfma_f32_16x16x4_f32 through the fragment helpers of msda_attn_tile.h, in msda_attn.hip's layouts:
// S^T tiles (rows = keys) in the forward and dQ, S tiles (rows = queries) in dK / dV.  No atomics; every sum has one fixed order
// (chunks in order, tiles in order), so all three kernels are bitwise reproducible.
// Mask: bytes [Lq][Lk], row stride mask_sq, shared by every pair; nonzero = hidden.  A hidden entry's score is -inf in the
// forward and its probability and dS are exactly 0 in the backward (selected, not computed), so a hidden key receives exactly
// nothing from the rows that cannot see it.  A query with every key hidden has sum = 0: its out row is 0 * inf = NaN, as the
// module's, its lse -inf; no other row sees it (the product sums over keys within a query's column).  Its gradients are outside
// the contract.
// Long sums (ax_tile_sums): a 16-row tile's product starts from a zero accumulator and the tile's partial is added to the running
// result on the vector unit, so a sum over 2048 rows is 128 rounded additions of partials, not a chain of 512 dependent MFMA
// accumulations — dV of a query block that attends to one key is a plain sum of its dO rows, and the chain measured 5 ulp there.
// Hidden tiles: dQ skips a 16 x 16 tile that the mask hides from all 16 queries of its wavefront (one ballot per tile, only when
// a mask is given; rows past Lq count as hidden).  The tile's dS are exact zeros and its partial product +0, so no result bit
// changes (checked against a build without the skip).  At 1098 rows under the denoising mask dQ went from 824 to 690 us.  The
// same skip in the forward and in dK / dV was measured and left out: 601 -> 590 and 1149 -> 1131 us masked, but 349 -> 389
// and 650 -> 678 us at 900 rows unmasked (the forward then holds the tiles' mask bits across its products: 90 VGPRs against 80).
// Dropout: msda_attn.hip's hash and counter — at_hash((query << 16) + key + at_mix(seed, pair)) — seed read from device memory.
// The bf16 form for bf16 autocast (msda_attn32x_*_bf16) follows the fp32 kernels below.
#include <math.h>
#include <string.h>

#include "msda_attn_args.h"
#include "msda_attn_tile.h"
#include "msda_common.h"
#include "msda_launch.h"

namespace msda {

constexpr int kAxWaves = 8, kAxBlock = kAxWaves * 64, kAxRows = kAxWaves * 16, kAxChunk = 64, kAxTiles = kAxChunk / 16;
constexpr int kAxMaxLen = 2048;
static_assert(kAxChunk * 8 == kAxBlock, "one float4 per thread and slice in ax_load_chunk2");

// rows [row0, row0 + kAxChunk) of two [L][32] slices -> dst0 / dst1 [kAxChunk][kAtRow]; rows past L zero
__device__ __forceinline__ void ax_load_chunk2(float *dst0, const float *src0, long long sl0, float *dst1, const float *src1,
                                               long long sl1, int row0, int L)
{
    const int row = threadIdx.x >> 3, c = (threadIdx.x & 7) * 4, g = row0 + row;
    const bool live = g < L;
    const float4 v0 = live ? ld4(src0 + (long long)g * sl0 + c) : at_zero4();
    const float4 v1 = live ? ld4(src1 + (long long)g * sl1 + c) : at_zero4();
    *reinterpret_cast<float4 *>(dst0 + row * kAtRow + c) = v0;
    *reinterpret_cast<float4 *>(dst1 + row * kAtRow + c) = v1;
}

// bit v set: key0 + v is hidden from this lane's query (mrow = its mask row, or null) or lies past Lk
__device__ __forceinline__ unsigned ax_hidden4(const unsigned char *mrow, int key0, int Lk)
{
    unsigned bits = 0;
    if (key0 + 3 < Lk) {
        if (mrow) {
            unsigned w;
            memcpy(&w, mrow + key0, 4);                 // (no alignment promised: mask_sq is any length)
            bits = ((w & 0xffu) ? 1u : 0u) | ((w & 0xff00u) ? 2u : 0u) | ((w & 0xff0000u) ? 4u : 0u) | ((w & 0xff000000u) ? 8u : 0u);
        }
    } else {
#pragma unroll
        for (int v = 0; v < 4; ++v)
            if (key0 + v >= Lk || (mrow && mrow[key0 + v])) bits |= 1u << v;
    }
    return bits;
}

// (the log-sum-exp crosses the ABI as an fp32 natural logarithm: at_lse_natural / at_lse_base2, msda_attn_tile.h)

// at_dot32 as four chains of two MFMA steps (eight channels each, every chain from a zero accumulator) summed pairwise on the
// vector unit.  dP = dO . v reaches |13| at unit-variance inputs, and every step of at_dot32's one chain of eight rounds at that
// magnitude: measured against fp64, the single chain left dq / dk of a one-query problem at up to 4.9 times torch's fp32 error,
// the split at up to 3.1.  The four chains are independent: the matrix pipe overlaps them.
__device__ __forceinline__ at_f4 ax_dot32(const float *arow, const float4 &b0, const float4 &b1)
{
    const float4 a0 = ld4(arow), a1 = ld4(arow + 16);
    const at_f4 z = {0.f, 0.f, 0.f, 0.f};
    at_f4 w = at_mfma(a0.x, b0.x, z), x = at_mfma(a0.z, b0.z, z), y = at_mfma(a1.x, b1.x, z), u = at_mfma(a1.z, b1.z, z);
    w = at_mfma(a0.y, b0.y, w); x = at_mfma(a0.w, b0.w, x); y = at_mfma(a1.y, b1.y, y); u = at_mfma(a1.w, b1.w, u);
    return (w + x) + (y + u);
}

__device__ __forceinline__ void ax_scale4(float4 &x, float s) { x.x *= s; x.y *= s; x.z *= s; x.w *= s; }

__global__ __launch_bounds__(kAxBlock) void attn32x_fwd_kernel(const AttnArgs<float> a)
{
    __shared__ __attribute__((aligned(16))) float Ks[kAxChunk * kAtRow], Vs[kAxChunk * kAtRow];
    const int pair = (int)blockIdx.x / a.wpp, blk = (int)blockIdx.x % a.wpp, n = pair / a.H, h = pair % a.H;
    const unsigned mix = at_mix(a.thresh ? a.seed[0] : 0ull, (unsigned)pair);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, c = lane & 15, r = lane >> 4;
    const int qi = blk * kAxRows + wave * 16 + c;
    const bool qok = qi < a.Lq;
    float4 q0 = at_zero4(), q1 = at_zero4();
    if (qok) {
        const float *qr = a.q.p + n * a.q.sn + h * 32 + (long long)qi * a.q.sl + 4 * r;
        q0 = ld4(qr); q1 = ld4(qr + 16);
    }
    ax_scale4(q0, a.scale2); ax_scale4(q1, a.scale2);
    const unsigned char *mrow = (a.mask && qok) ? a.mask + (long long)qi * a.mask_sq : nullptr;
    const float *kp = a.k.p + n * a.k.sn + h * 32, *vp = a.v.p + n * a.v.sn + h * 32;
    const unsigned ctr = ((unsigned)qi << 16) + 4 * r + mix;
    float m = -INFINITY, sum = 0.f;                     // running maximum (base 2) of the query; this lane's share of the sum
    at_f4 o0 = {0.f, 0.f, 0.f, 0.f}, o1 = o0;
    for (int k0 = 0; k0 < a.Lk; k0 += kAxChunk) {
        __syncthreads();                                // (the last chunk's readers are done)
        ax_load_chunk2(Ks, kp, a.k.sl, Vs, vp, a.v.sl, k0, a.Lk);
        __syncthreads();
        const int nt = min(kAxTiles, (a.Lk - k0 + 15) >> 4);
        // S^T tiles: s[t][v] = score (times log2 e) of key k0 + 16 t + 4 r + v for query qi
        at_f4 s[kAxTiles];
#pragma unroll
        for (int t = 0; t < kAxTiles; ++t)
            if (t < nt) s[t] = ax_dot32(Ks + (16 * t + c) * kAtRow + 4 * r, q0, q1);
        float cm = -INFINITY;
#pragma unroll
        for (int t = 0; t < kAxTiles; ++t) {
            if (t < nt) {
                const unsigned hid = ax_hidden4(mrow, k0 + 16 * t + 4 * r, a.Lk);
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    s[t][v] = (hid >> v & 1u) ? -INFINITY : s[t][v];
                    cm = fmaxf(cm, s[t][v]);
                }
            }
        }
        const float m_new = fmaxf(m, at_rmax(cm));
        const float m_ref = m_new == -INFINITY ? 0.f : m_new;       // (nothing visible yet: every term below is exp2(-inf) = 0)
        const float alpha = __builtin_amdgcn_exp2f(m - m_ref);
        sum *= alpha;
        o0 *= alpha; o1 *= alpha;
        m = m_new;
#pragma unroll
        for (int t = 0; t < kAxTiles; ++t) {
            if (t < nt) {
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    const float p = __builtin_amdgcn_exp2f(s[t][v] - m_ref);
                    sum += p;
                    const bool keep = at_hash(ctr + (unsigned)(k0 + 16 * t + v)) >= a.thresh;      // (thresh 0: always)
                    s[t][v] = keep ? p : 0.f;
                }
                at_f4 t0 = {0.f, 0.f, 0.f, 0.f}, t1 = t0;
                at_accum_t(Vs + 16 * t * kAtRow, r, c, s[t], t0, t1);       // O^T[channel][query] += V^T . P (ax_tile_sums)
                o0 += t0; o1 += t1;
            }
        }
    }
    sum = at_rsum(sum);
    if (qok) {
        if (r == 0) a.lse[(long long)pair * a.Lq + qi] = at_lse_natural(m, __builtin_amdgcn_logf(sum));
        const float inv = a.keep_scale / sum;           // (sum 0 — every key hidden: inf, and the row 0 * inf = NaN)
        float *orow = a.o.p + n * a.o.sn + h * 32 + (long long)qi * a.o.sl + 4 * r;
        *reinterpret_cast<float4 *>(orow) = make_float4(o0[0] * inv, o0[1] * inv, o0[2] * inv, o0[3] * inv);
        *reinterpret_cast<float4 *>(orow + 16) = make_float4(o1[0] * inv, o1[1] * inv, o1[2] * inv, o1[3] * inv);
    }
}

// dK, dV: a wavefront owns 16 keys; the workgroup walks the query chunks
__global__ __launch_bounds__(kAxBlock) void attn32x_bwd_kv_kernel(const AttnArgs<float> a)
{
    __shared__ __attribute__((aligned(16))) float Qs[kAxChunk * kAtRow], Gs[kAxChunk * kAtRow], lse_s[kAxChunk], lsl_s[kAxChunk],
        del_s[kAxChunk];
    const int pair = (int)blockIdx.x / a.wpp, blk = (int)blockIdx.x % a.wpp, n = pair / a.H, h = pair % a.H;
    const unsigned mix = at_mix(a.thresh ? a.seed[0] : 0ull, (unsigned)pair);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, c = lane & 15, r = lane >> 4;
    const int key = blk * kAxRows + wave * 16 + c;
    const bool kok = key < a.Lk;
    float4 k0 = at_zero4(), k1 = at_zero4(), v0 = at_zero4(), v1 = at_zero4();
    if (kok) {
        const float *kr = a.k.p + n * a.k.sn + h * 32 + (long long)key * a.k.sl + 4 * r;
        const float *vr = a.v.p + n * a.v.sn + h * 32 + (long long)key * a.v.sl + 4 * r;
        k0 = ld4(kr); k1 = ld4(kr + 16); v0 = ld4(vr); v1 = ld4(vr + 16);
    }
    ax_scale4(k0, a.scale2); ax_scale4(k1, a.scale2);
    const unsigned char *mcol = (a.mask && kok) ? a.mask + key : nullptr;
    const float *qp = a.q.p + n * a.q.sn + h * 32, *gp = a.go.p + n * a.go.sn + h * 32, *op = a.o.p + n * a.o.sn + h * 32;
    const unsigned ctr = (unsigned)key + ((unsigned)(4 * r) << 16) + mix;
    at_f4 dv0 = {0.f, 0.f, 0.f, 0.f}, dv1 = dv0, dk0 = dv0, dk1 = dv0;
    for (int c0 = 0; c0 < a.Lq; c0 += kAxChunk) {
        __syncthreads();
        ax_load_chunk2(Qs, qp, a.q.sl, Gs, gp, a.go.sl, c0, a.Lq);
        // per query of the chunk: delta = <dO, O> — four threads a query, the dQ kernel's terms in the dQ kernel's order — and
        // the log-sum-exp in base 2 (+inf for the rows past Lq: their probabilities vanish)
        if (threadIdx.x < 4 * kAxChunk) {               // (whole wavefronts)
            const int ql = threadIdx.x >> 2, part = threadIdx.x & 3, g = c0 + ql;
            float d = 0.f;
            if (g < a.Lq) {
                const float *gr = gp + (long long)g * a.go.sl + 4 * part, *orw = op + (long long)g * a.o.sl + 4 * part;
                const float4 g0 = ld4(gr), g1 = ld4(gr + 16), o0 = ld4(orw), o1 = ld4(orw + 16);
                d = g0.x * o0.x + g0.y * o0.y + g0.z * o0.z + g0.w * o0.w + g1.x * o1.x + g1.y * o1.y + g1.z * o1.z + g1.w * o1.w;
            }
            d += __shfl_xor(d, 1);
            d += __shfl_xor(d, 2);
            if (part == 0) {
                float hi, lo;
                at_lse_base2(g < a.Lq ? a.lse[(long long)pair * a.Lq + g] : INFINITY, hi, lo);
                del_s[ql] = d; lse_s[ql] = hi; lsl_s[ql] = lo;
            }
        }
        __syncthreads();
        const int nt = min(kAxTiles, (a.Lq - c0 + 15) >> 4);
        // S and dP tiles: entry v = (query c0 + 16 t + 4 r + v, key)
#pragma unroll 1
        for (int t = 0; t < nt; ++t) {
            const at_f4 s = ax_dot32(Qs + (16 * t + c) * kAtRow + 4 * r, k0, k1);
            const at_f4 dp = ax_dot32(Gs + (16 * t + c) * kAtRow + 4 * r, v0, v1);
            const float4 ls = ld4(lse_s + 16 * t + 4 * r), ll = ld4(lsl_s + 16 * t + 4 * r), dl = ld4(del_s + 16 * t + 4 * r);
            const float lsv[4] = {ls.x, ls.y, ls.z, ls.w}, llv[4] = {ll.x, ll.y, ll.z, ll.w}, dlv[4] = {dl.x, dl.y, dl.z, dl.w};
            const int qrow = c0 + 16 * t + 4 * r;
            at_f4 pd, ds;
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const bool hid = mcol != nullptr && qrow + v < a.Lq && mcol[(long long)(qrow + v) * a.mask_sq] != 0;
                const float p = hid ? 0.f : __builtin_amdgcn_exp2f((s[v] - lsv[v]) - llv[v]);
                const bool keep = at_hash(ctr + ((unsigned)(c0 + 16 * t + v) << 16)) >= a.thresh;
                pd[v] = keep ? p * a.keep_scale : 0.f;
                ds[v] = hid ? 0.f : p * ((keep ? dp[v] * a.keep_scale : 0.f) - dlv[v]);
            }
            at_f4 tv0 = {0.f, 0.f, 0.f, 0.f}, tv1 = tv0, tk0 = tv0, tk1 = tv0;
            at_accum_t(Gs + 16 * t * kAtRow, r, c, pd, tv0, tv1);           // dV^T[channel][key] += dO^T . P_drop
            at_accum_t(Qs + 16 * t * kAtRow, r, c, ds, tk0, tk1);           // dK^T[channel][key] += Q^T . dS
            dv0 += tv0; dv1 += tv1; dk0 += tk0; dk1 += tk1;
        }
    }
    if (kok) {
        float *gvr = a.gv.p + n * a.gv.sn + h * 32 + (long long)key * a.gv.sl + 4 * r;
        float *gkr = a.gk.p + n * a.gk.sn + h * 32 + (long long)key * a.gk.sl + 4 * r;
        *reinterpret_cast<float4 *>(gvr) = make_float4(dv0[0], dv0[1], dv0[2], dv0[3]);
        *reinterpret_cast<float4 *>(gvr + 16) = make_float4(dv1[0], dv1[1], dv1[2], dv1[3]);
        *reinterpret_cast<float4 *>(gkr) = make_float4(dk0[0] * a.scale, dk0[1] * a.scale, dk0[2] * a.scale, dk0[3] * a.scale);
        *reinterpret_cast<float4 *>(gkr + 16) = make_float4(dk1[0] * a.scale, dk1[1] * a.scale, dk1[2] * a.scale, dk1[3] * a.scale);
    }
}

// dQ: a wavefront owns 16 queries; the workgroup walks the key chunks (S^T tiles, as the forward)
__global__ __launch_bounds__(kAxBlock) void attn32x_bwd_q_kernel(const AttnArgs<float> a)
{
    __shared__ __attribute__((aligned(16))) float Ks[kAxChunk * kAtRow], Vs[kAxChunk * kAtRow];
    const int pair = (int)blockIdx.x / a.wpp, blk = (int)blockIdx.x % a.wpp, n = pair / a.H, h = pair % a.H;
    const unsigned mix = at_mix(a.thresh ? a.seed[0] : 0ull, (unsigned)pair);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, c = lane & 15, r = lane >> 4;
    const int qi = blk * kAxRows + wave * 16 + c;
    const bool qok = qi < a.Lq;
    float4 q0 = at_zero4(), q1 = at_zero4(), g0 = at_zero4(), g1 = at_zero4(), o0 = at_zero4(), o1 = at_zero4();
    float lse_n = INFINITY;                             // (rows past Lq: probabilities vanish)
    if (qok) {
        const float *qr = a.q.p + n * a.q.sn + h * 32 + (long long)qi * a.q.sl + 4 * r;
        const float *gr = a.go.p + n * a.go.sn + h * 32 + (long long)qi * a.go.sl + 4 * r;
        const float *orw = a.o.p + n * a.o.sn + h * 32 + (long long)qi * a.o.sl + 4 * r;
        q0 = ld4(qr); q1 = ld4(qr + 16); g0 = ld4(gr); g1 = ld4(gr + 16); o0 = ld4(orw); o1 = ld4(orw + 16);
        lse_n = a.lse[(long long)pair * a.Lq + qi];
    }
    float lse, lse_lo;
    at_lse_base2(lse_n, lse, lse_lo);
    ax_scale4(q0, a.scale2); ax_scale4(q1, a.scale2);
    const unsigned char *mrow = (a.mask && qok) ? a.mask + (long long)qi * a.mask_sq : nullptr;
    const float *kp = a.k.p + n * a.k.sn + h * 32, *vp = a.v.p + n * a.v.sn + h * 32;
    const unsigned ctr = ((unsigned)qi << 16) + 4 * r + mix;
    const float delta = at_rsum(g0.x * o0.x + g0.y * o0.y + g0.z * o0.z + g0.w * o0.w + g1.x * o1.x + g1.y * o1.y + g1.z * o1.z +
                                g1.w * o1.w);
    at_f4 dq0 = {0.f, 0.f, 0.f, 0.f}, dq1 = dq0;
    for (int k0 = 0; k0 < a.Lk; k0 += kAxChunk) {
        __syncthreads();
        ax_load_chunk2(Ks, kp, a.k.sl, Vs, vp, a.v.sl, k0, a.Lk);
        __syncthreads();
        const int nt = min(kAxTiles, (a.Lk - k0 + 15) >> 4);
        // S^T and dP^T tiles: entry v = (key k0 + 16 t + 4 r + v, query qi)
#pragma unroll 1
        for (int t = 0; t < nt; ++t) {
            const unsigned hid = ax_hidden4(mrow, k0 + 16 * t + 4 * r, a.Lk);
            if (a.mask != nullptr && __all(!qok || hid == 0xfu)) continue;      // hidden from the whole wavefront: exact zeros, skipped
            const at_f4 s = ax_dot32(Ks + (16 * t + c) * kAtRow + 4 * r, q0, q1);
            const at_f4 dp = ax_dot32(Vs + (16 * t + c) * kAtRow + 4 * r, g0, g1);
            at_f4 ds;
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const float p = __builtin_amdgcn_exp2f((s[v] - lse) - lse_lo);
                const bool keep = at_hash(ctr + (unsigned)(k0 + 16 * t + v)) >= a.thresh;
                ds[v] = (hid >> v & 1u) ? 0.f : p * ((keep ? dp[v] * a.keep_scale : 0.f) - delta);
            }
            at_f4 t0 = {0.f, 0.f, 0.f, 0.f}, t1 = t0;
            at_accum_t(Ks + 16 * t * kAtRow, r, c, ds, t0, t1);             // dQ^T[channel][query] += K^T . dS^T
            dq0 += t0; dq1 += t1;
        }
    }
    if (qok) {
        float *gq = a.gq.p + n * a.gq.sn + h * 32 + (long long)qi * a.gq.sl + 4 * r;
        *reinterpret_cast<float4 *>(gq) = make_float4(dq0[0] * a.scale, dq0[1] * a.scale, dq0[2] * a.scale, dq0[3] * a.scale);
        *reinterpret_cast<float4 *>(gq + 16) = make_float4(dq1[0] * a.scale, dq1[1] * a.scale, dq1[2] * a.scale, dq1[3] * a.scale);
    }
}

// LDS above 64 KB would be requested as msda_attn.hip's at_allow_lds does; the three kernels' static 18 KB need no opt-in.
static_assert((2 * kAxChunk * kAtRow + 3 * kAxChunk) * sizeof(float) <= 64 * 1024, "static LDS");

// ---- bf16 operands (msda_attn32x_*_bf16) -----------------------------------------------------------------------------------------
// The same three kernels and the same work split with q, k, v, out, dO and the gradients in bf16 and every product on
// v_mfma_f32_16x16x32_bf16 (fp32 accumulate) through the ab_* helpers of msda_attn_tile.h: a workgroup of 8 wavefronts owns
// kAxRows = 128 queries (keys), 16 per wavefront, and streams the other operand in chunks of kAxbChunk = 128 rows = 4 tile
// pairs of 32 — bf16 rows are [rows][kAbRow = 40], so two slices of 128 rows are 20 KB (dK / dV: + 3.5 KB), what the fp32
// kernels' 64-row chunks cost, with half the barriers per key; one 16-byte load per thread and slice fills a chunk.
// A lane (c, r) holds the 8 keys (queries) 32T + 8r + j of a pair (msda_attn_tile.h, "Relabelling").
// Rounding points — msda_attn32_*_bf16's, carried over to the online softmax:
//   * scores: the bf16 product accumulated in fp32, times scale * log2 e AFTER the product (a bf16 q cannot be prescaled without
//     a rounding); running maximum, running sum (of the unrounded, undropped 2^(s - m)) and the rescaling of O in fp32;
//   * forward: the operand of P . V is the chunk's UN-NORMALISED, dropout-selected 2^(s - m) rounded to bf16 — a value in
//     [0, 1], so its rounding error relative to the row's largest term is that of the resident core's normalised P; the row's
//     keep_scale / sum is applied once in fp32 at the end and out rounded once.  (The resident core rounds the normalised
//     P * keep_scale / sum: it knows the sum before the product.  The two differ by the rounding of one bf16 operand.)
//   * backward: P = 2^(s - lse) from the hi + lo lse, delta = rowsum(dO * O) from the saved bf16 out in fp32 (one function,
//     one order, in both launches), dP = dO v^T in fp32; P_drop rounded to bf16 as dV's operand, dS = P (dP_drop - delta) rounded
//     to bf16 as dQ's and dK's; dQ and dK scaled in fp32, then every gradient rounded once.
// Kept from the fp32 kernels: every 32-row pair's product starts from a zero accumulator and is added on the vector unit
// (ax_tile_sums — with bf16 operands the terms are exact products, but the chain's intermediate roundings are the same fp32
// ones); hidden and padding entries' P and dS selected to 0; the tile skip of dQ, now a 32-key pair decided by one ballot —
// every loop around ab_tr stays wave-uniform (the transposed LDS read needs all 64 lanes); the whole chunk zero-filled past
// L (a stale NaN row would meet P = 0 in the product); the dropout counter on the real (query, key) indices.
constexpr int kAxbChunk = 128, kAxbPairs = kAxbChunk / 32;
static_assert(kAxbChunk * 4 == kAxBlock, "one 16-byte load per thread and slice in axb_load_chunk2");


// rows [row0, row0 + kAxbChunk) of two [L][32] bf16 slices -> dst0 / dst1 [kAxbChunk][kAbRow]; rows past L zero
__device__ __forceinline__ void axb_load_chunk2(uint16_t *dst0, const uint16_t *src0, long long sl0, uint16_t *dst1,
                                                const uint16_t *src1, long long sl1, int row0, int L)
{
    const int row = threadIdx.x >> 2, c = (threadIdx.x & 3) * 8, g = row0 + row;
    const bool live = g < L;
    const at_bf8 v0 = live ? ab_ld8(src0 + (long long)g * sl0 + c) : ab_zero8();
    const at_bf8 v1 = live ? ab_ld8(src1 + (long long)g * sl1 + c) : ab_zero8();
    *reinterpret_cast<at_bf8 *>(dst0 + row * kAbRow + c) = v0;
    *reinterpret_cast<at_bf8 *>(dst1 + row * kAbRow + c) = v1;
}

// bit j set: key0 + j (j = 0..7) is hidden from this lane's query or lies past Lk
__device__ __forceinline__ unsigned axb_hidden8(const unsigned char *mrow, int key0, int Lk)
{
    return ax_hidden4(mrow, key0, Lk) | (ax_hidden4(mrow, key0 + 4, Lk) << 4);
}

// 8 channels of <dO, O> in fp32; both backward launches sum a row's four parts as (0 + 1) + (2 + 3)
__device__ __forceinline__ float axb_dot8(const at_bf8 &g, const at_bf8 &o)
{
    float d = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) d = fmaf(ab_f(g[j]), ab_f(o[j]), d);
    return d;
}

__global__ __launch_bounds__(kAxBlock) void attn32x_fwd_bf16_kernel(const AttnArgs<uint16_t> a)
{
    __shared__ __attribute__((aligned(16))) uint16_t Ks[kAxbChunk * kAbRow], Vs[kAxbChunk * kAbRow];
    const int pair = (int)blockIdx.x / a.wpp, blk = (int)blockIdx.x % a.wpp, n = pair / a.H, h = pair % a.H;
    const unsigned mix = at_mix(a.thresh ? a.seed[0] : 0ull, (unsigned)pair);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, c = lane & 15, r = lane >> 4;
    const int qi = blk * kAxRows + wave * 16 + c;
    const bool qok = qi < a.Lq;
    at_bf8 qf = ab_zero8();
    if (qok) qf = ab_ld8(a.q.p + n * a.q.sn + h * 32 + (long long)qi * a.q.sl + 8 * r);
    const unsigned char *mrow = (a.mask && qok) ? a.mask + (long long)qi * a.mask_sq : nullptr;
    const uint16_t *kp = a.k.p + n * a.k.sn + h * 32, *vp = a.v.p + n * a.v.sn + h * 32;
    const unsigned ctr = ((unsigned)qi << 16) + 8 * r + mix;
    float m = -INFINITY, sum = 0.f;                     // running maximum (base 2) of the query; this lane's share of the sum
    at_f4 o0 = {0.f, 0.f, 0.f, 0.f}, o1 = o0;
    for (int k0 = 0; k0 < a.Lk; k0 += kAxbChunk) {
        __syncthreads();                                // (the last chunk's readers are done)
        axb_load_chunk2(Ks, kp, a.k.sl, Vs, vp, a.v.sl, k0, a.Lk);
        __syncthreads();
        const int np = min(kAxbPairs, (a.Lk - k0 + 31) >> 5);
        // s[2T + b][v] = score of key k0 + 32T + 8r + 4b + v for query qi (raw, then times scale * log2 e)
        at_f4 s[2 * kAxbPairs];
#pragma unroll
        for (int T = 0; T < kAxbPairs; ++T)
            if (T < np) ab_pair(Ks, T, r, c, qf, s[2 * T], s[2 * T + 1]);
        float cm = -INFINITY;
#pragma unroll
        for (int T = 0; T < kAxbPairs; ++T) {
            if (T < np) {
                const unsigned hid = axb_hidden8(mrow, k0 + 32 * T + 8 * r, a.Lk);
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const float x = (hid >> j & 1u) ? -INFINITY : s[2 * T + (j >> 2)][j & 3] * a.scale2;
                    s[2 * T + (j >> 2)][j & 3] = x;
                    cm = fmaxf(cm, x);
                }
            }
        }
        const float m_new = fmaxf(m, at_rmax(cm));
        const float m_ref = m_new == -INFINITY ? 0.f : m_new;       // (nothing visible yet: every term below is exp2(-inf) = 0)
        const float alpha = __builtin_amdgcn_exp2f(m - m_ref);
        sum *= alpha;
        o0 *= alpha; o1 *= alpha;
        m = m_new;
#pragma unroll
        for (int T = 0; T < kAxbPairs; ++T) {
            if (T < np) {                               // (uniform over the workgroup: ab_tr sees all 64 lanes)
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const float p = __builtin_amdgcn_exp2f(s[2 * T + (j >> 2)][j & 3] - m_ref);
                    sum += p;
                    const bool keep = at_hash(ctr + (unsigned)(k0 + 32 * T + j)) >= a.thresh;       // (thresh 0: always)
                    s[2 * T + (j >> 2)][j & 3] = keep ? p : 0.f;
                }
                const at_bf8 pb = ab_pack(s[2 * T], s[2 * T + 1]);          // P^T[key k0 + 32T + 8r + j][query qi], un-normalised
                const at_f4 z = {0.f, 0.f, 0.f, 0.f};
                o0 += ab_mfma(ab_tr(Vs, T, 0, r, c), pb, z);                // O^T[channel][query] += V^T . P^T (ax_tile_sums)
                o1 += ab_mfma(ab_tr(Vs, T, 1, r, c), pb, z);
            }
        }
    }
    sum = at_rsum(sum);
    if (qok) {
        if (r == 0) a.lse[(long long)pair * a.Lq + qi] = at_lse_natural(m, __builtin_amdgcn_logf(sum));
        const float inv = a.keep_scale / sum;           // (sum 0 — every key hidden: inf, and the row 0 * inf = NaN)
        uint16_t *orow = a.o.p + n * a.o.sn + h * 32 + (long long)qi * a.o.sl + 4 * r;
        ab_st4(orow, o0, inv);
        ab_st4(orow + 16, o1, inv);
    }
}

// dK, dV: a wavefront owns 16 keys; the workgroup walks the query chunks
__global__ __launch_bounds__(kAxBlock) void attn32x_bwd_kv_bf16_kernel(const AttnArgs<uint16_t> a)
{
    __shared__ __attribute__((aligned(16))) uint16_t Qs[kAxbChunk * kAbRow], Gs[kAxbChunk * kAbRow];
    __shared__ __attribute__((aligned(16))) float lse_s[kAxbChunk], lsl_s[kAxbChunk], del_s[kAxbChunk];
    __shared__ __attribute__((aligned(16))) unsigned msk_s[4 * kAxbChunk];  // [32-key part of the block][query]: hidden bits
    const int pair = (int)blockIdx.x / a.wpp, blk = (int)blockIdx.x % a.wpp, n = pair / a.H, h = pair % a.H;
    const unsigned mix = at_mix(a.thresh ? a.seed[0] : 0ull, (unsigned)pair);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, c = lane & 15, r = lane >> 4;
    const int key = blk * kAxRows + wave * 16 + c;
    const bool kok = key < a.Lk;
    at_bf8 kf = ab_zero8(), vf = ab_zero8();
    if (kok) {
        kf = ab_ld8(a.k.p + n * a.k.sn + h * 32 + (long long)key * a.k.sl + 8 * r);
        vf = ab_ld8(a.v.p + n * a.v.sn + h * 32 + (long long)key * a.v.sl + 8 * r);
    }
    const int mpart = wave >> 1, mbit = (wave & 1) * 16 + c;       // this lane's key in msk_s: word [mpart][query], bit mbit
    const uint16_t *qp = a.q.p + n * a.q.sn + h * 32, *gp = a.go.p + n * a.go.sn + h * 32, *op = a.o.p + n * a.o.sn + h * 32;
    const unsigned ctr = (unsigned)key + ((unsigned)(8 * r) << 16) + mix;
    at_f4 dv0 = {0.f, 0.f, 0.f, 0.f}, dv1 = dv0, dk0 = dv0, dk1 = dv0;
    for (int c0 = 0; c0 < a.Lq; c0 += kAxbChunk) {
        __syncthreads();
        {
            // a thread loads 8 channels of one query's q, dO and O: the chunk's two slices, and its part of delta = <dO, O>;
            // the log-sum-exp in base 2 is +inf for the rows past Lq (their probabilities vanish).  The mask is read here too,
            // along the queries' rows (ax_hidden4's 4-byte reads) and kept as bits: a lane reading its key's column byte by
            // byte in the tile loop cost dK / dV 320 us of 653 at 1098 rows under the denoising mask.
            const int row = threadIdx.x >> 2, part = threadIdx.x & 3, g = c0 + row;
            const bool live = g < a.Lq;
            const at_bf8 qv = live ? ab_ld8(qp + (long long)g * a.q.sl + 8 * part) : ab_zero8();
            const at_bf8 gv = live ? ab_ld8(gp + (long long)g * a.go.sl + 8 * part) : ab_zero8();
            const at_bf8 ov = live ? ab_ld8(op + (long long)g * a.o.sl + 8 * part) : ab_zero8();
            *reinterpret_cast<at_bf8 *>(Qs + row * kAbRow + 8 * part) = qv;
            *reinterpret_cast<at_bf8 *>(Gs + row * kAbRow + 8 * part) = gv;
            float d = axb_dot8(gv, ov);
            d += __shfl_xor(d, 1);
            d += __shfl_xor(d, 2);
            if (part == 0) {
                float hi, lo;
                at_lse_base2(live ? a.lse[(long long)pair * a.Lq + g] : INFINITY, hi, lo);
                del_s[row] = d; lse_s[row] = hi; lsl_s[row] = lo;
            }
            if (a.mask != nullptr) {                    // the query's mask row over 32 of the block's keys as one word of bits
                const unsigned char *mrow = live ? a.mask + (long long)g * a.mask_sq : nullptr;
                const int key0 = blk * kAxRows + 32 * part;
                unsigned w = 0;
#pragma unroll
                for (int i = 0; i < 8; ++i) w |= ax_hidden4(mrow, key0 + 4 * i, a.Lk) << (4 * i);
                msk_s[part * kAxbChunk + row] = w;
            }
        }
        __syncthreads();
        const int np = min(kAxbPairs, (a.Lq - c0 + 31) >> 5);
#pragma unroll 1
        for (int T = 0; T < np; ++T) {                  // (uniform over the workgroup)
            // S and dP tiles of the pair: entry (b, v) = (query c0 + 32T + 8r + 4b + v, key)
            at_f4 s[2], dp[2];
            ab_pair(Qs, T, r, c, kf, s[0], s[1]);
            ab_pair(Gs, T, r, c, vf, dp[0], dp[1]);
            const int ql = 32 * T + 8 * r, qrow = c0 + ql;
            const float4 h0 = ld4(lse_s + ql), h1 = ld4(lse_s + ql + 4), w0 = ld4(lsl_s + ql), w1 = ld4(lsl_s + ql + 4);
            const float4 e0 = ld4(del_s + ql), e1 = ld4(del_s + ql + 4);
            const float lsv[8] = {h0.x, h0.y, h0.z, h0.w, h1.x, h1.y, h1.z, h1.w}, llv[8] = {w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, w1.z, w1.w};
            const float dlv[8] = {e0.x, e0.y, e0.z, e0.w, e1.x, e1.y, e1.z, e1.w};
            unsigned hb = 0;                            // bit j: this lane's key is hidden from query qrow + j
            if (a.mask != nullptr) {
                const uint4 m0 = *reinterpret_cast<const uint4 *>(msk_s + mpart * kAxbChunk + ql);
                const uint4 m1 = *reinterpret_cast<const uint4 *>(msk_s + mpart * kAxbChunk + ql + 4);
                const unsigned mw[8] = {m0.x, m0.y, m0.z, m0.w, m1.x, m1.y, m1.z, m1.w};
#pragma unroll
                for (int j = 0; j < 8; ++j) hb |= (mw[j] >> mbit & 1u) << j;
            }
            at_f4 pd[2], ds[2];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int b = j >> 2, v = j & 3;
                const bool hid = (hb >> j & 1u) != 0;
                const float p = hid ? 0.f : __builtin_amdgcn_exp2f(fmaf(s[b][v], a.scale2, -lsv[j]) - llv[j]);
                const bool keep = at_hash(ctr + ((unsigned)(qrow - 8 * r + j) << 16)) >= a.thresh;
                pd[b][v] = keep ? p * a.keep_scale : 0.f;
                ds[b][v] = hid ? 0.f : p * ((keep ? dp[b][v] * a.keep_scale : 0.f) - dlv[j]);
            }
            const at_bf8 pb = ab_pack(pd[0], pd[1]), sb = ab_pack(ds[0], ds[1]);
            const at_f4 z = {0.f, 0.f, 0.f, 0.f};
            dv0 += ab_mfma(ab_tr(Gs, T, 0, r, c), pb, z);                   // dV^T[channel][key] += dO^T . P_drop
            dv1 += ab_mfma(ab_tr(Gs, T, 1, r, c), pb, z);
            dk0 += ab_mfma(ab_tr(Qs, T, 0, r, c), sb, z);                   // dK^T[channel][key] += Q^T . dS
            dk1 += ab_mfma(ab_tr(Qs, T, 1, r, c), sb, z);
        }
    }
    if (kok) {
        uint16_t *gvr = a.gv.p + n * a.gv.sn + h * 32 + (long long)key * a.gv.sl + 4 * r;
        uint16_t *gkr = a.gk.p + n * a.gk.sn + h * 32 + (long long)key * a.gk.sl + 4 * r;
        ab_st4(gvr, dv0, 1.f); ab_st4(gvr + 16, dv1, 1.f);
        ab_st4(gkr, dk0, a.scale); ab_st4(gkr + 16, dk1, a.scale);
    }
}

// dQ: a wavefront owns 16 queries; the workgroup walks the key chunks (S^T tiles, as the forward)
__global__ __launch_bounds__(kAxBlock) void attn32x_bwd_q_bf16_kernel(const AttnArgs<uint16_t> a)
{
    __shared__ __attribute__((aligned(16))) uint16_t Ks[kAxbChunk * kAbRow], Vs[kAxbChunk * kAbRow];
    const int pair = (int)blockIdx.x / a.wpp, blk = (int)blockIdx.x % a.wpp, n = pair / a.H, h = pair % a.H;
    const unsigned mix = at_mix(a.thresh ? a.seed[0] : 0ull, (unsigned)pair);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, c = lane & 15, r = lane >> 4;
    const int qi = blk * kAxRows + wave * 16 + c;
    const bool qok = qi < a.Lq;
    at_bf8 qf = ab_zero8(), gf = ab_zero8(), of = ab_zero8();
    float lse_n = INFINITY;                             // (rows past Lq: probabilities vanish)
    if (qok) {
        qf = ab_ld8(a.q.p + n * a.q.sn + h * 32 + (long long)qi * a.q.sl + 8 * r);
        gf = ab_ld8(a.go.p + n * a.go.sn + h * 32 + (long long)qi * a.go.sl + 8 * r);
        of = ab_ld8(a.o.p + n * a.o.sn + h * 32 + (long long)qi * a.o.sl + 8 * r);
        lse_n = a.lse[(long long)pair * a.Lq + qi];
    }
    float lse, lse_lo;
    at_lse_base2(lse_n, lse, lse_lo);
    const unsigned char *mrow = (a.mask && qok) ? a.mask + (long long)qi * a.mask_sq : nullptr;
    const uint16_t *kp = a.k.p + n * a.k.sn + h * 32, *vp = a.v.p + n * a.v.sn + h * 32;
    const unsigned ctr = ((unsigned)qi << 16) + 8 * r + mix;
    const float delta = at_rsum(axb_dot8(gf, of));
    at_f4 dq0 = {0.f, 0.f, 0.f, 0.f}, dq1 = dq0;
    for (int k0 = 0; k0 < a.Lk; k0 += kAxbChunk) {
        __syncthreads();
        axb_load_chunk2(Ks, kp, a.k.sl, Vs, vp, a.v.sl, k0, a.Lk);
        __syncthreads();
        const int np = min(kAxbPairs, (a.Lk - k0 + 31) >> 5);
#pragma unroll 1
        for (int T = 0; T < np; ++T) {
            const unsigned hid = axb_hidden8(mrow, k0 + 32 * T + 8 * r, a.Lk);
            // hidden from the whole wavefront (rows past Lq count as hidden): exact zeros, skipped — one ballot, so the loop
            // stays wave-uniform around ab_tr
            if (a.mask != nullptr && __all(!qok || hid == 0xffu)) continue;
            // S^T and dP^T tiles of the pair: entry (b, v) = (key k0 + 32T + 8r + 4b + v, query qi)
            at_f4 s[2], dp[2];
            ab_pair(Ks, T, r, c, qf, s[0], s[1]);
            ab_pair(Vs, T, r, c, gf, dp[0], dp[1]);
            at_f4 ds[2];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int b = j >> 2, v = j & 3;
                const float p = __builtin_amdgcn_exp2f(fmaf(s[b][v], a.scale2, -lse) - lse_lo);
                const bool keep = at_hash(ctr + (unsigned)(k0 + 32 * T + j)) >= a.thresh;
                ds[b][v] = (hid >> j & 1u) ? 0.f : p * ((keep ? dp[b][v] * a.keep_scale : 0.f) - delta);
            }
            const at_bf8 sb = ab_pack(ds[0], ds[1]);
            const at_f4 z = {0.f, 0.f, 0.f, 0.f};
            dq0 += ab_mfma(ab_tr(Ks, T, 0, r, c), sb, z);                   // dQ^T[channel][query] += K^T . dS^T
            dq1 += ab_mfma(ab_tr(Ks, T, 1, r, c), sb, z);
        }
    }
    if (qok) {
        uint16_t *gq = a.gq.p + n * a.gq.sn + h * 32 + (long long)qi * a.gq.sl + 4 * r;
        ab_st4(gq, dq0, a.scale); ab_st4(gq + 16, dq1, a.scale);
    }
}

static_assert(2 * kAxbChunk * kAbRow * sizeof(uint16_t) + 7 * kAxbChunk * sizeof(float) <= 64 * 1024, "static LDS");

// workgroups that share a pair: kAxRows queries (forward, dQ) or keys (dK / dV) each
static int ax_blocks(int L) { return (int)(((long long)L + kAxRows - 1) / kAxRows); }

}  // namespace msda

using msda::attn_view;
using msda::ax_blocks;

extern "C" {

int msda_attn32x_supported(int Lq, int Lk, int head_dim)
{
    return head_dim == 32 && Lq >= 1 && Lk >= 1 && Lq <= msda::kAxMaxLen && Lk <= msda::kAxMaxLen;
}

// Each entry: check, bind (msda_attn_args.h: every refusal comes before any launch), size the grid, launch.  The check is given
// the larger of a backward's two grids; each launch then sets its own workgroups per pair.  LDS is static.

int msda_attn32x_forward_f32(const float *q, long long q_sn, long long q_sl, const float *k, long long k_sn, long long k_sl,
                             const float *v, long long v_sn, long long v_sl, int N, int H, int Lq, int Lk, float scale,
                             float dropout_p, const unsigned long long *seed, const unsigned char *mask, long long mask_sq,
                             float *out, long long o_sn, long long o_sl, float *lse, msda_stream_t stream)
{
    const char *who = "msda_attn32x_forward_f32";
    msda::AttnArgs<float> a{};
    if (int rc = msda::attn_check(a, who, msda::kAxMaxLen, N, H, Lq, Lk, ax_blocks(Lq), scale, dropout_p, seed, mask, mask_sq)) return rc;
    if (int rc = msda::attn_bind_forward(a, who, attn_view(q, q_sn, q_sl), attn_view(k, k_sn, k_sl), attn_view(v, v_sn, v_sl),
                                         attn_view(out, o_sn, o_sl), lse)) return rc;
    hipLaunchKernelGGL(msda::attn32x_fwd_kernel, dim3((unsigned)(N * H * a.wpp)), dim3(msda::kAxBlock), 0, (hipStream_t)stream, a);
    return msda::check_launch("msda long attention forward (head_dim 32)");
}

int msda_attn32x_backward_f32(const float *q, long long q_sn, long long q_sl, const float *k, long long k_sn, long long k_sl,
                              const float *v, long long v_sn, long long v_sl, const float *out, long long o_sn, long long o_sl,
                              const float *lse, const float *grad_out, long long go_sn, long long go_sl, int N, int H, int Lq,
                              int Lk, float scale, float dropout_p, const unsigned long long *seed, const unsigned char *mask,
                              long long mask_sq, float *grad_q, long long gq_sn, long long gq_sl, float *grad_k, long long gk_sn,
                              long long gk_sl, float *grad_v, long long gv_sn, long long gv_sl, msda_stream_t stream)
{
    const char *who = "msda_attn32x_backward_f32";
    msda::AttnArgs<float> a{};
    const int nblk_q = ax_blocks(Lq), nblk_k = ax_blocks(Lk);
    if (int rc = msda::attn_check(a, who, msda::kAxMaxLen, N, H, Lq, Lk, nblk_q > nblk_k ? nblk_q : nblk_k, scale, dropout_p, seed, mask,
                                  mask_sq)) return rc;
    if (int rc = msda::attn_bind_backward(a, who, attn_view(q, q_sn, q_sl), attn_view(k, k_sn, k_sl), attn_view(v, v_sn, v_sl),
                                          attn_view(out, o_sn, o_sl), lse, attn_view(grad_out, go_sn, go_sl),
                                          attn_view(grad_q, gq_sn, gq_sl), attn_view(grad_k, gk_sn, gk_sl),
                                          attn_view(grad_v, gv_sn, gv_sl))) return rc;
    a.wpp = nblk_k;
    hipLaunchKernelGGL(msda::attn32x_bwd_kv_kernel, dim3((unsigned)(N * H * nblk_k)), dim3(msda::kAxBlock), 0, (hipStream_t)stream, a);
    if (int rc = msda::check_launch("msda long attention backward (dK, dV)")) return rc;
    a.wpp = nblk_q;
    hipLaunchKernelGGL(msda::attn32x_bwd_q_kernel, dim3((unsigned)(N * H * nblk_q)), dim3(msda::kAxBlock), 0, (hipStream_t)stream, a);
    return msda::check_launch("msda long attention backward (dQ)");
}

// bf16 operands: the same checks, the fp32 entries' random stream and grids
int msda_attn32x_forward_bf16(const uint16_t *q, long long q_sn, long long q_sl, const uint16_t *k, long long k_sn, long long k_sl,
                              const uint16_t *v, long long v_sn, long long v_sl, int N, int H, int Lq, int Lk, float scale,
                              float dropout_p, const unsigned long long *seed, const unsigned char *mask, long long mask_sq,
                              uint16_t *out, long long o_sn, long long o_sl, float *lse, msda_stream_t stream)
{
    const char *who = "msda_attn32x_forward_bf16";
    msda::AttnArgs<uint16_t> a{};
    if (int rc = msda::attn_check(a, who, msda::kAxMaxLen, N, H, Lq, Lk, ax_blocks(Lq), scale, dropout_p, seed, mask, mask_sq)) return rc;
    if (int rc = msda::attn_bind_forward(a, who, attn_view(q, q_sn, q_sl), attn_view(k, k_sn, k_sl), attn_view(v, v_sn, v_sl),
                                         attn_view(out, o_sn, o_sl), lse)) return rc;
    hipLaunchKernelGGL(msda::attn32x_fwd_bf16_kernel, dim3((unsigned)(N * H * a.wpp)), dim3(msda::kAxBlock), 0, (hipStream_t)stream, a);
    return msda::check_launch("msda long attention forward (head_dim 32, bf16)");
}

int msda_attn32x_backward_bf16(const uint16_t *q, long long q_sn, long long q_sl, const uint16_t *k, long long k_sn, long long k_sl,
                               const uint16_t *v, long long v_sn, long long v_sl, const uint16_t *out, long long o_sn, long long o_sl,
                               const float *lse, const uint16_t *grad_out, long long go_sn, long long go_sl, int N, int H, int Lq,
                               int Lk, float scale, float dropout_p, const unsigned long long *seed, const unsigned char *mask,
                               long long mask_sq, uint16_t *grad_q, long long gq_sn, long long gq_sl, uint16_t *grad_k,
                               long long gk_sn, long long gk_sl, uint16_t *grad_v, long long gv_sn, long long gv_sl,
                               msda_stream_t stream)
{
    const char *who = "msda_attn32x_backward_bf16";
    msda::AttnArgs<uint16_t> a{};
    const int nblk_q = ax_blocks(Lq), nblk_k = ax_blocks(Lk);
    if (int rc = msda::attn_check(a, who, msda::kAxMaxLen, N, H, Lq, Lk, nblk_q > nblk_k ? nblk_q : nblk_k, scale, dropout_p, seed, mask,
                                  mask_sq)) return rc;
    if (int rc = msda::attn_bind_backward(a, who, attn_view(q, q_sn, q_sl), attn_view(k, k_sn, k_sl), attn_view(v, v_sn, v_sl),
                                          attn_view(out, o_sn, o_sl), lse, attn_view(grad_out, go_sn, go_sl),
                                          attn_view(grad_q, gq_sn, gq_sl), attn_view(grad_k, gk_sn, gk_sl),
                                          attn_view(grad_v, gv_sn, gv_sl))) return rc;
    a.wpp = nblk_k;
    hipLaunchKernelGGL(msda::attn32x_bwd_kv_bf16_kernel, dim3((unsigned)(N * H * nblk_k)), dim3(msda::kAxBlock), 0, (hipStream_t)stream, a);
    if (int rc = msda::check_launch("msda long attention backward (dK, dV; bf16)")) return rc;
    a.wpp = nblk_q;
    hipLaunchKernelGGL(msda::attn32x_bwd_q_bf16_kernel, dim3((unsigned)(N * H * nblk_q)), dim3(msda::kAxBlock), 0, (hipStream_t)stream, a);
    return msda::check_launch("msda long attention backward (dQ; bf16)");
}

}  // extern "C"
