// Decoder self-attention core: out = dropout(softmax(q k^T * scale)) v for head_dim 32, fp32, sequences of at most 320
// (models/arctic_transformer.py:351,374-376: nn.MultiheadAttention over the 300 queries, 8 heads of 32, batch = frames).
// The vendor's fused path spends 77 + 112 + 100 us per decoder layer on it at 32 frames (attn_fwd, bwd_kernel_dk_dv,
// bwd_kernel_dq, profiles/r05_layers_kernel_stats_fused.csv) — for 256 independent 300 x 300 x 32 problems that fit a CU's LDS.
//
// All three kernels: a workgroup of 12 wavefronts (three per SIMD; with 10 two SIMDs carry three and two carry two: 201 us forward +
// backward against 167 with 12 or 16, 174 with 8) owns one (batch, head) pair — its 16-row tiles dealt to the wavefronts, up to two
// each at 300 rows (two workgroups per pair re-load the pair's operands and measured 8 % slower: MSDA_ATTN_HALVES);
// the pair's other operand(s) sit in LDS row-major ([rows][36 floats]: 16-byte aligned rows, the 16 lanes of a ds_read_b128 on
// different bank groups).  Every product runs on v_mfma_f32_16x16x4_f32 (fp32 in, fp32 accumulate: the arithmetic of an fmaf
// chain), and the score tile never changes layout between the two products it takes part in (msda_attn_tile.h: the fragment
// helpers and the relabelling that makes it so).
// Softmax statistics: the forward keeps log-sum-exp per (pair, query); the backward recomputes the probabilities from it.
// Dropout: keep(seed, pair, query, key) is a 32-bit integer hash (at_hash) compared with p * 2^32 — recomputed in the backward, no mask
// tensor; the seed is READ FROM DEVICE MEMORY (the caller draws it with torch's generator: reproducible under manual_seed,
// safe under HIP-graph capture).  This is the kernel's own random stream, not nn.functional.dropout's.
#include <math.h>

#include "msda_attn_args.h"
#include "msda_attn_tile.h"
#include "msda_common.h"
#include "msda_launch.h"

namespace msda {

#ifndef MSDA_AT_WAVES
#define MSDA_AT_WAVES 12
#endif
constexpr int kAtWaves = MSDA_AT_WAVES, kAtBlock = kAtWaves * 64, kAtMaxTiles = 20, kAtMaxLen = 16 * kAtMaxTiles;

// Dropout: 32 bits per (pair, query, key) from at_hash of the counter (query << 16) + key + at_mix(seed, pair) (msda_attn_tile.h)

// rows [0, L) of two [L][32] slices (row strides sl0 / sl1) -> dst0 / dst1 [Lp][kAtRow]; rows [L, Lp) zero.  Lp * 8 float4 per
// slice on 768 threads: at most four rounds (Lp <= 320); all the loads of a thread are issued before its first LDS store.
// kScaled: slice 0 is stored times mul0 (dK / dV: Q times scale2, the forward's own operand of the scores).
template <bool kScaled = false>
__device__ __forceinline__ void at_load_rows2(float *dst0, const float *src0, long long sl0, float *dst1, const float *src1,
                                              long long sl1, int L, int Lp, float mul0 = 1.f)
{
    constexpr int R = (kAtMaxLen * 8 + kAtBlock - 1) / kAtBlock;
    float4 v0[R], v1[R];
#pragma unroll
    for (int k = 0; k < R; ++k) {
        const int i = threadIdx.x + k * kAtBlock, row = i >> 3, c = (i & 7) * 4;
        const bool live = row < L;
        v0[k] = live ? ld4(src0 + (long long)row * sl0 + c) : at_zero4();
        v1[k] = live ? ld4(src1 + (long long)row * sl1 + c) : at_zero4();
        if (kScaled) { v0[k].x *= mul0; v0[k].y *= mul0; v0[k].z *= mul0; v0[k].w *= mul0; }
    }
#pragma unroll
    for (int k = 0; k < R; ++k) {
        const int i = threadIdx.x + k * kAtBlock, row = i >> 3, c = (i & 7) * 4;
        if (row < Lp) {
            *reinterpret_cast<float4 *>(dst0 + row * kAtRow + c) = v0[k];
            *reinterpret_cast<float4 *>(dst1 + row * kAtRow + c) = v1[k];
        }
    }
}

__global__ __launch_bounds__(kAtBlock) void attn32_fwd_kernel(const AttnArgs<float> a)
{
    extern __shared__ __attribute__((aligned(16))) float at_smem[];
    const int Lkp = (a.Lk + 15) & ~15, ntk = Lkp >> 4, ntq = (a.Lq + 15) >> 4;
    float *Ks = at_smem, *Vs = at_smem + Lkp * kAtRow;
    const int pair = (int)blockIdx.x / a.wpp, part = (int)blockIdx.x % a.wpp, n = pair / a.H, h = pair % a.H;
    at_load_rows2(Ks, a.k.p + n * a.k.sn + h * 32, a.k.sl, Vs, a.v.p + n * a.v.sn + h * 32, a.v.sl, a.Lk, Lkp);
    const unsigned mix = at_mix(a.thresh ? a.seed[0] : 0ull, (unsigned)pair);
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, c = lane & 15, r = lane >> 4;
    const int per = (ntq + a.wpp - 1) / a.wpp, t_end = min(ntq, (part + 1) * per);
    const float *qp = a.q.p + n * a.q.sn + h * 32;
    float *op = a.o.p + n * a.o.sn + h * 32;
    for (int tq = part * per + wave; tq < t_end; tq += kAtWaves) {
        const int qi = tq * 16 + c;
        const bool qok = qi < a.Lq;
        float4 q0 = at_zero4(), q1 = at_zero4();
        if (qok) { q0 = ld4(qp + (long long)qi * a.q.sl + 4 * r); q1 = ld4(qp + (long long)qi * a.q.sl + 16 + 4 * r); }
        q0.x *= a.scale2; q0.y *= a.scale2; q0.z *= a.scale2; q0.w *= a.scale2;
        q1.x *= a.scale2; q1.y *= a.scale2; q1.z *= a.scale2; q1.w *= a.scale2;
        // S^T tiles: s[t][v] = score (times log2 e) of key 16 t + 4 r + v for query qi
        at_f4 s[kAtMaxTiles];
        float m = -INFINITY;
        // (all the products first — independent chains, the matrix pipe runs them back to back — then the row maximum)
#pragma unroll
        for (int t = 0; t < kAtMaxTiles; t += 2) {               // two tiles' chains interleaved (a dependent MFMA waits 40 cycles, an issue takes 32)
            if (t + 1 < ntk) at_dot32x2(Ks + (16 * t + c) * kAtRow + 4 * r, q0, q1, s[t], s[t + 1]);
            else if (t < ntk) s[t] = at_dot32(Ks + (16 * t + c) * kAtRow + 4 * r, q0, q1);
        }
#pragma unroll
        for (int t = 0; t < kAtMaxTiles; ++t) {
            if (t < ntk) {
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    if (t == ntk - 1) s[t][v] = 16 * t + 4 * r + v < a.Lk ? s[t][v] : -INFINITY;      // (only the last tile has padding keys)
                    m = fmaxf(m, s[t][v]);
                }
            }
        }
        m = at_rmax(m);
        float sum = 0.f;
#pragma unroll
        for (int t = 0; t < kAtMaxTiles; ++t) {
            if (t < ntk) {
#pragma unroll
                for (int v = 0; v < 4; ++v) { s[t][v] = __builtin_amdgcn_exp2f(s[t][v] - m); sum += s[t][v]; }
            }
        }
        sum = at_rsum(sum);
        if (qok && r == 0) a.lse[(long long)pair * a.Lq + qi] = at_lse_natural(m, __builtin_amdgcn_logf(sum));   // natural log, rounded once
        const float inv = a.keep_scale / sum;
        at_f4 o0 = {0.f, 0.f, 0.f, 0.f}, o1 = {0.f, 0.f, 0.f, 0.f};
        const unsigned ctr = ((unsigned)qi << 16) + 4 * r + mix;
#pragma unroll
        for (int t = 0; t < kAtMaxTiles; ++t) {
            if (t < ntk) {
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    const bool keep = at_hash(ctr + (16 * t + v)) >= a.thresh;      // (thresh 0: always)
                    s[t][v] = keep ? s[t][v] * inv : 0.f;
                }
                at_accum_t(Vs + 16 * t * kAtRow, r, c, s[t], o0, o1);       // O^T[channel][query] += V^T . P
            }
        }
        if (qok) {
            float *orow = op + (long long)qi * a.o.sl + 4 * r;
            *reinterpret_cast<float4 *>(orow) = make_float4(o0[0], o0[1], o0[2], o0[3]);
            *reinterpret_cast<float4 *>(orow + 16) = make_float4(o1[0], o1[1], o1[2], o1[3]);
        }
    }
}

// The backward's probabilities are exp2(s - lse * log2 e) with lse one fp32 number per row: whatever is lost between the
// forward's scores and that difference lands on every probability, the ones near 1 included (a peaked row: |s| of 30 .. 80
// in base 2, an ulp of which is 4e-6 .. 8e-6).  So both backward kernels form the scores from the forward's own products —
// (q * scale2) . k, in the forward's channel order — and take lse * log2 e as hi + lo (at_lse_base2; the forward rounds lse
// once, at_lse_natural): what remains is that one rounding of lse, half an ulp of |lse| on every probability of the row.

// dK, dV: a wavefront owns 16 keys and walks the query tiles; Q sits in LDS times scale2 (dK is scaled back at the end)
__global__ __launch_bounds__(kAtBlock) void attn32_bwd_kv_kernel(const AttnArgs<float> a)
{
    extern __shared__ __attribute__((aligned(16))) float at_smem[];
    const int Lqp = (a.Lq + 15) & ~15, ntq = Lqp >> 4, ntk = (a.Lk + 15) >> 4;
    float *Qs = at_smem, *Gs = at_smem + Lqp * kAtRow, *lse_s = Gs + Lqp * kAtRow, *del_s = lse_s + Lqp, *lsl_s = del_s + Lqp;
    const int pair = (int)blockIdx.x / a.wpp, part = (int)blockIdx.x % a.wpp, n = pair / a.H, h = pair % a.H;
    at_load_rows2<true>(Qs, a.q.p + n * a.q.sn + h * 32, a.q.sl, Gs, a.go.p + n * a.go.sn + h * 32, a.go.sl, a.Lq, Lqp, a.scale2);
    const unsigned mix = at_mix(a.thresh ? a.seed[0] : 0ull, (unsigned)pair);
    __syncthreads();
    // per query: log-sum-exp (+inf for the padding rows: their probabilities vanish) and delta = <dO, O>
    for (int qi = threadIdx.x; qi < Lqp; qi += kAtBlock) {
        float d = 0.f;
        if (qi < a.Lq) {
            const float *orow = a.o.p + n * a.o.sn + h * 32 + (long long)qi * a.o.sl, *grow = Gs + qi * kAtRow;
#pragma unroll
            for (int k4 = 0; k4 < 8; ++k4) {
                const float4 ov = ld4(orow + 4 * k4), gv = ld4(grow + 4 * k4);
                d += ov.x * gv.x + ov.y * gv.y + ov.z * gv.z + ov.w * gv.w;
            }
        }
        del_s[qi] = d;
        at_lse_base2(qi < a.Lq ? a.lse[(long long)pair * a.Lq + qi] : INFINITY, lse_s[qi], lsl_s[qi]);      // base 2, like the scores
    }
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, c = lane & 15, r = lane >> 4;
    const int per = (ntk + a.wpp - 1) / a.wpp, t_end = min(ntk, (part + 1) * per);
    const float unscale = a.scale2 != 0.f ? a.scale / a.scale2 : 0.f;       // dK = scale * Q^T dS, and Qs holds Q * scale2
    for (int tk = part * per + wave; tk < t_end; tk += kAtWaves) {
        const int key = tk * 16 + c;
        const bool kok = key < a.Lk;
        float4 k0 = at_zero4(), k1 = at_zero4(), v0 = at_zero4(), v1 = at_zero4();
        if (kok) {
            const float *kr = a.k.p + n * a.k.sn + h * 32 + (long long)key * a.k.sl + 4 * r;
            const float *vr = a.v.p + n * a.v.sn + h * 32 + (long long)key * a.v.sl + 4 * r;
            k0 = ld4(kr); k1 = ld4(kr + 16); v0 = ld4(vr); v1 = ld4(vr + 16);
        }
        const unsigned ctr = (unsigned)key + ((unsigned)(4 * r) << 16) + mix;
        at_f4 dv0 = {0.f, 0.f, 0.f, 0.f}, dv1 = dv0, dk0 = dv0, dk1 = dv0;
        // S and dP tiles: entry v = (query 16 t + 4 r + v, key).  The next tile's two products are issued before this tile's
        // exponentials and hashes: the matrix pipe works through them while the vector unit is busy.
        at_f4 s = at_dot32(Qs + c * kAtRow + 4 * r, k0, k1), dp = at_dot32(Gs + c * kAtRow + 4 * r, v0, v1);
#pragma unroll 1
        for (int t = 0; t < ntq; ++t) {
            const int tn = min(t + 1, ntq - 1);
            const at_f4 s_next = at_dot32(Qs + (16 * tn + c) * kAtRow + 4 * r, k0, k1);
            const at_f4 dp_next = at_dot32(Gs + (16 * tn + c) * kAtRow + 4 * r, v0, v1);
            __builtin_amdgcn_sched_barrier(0);
            const float4 ls = ld4(lse_s + 16 * t + 4 * r), ll = ld4(lsl_s + 16 * t + 4 * r), dl = ld4(del_s + 16 * t + 4 * r);
            const float lsv[4] = {ls.x, ls.y, ls.z, ls.w}, llv[4] = {ll.x, ll.y, ll.z, ll.w}, dlv[4] = {dl.x, dl.y, dl.z, dl.w};
            at_f4 pd, ds;
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const float p = __builtin_amdgcn_exp2f((s[v] - lsv[v]) - llv[v]);
                const bool keep = at_hash(ctr + ((unsigned)(16 * t + v) << 16)) >= a.thresh;
                pd[v] = keep ? p * a.keep_scale : 0.f;
                ds[v] = p * ((keep ? dp[v] * a.keep_scale : 0.f) - dlv[v]);
            }
            at_accum_t(Gs + 16 * t * kAtRow, r, c, pd, dv0, dv1);           // dV^T[channel][key] += dO^T . P_drop
            at_accum_t(Qs + 16 * t * kAtRow, r, c, ds, dk0, dk1);           // dK^T[channel][key] += Q^T . dS
            s = s_next; dp = dp_next;
        }
        if (kok) {
            float *gvr = a.gv.p + n * a.gv.sn + h * 32 + (long long)key * a.gv.sl + 4 * r;
            float *gkr = a.gk.p + n * a.gk.sn + h * 32 + (long long)key * a.gk.sl + 4 * r;
            *reinterpret_cast<float4 *>(gvr) = make_float4(dv0[0], dv0[1], dv0[2], dv0[3]);
            *reinterpret_cast<float4 *>(gvr + 16) = make_float4(dv1[0], dv1[1], dv1[2], dv1[3]);
            *reinterpret_cast<float4 *>(gkr) = make_float4(dk0[0] * unscale, dk0[1] * unscale, dk0[2] * unscale, dk0[3] * unscale);
            *reinterpret_cast<float4 *>(gkr + 16) = make_float4(dk1[0] * unscale, dk1[1] * unscale, dk1[2] * unscale, dk1[3] * unscale);
        }
    }
}

// dQ: a wavefront owns 16 queries and walks the key tiles (S^T tiles, as the forward)
__global__ __launch_bounds__(kAtBlock) void attn32_bwd_q_kernel(const AttnArgs<float> a)
{
    extern __shared__ __attribute__((aligned(16))) float at_smem[];
    const int Lkp = (a.Lk + 15) & ~15, ntk = Lkp >> 4, ntq = (a.Lq + 15) >> 4;
    float *Ks = at_smem, *Vs = at_smem + Lkp * kAtRow;
    const int pair = (int)blockIdx.x / a.wpp, part = (int)blockIdx.x % a.wpp, n = pair / a.H, h = pair % a.H;
    at_load_rows2(Ks, a.k.p + n * a.k.sn + h * 32, a.k.sl, Vs, a.v.p + n * a.v.sn + h * 32, a.v.sl, a.Lk, Lkp);
    const unsigned mix = at_mix(a.thresh ? a.seed[0] : 0ull, (unsigned)pair);
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, c = lane & 15, r = lane >> 4;
    const int per = (ntq + a.wpp - 1) / a.wpp, t_end = min(ntq, (part + 1) * per);
    for (int tq = part * per + wave; tq < t_end; tq += kAtWaves) {
        const int qi = tq * 16 + c;
        const bool qok = qi < a.Lq;
        float4 q0 = at_zero4(), q1 = at_zero4(), g0 = at_zero4(), g1 = at_zero4(), o0 = at_zero4(), o1 = at_zero4();
        float lse_n = INFINITY;
        if (qok) {
            const float *qr = a.q.p + n * a.q.sn + h * 32 + (long long)qi * a.q.sl + 4 * r;
            const float *gr = a.go.p + n * a.go.sn + h * 32 + (long long)qi * a.go.sl + 4 * r;
            const float *orw = a.o.p + n * a.o.sn + h * 32 + (long long)qi * a.o.sl + 4 * r;
            q0 = ld4(qr); q1 = ld4(qr + 16); g0 = ld4(gr); g1 = ld4(gr + 16); o0 = ld4(orw); o1 = ld4(orw + 16);
            lse_n = a.lse[(long long)pair * a.Lq + qi];
        }
        float lse, lse_lo;
        at_lse_base2(lse_n, lse, lse_lo);
        q0.x *= a.scale2; q0.y *= a.scale2; q0.z *= a.scale2; q0.w *= a.scale2;
        q1.x *= a.scale2; q1.y *= a.scale2; q1.z *= a.scale2; q1.w *= a.scale2;
        const unsigned ctr = ((unsigned)qi << 16) + 4 * r + mix;
        const float delta = at_rsum(g0.x * o0.x + g0.y * o0.y + g0.z * o0.z + g0.w * o0.w + g1.x * o1.x + g1.y * o1.y + g1.z * o1.z +
                                    g1.w * o1.w);
        at_f4 dq0 = {0.f, 0.f, 0.f, 0.f}, dq1 = dq0;
        // S^T and dP^T tiles: entry v = (key 16 t + 4 r + v, query qi); the next tile's products issued ahead, as in the dK / dV kernel
        at_f4 s = at_dot32(Ks + c * kAtRow + 4 * r, q0, q1), dp = at_dot32(Vs + c * kAtRow + 4 * r, g0, g1);
#pragma unroll 1
        for (int t = 0; t < ntk; ++t) {
            const int tn = min(t + 1, ntk - 1);
            const at_f4 s_next = at_dot32(Ks + (16 * tn + c) * kAtRow + 4 * r, q0, q1);
            const at_f4 dp_next = at_dot32(Vs + (16 * tn + c) * kAtRow + 4 * r, g0, g1);
            __builtin_amdgcn_sched_barrier(0);
            at_f4 ds;
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                float p = __builtin_amdgcn_exp2f((s[v] - lse) - lse_lo);
                if (t == ntk - 1) p = 16 * t + 4 * r + v < a.Lk ? p : 0.f;      // (uniform: only the last tile has padding keys)
                const bool keep = at_hash(ctr + (16 * t + v)) >= a.thresh;
                ds[v] = p * ((keep ? dp[v] * a.keep_scale : 0.f) - delta);
            }
            at_accum_t(Ks + 16 * t * kAtRow, r, c, ds, dq0, dq1);           // dQ^T[channel][query] += K^T . dS^T
            s = s_next; dp = dp_next;
        }
        if (qok) {
            float *gq = a.gq.p + n * a.gq.sn + h * 32 + (long long)qi * a.gq.sl + 4 * r;
            *reinterpret_cast<float4 *>(gq) = make_float4(dq0[0] * a.scale, dq0[1] * a.scale, dq0[2] * a.scale, dq0[3] * a.scale);
            *reinterpret_cast<float4 *>(gq + 16) = make_float4(dq1[0] * a.scale, dq1[1] * a.scale, dq1[2] * a.scale, dq1[3] * a.scale);
        }
    }
}

static int at_allow_lds(const void *fn, size_t bytes)
{
    if (bytes <= 64 * 1024) return MSDA_OK;
    const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    return e == hipSuccess ? MSDA_OK : set_error(MSDA_ERR_LAUNCH, hipGetErrorString(e));
}


// ---- bf16 operands (msda_attn32_*_bf16) ------------------------------------------------------------------------------------------
// The same three kernels and the same work split with q, k, v, out, dO and the gradients in bf16 and every product on
// v_mfma_f32_16x16x32_bf16 (fp32 accumulate): one instruction covers a 16 x 16 score tile's whole head dimension.  Softmax,
// log-sum-exp, delta = <dO, O> and dP stay fp32; P (forward, dV) and dS (dK, dQ) are rounded to bf16 only as the operands of
// the products that sum over them; out and the gradients are rounded once.  The pair's operands sit in LDS as bf16 rows
// ([rows][40]: 80-byte rows, 16-byte aligned) and are read two ways: a row (8 channels of one key / query) with one
// ds_read_b128 as the operand of the products over channels, and transposed (4 keys / queries of one channel) with
// ds_read_b64_tr_b16 as the operand of the products over keys / queries.  Every kernel keeps its loops wave-uniform: the
// transposed read needs all 64 lanes active.  LDS <= 2 * 320 * 80 B + 2 * 320 * 4 B = 53.8 KB: at_allow_lds has nothing to ask for.
// The row and transposed reads and the relabelling of the score-tile pairs: msda_attn_tile.h.
// Padding: rows up to a multiple of 32 are zero in LDS; padding keys get -inf scores / zero probabilities, padding queries
// an lse of +inf.  The dropout hash takes the real (query, key) indices: the mask is the fp32 kernels' bit for bit.

// rows [0, L) of two [L][32] bf16 slices -> dst0 / dst1 [Lp][kAbRow]; rows [L, Lp) zero (Lp * 4 16-byte chunks per slice)
__device__ __forceinline__ void ab_load_rows2(uint16_t *dst0, const uint16_t *src0, long long sl0, uint16_t *dst1,
                                              const uint16_t *src1, long long sl1, int L, int Lp)
{
    constexpr int R = (kAtMaxLen * 4 + kAtBlock - 1) / kAtBlock;
    at_bf8 v0[R], v1[R];
#pragma unroll
    for (int k = 0; k < R; ++k) {
        const int i = threadIdx.x + k * kAtBlock, row = i >> 2, c = (i & 3) * 8;
        const bool live = row < L;
        v0[k] = live ? ab_ld8(src0 + (long long)row * sl0 + c) : ab_zero8();
        v1[k] = live ? ab_ld8(src1 + (long long)row * sl1 + c) : ab_zero8();
    }
#pragma unroll
    for (int k = 0; k < R; ++k) {
        const int i = threadIdx.x + k * kAtBlock, row = i >> 2, c = (i & 3) * 8;
        if (row < Lp) {
            *reinterpret_cast<at_bf8 *>(dst0 + row * kAbRow + c) = v0[k];
            *reinterpret_cast<at_bf8 *>(dst1 + row * kAbRow + c) = v1[k];
        }
    }
}

__global__ __launch_bounds__(kAtBlock) void attn32_fwd_bf16_kernel(const AttnArgs<uint16_t> a)
{
    extern __shared__ __attribute__((aligned(16))) uint16_t ab_smem[];
    const int Lkp = (a.Lk + 31) & ~31, npair = Lkp >> 5, ntq = (a.Lq + 15) >> 4;
    uint16_t *Ks = ab_smem, *Vs = ab_smem + Lkp * kAbRow;
    const int pair = (int)blockIdx.x, n = pair / a.H, h = pair % a.H;
    ab_load_rows2(Ks, a.k.p + n * a.k.sn + h * 32, a.k.sl, Vs, a.v.p + n * a.v.sn + h * 32, a.v.sl, a.Lk, Lkp);
    const unsigned mix = at_mix(a.thresh ? a.seed[0] : 0ull, (unsigned)pair);
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, c = lane & 15, r = lane >> 4;
    const uint16_t *qp = a.q.p + n * a.q.sn + h * 32;
    uint16_t *op = a.o.p + n * a.o.sn + h * 32;
    for (int tq = wave; tq < ntq; tq += kAtWaves) {
        const int qi = tq * 16 + c;
        const bool qok = qi < a.Lq;
        at_bf8 qf = ab_zero8();
        if (qok) qf = ab_ld8(qp + (long long)qi * a.q.sl + 8 * r);
        // s[2T + b][v] = score of key 32T + 8r + 4b + v for query qi (raw, then times scale * log2 e)
        at_f4 s[kAtMaxTiles];
#pragma unroll
        for (int T = 0; T < kAtMaxTiles / 2; ++T)
            if (T < npair) ab_pair(Ks, T, r, c, qf, s[2 * T], s[2 * T + 1]);
        float m = -INFINITY;
#pragma unroll
        for (int T = 0; T < kAtMaxTiles / 2; ++T) {
            if (T < npair) {
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    float x = s[2 * T + (j >> 2)][j & 3] * a.scale2;        // (base 2, like the fp32 kernels)
                    if (T == npair - 1) x = 32 * T + 8 * r + j < a.Lk ? x : -INFINITY;
                    s[2 * T + (j >> 2)][j & 3] = x;
                    m = fmaxf(m, x);
                }
            }
        }
        m = at_rmax(m);
        float sum = 0.f;
#pragma unroll
        for (int t = 0; t < kAtMaxTiles; ++t) {
            if (t < 2 * npair) {
#pragma unroll
                for (int v = 0; v < 4; ++v) { s[t][v] = __builtin_amdgcn_exp2f(s[t][v] - m); sum += s[t][v]; }
            }
        }
        sum = at_rsum(sum);
        if (qok && r == 0) a.lse[(long long)pair * a.Lq + qi] = (m + __builtin_amdgcn_logf(sum)) * 0.6931471805599453f;
        const float inv = a.keep_scale / sum;
        at_f4 o0 = {0.f, 0.f, 0.f, 0.f}, o1 = o0;
        const unsigned ctr = ((unsigned)qi << 16) + 8 * r + mix;
#pragma unroll
        for (int T = 0; T < kAtMaxTiles / 2; ++T) {
            if (T < npair) {
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const bool keep = at_hash(ctr + (32 * T + j)) >= a.thresh;
                    s[2 * T + (j >> 2)][j & 3] = keep ? s[2 * T + (j >> 2)][j & 3] * inv : 0.f;
                }
                const at_bf8 pb = ab_pack(s[2 * T], s[2 * T + 1]);          // P^T[key 32T + 8r + j][query qi]
                o0 = ab_mfma(ab_tr(Vs, T, 0, r, c), pb, o0);                // O^T[channel][query] += V^T . P^T
                o1 = ab_mfma(ab_tr(Vs, T, 1, r, c), pb, o1);
            }
        }
        if (qok) {
            uint16_t *orow = op + (long long)qi * a.o.sl + 4 * r;
            ab_st4(orow, o0, 1.f);
            ab_st4(orow + 16, o1, 1.f);
        }
    }
}

// dK, dV: a wavefront owns 16 keys and walks the query pairs
__global__ __launch_bounds__(kAtBlock) void attn32_bwd_kv_bf16_kernel(const AttnArgs<uint16_t> a)
{
    extern __shared__ __attribute__((aligned(16))) uint16_t ab_smem[];
    const int Lqp = (a.Lq + 31) & ~31, npair = Lqp >> 5, ntk = (a.Lk + 15) >> 4;
    uint16_t *Qs = ab_smem, *Gs = ab_smem + Lqp * kAbRow;
    float *lse_s = reinterpret_cast<float *>(Gs + Lqp * kAbRow), *del_s = lse_s + Lqp;
    const int pair = (int)blockIdx.x, n = pair / a.H, h = pair % a.H;
    ab_load_rows2(Qs, a.q.p + n * a.q.sn + h * 32, a.q.sl, Gs, a.go.p + n * a.go.sn + h * 32, a.go.sl, a.Lq, Lqp);
    const unsigned mix = at_mix(a.thresh ? a.seed[0] : 0ull, (unsigned)pair);
    __syncthreads();
    for (int qi = threadIdx.x; qi < Lqp; qi += kAtBlock) {
        float d = 0.f;
        if (qi < a.Lq) {
            const uint16_t *orow = a.o.p + n * a.o.sn + h * 32 + (long long)qi * a.o.sl, *grow = Gs + qi * kAbRow;
#pragma unroll
            for (int k8 = 0; k8 < 4; ++k8) {
                const at_bf8 ov = ab_ld8(orow + 8 * k8), gv = ab_ld8(grow + 8 * k8);
#pragma unroll
                for (int j = 0; j < 8; ++j) d += ab_f(ov[j]) * ab_f(gv[j]);
            }
        }
        del_s[qi] = d;
        lse_s[qi] = qi < a.Lq ? a.lse[(long long)pair * a.Lq + qi] * 1.4426950408889634f : INFINITY;
    }
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, c = lane & 15, r = lane >> 4;
    for (int tk = wave; tk < ntk; tk += kAtWaves) {
        const int key = tk * 16 + c;
        const bool kok = key < a.Lk;
        at_bf8 kf = ab_zero8(), vf = ab_zero8();
        if (kok) {
            kf = ab_ld8(a.k.p + n * a.k.sn + h * 32 + (long long)key * a.k.sl + 8 * r);
            vf = ab_ld8(a.v.p + n * a.v.sn + h * 32 + (long long)key * a.v.sl + 8 * r);
        }
        const unsigned ctr = (unsigned)key + ((unsigned)(8 * r) << 16) + mix;
        at_f4 dv0 = {0.f, 0.f, 0.f, 0.f}, dv1 = dv0, dk0 = dv0, dk1 = dv0;
#pragma unroll 1
        for (int T = 0; T < npair; ++T) {
            // S and dP tiles of the pair: entry (b, v) = (query 32T + 8r + 4b + v, key)
            at_f4 s[2], dp[2];
            ab_pair(Qs, T, r, c, kf, s[0], s[1]);
            ab_pair(Gs, T, r, c, vf, dp[0], dp[1]);
            const float *lq = lse_s + 32 * T + 8 * r, *dq = del_s + 32 * T + 8 * r;
            const float4 l0 = *reinterpret_cast<const float4 *>(lq), l1 = *reinterpret_cast<const float4 *>(lq + 4);
            const float4 d0 = *reinterpret_cast<const float4 *>(dq), d1 = *reinterpret_cast<const float4 *>(dq + 4);
            const float lsv[8] = {l0.x, l0.y, l0.z, l0.w, l1.x, l1.y, l1.z, l1.w}, dlv[8] = {d0.x, d0.y, d0.z, d0.w, d1.x, d1.y, d1.z, d1.w};
            at_f4 pd[2], ds[2];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int b = j >> 2, v = j & 3;
                const float p = __builtin_amdgcn_exp2f(fmaf(s[b][v], a.scale2, -lsv[j]));
                const bool keep = at_hash(ctr + ((unsigned)(32 * T + j) << 16)) >= a.thresh;
                pd[b][v] = keep ? p * a.keep_scale : 0.f;
                ds[b][v] = p * ((keep ? dp[b][v] * a.keep_scale : 0.f) - dlv[j]);
            }
            const at_bf8 pb = ab_pack(pd[0], pd[1]), sb = ab_pack(ds[0], ds[1]);
            dv0 = ab_mfma(ab_tr(Gs, T, 0, r, c), pb, dv0);                  // dV^T[channel][key] += dO^T . P_drop
            dv1 = ab_mfma(ab_tr(Gs, T, 1, r, c), pb, dv1);
            dk0 = ab_mfma(ab_tr(Qs, T, 0, r, c), sb, dk0);                  // dK^T[channel][key] += Q^T . dS
            dk1 = ab_mfma(ab_tr(Qs, T, 1, r, c), sb, dk1);
        }
        if (kok) {
            uint16_t *gvr = a.gv.p + n * a.gv.sn + h * 32 + (long long)key * a.gv.sl + 4 * r;
            uint16_t *gkr = a.gk.p + n * a.gk.sn + h * 32 + (long long)key * a.gk.sl + 4 * r;
            ab_st4(gvr, dv0, 1.f); ab_st4(gvr + 16, dv1, 1.f);
            ab_st4(gkr, dk0, a.scale); ab_st4(gkr + 16, dk1, a.scale);
        }
    }
}

// dQ: a wavefront owns 16 queries and walks the key pairs
__global__ __launch_bounds__(kAtBlock) void attn32_bwd_q_bf16_kernel(const AttnArgs<uint16_t> a)
{
    extern __shared__ __attribute__((aligned(16))) uint16_t ab_smem[];
    const int Lkp = (a.Lk + 31) & ~31, npair = Lkp >> 5, ntq = (a.Lq + 15) >> 4;
    uint16_t *Ks = ab_smem, *Vs = ab_smem + Lkp * kAbRow;
    const int pair = (int)blockIdx.x, n = pair / a.H, h = pair % a.H;
    ab_load_rows2(Ks, a.k.p + n * a.k.sn + h * 32, a.k.sl, Vs, a.v.p + n * a.v.sn + h * 32, a.v.sl, a.Lk, Lkp);
    const unsigned mix = at_mix(a.thresh ? a.seed[0] : 0ull, (unsigned)pair);
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, c = lane & 15, r = lane >> 4;
    for (int tq = wave; tq < ntq; tq += kAtWaves) {
        const int qi = tq * 16 + c;
        const bool qok = qi < a.Lq;
        at_bf8 qf = ab_zero8(), gf = ab_zero8(), of = ab_zero8();
        float lse = INFINITY;
        if (qok) {
            qf = ab_ld8(a.q.p + n * a.q.sn + h * 32 + (long long)qi * a.q.sl + 8 * r);
            gf = ab_ld8(a.go.p + n * a.go.sn + h * 32 + (long long)qi * a.go.sl + 8 * r);
            of = ab_ld8(a.o.p + n * a.o.sn + h * 32 + (long long)qi * a.o.sl + 8 * r);
            lse = a.lse[(long long)pair * a.Lq + qi] * 1.4426950408889634f;
        }
        float d = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) d += ab_f(gf[j]) * ab_f(of[j]);
        const float delta = at_rsum(d);
        const unsigned ctr = ((unsigned)qi << 16) + 8 * r + mix;
        at_f4 dq0 = {0.f, 0.f, 0.f, 0.f}, dq1 = dq0;
#pragma unroll 1
        for (int T = 0; T < npair; ++T) {
            // S^T and dP^T tiles of the pair: entry (b, v) = (key 32T + 8r + 4b + v, query qi)
            at_f4 s[2], dp[2];
            ab_pair(Ks, T, r, c, qf, s[0], s[1]);
            ab_pair(Vs, T, r, c, gf, dp[0], dp[1]);
            at_f4 ds[2];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int b = j >> 2, v = j & 3;
                float p = __builtin_amdgcn_exp2f(fmaf(s[b][v], a.scale2, -lse));
                p = 32 * T + 8 * r + j < a.Lk ? p : 0.f;
                const bool keep = at_hash(ctr + (32 * T + j)) >= a.thresh;
                ds[b][v] = p * ((keep ? dp[b][v] * a.keep_scale : 0.f) - delta);
            }
            const at_bf8 sb = ab_pack(ds[0], ds[1]);
            dq0 = ab_mfma(ab_tr(Ks, T, 0, r, c), sb, dq0);                  // dQ^T[channel][query] += K^T . dS^T
            dq1 = ab_mfma(ab_tr(Ks, T, 1, r, c), sb, dq1);
        }
        if (qok) {
            uint16_t *gq = a.gq.p + n * a.gq.sn + h * 32 + (long long)qi * a.gq.sl + 4 * r;
            ab_st4(gq, dq0, a.scale); ab_st4(gq + 16, dq1, a.scale);
        }
    }
}

}  // namespace msda

using msda::attn_view;

extern "C" {

int msda_attn32_supported(int Lq, int Lk, int head_dim)
{
    return head_dim == 32 && Lq >= 1 && Lk >= 1 && Lq <= msda::kAtMaxLen && Lk <= msda::kAtMaxLen;
}

// Each entry: check, bind (msda_attn_args.h: every refusal comes before any launch), size the grid and the LDS, launch.
// One workgroup per pair, or two of the fp32 kernels under MSDA_ATTN_HALVES=2; a row of LDS per key (forward, dQ) or query (dK / dV).

int msda_attn32_forward_f32(const float *q, long long q_sn, long long q_sl, const float *k, long long k_sn, long long k_sl,
                            const float *v, long long v_sn, long long v_sl, int N, int H, int Lq, int Lk, float scale,
                            float dropout_p, const unsigned long long *seed, float *out, long long o_sn, long long o_sl, float *lse,
                            msda_stream_t stream)
{
    const char *who = "msda_attn32_forward_f32";
    msda::AttnArgs<float> a{};
    const int halves = msda::tuning_int("MSDA_ATTN_HALVES", 1) == 2 ? 2 : 1;
    if (int rc = msda::attn_check(a, who, msda::kAtMaxLen, N, H, Lq, Lk, halves, scale, dropout_p, seed, nullptr, 0)) return rc;
    if (int rc = msda::attn_bind_forward(a, who, attn_view(q, q_sn, q_sl), attn_view(k, k_sn, k_sl), attn_view(v, v_sn, v_sl),
                                         attn_view(out, o_sn, o_sl), lse)) return rc;
    const size_t lds = (size_t)2 * ((Lk + 15) & ~15) * msda::kAtRow * sizeof(float);
    if (int rc = msda::at_allow_lds(reinterpret_cast<const void *>(msda::attn32_fwd_kernel), lds)) return rc;
    hipLaunchKernelGGL(msda::attn32_fwd_kernel, dim3((unsigned)(N * H * a.wpp)), dim3(msda::kAtBlock), lds, (hipStream_t)stream, a);
    return msda::check_launch("msda attention forward (head_dim 32)");
}

int msda_attn32_backward_f32(const float *q, long long q_sn, long long q_sl, const float *k, long long k_sn, long long k_sl,
                             const float *v, long long v_sn, long long v_sl, const float *out, long long o_sn, long long o_sl,
                             const float *lse, const float *grad_out, long long go_sn, long long go_sl, int N, int H, int Lq, int Lk,
                             float scale, float dropout_p, const unsigned long long *seed, float *grad_q, long long gq_sn,
                             long long gq_sl, float *grad_k, long long gk_sn, long long gk_sl, float *grad_v, long long gv_sn,
                             long long gv_sl, msda_stream_t stream)
{
    const char *who = "msda_attn32_backward_f32";
    msda::AttnArgs<float> a{};
    const int halves = msda::tuning_int("MSDA_ATTN_HALVES", 1) == 2 ? 2 : 1;
    if (int rc = msda::attn_check(a, who, msda::kAtMaxLen, N, H, Lq, Lk, halves, scale, dropout_p, seed, nullptr, 0)) return rc;
    if (int rc = msda::attn_bind_backward(a, who, attn_view(q, q_sn, q_sl), attn_view(k, k_sn, k_sl), attn_view(v, v_sn, v_sl),
                                          attn_view(out, o_sn, o_sl), lse, attn_view(grad_out, go_sn, go_sl),
                                          attn_view(grad_q, gq_sn, gq_sl), attn_view(grad_k, gk_sn, gk_sl),
                                          attn_view(grad_v, gv_sn, gv_sl))) return rc;
    const int Lqp = (Lq + 15) & ~15, Lkp = (Lk + 15) & ~15;
    const size_t lds_kv = ((size_t)2 * Lqp * msda::kAtRow + 3 * Lqp) * sizeof(float), lds_q = (size_t)2 * Lkp * msda::kAtRow * sizeof(float);
    if (int rc = msda::at_allow_lds(reinterpret_cast<const void *>(msda::attn32_bwd_kv_kernel), lds_kv)) return rc;
    if (int rc = msda::at_allow_lds(reinterpret_cast<const void *>(msda::attn32_bwd_q_kernel), lds_q)) return rc;
    const dim3 grid((unsigned)(N * H * a.wpp));
    hipLaunchKernelGGL(msda::attn32_bwd_kv_kernel, grid, dim3(msda::kAtBlock), lds_kv, (hipStream_t)stream, a);
    if (int rc = msda::check_launch("msda attention backward (dK, dV)")) return rc;
    hipLaunchKernelGGL(msda::attn32_bwd_q_kernel, grid, dim3(msda::kAtBlock), lds_q, (hipStream_t)stream, a);
    return msda::check_launch("msda attention backward (dQ)");
}

// bf16 operands: the same checks, the fp32 entries' random stream; one workgroup per pair, rows padded to a multiple of 32
int msda_attn32_forward_bf16(const uint16_t *q, long long q_sn, long long q_sl, const uint16_t *k, long long k_sn, long long k_sl,
                             const uint16_t *v, long long v_sn, long long v_sl, int N, int H, int Lq, int Lk, float scale,
                             float dropout_p, const unsigned long long *seed, uint16_t *out, long long o_sn, long long o_sl,
                             float *lse, msda_stream_t stream)
{
    const char *who = "msda_attn32_forward_bf16";
    msda::AttnArgs<uint16_t> a{};
    if (int rc = msda::attn_check(a, who, msda::kAtMaxLen, N, H, Lq, Lk, 1, scale, dropout_p, seed, nullptr, 0)) return rc;
    if (int rc = msda::attn_bind_forward(a, who, attn_view(q, q_sn, q_sl), attn_view(k, k_sn, k_sl), attn_view(v, v_sn, v_sl),
                                         attn_view(out, o_sn, o_sl), lse)) return rc;
    const size_t lds = (size_t)2 * ((Lk + 31) & ~31) * msda::kAbRow * sizeof(uint16_t);
    if (int rc = msda::at_allow_lds(reinterpret_cast<const void *>(msda::attn32_fwd_bf16_kernel), lds)) return rc;
    hipLaunchKernelGGL(msda::attn32_fwd_bf16_kernel, dim3((unsigned)(N * H)), dim3(msda::kAtBlock), lds, (hipStream_t)stream, a);
    return msda::check_launch("msda attention forward (head_dim 32, bf16)");
}

int msda_attn32_backward_bf16(const uint16_t *q, long long q_sn, long long q_sl, const uint16_t *k, long long k_sn, long long k_sl,
                              const uint16_t *v, long long v_sn, long long v_sl, const uint16_t *out, long long o_sn, long long o_sl,
                              const float *lse, const uint16_t *grad_out, long long go_sn, long long go_sl, int N, int H, int Lq,
                              int Lk, float scale, float dropout_p, const unsigned long long *seed, uint16_t *grad_q,
                              long long gq_sn, long long gq_sl, uint16_t *grad_k, long long gk_sn, long long gk_sl,
                              uint16_t *grad_v, long long gv_sn, long long gv_sl, msda_stream_t stream)
{
    const char *who = "msda_attn32_backward_bf16";
    msda::AttnArgs<uint16_t> a{};
    if (int rc = msda::attn_check(a, who, msda::kAtMaxLen, N, H, Lq, Lk, 1, scale, dropout_p, seed, nullptr, 0)) return rc;
    if (int rc = msda::attn_bind_backward(a, who, attn_view(q, q_sn, q_sl), attn_view(k, k_sn, k_sl), attn_view(v, v_sn, v_sl),
                                          attn_view(out, o_sn, o_sl), lse, attn_view(grad_out, go_sn, go_sl),
                                          attn_view(grad_q, gq_sn, gq_sl), attn_view(grad_k, gk_sn, gk_sl),
                                          attn_view(grad_v, gv_sn, gv_sl))) return rc;
    const int Lqp = (Lq + 31) & ~31, Lkp = (Lk + 31) & ~31;
    const size_t lds_kv = (size_t)2 * Lqp * msda::kAbRow * sizeof(uint16_t) + (size_t)2 * Lqp * sizeof(float);
    const size_t lds_q = (size_t)2 * Lkp * msda::kAbRow * sizeof(uint16_t);
    if (int rc = msda::at_allow_lds(reinterpret_cast<const void *>(msda::attn32_bwd_kv_bf16_kernel), lds_kv)) return rc;
    if (int rc = msda::at_allow_lds(reinterpret_cast<const void *>(msda::attn32_bwd_q_bf16_kernel), lds_q)) return rc;
    const dim3 grid((unsigned)(N * H));
    hipLaunchKernelGGL(msda::attn32_bwd_kv_bf16_kernel, grid, dim3(msda::kAtBlock), lds_kv, (hipStream_t)stream, a);
    if (int rc = msda::check_launch("msda attention backward (dK, dV; bf16)")) return rc;
    hipLaunchKernelGGL(msda::attn32_bwd_q_bf16_kernel, grid, dim3(msda::kAtBlock), lds_q, (hipStream_t)stream, a);
    return msda::check_launch("msda attention backward (dQ; bf16)");
}

}  // extern "C"
