// Swin window attention (UVHand models/swin_transformer.py:68-142 WindowAttention, :199-245 SwinTransformerBlock's pad / roll /
// partition / reverse / crop, :339-357 BasicLayer's shift mask) for head_dim 32 and windows of at most 12 x 12, fp32.
//
// Input: the qkv Linear's output on the REAL tokens only, qkv [B * H * W, 3 C] with columns (3, nH, 32); output [B * H * W, C]
// with columns (nH, 32) for the proj Linear.  Pad, roll, partition, reverse and crop are index arithmetic: window position
// (Y, X) = (wy ws + i, wx ws + j) of the shifted frame reads source ((Y + s) mod Hp, (X + s) mod Wp); a source inside H x W is
// row b H W + y W + x, anything else is a padded token.  norm1 runs before F.pad, so a padded token's qkv is exactly qkv.bias:
// its k and v are the bias's k and v parts, and its query's output is cropped away (never computed past the tile it shares
// with real queries, never written).
// Scores: (q * scale) . k + table[(dy + ws - 1) (2 ws - 1) + dx + ws - 1] (dy, dx = query - key in window coordinates: the
// reference's relative_position_index) + (-100 where the shift regions 3 r(Y) + r(X) of query and key differ, s > 0).
//
// A workgroup owns one (image, window, head) pair and has one wavefront per 16-token tile of the window.  The products run on
// v_mfma_f32_16x16x4_f32 with the helpers and conventions of msda_attn_tile.h (S^T tiles in the forward and dQ, S tiles in dK / dV, operands
// in LDS as [rows][36]).
//   forward   one launch: out for real queries, the log-sum-exp (natural log) of every real query, lse [pairs][N].
//   backward  three launches.  kv: a wavefront owns 16 keys and walks the query tiles: dK, dV of real keys into grad_qkv, and
//             the sum over the pair's padded keys (the bias part of their gradient) into a per-pair partial.  q: a wavefront
//             owns 16 queries: dQ into grad_qkv, its dS rows into LDS; then the thread that owns table entry e sums
//             dS[i][j(i, e)] over the queries i in order (at most one key j per query has offset e) into a per-pair partial.
//             reduce: one wavefront per output of grad_table [(2 ws - 1)^2, nH] and grad_bias [3 C] (q part zero) sums the
//             partials of its head over (image, window): lane l takes every 64th partial in order, then a fixed butterfly.
// Every real token is one query and one key of exactly one window per head: grad_qkv's elements are each written once.
// No atomics, fixed summation order: bitwise reproducible.  No allocation, no host synchronisation.
#include <math.h>

#include "msda_attn_tile.h"
#include "msda_common.h"
#include "msda_launch.h"

namespace msda {

namespace {

constexpr int kSwMaxWs = 12, kSwMaxN = kSwMaxWs * kSwMaxWs, kSwMaxTiles = (kSwMaxN + 15) / 16;
constexpr int kSwMaxBlock = kSwMaxTiles * 64, kSwRedBlock = 256;
constexpr float kLog2e = 1.4426950408889634f;

__device__ __forceinline__ void sw_st4(float *p, const at_f4 &v) { *reinterpret_cast<float4 *>(p) = make_float4(v[0], v[1], v[2], v[3]); }
__device__ __forceinline__ float4 sw_scale4(float4 v, float s) { return make_float4(v.x * s, v.y * s, v.z * s, v.w * s); }

struct SwArgs {
    int B, H, W, C, nH, ws, s, Hp, Wp, nWx, nW, N, E;
    float scale;
    const float *qkv, *bias, *table, *out, *gout;      // bias: null when the Linear has none (padded k, v = 0)
    float *o, *lse, *gqkv, *gtable, *gbias, *pt, *pb;  // pt [pairs][E], pb [pairs][64]: the backward's per-pair partials
};

// token t (< N) of window w of image b: its qkv row (-1: padded), its relative-position part and its shift region
struct SwTok { int row, rel, reg; };

__device__ __forceinline__ int sw_region(int Y, int Hp, int ws, int s) { return Y < Hp - ws ? 0 : (Y < Hp - s ? 1 : 2); }

__device__ __forceinline__ SwTok sw_token(const SwArgs &a, int b, int w, int t, bool as_key)
{
    const int i = t / a.ws, j = t - i * a.ws;
    const int Y = (w / a.nWx) * a.ws + i, X = (w % a.nWx) * a.ws + j;
    int y = Y + a.s, x = X + a.s;
    y -= y >= a.Hp ? a.Hp : 0;
    x -= x >= a.Wp ? a.Wp : 0;
    SwTok k;
    k.row = (y < a.H && x < a.W) ? (b * a.H + y) * a.W + x : -1;
    const int w2 = 2 * a.ws - 1;
    k.rel = as_key ? (a.ws - 1 - i) * w2 + (a.ws - 1 - j) : i * w2 + j;      // query part + key part = the table index
    k.reg = a.s > 0 ? 3 * sw_region(Y, a.Hp, a.ws, a.s) + sw_region(X, a.Wp, a.ws, a.s) : 0;
    return k;
}

// the k (part 1) or v (part 2) channels c4 .. c4 + 3 of token `row` (padded: the bias's, or zero), head h
__device__ __forceinline__ float4 sw_kv4(const SwArgs &a, int row, int part, int h, int c4)
{
    if (row >= 0) return ld4(a.qkv + (long long)row * 3 * a.C + part * a.C + h * 32 + c4);
    return a.bias != nullptr ? ld4(a.bias + part * a.C + h * 32 + c4) : at_zero4();
}

__device__ __forceinline__ void sw_pair(const SwArgs &a, int &b, int &w, int &h)
{
    const int pair = (int)blockIdx.x;
    h = pair % a.nH;
    w = (pair / a.nH) % a.nW;
    b = pair / (a.nH * a.nW);
}

// LDS: rows [Np][kAtRow] of k and v (part 1, 2) or q (scaled) and dO; the head's table slice; per token info (int)
__device__ __forceinline__ void sw_load_table(const SwArgs &a, int h, float *tbl)
{
    for (int e = threadIdx.x; e < a.E; e += blockDim.x) tbl[e] = a.table[(long long)e * a.nH + h];
}

// score of (query info qrel / qreg, key info kinf = rel | reg << 16) in base 2; key >= N: -inf
__device__ __forceinline__ float sw_score2(float dot, const float *tbl, int qrel, int qreg, int kinf, bool kok)
{
    float sc = dot + tbl[qrel + (kinf & 0xffff)];
    if ((kinf >> 16) != qreg) sc += -100.0f;
    return kok ? sc * kLog2e : -INFINITY;
}

__global__ __launch_bounds__(kSwMaxBlock) void swin_fwd_kernel(const SwArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float sw_smem[];
    const int Np = (a.N + 15) & ~15, Ep = (a.E + 3) & ~3;
    float *Ks = sw_smem, *Vs = Ks + Np * kAtRow, *tbl = Vs + Np * kAtRow;
    int *kinf = reinterpret_cast<int *>(tbl + Ep), *rows = kinf + Np;
    int b, w, h;
    sw_pair(a, b, w, h);
    for (int t = threadIdx.x; t < Np; t += blockDim.x) {
        SwTok k = {-1, 0, 0};
        if (t < a.N) k = sw_token(a, b, w, t, true);
        kinf[t] = k.rel | (k.reg << 16);
        rows[t] = k.row;
    }
    sw_load_table(a, h, tbl);
    for (int i = threadIdx.x; i < Np * 8; i += blockDim.x) {
        const int t = i >> 3, c4 = (i & 7) * 4;
        float4 kv = at_zero4(), vv = at_zero4();
        if (t < a.N) {
            const int row = sw_token(a, b, w, t, true).row;
            kv = sw_kv4(a, row, 1, h, c4);
            vv = sw_kv4(a, row, 2, h, c4);
        }
        *reinterpret_cast<float4 *>(Ks + t * kAtRow + c4) = kv;
        *reinterpret_cast<float4 *>(Vs + t * kAtRow + c4) = vv;
    }
    __syncthreads();
    const int ntk = Np >> 4, tq = threadIdx.x >> 6, lane = threadIdx.x & 63, c = lane & 15, r = lane >> 4;
    const int qi = tq * 16 + c;
    const int qrow = qi < a.N ? rows[qi] : -1;
    if (!__any(qrow >= 0)) return;                                      // a tile of padded tokens only: nothing to write
    const SwTok qt = sw_token(a, b, w, qi < a.N ? qi : 0, false);
    float4 q0 = at_zero4(), q1 = at_zero4();
    if (qrow >= 0) {
        const float *qp = a.qkv + (long long)qrow * 3 * a.C + h * 32 + 4 * r;
        q0 = sw_scale4(ld4(qp), a.scale);
        q1 = sw_scale4(ld4(qp + 16), a.scale);
    }
    at_f4 s[kSwMaxTiles];
    float m = -INFINITY;
#pragma unroll
    for (int t = 0; t < kSwMaxTiles; ++t) {
        if (t < ntk) {
            s[t] = at_dot32(Ks + (16 * t + c) * kAtRow + 4 * r, q0, q1);
            const int4 ki = *reinterpret_cast<const int4 *>(kinf + 16 * t + 4 * r);
            const int kv[4] = {ki.x, ki.y, ki.z, ki.w};
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                s[t][v] = sw_score2(s[t][v], tbl, qt.rel, qt.reg, kv[v], 16 * t + 4 * r + v < a.N);
                m = fmaxf(m, s[t][v]);
            }
        }
    }
    m = at_rmax(m);
    float sum = 0.f;
#pragma unroll
    for (int t = 0; t < kSwMaxTiles; ++t) {
        if (t < ntk) {
#pragma unroll
            for (int v = 0; v < 4; ++v) { s[t][v] = __builtin_amdgcn_exp2f(s[t][v] - m); sum += s[t][v]; }
        }
    }
    sum = at_rsum(sum);
    const long long pair = blockIdx.x;
    if (qrow >= 0 && r == 0) a.lse[pair * a.N + qi] = (m + __builtin_amdgcn_logf(sum)) * 0.6931471805599453f;
    const float inv = 1.f / sum;
    at_f4 o0 = {0.f, 0.f, 0.f, 0.f}, o1 = o0;
#pragma unroll
    for (int t = 0; t < kSwMaxTiles; ++t) {
        if (t < ntk) {
#pragma unroll
            for (int v = 0; v < 4; ++v) s[t][v] *= inv;
            at_accum_t(Vs + 16 * t * kAtRow, r, c, s[t], o0, o1);
        }
    }
    if (qrow >= 0) {
        float *op = a.o + (long long)qrow * a.C + h * 32 + 4 * r;
        sw_st4(op, o0);
        sw_st4(op + 16, o1);
    }
}

// dK, dV: wavefront tk owns keys 16 tk .. 16 tk + 15 and walks the query tiles (S tiles: rows = queries)
__global__ __launch_bounds__(kSwMaxBlock) void swin_bwd_kv_kernel(const SwArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float sw_smem[];
    const int Np = (a.N + 15) & ~15, Ep = (a.E + 3) & ~3, ntq = Np >> 4;
    float *Qs = sw_smem, *Gs = Qs + Np * kAtRow, *tbl = Gs + Np * kAtRow, *lse_s = tbl + Ep, *del_s = lse_s + Np;
    float *part = del_s + Np;                                           // [waves][64]
    int *qinf = reinterpret_cast<int *>(part + ntq * 64), *rows = qinf + Np, *tany = rows + Np;
    int b, w, h;
    sw_pair(a, b, w, h);
    const long long pair = blockIdx.x;
    for (int t = threadIdx.x; t < Np; t += blockDim.x) {
        SwTok q = {-1, 0, 0};
        if (t < a.N) q = sw_token(a, b, w, t, false);
        qinf[t] = q.rel | (q.reg << 16);
        rows[t] = q.row;
    }
    sw_load_table(a, h, tbl);
    for (int i = threadIdx.x; i < Np * 8; i += blockDim.x) {
        const int t = i >> 3, c4 = (i & 7) * 4;
        const int row = t < a.N ? sw_token(a, b, w, t, false).row : -1;
        float4 qv = at_zero4(), gv = at_zero4();
        if (row >= 0) {
            qv = sw_scale4(ld4(a.qkv + (long long)row * 3 * a.C + h * 32 + c4), a.scale);
            gv = ld4(a.gout + (long long)row * a.C + h * 32 + c4);
        }
        *reinterpret_cast<float4 *>(Qs + t * kAtRow + c4) = qv;
        *reinterpret_cast<float4 *>(Gs + t * kAtRow + c4) = gv;
    }
    __syncthreads();
    for (int t = threadIdx.x; t < Np; t += blockDim.x) {
        const int row = rows[t];
        float d = 0.f;
        if (row >= 0) {
            const float *orow = a.o + (long long)row * a.C + h * 32, *grow = Gs + t * kAtRow;
#pragma unroll
            for (int k4 = 0; k4 < 8; ++k4) {
                const float4 ov = ld4(orow + 4 * k4), gv = ld4(grow + 4 * k4);
                d += ov.x * gv.x + ov.y * gv.y + ov.z * gv.z + ov.w * gv.w;
            }
        }
        del_s[t] = d;
        lse_s[t] = row >= 0 ? a.lse[pair * a.N + t] * kLog2e : INFINITY;    // padded queries: probabilities 0
    }
    for (int t = threadIdx.x; t < ntq; t += blockDim.x) {
        int any = 0;
        for (int u = 0; u < 16; ++u) any |= rows[16 * t + u] >= 0;
        tany[t] = any;
    }
    __syncthreads();
    const int tk = threadIdx.x >> 6, lane = threadIdx.x & 63, c = lane & 15, r = lane >> 4;
    const int key = tk * 16 + c;
    const bool kok = key < a.N;
    const SwTok kt = sw_token(a, b, w, kok ? key : 0, true);
    const int krow = kok ? kt.row : -1;
    float4 k0 = at_zero4(), k1 = at_zero4(), v0 = at_zero4(), v1 = at_zero4();
    if (kok) {
        k0 = sw_kv4(a, krow, 1, h, 4 * r); k1 = sw_kv4(a, krow, 1, h, 16 + 4 * r);
        v0 = sw_kv4(a, krow, 2, h, 4 * r); v1 = sw_kv4(a, krow, 2, h, 16 + 4 * r);
    }
    at_f4 dv0 = {0.f, 0.f, 0.f, 0.f}, dv1 = dv0, dk0 = dv0, dk1 = dv0;
#pragma unroll 1
    for (int t = 0; t < ntq; ++t) {
        if (!tany[t]) continue;
        const at_f4 s = at_dot32(Qs + (16 * t + c) * kAtRow + 4 * r, k0, k1);
        const at_f4 dp = at_dot32(Gs + (16 * t + c) * kAtRow + 4 * r, v0, v1);
        const float4 ls = ld4(lse_s + 16 * t + 4 * r), dl = ld4(del_s + 16 * t + 4 * r);
        const int4 qi4 = *reinterpret_cast<const int4 *>(qinf + 16 * t + 4 * r);
        const float lsv[4] = {ls.x, ls.y, ls.z, ls.w}, dlv[4] = {dl.x, dl.y, dl.z, dl.w};
        const int qv[4] = {qi4.x, qi4.y, qi4.z, qi4.w};
        at_f4 pd, ds;
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            // (query info and key info swap roles: the table index is the sum of the two parts either way)
            const float sc = sw_score2(s[v], tbl, qv[v] & 0xffff, qv[v] >> 16, (kt.rel & 0xffff) | (kt.reg << 16), true);
            const float p = __builtin_amdgcn_exp2f(sc - lsv[v]);
            pd[v] = p;
            ds[v] = p * (dp[v] - dlv[v]);
        }
        at_accum_t(Gs + 16 * t * kAtRow, r, c, pd, dv0, dv1);           // dV^T[channel][key] += dO^T . P
        at_accum_t(Qs + 16 * t * kAtRow, r, c, ds, dk0, dk1);           // dK^T[channel][key] += (q scale)^T . dS
    }
    if (krow >= 0) {
        float *gk = a.gqkv + (long long)krow * 3 * a.C + a.C + h * 32 + 4 * r, *gv = gk + a.C;
        sw_st4(gk, dk0); sw_st4(gk + 16, dk1);
        sw_st4(gv, dv0); sw_st4(gv + 16, dv1);
    }
    // padded keys of this tile: their k / v gradients summed (a butterfly over the 16 keys), then over the wavefronts in order
    const bool kpad = kok && krow < 0;
    float acc[16];
#pragma unroll
    for (int v = 0; v < 4; ++v) {
        acc[v] = kpad ? dk0[v] : 0.f; acc[4 + v] = kpad ? dk1[v] : 0.f;
        acc[8 + v] = kpad ? dv0[v] : 0.f; acc[12 + v] = kpad ? dv1[v] : 0.f;
    }
#pragma unroll
    for (int m = 1; m < 16; m <<= 1) {
#pragma unroll
        for (int u = 0; u < 16; ++u) acc[u] += __shfl_xor(acc[u], m);
    }
    if (c == 0) {
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            part[tk * 64 + 4 * r + v] = acc[v];
            part[tk * 64 + 16 + 4 * r + v] = acc[4 + v];
            part[tk * 64 + 32 + 4 * r + v] = acc[8 + v];
            part[tk * 64 + 48 + 4 * r + v] = acc[12 + v];
        }
    }
    __syncthreads();
    if (threadIdx.x < 64) {
        float sum = 0.f;
        for (int u = 0; u < ntq; ++u) sum += part[u * 64 + threadIdx.x];
        a.pb[pair * 64 + threadIdx.x] = sum;
    }
}

// dQ: wavefront tq owns queries 16 tq .. 16 tq + 15 and walks the key tiles (S^T tiles, as the forward); dS rows into LDS,
// then the per-pair table partial
__global__ __launch_bounds__(kSwMaxBlock) void swin_bwd_q_kernel(const SwArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float sw_smem[];
    const int Np = (a.N + 15) & ~15, Ep = (a.E + 3) & ~3, ntk = Np >> 4, dss = Np + 4;
    float *Ks = sw_smem, *Vs = Ks + Np * kAtRow, *tbl = Vs + Np * kAtRow, *dS = tbl + Ep;
    int *kinf = reinterpret_cast<int *>(dS + Np * dss), *rows = kinf + Np;
    int b, w, h;
    sw_pair(a, b, w, h);
    const long long pair = blockIdx.x;
    for (int t = threadIdx.x; t < Np; t += blockDim.x) {
        SwTok k = {-1, 0, 0};
        if (t < a.N) k = sw_token(a, b, w, t, true);
        kinf[t] = k.rel | (k.reg << 16);
        rows[t] = k.row;
    }
    sw_load_table(a, h, tbl);
    for (int i = threadIdx.x; i < Np * 8; i += blockDim.x) {
        const int t = i >> 3, c4 = (i & 7) * 4;
        float4 kv = at_zero4(), vv = at_zero4();
        if (t < a.N) {
            const int row = sw_token(a, b, w, t, true).row;
            kv = sw_kv4(a, row, 1, h, c4);
            vv = sw_kv4(a, row, 2, h, c4);
        }
        *reinterpret_cast<float4 *>(Ks + t * kAtRow + c4) = kv;
        *reinterpret_cast<float4 *>(Vs + t * kAtRow + c4) = vv;
    }
    __syncthreads();
    const int tq = threadIdx.x >> 6, lane = threadIdx.x & 63, c = lane & 15, r = lane >> 4;
    const int qi = tq * 16 + c;
    const int qrow = qi < a.N ? rows[qi] : -1;
    float *dsrow = dS + qi * dss;
    if (__any(qrow >= 0)) {
        const SwTok qt = sw_token(a, b, w, qi < a.N ? qi : 0, false);
        float4 q0 = at_zero4(), q1 = at_zero4(), g0 = at_zero4(), g1 = at_zero4(), o0 = at_zero4(), o1 = at_zero4();
        float lse = INFINITY;
        if (qrow >= 0) {
            const float *qp = a.qkv + (long long)qrow * 3 * a.C + h * 32 + 4 * r;
            const float *gp = a.gout + (long long)qrow * a.C + h * 32 + 4 * r, *opp = a.o + (long long)qrow * a.C + h * 32 + 4 * r;
            q0 = sw_scale4(ld4(qp), a.scale); q1 = sw_scale4(ld4(qp + 16), a.scale);
            g0 = ld4(gp); g1 = ld4(gp + 16); o0 = ld4(opp); o1 = ld4(opp + 16);
            lse = a.lse[pair * a.N + qi] * kLog2e;
        }
        const float delta = at_rsum(g0.x * o0.x + g0.y * o0.y + g0.z * o0.z + g0.w * o0.w + g1.x * o1.x + g1.y * o1.y + g1.z * o1.z +
                                    g1.w * o1.w);
        at_f4 dq0 = {0.f, 0.f, 0.f, 0.f}, dq1 = dq0;
#pragma unroll 1
        for (int t = 0; t < ntk; ++t) {
            const at_f4 s = at_dot32(Ks + (16 * t + c) * kAtRow + 4 * r, q0, q1);
            const at_f4 dp = at_dot32(Vs + (16 * t + c) * kAtRow + 4 * r, g0, g1);
            const int4 ki = *reinterpret_cast<const int4 *>(kinf + 16 * t + 4 * r);
            const int kv[4] = {ki.x, ki.y, ki.z, ki.w};
            at_f4 ds;
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const float sc = sw_score2(s[v], tbl, qt.rel, qt.reg, kv[v], 16 * t + 4 * r + v < a.N);
                const float p = __builtin_amdgcn_exp2f(sc - lse);
                ds[v] = p * (dp[v] - delta);
            }
            at_accum_t(Ks + 16 * t * kAtRow, r, c, ds, dq0, dq1);       // dQ^T[channel][query] += K^T . dS^T
            sw_st4(dsrow + 16 * t + 4 * r, ds);
        }
        if (qrow >= 0) {
            float *gq = a.gqkv + (long long)qrow * 3 * a.C + h * 32 + 4 * r;
            for (int v = 0; v < 4; ++v) { dq0[v] *= a.scale; dq1[v] *= a.scale; }
            sw_st4(gq, dq0);
            sw_st4(gq + 16, dq1);
        }
    } else {
        for (int t = 0; t < ntk; ++t) sw_st4(dsrow + 16 * t + 4 * r, at_f4{0.f, 0.f, 0.f, 0.f});
    }
    __syncthreads();
    // table entry e = (dy + ws - 1) (2 ws - 1) + dx + ws - 1: the queries (yi, xi) whose key (yi - dy, xi - dx) lies in the
    // window form a rectangle; summed in query order
    const int w2 = 2 * a.ws - 1;
    for (int e = threadIdx.x; e < a.E; e += blockDim.x) {
        const int dy = e / w2 - (a.ws - 1), dx = e % w2 - (a.ws - 1), off = dy * a.ws + dx;
        const int y0 = max(0, dy), y1 = min(a.ws, a.ws + dy), x0 = max(0, dx), x1 = min(a.ws, a.ws + dx);
        float acc = 0.f;
        for (int yi = y0; yi < y1; ++yi)
            for (int xi = x0; xi < x1; ++xi) {
                const int i = yi * a.ws + xi;
                acc += dS[i * dss + i - off];
            }
        a.pt[pair * a.E + e] = acc;
    }
}

// grad_table [E, nH] and grad_bias [3 C]: one wavefront per output, over the (image, window) partials of its head
__global__ __launch_bounds__(kSwRedBlock) void swin_bwd_reduce_kernel(const SwArgs a)
{
    const long long out = (long long)blockIdx.x * (kSwRedBlock / 64) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63, P = a.B * a.nW;
    const long long ntab = (long long)a.E * a.nH;
    if (out >= ntab + 3LL * a.C) return;
    const float *src;
    long long stride;
    if (out < ntab) {
        const int e = (int)(out / a.nH), h = (int)(out % a.nH);
        src = a.pt + (long long)h * a.E + e;
        stride = (long long)a.nH * a.E;
    } else {
        const int k = (int)(out - ntab), part = k / a.C, h = (k % a.C) / 32, ch = k % 32;
        if (part == 0 || a.gbias == nullptr) {
            if (part == 0 && lane == 0 && a.gbias != nullptr) a.gbias[k] = 0.f;
            return;
        }
        src = a.pb + (long long)h * 64 + (part - 1) * 32 + ch;
        stride = (long long)a.nH * 64;
    }
    float acc = 0.f;
    for (int p = lane; p < P; p += 64) acc += src[(long long)p * stride];
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) acc += __shfl_xor(acc, m);
    if (lane == 0) {
        if (out < ntab) a.gtable[out] = acc;
        else a.gbias[out - ntab] = acc;
    }
}

int serr(const char *msg) { return set_error(MSDA_ERR_ARGUMENT, msg); }

size_t sw_lds_fwd(int N, int E) { const int Np = (N + 15) & ~15; return (size_t)(2 * Np * kAtRow + ((E + 3) & ~3) + 2 * Np) * 4; }
size_t sw_lds_kv(int N, int E)
{
    const int Np = (N + 15) & ~15;
    return (size_t)(2 * Np * kAtRow + ((E + 3) & ~3) + 2 * Np + (Np >> 4) * 64 + 2 * Np + (Np >> 4)) * 4;
}
size_t sw_lds_q(int N, int E)
{
    const int Np = (N + 15) & ~15;
    return (size_t)(2 * Np * kAtRow + ((E + 3) & ~3) + Np * (Np + 4) + 2 * Np) * 4;
}

int sw_allow_lds(const void *fn, size_t bytes)
{
    if (bytes <= 64 * 1024) return MSDA_OK;
    const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    return e == hipSuccess ? MSDA_OK : set_error(MSDA_ERR_LAUNCH, hipGetErrorString(e));
}

bool aligned16(const void *p) { return ((uintptr_t)p & 15u) == 0; }

// ---- bf16 operands (msda_swin_attn_*_bf16) ---------------------------------------------------------------------------------------
// The same four launches and the same work split with qkv, out, dO and grad_qkv in bf16 and every product on
// v_mfma_f32_16x16x32_bf16 (fp32 accumulate), following the bf16 block of msda_attn_tile.h: the pair's operands sit in LDS as bf16
// rows [Np][40] (N padded to a multiple of 32, padding rows zero), read as a row (ds_read_b128) for the products over channels and
// transposed (ds_read_b64_tr_b16) for the products over keys / queries; score tiles come in pairs covering 32 keys (queries), tile
// b's row i being key 32T + 8 (i >> 2) + 4b + (i & 3), so that the accumulators of a pair are the next product's 8-wide operand.
// fp32: the scores (scale on the fp32 dot product, table term, shift mask), softmax, log-sum-exp, delta, dP, the dS rows the table
// pass sums (LDS) and every partial.  bf16: P and dS as MFMA operands only; out and grad_qkv, rounded once.  A padded token's k and
// v are the bias's parts rounded to bf16 (a bf16 Linear on a zero row).  Every loop around a transposed read is wave-uniform.
// LDS of the q kernel at ws 12: 2 * 160 * 80 + 532 * 4 + 144 * 164 * 4 + 2 * 160 * 4 = 123472 B (the fp32 one: 130000 B).
constexpr int kSbMaxPairs = (kSwMaxN + 31) / 32;

// g: geometry, bias, table, lse, gtable, gbias, pt, pb (its fp32 tensor pointers stay null); the bf16 tensors
struct SbArgs {
    SwArgs g;
    const uint16_t *qkv, *out, *gout;
    uint16_t *o, *gqkv;
};

// the k (part 1) or v (part 2) channels c8 .. c8 + 7 of token `row` (padded: the bias's rounded to bf16, or zero), head h
__device__ __forceinline__ at_bf8 sb_kv8(const SbArgs &a, int row, int part, int h, int c8)
{
    if (row >= 0) return ab_ld8(a.qkv + (long long)row * 3 * a.g.C + part * a.g.C + h * 32 + c8);
    if (a.g.bias == nullptr) return ab_zero8();
    const float *bp = a.g.bias + part * a.g.C + h * 32 + c8;
    const float4 b0 = ld4(bp), b1 = ld4(bp + 4);
    return at_bf8{(__bf16)b0.x, (__bf16)b0.y, (__bf16)b0.z, (__bf16)b0.w, (__bf16)b1.x, (__bf16)b1.y, (__bf16)b1.z, (__bf16)b1.w};
}

// the window's keys: info and qkv row per token, k and v rows into LDS (rows N .. Np - 1 zero)
__device__ __forceinline__ void sb_fill_kv(const SbArgs &a, int b, int w, int h, int Np, uint16_t *Ks, uint16_t *Vs, int *kinf, int *rows)
{
    for (int t = threadIdx.x; t < Np; t += blockDim.x) {
        SwTok k = {-1, 0, 0};
        if (t < a.g.N) k = sw_token(a.g, b, w, t, true);
        kinf[t] = k.rel | (k.reg << 16);
        rows[t] = k.row;
    }
    for (int i = threadIdx.x; i < Np * 4; i += blockDim.x) {
        const int t = i >> 2, c8 = (i & 3) * 8;
        at_bf8 kv = ab_zero8(), vv = ab_zero8();
        if (t < a.g.N) {
            const int row = sw_token(a.g, b, w, t, true).row;
            kv = sb_kv8(a, row, 1, h, c8);
            vv = sb_kv8(a, row, 2, h, c8);
        }
        *reinterpret_cast<at_bf8 *>(Ks + t * kAbRow + c8) = kv;
        *reinterpret_cast<at_bf8 *>(Vs + t * kAbRow + c8) = vv;
    }
}

// the 8 infos of tokens 32T + 8r .. + 7
__device__ __forceinline__ void sb_info8(const int *inf, int T, int r, int (&v)[8])
{
    const int4 x = *reinterpret_cast<const int4 *>(inf + 32 * T + 8 * r), y = *reinterpret_cast<const int4 *>(inf + 32 * T + 8 * r + 4);
    v[0] = x.x; v[1] = x.y; v[2] = x.z; v[3] = x.w; v[4] = y.x; v[5] = y.y; v[6] = y.z; v[7] = y.w;
}

__global__ __launch_bounds__(kSwMaxBlock) void swin_fwd_bf16_kernel(const SbArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float sw_smem[];
    const SwArgs &g = a.g;
    const int Np = (g.N + 31) & ~31, Ep = (g.E + 3) & ~3, npair = Np >> 5;
    uint16_t *Ks = reinterpret_cast<uint16_t *>(sw_smem), *Vs = Ks + Np * kAbRow;
    float *tbl = reinterpret_cast<float *>(Vs + Np * kAbRow);
    int *kinf = reinterpret_cast<int *>(tbl + Ep), *rows = kinf + Np;
    int b, w, h;
    sw_pair(g, b, w, h);
    sb_fill_kv(a, b, w, h, Np, Ks, Vs, kinf, rows);
    sw_load_table(g, h, tbl);
    __syncthreads();
    const int tq = threadIdx.x >> 6, lane = threadIdx.x & 63, c = lane & 15, r = lane >> 4;
    const int qi = tq * 16 + c;
    const int qrow = qi < g.N ? rows[qi] : -1;
    if (!__any(qrow >= 0)) return;                                      // a tile of padded tokens only: nothing to write
    const SwTok qt = sw_token(g, b, w, qi < g.N ? qi : 0, false);
    at_bf8 qf = ab_zero8();
    if (qrow >= 0) qf = ab_ld8(a.qkv + (long long)qrow * 3 * g.C + h * 32 + 8 * r);
    // s[2T + b][v] = score (base 2) of key 32T + 8r + 4b + v for query qi
    at_f4 s[2 * kSbMaxPairs];
    float m = -INFINITY;
#pragma unroll
    for (int T = 0; T < kSbMaxPairs; ++T) {
        if (T < npair) {
            ab_pair(Ks, T, r, c, qf, s[2 * T], s[2 * T + 1]);
            int kv[8];
            sb_info8(kinf, T, r, kv);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float x = sw_score2(s[2 * T + (j >> 2)][j & 3] * g.scale, tbl, qt.rel, qt.reg, kv[j], 32 * T + 8 * r + j < g.N);
                s[2 * T + (j >> 2)][j & 3] = x;
                m = fmaxf(m, x);
            }
        }
    }
    m = at_rmax(m);
    float sum = 0.f;
#pragma unroll
    for (int t = 0; t < 2 * kSbMaxPairs; ++t) {
        if (t < 2 * npair) {
#pragma unroll
            for (int v = 0; v < 4; ++v) { s[t][v] = __builtin_amdgcn_exp2f(s[t][v] - m); sum += s[t][v]; }
        }
    }
    sum = at_rsum(sum);
    const long long pair = blockIdx.x;
    if (qrow >= 0 && r == 0) g.lse[pair * g.N + qi] = (m + __builtin_amdgcn_logf(sum)) * 0.6931471805599453f;
    const float inv = 1.f / sum;
    at_f4 o0 = {0.f, 0.f, 0.f, 0.f}, o1 = o0;
#pragma unroll
    for (int T = 0; T < kSbMaxPairs; ++T) {
        if (T < npair) {
#pragma unroll
            for (int v = 0; v < 4; ++v) { s[2 * T][v] *= inv; s[2 * T + 1][v] *= inv; }
            const at_bf8 pb = ab_pack(s[2 * T], s[2 * T + 1]);          // P^T[key 32T + 8r + j][query qi]
            o0 = ab_mfma(ab_tr(Vs, T, 0, r, c), pb, o0);                // O^T[channel][query] += V^T . P^T
            o1 = ab_mfma(ab_tr(Vs, T, 1, r, c), pb, o1);
        }
    }
    if (qrow >= 0) {
        uint16_t *op = a.o + (long long)qrow * g.C + h * 32 + 4 * r;
        ab_st4(op, o0, 1.f);
        ab_st4(op + 16, o1, 1.f);
    }
}

// dK, dV: wavefront tk owns keys 16 tk .. 16 tk + 15 and walks the query pairs (S tiles: rows = queries)
__global__ __launch_bounds__(kSwMaxBlock) void swin_bwd_kv_bf16_kernel(const SbArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float sw_smem[];
    const SwArgs &g = a.g;
    const int Np = (g.N + 31) & ~31, Ep = (g.E + 3) & ~3, npair = Np >> 5, nwave = blockDim.x >> 6;
    uint16_t *Qs = reinterpret_cast<uint16_t *>(sw_smem), *Gs = Qs + Np * kAbRow;
    float *tbl = reinterpret_cast<float *>(Gs + Np * kAbRow), *lse_s = tbl + Ep, *del_s = lse_s + Np;
    float *part = del_s + Np;                                           // [waves][64]
    int *qinf = reinterpret_cast<int *>(part + nwave * 64), *rows = qinf + Np, *pany = rows + Np;
    int b, w, h;
    sw_pair(g, b, w, h);
    const long long pair = blockIdx.x;
    for (int t = threadIdx.x; t < Np; t += blockDim.x) {
        SwTok q = {-1, 0, 0};
        if (t < g.N) q = sw_token(g, b, w, t, false);
        qinf[t] = q.rel | (q.reg << 16);
        rows[t] = q.row;
    }
    sw_load_table(g, h, tbl);
    for (int i = threadIdx.x; i < Np * 4; i += blockDim.x) {
        const int t = i >> 2, c8 = (i & 3) * 8;
        const int row = t < g.N ? sw_token(g, b, w, t, false).row : -1;
        at_bf8 qv = ab_zero8(), gv = ab_zero8();
        if (row >= 0) {
            qv = ab_ld8(a.qkv + (long long)row * 3 * g.C + h * 32 + c8);
            gv = ab_ld8(a.gout + (long long)row * g.C + h * 32 + c8);
        }
        *reinterpret_cast<at_bf8 *>(Qs + t * kAbRow + c8) = qv;
        *reinterpret_cast<at_bf8 *>(Gs + t * kAbRow + c8) = gv;
    }
    __syncthreads();
    for (int t = threadIdx.x; t < Np; t += blockDim.x) {
        const int row = rows[t];
        float d = 0.f;
        if (row >= 0) {
            const uint16_t *orow = a.out + (long long)row * g.C + h * 32, *grow = Gs + t * kAbRow;
#pragma unroll
            for (int k8 = 0; k8 < 4; ++k8) {
                const at_bf8 ov = ab_ld8(orow + 8 * k8), gv = ab_ld8(grow + 8 * k8);
#pragma unroll
                for (int j = 0; j < 8; ++j) d += ab_f(ov[j]) * ab_f(gv[j]);
            }
        }
        del_s[t] = d;
        lse_s[t] = row >= 0 ? g.lse[pair * g.N + t] * kLog2e : INFINITY;    // padded queries: probabilities 0
    }
    for (int t = threadIdx.x; t < npair; t += blockDim.x) {
        int any = 0;
        for (int u = 0; u < 32; ++u) any |= rows[32 * t + u] >= 0;
        pany[t] = any;
    }
    __syncthreads();
    const int tk = threadIdx.x >> 6, lane = threadIdx.x & 63, c = lane & 15, r = lane >> 4;
    const int key = tk * 16 + c;
    const bool kok = key < g.N;
    const SwTok kt = sw_token(g, b, w, kok ? key : 0, true);
    const int krow = kok ? kt.row : -1;
    at_bf8 kf = ab_zero8(), vf = ab_zero8();
    if (kok) {
        kf = sb_kv8(a, krow, 1, h, 8 * r);
        vf = sb_kv8(a, krow, 2, h, 8 * r);
    }
    const int kinfo = (kt.rel & 0xffff) | (kt.reg << 16);
    at_f4 dv0 = {0.f, 0.f, 0.f, 0.f}, dv1 = dv0, dk0 = dv0, dk1 = dv0;
#pragma unroll 1
    for (int T = 0; T < npair; ++T) {
        if (!pany[T]) continue;                                         // (the same for every lane of the workgroup)
        // S and dP tiles of the pair: entry (b, v) = (query 32T + 8r + 4b + v, key)
        at_f4 s[2], dp[2];
        ab_pair(Qs, T, r, c, kf, s[0], s[1]);
        ab_pair(Gs, T, r, c, vf, dp[0], dp[1]);
        const float *lq = lse_s + 32 * T + 8 * r, *dq = del_s + 32 * T + 8 * r;
        const float4 l0 = ld4(lq), l1 = ld4(lq + 4), d0 = ld4(dq), d1 = ld4(dq + 4);
        const float lsv[8] = {l0.x, l0.y, l0.z, l0.w, l1.x, l1.y, l1.z, l1.w}, dlv[8] = {d0.x, d0.y, d0.z, d0.w, d1.x, d1.y, d1.z, d1.w};
        int qv[8];
        sb_info8(qinf, T, r, qv);
        at_f4 pd[2], ds[2];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int bb = j >> 2, v = j & 3;
            // (query info and key info swap roles: the table index is the sum of the two parts either way)
            const float sc = sw_score2(s[bb][v] * g.scale, tbl, qv[j] & 0xffff, qv[j] >> 16, kinfo, true);
            const float p = __builtin_amdgcn_exp2f(sc - lsv[j]);
            pd[bb][v] = p;
            ds[bb][v] = p * (dp[bb][v] - dlv[j]);
        }
        const at_bf8 pb = ab_pack(pd[0], pd[1]), sb = ab_pack(ds[0], ds[1]);
        dv0 = ab_mfma(ab_tr(Gs, T, 0, r, c), pb, dv0);                  // dV^T[channel][key] += dO^T . P
        dv1 = ab_mfma(ab_tr(Gs, T, 1, r, c), pb, dv1);
        dk0 = ab_mfma(ab_tr(Qs, T, 0, r, c), sb, dk0);                  // dK^T[channel][key] += Q^T . dS
        dk1 = ab_mfma(ab_tr(Qs, T, 1, r, c), sb, dk1);
    }
#pragma unroll
    for (int v = 0; v < 4; ++v) { dk0[v] *= g.scale; dk1[v] *= g.scale; }
    if (krow >= 0) {
        uint16_t *gk = a.gqkv + (long long)krow * 3 * g.C + g.C + h * 32 + 4 * r, *gv = gk + g.C;
        ab_st4(gk, dk0, 1.f); ab_st4(gk + 16, dk1, 1.f);
        ab_st4(gv, dv0, 1.f); ab_st4(gv + 16, dv1, 1.f);
    }
    // padded keys of this tile: their k / v gradients summed (a butterfly over the 16 keys), then over the wavefronts in order
    const bool kpad = kok && krow < 0;
    float acc[16];
#pragma unroll
    for (int v = 0; v < 4; ++v) {
        acc[v] = kpad ? dk0[v] : 0.f; acc[4 + v] = kpad ? dk1[v] : 0.f;
        acc[8 + v] = kpad ? dv0[v] : 0.f; acc[12 + v] = kpad ? dv1[v] : 0.f;
    }
#pragma unroll
    for (int m = 1; m < 16; m <<= 1) {
#pragma unroll
        for (int u = 0; u < 16; ++u) acc[u] += __shfl_xor(acc[u], m);
    }
    if (c == 0) {
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            part[tk * 64 + 4 * r + v] = acc[v];
            part[tk * 64 + 16 + 4 * r + v] = acc[4 + v];
            part[tk * 64 + 32 + 4 * r + v] = acc[8 + v];
            part[tk * 64 + 48 + 4 * r + v] = acc[12 + v];
        }
    }
    __syncthreads();
    if (threadIdx.x < 64) {
        float sum = 0.f;
        for (int u = 0; u < nwave; ++u) sum += part[u * 64 + threadIdx.x];
        g.pb[pair * 64 + threadIdx.x] = sum;
    }
}

// dQ: wavefront tq owns queries 16 tq .. 16 tq + 15 and walks the key pairs (S^T tiles, as the forward); fp32 dS rows into LDS,
// then the per-pair table partial
__global__ __launch_bounds__(kSwMaxBlock) void swin_bwd_q_bf16_kernel(const SbArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float sw_smem[];
    const SwArgs &g = a.g;
    const int Np = (g.N + 31) & ~31, Ep = (g.E + 3) & ~3, npair = Np >> 5, dss = Np + 4, nq = (blockDim.x >> 6) * 16;
    uint16_t *Ks = reinterpret_cast<uint16_t *>(sw_smem), *Vs = Ks + Np * kAbRow;
    float *tbl = reinterpret_cast<float *>(Vs + Np * kAbRow), *dS = tbl + Ep;       // dS [nq][dss]
    int *kinf = reinterpret_cast<int *>(dS + nq * dss), *rows = kinf + Np;
    int b, w, h;
    sw_pair(g, b, w, h);
    const long long pair = blockIdx.x;
    sb_fill_kv(a, b, w, h, Np, Ks, Vs, kinf, rows);
    sw_load_table(g, h, tbl);
    __syncthreads();
    const int tq = threadIdx.x >> 6, lane = threadIdx.x & 63, c = lane & 15, r = lane >> 4;
    const int qi = tq * 16 + c;
    const int qrow = qi < g.N ? rows[qi] : -1;
    float *dsrow = dS + qi * dss;
    if (__any(qrow >= 0)) {
        const SwTok qt = sw_token(g, b, w, qi < g.N ? qi : 0, false);
        at_bf8 qf = ab_zero8(), gf = ab_zero8(), of = ab_zero8();
        float lse = INFINITY;
        if (qrow >= 0) {
            qf = ab_ld8(a.qkv + (long long)qrow * 3 * g.C + h * 32 + 8 * r);
            gf = ab_ld8(a.gout + (long long)qrow * g.C + h * 32 + 8 * r);
            of = ab_ld8(a.out + (long long)qrow * g.C + h * 32 + 8 * r);
            lse = g.lse[pair * g.N + qi] * kLog2e;
        }
        float d = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) d += ab_f(gf[j]) * ab_f(of[j]);
        const float delta = at_rsum(d);
        at_f4 dq0 = {0.f, 0.f, 0.f, 0.f}, dq1 = dq0;
#pragma unroll 1
        for (int T = 0; T < npair; ++T) {
            // S^T and dP^T tiles of the pair: entry (b, v) = (key 32T + 8r + 4b + v, query qi)
            at_f4 s[2], dp[2], ds[2];
            ab_pair(Ks, T, r, c, qf, s[0], s[1]);
            ab_pair(Vs, T, r, c, gf, dp[0], dp[1]);
            int kv[8];
            sb_info8(kinf, T, r, kv);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int bb = j >> 2, v = j & 3;
                const float sc = sw_score2(s[bb][v] * g.scale, tbl, qt.rel, qt.reg, kv[j], 32 * T + 8 * r + j < g.N);
                const float p = __builtin_amdgcn_exp2f(sc - lse);
                ds[bb][v] = p * (dp[bb][v] - delta);
            }
            const at_bf8 sb = ab_pack(ds[0], ds[1]);
            dq0 = ab_mfma(ab_tr(Ks, T, 0, r, c), sb, dq0);              // dQ^T[channel][query] += K^T . dS^T
            dq1 = ab_mfma(ab_tr(Ks, T, 1, r, c), sb, dq1);
            sw_st4(dsrow + 32 * T + 8 * r, ds[0]);
            sw_st4(dsrow + 32 * T + 8 * r + 4, ds[1]);
        }
        if (qrow >= 0) {
            uint16_t *gq = a.gqkv + (long long)qrow * 3 * g.C + h * 32 + 4 * r;
            ab_st4(gq, dq0, g.scale);
            ab_st4(gq + 16, dq1, g.scale);
        }
    } else {
        for (int T = 0; T < npair; ++T) {
            sw_st4(dsrow + 32 * T + 8 * r, at_f4{0.f, 0.f, 0.f, 0.f});
            sw_st4(dsrow + 32 * T + 8 * r + 4, at_f4{0.f, 0.f, 0.f, 0.f});
        }
    }
    __syncthreads();
    // (the table pass of swin_bwd_q_kernel)
    const int w2 = 2 * g.ws - 1;
    for (int e = threadIdx.x; e < g.E; e += blockDim.x) {
        const int dy = e / w2 - (g.ws - 1), dx = e % w2 - (g.ws - 1), off = dy * g.ws + dx;
        const int y0 = max(0, dy), y1 = min(g.ws, g.ws + dy), x0 = max(0, dx), x1 = min(g.ws, g.ws + dx);
        float acc = 0.f;
        for (int yi = y0; yi < y1; ++yi)
            for (int xi = x0; xi < x1; ++xi) {
                const int i = yi * g.ws + xi;
                acc += dS[i * dss + i - off];
            }
        g.pt[pair * g.E + e] = acc;
    }
}

size_t sb_lds_fwd(int N, int E) { const int Np = (N + 31) & ~31; return (size_t)2 * Np * kAbRow * 2 + (size_t)(((E + 3) & ~3) + 2 * Np) * 4; }
size_t sb_lds_kv(int N, int E)
{
    const int Np = (N + 31) & ~31, nwave = (N + 15) / 16;
    return (size_t)2 * Np * kAbRow * 2 + (size_t)(((E + 3) & ~3) + 2 * Np + nwave * 64 + 2 * Np + (Np >> 5)) * 4;
}
size_t sb_lds_q(int N, int E)
{
    const int Np = (N + 31) & ~31, nq = (N + 15) / 16 * 16;
    return (size_t)2 * Np * kAbRow * 2 + (size_t)(((E + 3) & ~3) + nq * (Np + 4) + 2 * Np) * 4;
}

}  // namespace

bool swin_supported(int B, int H, int W, int C, int nH, int ws, int shift)
{
    if (B < 1 || H < 1 || W < 1 || nH < 1 || ws < 1 || ws > kSwMaxWs || shift < 0 || shift >= ws) return false;
    if (C != 32 * nH) return false;
    const long long Hp = (H + ws - 1) / ws * ws, Wp = (W + ws - 1) / ws * ws;
    const long long pairs = (long long)B * (Hp / ws) * (Wp / ws) * nH;
    const long long rows = (long long)B * H * W;
    return rows * 3 * C < (1LL << 31) && pairs * ws * ws < (1LL << 31) && pairs * 64 < (1LL << 31)
           && pairs * (2 * ws - 1) * (2 * ws - 1) < (1LL << 31);
}

unsigned long long swin_workspace_bytes(int B, int H, int W, int C, int nH, int ws, int shift, int which)
{
    if (!swin_supported(B, H, W, C, nH, ws, shift)) return 0;
    const long long Hp = (H + ws - 1) / ws * ws, Wp = (W + ws - 1) / ws * ws;
    const long long pairs = (long long)B * (Hp / ws) * (Wp / ws) * nH;
    if (which == 0) return (unsigned long long)(pairs * ws * ws) * 4;                         // lse [pairs][N]
    if (which == 1) return (unsigned long long)(pairs * ((2 * ws - 1) * (2 * ws - 1) + 64)) * 4;
    return 0;
}

static SwArgs sw_args(int B, int H, int W, int C, int nH, int ws, int shift)
{
    SwArgs a = {};
    a.B = B; a.H = H; a.W = W; a.C = C; a.nH = nH; a.ws = ws; a.s = shift;
    a.Hp = (H + ws - 1) / ws * ws; a.Wp = (W + ws - 1) / ws * ws;
    a.nWx = a.Wp / ws; a.nW = (a.Hp / ws) * a.nWx; a.N = ws * ws; a.E = (2 * ws - 1) * (2 * ws - 1);
    a.scale = 1.0f / sqrtf(32.0f);
    return a;
}

int swin_forward(int B, int H, int W, int C, int nH, int ws, int shift, const float *qkv, const float *bias, const float *table,
                 float *out, float *lse, unsigned long long lse_bytes, hipStream_t stream)
{
    if (!swin_supported(B, H, W, C, nH, ws, shift))
        return serr("msda_swin_attn: need B, H, W, nH >= 1, C == 32 nH, 1 <= ws <= 12, 0 <= shift < ws, tensors below 2^31 elements");
    if (qkv == nullptr || table == nullptr || out == nullptr || lse == nullptr) return serr("msda_swin_attn: null pointer");
    if (!aligned16(qkv) || !aligned16(out) || (bias != nullptr && !aligned16(bias)))
        return serr("msda_swin_attn: qkv, qkv_bias and out must be 16-byte aligned");
    if (lse_bytes < swin_workspace_bytes(B, H, W, C, nH, ws, shift, 0))
        return serr("msda_swin_attn: lse buffer smaller than msda_swin_attn_workspace_bytes(..., 0)");
    SwArgs a = sw_args(B, H, W, C, nH, ws, shift);
    a.qkv = qkv; a.bias = bias; a.table = table; a.o = out; a.lse = lse;
    const int pairs = B * a.nW * nH, threads = 64 * ((a.N + 15) / 16);
    const size_t lds = sw_lds_fwd(a.N, a.E);
    int rc = sw_allow_lds(reinterpret_cast<const void *>(swin_fwd_kernel), lds);
    if (rc != MSDA_OK) return rc;
    hipLaunchKernelGGL(swin_fwd_kernel, dim3((unsigned)pairs), dim3((unsigned)threads), lds, stream, a);
    return check_launch("swin_fwd_kernel");
}

int swin_backward(int B, int H, int W, int C, int nH, int ws, int shift, const float *qkv, const float *bias, const float *table,
                  const float *out, const float *lse, unsigned long long lse_bytes, const float *grad_out, float *grad_qkv,
                  float *grad_table, float *grad_bias, void *workspace, unsigned long long workspace_bytes, hipStream_t stream)
{
    if (!swin_supported(B, H, W, C, nH, ws, shift))
        return serr("msda_swin_attn: need B, H, W, nH >= 1, C == 32 nH, 1 <= ws <= 12, 0 <= shift < ws, tensors below 2^31 elements");
    if (qkv == nullptr || table == nullptr || out == nullptr || lse == nullptr || grad_out == nullptr || grad_qkv == nullptr
        || grad_table == nullptr || workspace == nullptr)
        return serr("msda_swin_attn: null pointer");
    if (!aligned16(qkv) || !aligned16(out) || !aligned16(grad_out) || !aligned16(grad_qkv) || !aligned16(workspace)
        || (bias != nullptr && !aligned16(bias)))
        return serr("msda_swin_attn: qkv, qkv_bias, out, grad_out, grad_qkv and the workspace must be 16-byte aligned");
    if (lse_bytes < swin_workspace_bytes(B, H, W, C, nH, ws, shift, 0))
        return serr("msda_swin_attn: lse buffer smaller than msda_swin_attn_workspace_bytes(..., 0)");
    if (workspace_bytes < swin_workspace_bytes(B, H, W, C, nH, ws, shift, 1))
        return serr("msda_swin_attn: workspace smaller than msda_swin_attn_workspace_bytes(..., 1)");
    SwArgs a = sw_args(B, H, W, C, nH, ws, shift);
    a.qkv = qkv; a.bias = bias; a.table = table; a.out = out; a.o = const_cast<float *>(out); a.lse = const_cast<float *>(lse);
    a.gout = grad_out; a.gqkv = grad_qkv; a.gtable = grad_table; a.gbias = grad_bias;
    const int pairs = B * a.nW * nH, threads = 64 * ((a.N + 15) / 16);
    a.pt = static_cast<float *>(workspace);
    a.pb = a.pt + (long long)pairs * a.E;
    const size_t lkv = sw_lds_kv(a.N, a.E), lq = sw_lds_q(a.N, a.E);
    int rc = sw_allow_lds(reinterpret_cast<const void *>(swin_bwd_kv_kernel), lkv);
    if (rc == MSDA_OK) rc = sw_allow_lds(reinterpret_cast<const void *>(swin_bwd_q_kernel), lq);
    if (rc != MSDA_OK) return rc;
    hipLaunchKernelGGL(swin_bwd_kv_kernel, dim3((unsigned)pairs), dim3((unsigned)threads), lkv, stream, a);
    rc = check_launch("swin_bwd_kv_kernel");
    if (rc != MSDA_OK) return rc;
    hipLaunchKernelGGL(swin_bwd_q_kernel, dim3((unsigned)pairs), dim3((unsigned)threads), lq, stream, a);
    rc = check_launch("swin_bwd_q_kernel");
    if (rc != MSDA_OK) return rc;
    const long long outs = (long long)a.E * nH + 3LL * C;
    const unsigned blocks = (unsigned)((outs + kSwRedBlock / 64 - 1) / (kSwRedBlock / 64));
    hipLaunchKernelGGL(swin_bwd_reduce_kernel, dim3(blocks), dim3(kSwRedBlock), 0, stream, a);
    return check_launch("swin_bwd_reduce_kernel");
}

int swin_forward_bf16(int B, int H, int W, int C, int nH, int ws, int shift, const uint16_t *qkv, const float *bias,
                      const float *table, uint16_t *out, float *lse, unsigned long long lse_bytes, hipStream_t stream)
{
    if (!swin_supported(B, H, W, C, nH, ws, shift))
        return serr("msda_swin_attn: need B, H, W, nH >= 1, C == 32 nH, 1 <= ws <= 12, 0 <= shift < ws, tensors below 2^31 elements");
    if (qkv == nullptr || table == nullptr || out == nullptr || lse == nullptr) return serr("msda_swin_attn: null pointer");
    if (!aligned16(qkv) || !aligned16(out) || (bias != nullptr && !aligned16(bias)))
        return serr("msda_swin_attn: qkv, qkv_bias and out must be 16-byte aligned");
    if (lse_bytes < swin_workspace_bytes(B, H, W, C, nH, ws, shift, 0))
        return serr("msda_swin_attn: lse buffer smaller than msda_swin_attn_workspace_bytes(..., 0)");
    SbArgs a = {};
    a.g = sw_args(B, H, W, C, nH, ws, shift);
    a.g.bias = bias; a.g.table = table; a.g.lse = lse; a.qkv = qkv; a.o = out;
    const int pairs = B * a.g.nW * nH, threads = 64 * ((a.g.N + 15) / 16);
    const size_t lds = sb_lds_fwd(a.g.N, a.g.E);
    int rc = sw_allow_lds(reinterpret_cast<const void *>(swin_fwd_bf16_kernel), lds);
    if (rc != MSDA_OK) return rc;
    hipLaunchKernelGGL(swin_fwd_bf16_kernel, dim3((unsigned)pairs), dim3((unsigned)threads), lds, stream, a);
    return check_launch("swin_fwd_bf16_kernel");
}

int swin_backward_bf16(int B, int H, int W, int C, int nH, int ws, int shift, const uint16_t *qkv, const float *bias,
                       const float *table, const uint16_t *out, const float *lse, unsigned long long lse_bytes,
                       const uint16_t *grad_out, uint16_t *grad_qkv, float *grad_table, float *grad_bias, void *workspace,
                       unsigned long long workspace_bytes, hipStream_t stream)
{
    if (!swin_supported(B, H, W, C, nH, ws, shift))
        return serr("msda_swin_attn: need B, H, W, nH >= 1, C == 32 nH, 1 <= ws <= 12, 0 <= shift < ws, tensors below 2^31 elements");
    if (qkv == nullptr || table == nullptr || out == nullptr || lse == nullptr || grad_out == nullptr || grad_qkv == nullptr
        || grad_table == nullptr || workspace == nullptr)
        return serr("msda_swin_attn: null pointer");
    if (!aligned16(qkv) || !aligned16(out) || !aligned16(grad_out) || !aligned16(grad_qkv) || !aligned16(workspace)
        || (bias != nullptr && !aligned16(bias)))
        return serr("msda_swin_attn: qkv, qkv_bias, out, grad_out, grad_qkv and the workspace must be 16-byte aligned");
    if (lse_bytes < swin_workspace_bytes(B, H, W, C, nH, ws, shift, 0))
        return serr("msda_swin_attn: lse buffer smaller than msda_swin_attn_workspace_bytes(..., 0)");
    if (workspace_bytes < swin_workspace_bytes(B, H, W, C, nH, ws, shift, 1))
        return serr("msda_swin_attn: workspace smaller than msda_swin_attn_workspace_bytes(..., 1)");
    SbArgs a = {};
    a.g = sw_args(B, H, W, C, nH, ws, shift);
    a.g.bias = bias; a.g.table = table; a.g.lse = const_cast<float *>(lse); a.g.gtable = grad_table; a.g.gbias = grad_bias;
    a.qkv = qkv; a.out = out; a.gout = grad_out; a.gqkv = grad_qkv;
    const int pairs = B * a.g.nW * nH, threads = 64 * ((a.g.N + 15) / 16);
    a.g.pt = static_cast<float *>(workspace);
    a.g.pb = a.g.pt + (long long)pairs * a.g.E;
    const size_t lkv = sb_lds_kv(a.g.N, a.g.E), lq = sb_lds_q(a.g.N, a.g.E);
    int rc = sw_allow_lds(reinterpret_cast<const void *>(swin_bwd_kv_bf16_kernel), lkv);
    if (rc == MSDA_OK) rc = sw_allow_lds(reinterpret_cast<const void *>(swin_bwd_q_bf16_kernel), lq);
    if (rc != MSDA_OK) return rc;
    hipLaunchKernelGGL(swin_bwd_kv_bf16_kernel, dim3((unsigned)pairs), dim3((unsigned)threads), lkv, stream, a);
    rc = check_launch("swin_bwd_kv_bf16_kernel");
    if (rc != MSDA_OK) return rc;
    hipLaunchKernelGGL(swin_bwd_q_bf16_kernel, dim3((unsigned)pairs), dim3((unsigned)threads), lq, stream, a);
    rc = check_launch("swin_bwd_q_bf16_kernel");
    if (rc != MSDA_OK) return rc;
    const long long outs = (long long)a.g.E * nH + 3LL * C;             // the fp32 form's reduce: every partial is fp32
    const unsigned blocks = (unsigned)((outs + kSwRedBlock / 64 - 1) / (kSwRedBlock / 64));
    hipLaunchKernelGGL(swin_bwd_reduce_kernel, dim3(blocks), dim3(kSwRedBlock), 0, stream, a.g);
    return check_launch("swin_bwd_reduce_kernel");
}

}  // namespace msda
