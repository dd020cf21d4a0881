// The bf16-autocast form of the DeformableDETR prediction heads (msda_heads.hip holds the fp32 form and the decomposition):
// the same grouped problems, the same launch budget (3 forward, 5 backward), every product on v_mfma_f32_16x16x32_bf16 with
// fp32 accumulation.
//
// What is bf16 and what is fp32 follows torch's bf16 autocast over the reference's composition ("bf16-autocast
// prediction heads"): hs, the parameters, the references and the saved sigmoids are fp32; the hidden activations, the hidden
// gradients, ARCTIC's six shared outputs and every AssemblyHands output are bf16; ARCTIC's logits and keypoints are fp32.
// fp32 operands (hs, weights, incoming fp32 gradients) are rounded to bf16, to nearest even, in the load that stages them to
// LDS: no cast kernel, no bf16 copy of a weight.  A Linear's output is rounded to bf16 once, bias included, before its
// epilogue.  grad_hs and the weight / bias gradients are accumulated and written in fp32 with no bf16 rounding.
//
// Kernel: 64 x 64 output tile per 256-thread workgroup, 2 x 2 wavefronts of 32 x 32 = 2 x 2 MFMA tiles of 16 x 16, reduction
// in stages of 32 (one MFMA step) through double-buffered LDS, one barrier per stage, the next stage's global loads in flight
// during the MFMAs.  An operand is staged as it lies in memory, 8 consecutive elements of one row per thread and stage (16- or
// 32-byte loads where rows are 8-element multiples and 16-byte aligned, element loads where they are a head's width: 14, 42,
// 63 ...), rounded to bf16 on the way:
//   K-major (x, W of the forward, dy of dgrad): LDS rows [64][kAbRow = 40], the fragment layout of msda_attn_tile.h: lane
//     (c, r) reads k = 8 r .. 8 r + 7 of row c with one ds_read_b128;
//   MN-major (W of dgrad, dy and x of wgrad): LDS rows [32][kTrRow = 72], read transposed with ds_read_b64_tr_b16 (ab_tr's
//     addressing on a 64-column row): lane (c, r) supplies 4 columns of row 8 r + c / 4 and receives rows 8 r .. 8 r + 3 of
//     column c; two reads give the 8 k of an MFMA operand.  The transposed read needs all 64 lanes: the stage loop is uniform.
// Fixed summation order everywhere, no atomics: bitwise reproducible.
#include <cstring>

#include "msda_attn_tile.h"
#include "msda_common.h"
#include "msda_launch.h"

namespace msda {

namespace {

constexpr int kBBlock = 256, kBT = 64, kBS = 32, kTrRow = kBT + 8;
constexpr int kBLds = kBT * kAbRow > kBS * kTrRow ? kBT * kAbRow : kBS * kTrRow;
constexpr int kSrcBf16 = 1, kSrcVec = 2;

// ---- problem tables: the fp32 form's (msda_launch.h), with a dtype beside every pointer that can be either -------------
struct BfFwdGroup {
    const float *w, *b;
    void *out;
    int n, off, out_bf16, pad;
};
struct BfFwdProb {
    const void *a;
    float *sig;
    int row0, rows, n, epi, g0, ng, tile0, a_bf16;
};
struct BfFwdArgs {
    BfFwdProb p[kHeadsFwdMaxProbs];
    BfFwdGroup g[kHeadsFwdMaxGroups];
    const float *init_ref, *inter_ref;
    int nprob, M, C, R;
};
struct BfDgradSeg {             // dy [L * M, k] (fp32 or bf16) o mode (aux: fp32 sigmoids / bf16 activations) times w [k, C]
    const void *a, *aux;
    const float *w;
    int k, mode, a_bf16, vec;   // vec: k % 8 == 0, 16-byte aligned rows, no sigmoid: 8 elements per load
};
struct BfDgradProb {
    void *out;                  // [L * M, C]: bf16 hidden gradient, or fp32 grad_hs
    int row0, rows, s0, ns, tile0, out_bf16;
};
struct BfDgradArgs {
    BfDgradProb p[kHeadsDgradMaxProbs];
    BfDgradSeg s[kHeadsDgradMaxSegs];
    int nprob, C;
};
struct BfWgradProb {
    const void *dy, *aux, *x;
    long long part;
    int row0, rows, n, mode, chunks, tile0, dy_flags, x_bf16;      // dy_flags: kSrcBf16 | kSrcVec (as BfDgradSeg::vec)
};
struct BfWgradArgs {
    BfWgradProb p[kHeadsWgradMaxProbs];
    float *ws;
    int nprob, C;
};
static_assert(sizeof(BfFwdArgs) <= 4000 && sizeof(BfDgradArgs) <= 4000 && sizeof(BfWgradArgs) <= 4000, "kernel argument tables");

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

// the reference's inverse_sigmoid (util/misc.py:614-618)
__device__ __forceinline__ float inv_sigmoid(float x)
{
    x = fminf(fmaxf(x, 0.f), 1.f);
    const float x1 = fmaxf(x, 1e-5f), x2 = fmaxf(1.f - x, 1e-5f);
    return logf(x1 / x2);
}

// dy o mode in fp32 (the staging rounds it to bf16): sigmoid' from the saved fp32 s, or the ReLU mask of the saved bf16 activation
__device__ __forceinline__ float apply_mode(float a, const void *aux, long long e, int mode)
{
    if (mode == kHeadsModeSigmoid) {
        const float s = static_cast<const float *>(aux)[e];
        return (a * 2.f) * (1.f - s) * s;
    }
    if (mode == kHeadsModeRelu) return bf_f(static_cast<const uint16_t *>(aux)[e]) > 0.f ? a : 0.f;
    return a;
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
// 8 consecutive dy o mode of one row from element e on, of which `valid` exist, rounded to bf16
__device__ __forceinline__ uint4 ld_dy8(const void *dy, const void *aux, long long e, int valid, int bf16, int vec, int mode)
{
    if (vec) {                                                          // valid == 8
        const uint4 a = ld_row8(dy, e, bf16);
        return mode == kHeadsModeRelu ? relu_mask8(a, ld_row8(aux, e, 1)) : a;
    }
    float v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = u < valid ? apply_mode(ld_elem(dy, e + u, bf16), aux, e + u, mode) : 0.f;
    return pack8(v);
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

// ---- forward: y = rnd(x . W^T + b), one launch per depth -----------------------------------------------------------------
__global__ __launch_bounds__(kBBlock) void heads_fwd_bf16_kernel(BfFwdArgs P)
{
    __shared__ __attribute__((aligned(16))) uint16_t As[2][kBLds];
    __shared__ __attribute__((aligned(16))) uint16_t Bs[2][kBLds];
    __shared__ float refoff[kBT][2];
    int pi = 0;
    while (pi + 1 < P.nprob && (int)blockIdx.x >= P.p[pi + 1].tile0) ++pi;
    const BfFwdProb &p = P.p[pi];
    const int tiles_n = (p.n + kBT - 1) / kBT;
    const int local = (int)blockIdx.x - p.tile0;
    if (local >= ((p.rows + kBT - 1) / kBT) * tiles_n) return;
    const int m0 = (local / tiles_n) * kBT, n0 = (local % tiles_n) * kBT;
    const int C = P.C, tid = threadIdx.x;

    // this thread's rows: x row m, weight row j of group gi (both K-major, rows C long)
    const int m = m0 + (tid >> 2), j = n0 + (tid >> 2), kq = (tid & 3) * 8;
    const float *wrow = nullptr;
    if (j < p.n) {
        int gi = p.g0;
        while (gi + 1 < p.g0 + p.ng && j >= P.g[gi + 1].off) ++gi;
        wrow = P.g[gi].w + (long long)(j - P.g[gi].off) * C;
    }
    const long long arow = ((long long)p.row0 + m) * C;
    auto load = [&](int s, uint4 &ra, uint4 &rb) {
        const int k = s * kBS + kq;
        ra = make_uint4(0u, 0u, 0u, 0u);
        rb = ra;
        if (m < p.rows && k < C) ra = ld_row8(p.a, arow + k, p.a_bf16);
        if (wrow != nullptr && k < C) rb = ld_row8(wrow, k, 0);
    };
    at_f4 acc[2][2];
    tile_loop<true, true>(As, Bs, (C + kBS - 1) / kBS, load, NoStage(), acc);

    // AssemblyHands keypoints: the x / y offsets of each row of the tile, as in the fp32 form (fp32 under autocast as well)
    if (p.epi == kHeadsEpiAssembly) {
        if (tid < 2 * kBT) {
            const int row = tid >> 1, coord = tid & 1, gr = p.row0 + m0 + row;
            float v = 0.f;
            if (m0 + row < p.rows) {
                const bool first = gr < P.M;
                const float *ref = first ? P.init_ref + (long long)gr * P.R : P.inter_ref + (long long)(gr - P.M) * P.R;
                if (P.R == 2) {
                    const float q = ref[coord];
                    v = inv_sigmoid(first ? q : (q + 0.5f) / 2.f);
                } else {
                    float sum = 0.f;
                    for (int q = 0; q < P.R / 2; ++q) {
                        const float x = ref[2 * q + coord];
                        sum += inv_sigmoid(first ? x : (x + 0.5f) / 2.f);
                    }
                    v = sum / (float)(P.R / 2);
                }
            }
            refoff[row][coord] = v;
        }
        __syncthreads();
    }

    const int wave = tid >> 6, lane = tid & 63;
    const int i0 = (wave >> 1) * 32, r = lane >> 4, c = lane & 15;
#pragma unroll
    for (int tj = 0; tj < 2; ++tj) {
        const int jo = n0 + (wave & 1) * 32 + 16 * tj + c;
        if (jo >= p.n) continue;
        int gi = p.g0;
        while (gi + 1 < p.g0 + p.ng && jo >= P.g[gi + 1].off) ++gi;
        const BfFwdGroup &G = P.g[gi];
        const int jj = jo - G.off;
        const float bj = G.b[jj];
#pragma unroll
        for (int ti = 0; ti < 2; ++ti)
#pragma unroll
            for (int v4 = 0; v4 < 4; ++v4) {
                const int lr = i0 + 16 * ti + 4 * r + v4, mo = m0 + lr;
                if (mo >= p.rows) continue;
                const long long gr = (long long)p.row0 + mo, e = gr * G.n + jj;
                float v = bf_round(acc[ti][tj][v4] + bj);                   // the Linear's bf16 output
                if (p.epi == kHeadsEpiRelu) {
                    v = fmaxf(v, 0.f);
                } else if (p.epi == kHeadsEpiArctic) {
                    // fp32 from here: (delta + inverse_sigmoid(reference)).sigmoid() * 2 - 1
                    const float *ref = gr < P.M ? P.init_ref + gr * P.R : P.inter_ref + (gr - P.M) * P.R;
                    const float s = 1.f / (1.f + expf(-(v + inv_sigmoid(ref[jj]))));
                    p.sig[e] = s;
                    v = s * 2.f - 1.f;
                } else if (p.epi == kHeadsEpiAssembly) {
                    // bf16 tensor ops: key[..., :2] += offset (fp32 sum, rounded), sigmoid (fp32, rounded), * 2 (exact), - 0.5 (rounded)
                    const int coord = jj % 3;
                    if (coord < 2) v = bf_round(v + refoff[lr][coord]);
                    const float s = 1.f / (1.f + expf(-v));
                    p.sig[e] = s;
                    v = bf_round(bf_round(s) * 2.f) - 0.5f;
                }
                if (G.out_bf16) static_cast<uint16_t *>(G.out)[e] = f_bf(v);
                else static_cast<float *>(G.out)[e] = v;
            }
    }
}

// ---- input gradients: dx [rows, C] = sum over segments rnd(dy o mode) . rnd(W) -----------------------------------------
__global__ __launch_bounds__(kBBlock) void heads_dgrad_bf16_kernel(BfDgradArgs P)
{
    __shared__ __attribute__((aligned(16))) uint16_t As[2][kBLds];
    __shared__ __attribute__((aligned(16))) uint16_t Bs[2][kBLds];
    int pi = 0;
    while (pi + 1 < P.nprob && (int)blockIdx.x >= P.p[pi + 1].tile0) ++pi;
    const BfDgradProb &p = P.p[pi];
    const int C = P.C, tiles_n = (C + kBT - 1) / kBT;
    const int local = (int)blockIdx.x - p.tile0;
    if (local >= ((p.rows + kBT - 1) / kBT) * tiles_n) return;
    const int m0 = (local / tiles_n) * kBT, n0 = (local % tiles_n) * kBT, tid = threadIdx.x;
    int nstages = 0;
    for (int s = p.s0; s < p.s0 + p.ns; ++s) nstages += (P.s[s].k + kBS - 1) / kBS;
    // stage -> (segment, k0): the cursor only moves forward, one stage per call
    int cseg = p.s0, ck0 = 0, cstage = 0;
    const int m = m0 + slot_row<true>(tid), ka = slot_k<true>(tid);         // A = dy o mode [row, k], K-major
    const int kb = slot_row<false>(tid), jn = n0 + slot_k<false>(tid);      // B = W [k, C], MN-major
    auto load = [&](int s, uint4 &ra, uint4 &rb) {
        while (cstage < s) {
            ck0 += kBS;
            if (ck0 >= P.s[cseg].k) { ++cseg; ck0 = 0; }
            ++cstage;
        }
        const BfDgradSeg &S = P.s[cseg];
        ra = make_uint4(0u, 0u, 0u, 0u);
        rb = ra;
        const int k = ck0 + ka;
        if (m < p.rows && k < S.k)
            ra = ld_dy8(S.a, S.aux, ((long long)p.row0 + m) * S.k + k, min(8, S.k - k), S.a_bf16, S.vec, S.mode);
        if (ck0 + kb < S.k && jn < C) rb = ld_row8(S.w, (long long)(ck0 + kb) * C + jn, 0);
    };
    at_f4 acc[2][2];
    tile_loop<true, false>(As, Bs, nstages, load, NoStage(), acc);
    const int wave = tid >> 6, lane = tid & 63;
    const int i0 = (wave >> 1) * 32, r = lane >> 4, c = lane & 15;
#pragma unroll
    for (int tj = 0; tj < 2; ++tj) {
        const int jo = n0 + (wave & 1) * 32 + 16 * tj + c;
        if (jo >= C) continue;
#pragma unroll
        for (int ti = 0; ti < 2; ++ti)
#pragma unroll
            for (int v4 = 0; v4 < 4; ++v4) {
                const int mo = m0 + i0 + 16 * ti + 4 * r + v4;
                if (mo >= p.rows) continue;
                const long long e = ((long long)p.row0 + mo) * C + jo;
                if (p.out_bf16) static_cast<uint16_t *>(p.out)[e] = f_bf(acc[ti][tj][v4]);
                else static_cast<float *>(p.out)[e] = acc[ti][tj][v4];
            }
    }
}

// ---- weight gradients, per row chunk: part[chunk] [n, C] = rnd(dy o mode)^T . rnd(x), bpart[chunk] [n] = column sums ---------
__global__ __launch_bounds__(kBBlock) void heads_wgrad_bf16_kernel(BfWgradArgs P)
{
    __shared__ __attribute__((aligned(16))) uint16_t As[2][kBLds];
    __shared__ __attribute__((aligned(16))) uint16_t Bs[2][kBLds];
    __shared__ float bred[4][kBT];
    int pi = 0;
    while (pi + 1 < P.nprob && (int)blockIdx.x >= P.p[pi + 1].tile0) ++pi;
    const BfWgradProb &p = P.p[pi];
    const int C = P.C, tiles_j = (C + kBT - 1) / kBT, tiles_i = (p.n + kBT - 1) / kBT;
    const int local = (int)blockIdx.x - p.tile0;
    if (local >= p.chunks * tiles_i * tiles_j) return;
    const int chunk = local / (tiles_i * tiles_j), rem = local % (tiles_i * tiles_j);
    const int i0t = (rem / tiles_j) * kBT, j0t = (rem % tiles_j) * kBT, tid = threadIdx.x;
    const int r0 = chunk * kHeadsWgradChunk;
    const int nrows = min(kHeadsWgradChunk, p.rows - r0);
    const long long base = (long long)p.row0 + r0;
    // A(i, m) = (dy o mode)[m, i] and B(j, m) = x[m, j]: both MN-major, 8 columns of one row m per thread
    const int km = slot_row<false>(tid), ic = i0t + slot_k<false>(tid), jc = j0t + slot_k<false>(tid);
    auto load = [&](int s, uint4 &ra, uint4 &rb) {
        const int mm = s * kBS + km;
        ra = make_uint4(0u, 0u, 0u, 0u);
        rb = ra;
        if (mm < nrows) {
            if (ic < p.n)
                ra = ld_dy8(p.dy, p.aux, (base + mm) * p.n + ic, min(8, p.n - ic), p.dy_flags & kSrcBf16, p.dy_flags & kSrcVec, p.mode);
            if (jc < C) rb = ld_row8(p.x, (base + mm) * C + jc, p.x_bf16);
        }
    };
    // bias: the column tile 0 workgroups also sum their staged rnd(dy o mode), thread (q, i) over 8 rows of each stage
    float bsum = 0.f;
    const bool with_bias = j0t == 0;
    auto per_stage = [&](const uint16_t *S) {
        if (with_bias) {
            const uint16_t *col = S + (tid >> 6) * 8 * kTrRow + (tid & 63);
#pragma unroll
            for (int u = 0; u < 8; ++u) bsum += bf_f(col[u * kTrRow]);
        }
    };
    at_f4 acc[2][2];
    tile_loop<false, false>(As, Bs, (nrows + kBS - 1) / kBS, load, per_stage, acc);
    float *part = P.ws + p.part;
    if (with_bias) {                                                            // uniform per workgroup
        bred[tid >> 6][tid & 63] = bsum;
        __syncthreads();
        if (tid < kBT && i0t + tid < p.n)
            part[(long long)p.chunks * p.n * C + (long long)chunk * p.n + i0t + tid] =
                ((bred[0][tid] + bred[1][tid]) + bred[2][tid]) + bred[3][tid];
    }
    const int wave = tid >> 6, lane = tid & 63;
    const int i0 = (wave >> 1) * 32, r = lane >> 4, c = lane & 15;
#pragma unroll
    for (int tj = 0; tj < 2; ++tj) {
        const int jo = j0t + (wave & 1) * 32 + 16 * tj + c;
        if (jo >= C) continue;
#pragma unroll
        for (int ti = 0; ti < 2; ++ti)
#pragma unroll
            for (int v4 = 0; v4 < 4; ++v4) {
                const int io = i0t + i0 + 16 * ti + 4 * r + v4;
                if (io < p.n) part[((long long)chunk * p.n + io) * C + jo] = acc[ti][tj][v4];
            }
    }
}

// ---- host side ----------------------------------------------------------------------------------------------------------
const int kSharedN[kHeadsShared] = {48, 10, 3, 3, 3, 1};   // mano pose, mano beta, hand cam, obj cam, obj rot, obj rad

int heads_D(int kind) { return kind == MSDA_HEADS_ARCTIC ? 42 : 63; }
int tiles_of(long long rows, int n) { return (int)(((rows + kBT - 1) / kBT) * ((n + kBT - 1) / kBT)); }
int chunks_of(long long rows) { return (int)((rows + kHeadsWgradChunk - 1) / kHeadsWgradChunk); }
bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
int herr(const char *msg) { return set_error(MSDA_ERR_ARGUMENT, msg); }
// dy rows of width n can be staged 8 elements per load: whole groups, aligned rows (fp32 rows: two 16-byte loads each)
int vec_ok(const void *dy, const void *aux, int n, int mode)
{
    return n % 8 == 0 && mode != kHeadsModeSigmoid && aligned16(dy) && (mode != kHeadsModeRelu || aligned16(aux)) ? 1 : 0;
}

struct BfFwdPlan {
    BfFwdArgs a[3];
    int tiles[3];
};
struct BfBwdPlan {
    BfDgradArgs d[3];
    int dtiles[3];
    BfWgradArgs w;
    int wtiles;
    HeadsReduceArgs r;
    int rblocks;
};
thread_local BfFwdPlan t_fwd;
thread_local BfBwdPlan t_bwd;

// The weight problems of the backward in the fp32 form's order: class head(s), MLP layers (head, layer, level), the six
// shared Linears.  `emit(dy, dy_bf16, aux, x, x_bf16, row0, rows, n, mode, dw, db)`.
template <class Emit>
void weight_problems(const HeadsBf16Call &c, Emit emit)
{
    const long long LM = (long long)c.L * c.M;
    const int M = (int)c.M, C = c.C, D = heads_D(c.kind);
    const bool shc = (c.flags & MSDA_HEADS_SHARED_CLS) != 0, shm = (c.flags & MSDA_HEADS_SHARED_MLP) != 0;
    const int Lc = shc ? 1 : c.L, Lw = shm ? 1 : c.L;
    const int out_bf16 = c.kind == MSDA_HEADS_ASSEMBLY;                  // logits / keypoint gradients: fp32 for ARCTIC
    for (int l = 0; l < Lc; ++l)
        emit(c.grad_logits, out_bf16, (const void *)nullptr, (const void *)c.hs, 0, shc ? 0 : l * M, shc ? (int)LM : M, c.K,
             kHeadsModePlain, c.grad_cls_w ? c.grad_cls_w[l] : nullptr, c.grad_cls_b ? c.grad_cls_b[l] : nullptr);
    const uint16_t *dH = static_cast<const uint16_t *>(c.ws);            // [n_mlp][2][LM][C] bf16: dH1, dH2
    for (int h = 0; h < c.n_mlp; ++h)
        for (int layer = 0; layer < 3; ++layer)
            for (int l = 0; l < Lw; ++l) {
                const int wi = (h * 3 + layer) * Lw + l;
                const uint16_t *H1 = c.hidden + (long long)(h * 2) * LM * C, *H2 = H1 + LM * C;
                const uint16_t *dH1 = dH ? dH + (long long)(h * 2) * LM * C : nullptr, *dH2 = dH ? dH1 + LM * C : nullptr;
                const void *dy = layer == 0 ? (const void *)dH1 : layer == 1 ? (const void *)dH2 : (c.grad_kp ? c.grad_kp[h] : nullptr);
                const void *aux = layer == 0 ? (const void *)H1 : layer == 1 ? (const void *)H2 : (const void *)(c.sig + (long long)h * LM * D);
                const void *x = layer == 0 ? (const void *)c.hs : layer == 1 ? (const void *)H1 : (const void *)H2;
                emit(dy, layer == 2 ? out_bf16 : 1, aux, x, layer == 0 ? 0 : 1, shm ? 0 : l * M, shm ? (int)LM : M,
                     layer == 2 ? D : C, layer == 2 ? kHeadsModeSigmoid : kHeadsModeRelu, c.grad_mlp_w ? c.grad_mlp_w[wi] : nullptr,
                     c.grad_mlp_b ? c.grad_mlp_b[wi] : nullptr);
            }
    if (c.kind == MSDA_HEADS_ARCTIC)
        for (int g = 0; g < kHeadsShared; ++g)
            emit(c.grad_shared ? (const void *)c.grad_shared[g] : nullptr, 1, (const void *)nullptr, (const void *)c.hs, 0, 0, (int)LM,
                 kSharedN[g], kHeadsModePlain, c.grad_shared_w ? c.grad_shared_w[g] : nullptr,
                 c.grad_shared_b ? c.grad_shared_b[g] : nullptr);
}

// The fp32 form's argument checks (sizes, flags, null pointers) on the same operands, then this form's own: widths and alignment.
int check(const HeadsBf16Call &c, bool backward)
{
    if (!heads_bf16_supported(c.C)) return herr("msda_heads_bf16: need a hidden size C with C % 8 == 0, 8 <= C <= 4096");
    HeadsCall f = {};
    f.kind = c.kind; f.L = c.L; f.n_mlp = c.n_mlp; f.R = c.R; f.C = c.C; f.K = c.K; f.M = c.M; f.flags = c.flags;
    f.hs = c.hs; f.init_ref = c.init_ref; f.inter_ref = c.inter_ref;
    f.cls_w = c.cls_w; f.cls_b = c.cls_b; f.mlp_w = c.mlp_w; f.mlp_b = c.mlp_b; f.shared_w = c.shared_w; f.shared_b = c.shared_b;
    f.logits = static_cast<float *>(c.logits);
    f.kp_out = reinterpret_cast<float *const *>(c.kp_out);
    f.shared_out = reinterpret_cast<float *const *>(c.shared_out);
    f.hidden = reinterpret_cast<float *>(c.hidden);
    f.sig = c.sig;
    f.grad_logits = static_cast<const float *>(c.grad_logits);
    f.grad_kp = reinterpret_cast<const float *const *>(c.grad_kp);
    f.grad_shared = reinterpret_cast<const float *const *>(c.grad_shared);
    f.grad_hs = c.grad_hs; f.grad_cls_w = c.grad_cls_w; f.grad_cls_b = c.grad_cls_b; f.grad_mlp_w = c.grad_mlp_w;
    f.grad_mlp_b = c.grad_mlp_b; f.grad_shared_w = c.grad_shared_w; f.grad_shared_b = c.grad_shared_b;
    f.ws = c.ws;
    f.ws_bytes = ~0ULL;                                                   // this form's workspace is checked below
    const int rc = heads_check(f, backward);
    if (rc != MSDA_OK) return rc;
    const int Lc = (c.flags & MSDA_HEADS_SHARED_CLS) ? 1 : c.L, Lw = (c.flags & MSDA_HEADS_SHARED_MLP) ? 1 : c.L;
    bool ok = aligned16(c.hs) && (c.n_mlp == 0 || aligned16(c.hidden));
    for (int l = 0; l < Lc; ++l) ok = ok && aligned16(c.cls_w[l]);
    for (int i = 0; i < c.n_mlp * 3 * Lw; ++i) ok = ok && aligned16(c.mlp_w[i]);
    for (int g = 0; c.kind == MSDA_HEADS_ARCTIC && g < kHeadsShared; ++g) ok = ok && aligned16(c.shared_w[g]);
    if (!ok) return herr("msda_heads_bf16: hs, hidden and the weights must be 16-byte aligned");
    if (backward) {
        if (c.ws == nullptr || !aligned16(c.ws)) return herr("msda_heads_bf16: the workspace must be 16-byte aligned");
        if (c.ws_bytes < heads_bf16_workspace_bytes(c.kind, c.L, c.M, c.C, c.K, c.n_mlp, c.flags))
            return herr("msda_heads_bf16: workspace smaller than msda_heads_bf16_workspace_bytes");
    }
    return MSDA_OK;
}

}  // namespace

bool heads_bf16_supported(int C) { return C >= 8 && C <= 4096 && C % 8 == 0; }

// bf16 hidden gradients [n_mlp][2][L * M][C] (an even count: the float partials behind them stay 4-byte aligned), then per
// weight problem fp32 partials [chunks][n][C] and [chunks][n].
unsigned long long heads_bf16_workspace_bytes(int kind, int L, long long M, int C, int K, int n_mlp, unsigned flags)
{
    HeadsBf16Call c = {};
    c.kind = kind; c.L = L; c.M = M; c.C = C; c.K = K; c.n_mlp = n_mlp; c.flags = flags;
    const long long LM = (long long)L * M;
    unsigned long long bytes = (unsigned long long)n_mlp * 2 * LM * C * sizeof(uint16_t);
    weight_problems(c, [&](const void *, int, const void *, const void *, int, int, int rows, int n, int, float *, float *) {
        bytes += (unsigned long long)chunks_of(rows) * n * (C + 1) * sizeof(float);
    });
    return bytes;
}

int heads_bf16_plan_forward(const HeadsBf16Call &c)
{
    const int rc = check(c, false);
    if (rc != MSDA_OK) return rc;
    BfFwdPlan &plan = t_fwd;
    std::memset(&plan, 0, sizeof(plan));
    const long long LM = (long long)c.L * c.M;
    const int M = (int)c.M, C = c.C, D = heads_D(c.kind);
    const bool shc = (c.flags & MSDA_HEADS_SHARED_CLS) != 0, shm = (c.flags & MSDA_HEADS_SHARED_MLP) != 0;
    const int Lw = shm ? 1 : c.L;
    const int out_bf16 = c.kind == MSDA_HEADS_ASSEMBLY;                  // logits and keypoints: fp32 for ARCTIC
    for (int d = 0; d < 3; ++d) {
        BfFwdArgs &a = plan.a[d];
        a.init_ref = c.init_ref;
        a.inter_ref = c.inter_ref;
        a.M = M;
        a.C = C;
        a.R = c.R;
        int ng = 0, tiles = 0;
        auto add = [&](const void *x, int x_bf16, int row0, int rows, int epi, float *sig) -> BfFwdProb & {
            BfFwdProb &p = a.p[a.nprob++];
            p.a = x; p.a_bf16 = x_bf16; p.sig = sig; p.row0 = row0; p.rows = rows; p.epi = epi; p.g0 = ng; p.ng = 0; p.n = 0;
            p.tile0 = tiles;
            return p;
        };
        auto group = [&](BfFwdProb &p, const float *w, const float *b, void *out, int bf16, int n) {
            BfFwdGroup &g = a.g[ng++];
            g.w = w; g.b = b; g.out = out; g.out_bf16 = bf16; g.n = n; g.off = p.n;
            p.n += n;
            ++p.ng;
        };
        for (int l = 0; l < c.L; ++l) {
            if (d == 0) {
                BfFwdProb &p = add(c.hs, 0, l * M, M, kHeadsEpiBias, nullptr);
                group(p, c.cls_w[shc ? 0 : l], c.cls_b[shc ? 0 : l], c.logits, out_bf16, c.K);
                tiles += tiles_of(M, p.n);
            }
            for (int h = 0; h < c.n_mlp; ++h) {
                const int wi = (h * 3 + d) * Lw + (shm ? 0 : l);
                uint16_t *H1 = c.hidden + (long long)(h * 2) * LM * C, *H2 = H1 + LM * C;
                const void *x = d == 0 ? (const void *)c.hs : d == 1 ? (const void *)H1 : (const void *)H2;
                void *out = d == 0 ? (void *)H1 : d == 1 ? (void *)H2 : c.kp_out[h];
                const int epi = d < 2 ? kHeadsEpiRelu : c.kind == MSDA_HEADS_ARCTIC ? kHeadsEpiArctic : kHeadsEpiAssembly;
                BfFwdProb &p = add(x, d == 0 ? 0 : 1, l * M, M, epi, d == 2 ? c.sig + (long long)h * LM * D : nullptr);
                group(p, c.mlp_w[wi], c.mlp_b[wi], out, d < 2 ? 1 : out_bf16, d < 2 ? C : D);
                tiles += tiles_of(M, p.n);
            }
        }
        if (d == 0 && c.kind == MSDA_HEADS_ARCTIC) {                    // the six shared Linears: ONE problem over L * M rows
            BfFwdProb &p = add(c.hs, 0, 0, (int)LM, kHeadsEpiBias, nullptr);
            for (int g = 0; g < kHeadsShared; ++g) group(p, c.shared_w[g], c.shared_b[g], c.shared_out[g], 1, kSharedN[g]);
            tiles += tiles_of(LM, p.n);
        }
        plan.tiles[d] = tiles;
    }
    return MSDA_OK;
}

int heads_bf16_plan_backward(const HeadsBf16Call &c)
{
    const int rc = check(c, true);
    if (rc != MSDA_OK) return rc;
    BfBwdPlan &plan = t_bwd;
    std::memset(&plan, 0, sizeof(plan));
    const long long LM = (long long)c.L * c.M;
    const int M = (int)c.M, C = c.C, D = heads_D(c.kind);
    const bool shc = (c.flags & MSDA_HEADS_SHARED_CLS) != 0, shm = (c.flags & MSDA_HEADS_SHARED_MLP) != 0;
    const int Lw = shm ? 1 : c.L;
    const int out_bf16 = c.kind == MSDA_HEADS_ASSEMBLY;
    uint16_t *dH = static_cast<uint16_t *>(c.ws);
    // input gradients: d[0] depth 3 -> dH2, d[1] depth 2 -> dH1 (bf16), d[2] depth 1 -> grad_hs (fp32)
    for (int step = 0; step < 3; ++step) {
        BfDgradArgs &a = plan.d[step];
        a.C = C;
        int ns = 0, tiles = 0;
        for (int l = 0; l < c.L; ++l) {
            auto seg = [&](const void *x, int x_bf16, const void *aux, const float *w, int k, int mode) {
                BfDgradSeg &s = a.s[ns++];
                s.a = x; s.a_bf16 = x_bf16; s.aux = aux; s.w = w; s.k = k; s.mode = mode;
                s.vec = vec_ok(x, aux, k, mode);
            };
            auto prob = [&](void *out, int bf16, int s0) {
                BfDgradProb &p = a.p[a.nprob++];
                p.out = out; p.out_bf16 = bf16; p.row0 = l * M; p.rows = M; p.s0 = s0; p.ns = ns - s0; p.tile0 = tiles;
                tiles += tiles_of(M, C);
            };
            if (step < 2) {
                for (int h = 0; h < c.n_mlp; ++h) {
                    const uint16_t *H1 = c.hidden + (long long)(h * 2) * LM * C, *H2 = H1 + LM * C;
                    uint16_t *dH1 = dH + (long long)(h * 2) * LM * C, *dH2 = dH1 + LM * C;
                    const int layer = 2 - step, wi = (h * 3 + layer) * Lw + (shm ? 0 : l);
                    const int s0 = ns;
                    if (step == 0) seg(c.grad_kp[h], out_bf16, c.sig + (long long)h * LM * D, c.mlp_w[wi], D, kHeadsModeSigmoid);
                    else seg(dH2, 1, H2, c.mlp_w[wi], C, kHeadsModeRelu);
                    prob(step == 0 ? dH2 : dH1, 1, s0);
                }
            } else {
                const int s0 = ns;
                seg(c.grad_logits, out_bf16, nullptr, c.cls_w[shc ? 0 : l], c.K, kHeadsModePlain);
                for (int h = 0; h < c.n_mlp; ++h) {
                    const uint16_t *H1 = c.hidden + (long long)(h * 2) * LM * C;
                    seg(dH + (long long)(h * 2) * LM * C, 1, H1, c.mlp_w[(h * 3) * Lw + (shm ? 0 : l)], C, kHeadsModeRelu);
                }
                if (c.kind == MSDA_HEADS_ARCTIC)
                    for (int g = 0; g < kHeadsShared; ++g) seg(c.grad_shared[g], 1, nullptr, c.shared_w[g], kSharedN[g], kHeadsModePlain);
                prob(c.grad_hs, 0, s0);
            }
        }
        plan.dtiles[step] = tiles;
    }
    // weight gradients: fp32 partials per chunk behind the bf16 hidden gradients, then the fp32 form's chunk-ordered reduce
    float *wsf = static_cast<float *>(c.ws);
    long long off = (long long)c.n_mlp * LM * C;                          // in floats: n_mlp * 2 * LM * C bf16
    plan.w.ws = wsf;
    plan.w.C = C;
    plan.r.ws = wsf;
    plan.r.C = C;
    int wt = 0, rb = 0;
    weight_problems(c, [&](const void *dy, int dy_bf16, const void *aux, const void *x, int x_bf16, int row0, int rows, int n,
                           int mode, float *dw, float *db) {
        BfWgradProb &p = plan.w.p[plan.w.nprob++];
        p.dy = dy; p.dy_flags = (dy_bf16 ? kSrcBf16 : 0) | (vec_ok(dy, aux, n, mode) ? kSrcVec : 0); p.aux = aux; p.x = x; p.x_bf16 = x_bf16; p.part = off; p.row0 = row0; p.rows = rows;
        p.n = n; p.mode = mode; p.chunks = chunks_of(rows); p.tile0 = wt;
        wt += p.chunks * ((n + kBT - 1) / kBT) * ((C + kBT - 1) / kBT);
        HeadsReduceProb &r = plan.r.p[plan.r.nprob++];
        r.part = off; r.dw = dw; r.db = db; r.n = n; r.chunks = p.chunks; r.blk0 = rb;
        rb += (int)(((long long)n * (C + 1) + kHeadsReduceBlock - 1) / kHeadsReduceBlock);
        off += (long long)p.chunks * n * (C + 1);
    });
    plan.wtiles = wt;
    plan.rblocks = rb;
    return MSDA_OK;
}

int heads_bf16_run_forward(hipStream_t stream)
{
    const BfFwdPlan &plan = t_fwd;
    for (int d = 0; d < 3; ++d) {
        if (plan.tiles[d] == 0) continue;
        hipLaunchKernelGGL(heads_fwd_bf16_kernel, dim3((unsigned)plan.tiles[d]), dim3(kBBlock), 0, stream, plan.a[d]);
        const int rc = check_launch("heads_fwd_bf16_kernel");
        if (rc != MSDA_OK) return rc;
    }
    return MSDA_OK;
}

int heads_bf16_run_backward(hipStream_t stream)
{
    const BfBwdPlan &plan = t_bwd;
    for (int s = 0; s < 3; ++s) {
        if (plan.dtiles[s] == 0) continue;
        hipLaunchKernelGGL(heads_dgrad_bf16_kernel, dim3((unsigned)plan.dtiles[s]), dim3(kBBlock), 0, stream, plan.d[s]);
        const int rc = check_launch("heads_dgrad_bf16_kernel");
        if (rc != MSDA_OK) return rc;
    }
    if (plan.wtiles > 0) {
        hipLaunchKernelGGL(heads_wgrad_bf16_kernel, dim3((unsigned)plan.wtiles), dim3(kBBlock), 0, stream, plan.w);
        const int rc = check_launch("heads_wgrad_bf16_kernel");
        if (rc != MSDA_OK) return rc;
    }
    return launch_heads_reduce(plan.r, plan.rblocks, stream);
}

}  // namespace msda
