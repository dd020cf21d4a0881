// The kernels of the bf16-autocast form of the DeformableDETR prediction heads.  msda_heads.hip holds the decomposition, the fp32
// kernels and the one planner of both forms (argument check, problem tables, workspace layout, launch order): this file
// receives the tables it built (msda_launch.h: a bf16 flag beside every pointer that can be either) and launches them, so the
// grouped problems and the launch budget (3 forward, 5 backward) are the fp32 form's by construction.  Every product runs on
// v_mfma_f32_16x16x32_bf16 with fp32 accumulation.
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
#include "msda_attn_tile.h"
#include "msda_heads_common.h"

namespace msda {

namespace {

constexpr int kBBlock = 256, kBT = 64, kBS = 32, kTrRow = kBT + 8;
constexpr int kBLds = kBT * kAbRow > kBS * kTrRow ? kBT * kAbRow : kBS * kTrRow;
static_assert(kBBlock == kHeadsReduceBlock && kBT == kHeadsTile, "what the planner (msda_heads.hip) counts workgroups with");

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
__global__ __launch_bounds__(kBBlock) void heads_fwd_bf16_kernel(HeadsFwdArgs P)
{
    __shared__ __attribute__((aligned(16))) uint16_t As[2][kBLds];
    __shared__ __attribute__((aligned(16))) uint16_t Bs[2][kBLds];
    __shared__ float refoff[kBT][2];
    const HeadsFwdProb &p = P.p[heads_problem(P)];
    const int tiles_n = (p.n + kBT - 1) / kBT;
    const int local = (int)blockIdx.x - p.tile0;
    if (local >= ((p.rows + kBT - 1) / kBT) * tiles_n) return;
    const int m0 = (local / tiles_n) * kBT, n0 = (local % tiles_n) * kBT;
    const int C = P.C, tid = threadIdx.x;

    // this thread's rows: x row m, weight row j of group gi (both K-major, rows C long)
    const int m = m0 + (tid >> 2), j = n0 + (tid >> 2), kq = (tid & 3) * 8;
    const float *wrow = nullptr;
    if (j < p.n) {
        const HeadsFwdGroup &G = P.g[heads_group(P, p, j)];
        wrow = G.w + (long long)(j - G.off) * C;
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

    if (p.epi == kHeadsEpiAssembly) heads_refoff(P, p, m0, refoff);           // fp32 under autocast as well

    const int wave = tid >> 6, lane = tid & 63;
    const int i0 = (wave >> 1) * 32, r = lane >> 4, c = lane & 15;
#pragma unroll
    for (int tj = 0; tj < 2; ++tj) {
        const int jo = n0 + (wave & 1) * 32 + 16 * tj + c;
        if (jo >= p.n) continue;
        const HeadsFwdGroup &G = P.g[heads_group(P, p, jo)];
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
__global__ __launch_bounds__(kBBlock) void heads_dgrad_bf16_kernel(HeadsDgradArgs P)
{
    __shared__ __attribute__((aligned(16))) uint16_t As[2][kBLds];
    __shared__ __attribute__((aligned(16))) uint16_t Bs[2][kBLds];
    const HeadsDgradProb &p = P.p[heads_problem(P)];
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
        const HeadsDgradSeg &S = P.s[cseg];
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
__global__ __launch_bounds__(kBBlock) void heads_wgrad_bf16_kernel(HeadsWgradArgs P)
{
    __shared__ __attribute__((aligned(16))) uint16_t As[2][kBLds];
    __shared__ __attribute__((aligned(16))) uint16_t Bs[2][kBLds];
    __shared__ float bred[4][kBT];
    const HeadsWgradProb &p = P.p[heads_problem(P)];
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
                ra = ld_dy8(p.dy, p.aux, (base + mm) * p.n + ic, min(8, p.n - ic), p.dy_flags & kHeadsSrcBf16, p.dy_flags & kHeadsSrcVec, p.mode);
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

}  // namespace

int launch_heads_forward_bf16(const HeadsFwdArgs &a, int tiles, hipStream_t stream)
{
    return heads_launch(heads_fwd_bf16_kernel, "heads_fwd_bf16_kernel", a, tiles, stream);
}

int launch_heads_dgrad_bf16(const HeadsDgradArgs &a, int tiles, hipStream_t stream)
{
    return heads_launch(heads_dgrad_bf16_kernel, "heads_dgrad_bf16_kernel", a, tiles, stream);
}

int launch_heads_wgrad_bf16(const HeadsWgradArgs &a, int tiles, hipStream_t stream)
{
    return heads_launch(heads_wgrad_bf16_kernel, "heads_wgrad_bf16_kernel", a, tiles, stream);
}

}  // namespace msda
