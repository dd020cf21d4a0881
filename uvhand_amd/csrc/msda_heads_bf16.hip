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
// Kernel: the 64 x 64 staged tile loop of msda_bf16_tile.h (shared with the FFN's bf16 form): an operand is staged as it lies in
// memory, 8 consecutive elements of one row per thread and stage (16- or 32-byte loads where rows are 8-element multiples and
// 16-byte aligned, element loads where they are a head's width: 14, 42, 63 ...), rounded to bf16 on the way; x, W of the forward
// and dy of dgrad are K-major operands, W of dgrad and dy and x of wgrad MN-major ones.
// Fixed summation order everywhere, no atomics: bitwise reproducible.
#include "msda_bf16_tile.h"
#include "msda_heads_common.h"

namespace msda {

namespace {

static_assert(kBBlock == kHeadsReduceBlock && kBT == kHeadsTile, "what the planner (msda_heads.hip) counts workgroups with");

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
