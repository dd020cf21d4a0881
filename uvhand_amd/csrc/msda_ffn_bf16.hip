// The bf16-autocast form of the layers' FFN, linear2(dropout(relu(linear1(x)))) (models/arctic_transformer.py:283-287,
// :366-370): one fused forward kernel and the two input-gradient kernels of its backward; the weight gradients take the
// existing bf16-operand path of msda_linear.hip.  Every product runs on v_mfma_f32_16x16x32_bf16 with fp32 accumulation.
//
// Rounding points (torch's bf16 autocast over the composition; DESIGN.md, "bf16-autocast FFN"): x, W1 and W2 are rounded to
// bf16, to nearest even, in the loads that stage them (no cast kernel, no bf16 copy of a weight); h = rnd(x . W1^T + b1) with
// the fp32 bias added before the one rounding; a = rnd(relu(h) * keep * scale); y = rnd(a . W2^T + b2).  h exists in registers
// only.  Backward: gh = rnd((go . W2) * scale * [a > 0]) in the workspace; gx = gh . W1, unrounded fp32 or rounded once to bf16.
//
// Forward: a workgroup of 256 threads owns 64 rows.  Their bf16 x panel [64][C + 8] stays in LDS; F is walked in chunks of 64:
//   1. h chunk [64 x 64] = x panel . W1[f0 .. f0 + 63]^T, the 2 x 2 wavefront layout of msda_bf16_tile.h, W1 through
//      double-buffered K-major stages of 32;
//   2. bias, rounding, ReLU, the hash mask and the scale; the a chunk goes to LDS [64][72], and from there to memory in 16-byte
//      stores;
//   3. y panel [64 x C] += a chunk . W2[:, f0 .. f0 + 63]^T in two steps of 32 through one K-major stage [C][40]: wavefront w
//      owns all 64 rows of the columns [w C / 4, (w + 1) C / 4), so its 4 x C / 64 accumulator tiles (64 fp32 per thread at
//      C = 256) live in registers over the whole walk.  The first step's W2 loads are issued before 1., the second's before
//      the first step's MFMAs.
// y = rnd(acc + b2) leaves through the x panel's LDS in 16-byte stores.  LDS at C = 256: 33.0 + 9.0 + 10.0 + 20.0 = 72 KB, two
// workgroups (8 wavefronts) per CU of 160 KB.
// Dropout: keep iff at_hash(row * F + col + at_mix(seed, 0)) >= p * 2^32 (msda_attn_tile.h); the backward reads a > 0, so no
// mask and no seed outlive the forward.  Fixed summation order, no atomics: bitwise reproducible.
#include "msda_bf16_tile.h"
#include "msda_launch.h"

namespace msda {

namespace {

constexpr int kFfChunk = 64, kFfARow = kFfChunk + 8;
constexpr int kFfMinC = 64, kFfMaxC = 256, kFfMinF = 64, kFfMaxF = 8192;
static_assert(kFfChunk == kBT && 2 * kBLds >= kBT * kFfARow, "the dgrad epilogue's tile fits the two A stages");

struct FfnFwdArgs {
    const void *x;
    const float *w1, *b1, *w2, *b2;
    const unsigned long long *seed;         // device; null when thresh == 0
    uint16_t *xb, *a, *y;
    int x_bf16, M, F;
    unsigned thresh;                        // keep iff hash >= thresh (p * 2^32; 0: no dropout)
    float scale;
};

template <int NC>
__global__ __launch_bounds__(kBBlock) void ffn_fwd_bf16_kernel(FfnFwdArgs P)
{
    constexpr int C = 64 * NC, XR = C + 8, KS = C / kBS;
    __shared__ __attribute__((aligned(16))) uint16_t xs[kBT * XR];
    __shared__ __attribute__((aligned(16))) uint16_t as[kBT * kFfARow];
    __shared__ __attribute__((aligned(16))) uint16_t w1s[2][kBT * kAbRow];
    __shared__ __attribute__((aligned(16))) uint16_t w2s[C * kAbRow];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane >> 4, c = lane & 15;
    const int m0 = (int)blockIdx.x * kBT, M = P.M, F = P.F;

    // the x panel, rounded once; an fp32 x leaves its bf16 form behind for the backward (rows past M: zeros, never stored)
    for (int e = tid; e < kBT * (C / 8); e += kBBlock) {
        const int row = e / (C / 8), k = (e % (C / 8)) * 8;
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (m0 + row < M) {
            const long long g = (long long)(m0 + row) * C + k;
            v = ld_row8(P.x, g, P.x_bf16);
            if (!P.x_bf16) *reinterpret_cast<uint4 *>(P.xb + g) = v;
        }
        *reinterpret_cast<uint4 *>(xs + row * XR + k) = v;
    }

    const int i0 = (wave >> 1) * 32, j0 = (wave & 1) * 32;
    const int sr = slot_row<true>(tid), sk = slot_k<true>(tid);     // this thread's slot of a K-major stage
    const unsigned mix = P.thresh ? at_mix(P.seed[0], 0u) : 0u;
    at_f4 yacc[4][NC];
#pragma unroll
    for (int ti = 0; ti < 4; ++ti)
#pragma unroll
        for (int tj = 0; tj < NC; ++tj) yacc[ti][tj] = at_f4{0.f, 0.f, 0.f, 0.f};

    auto load_w2 = [&](int k0, uint4 (&rw)[NC]) {                  // W2 [C, F]: rows sr + 64 u, k k0 + sk ..
#pragma unroll
        for (int u = 0; u < NC; ++u) rw[u] = ld_row8(P.w2, (long long)(sr + 64 * u) * F + k0 + sk, 0);
    };
    auto store_w2 = [&](const uint4 (&rw)[NC]) {
#pragma unroll
        for (int u = 0; u < NC; ++u) *reinterpret_cast<uint4 *>(w2s + (sr + 64 * u) * kAbRow + sk) = rw[u];
    };
    auto y_step = [&](int ks) {                                     // y panel += a chunk[:, 32 ks ..] . W2 stage^T
        at_bf8 av[4];
#pragma unroll
        for (int ti = 0; ti < 4; ++ti) av[ti] = ab_ld8(as + (16 * ti + c) * kFfARow + kBS * ks + 8 * r);
#pragma unroll
        for (int tj = 0; tj < NC; ++tj) {
            const at_bf8 b = ab_ld8(w2s + (wave * (C / 4) + 16 * tj + c) * kAbRow + 8 * r);
#pragma unroll
            for (int ti = 0; ti < 4; ++ti) yacc[ti][tj] = ab_mfma(av[ti], b, yacc[ti][tj]);
        }
    };

    for (int f0 = 0; f0 < F; f0 += kFfChunk) {
        uint4 rw2[NC];
        load_w2(f0, rw2);

        // 1. h chunk.  The stores into w1s / as / w2s below need no barrier of their own against the previous chunk's reads:
        //    every thread has passed the barriers that follow those reads (C / 32 >= 2 of them in this loop alone).
        at_f4 h[2][2];
#pragma unroll
        for (int ti = 0; ti < 2; ++ti)
#pragma unroll
            for (int tj = 0; tj < 2; ++tj) h[ti][tj] = at_f4{0.f, 0.f, 0.f, 0.f};
        const float *w1row = P.w1 + (long long)(f0 + sr) * C + sk;
        uint4 rb = ld_row8(w1row, 0, 0);
        stage_store<true>(w1s[0], tid, rb);
        __syncthreads();
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            const int cur = s & 1;
            if (s + 1 < KS) rb = ld_row8(w1row, (s + 1) * kBS, 0);
            const at_bf8 a0 = ab_ld8(xs + (i0 + c) * XR + kBS * s + 8 * r), a1 = ab_ld8(xs + (i0 + 16 + c) * XR + kBS * s + 8 * r);
            const at_bf8 b0 = operand<true>(w1s[cur], j0, r, c), b1 = operand<true>(w1s[cur], j0 + 16, r, c);
            h[0][0] = ab_mfma(a0, b0, h[0][0]);
            h[0][1] = ab_mfma(a0, b1, h[0][1]);
            h[1][0] = ab_mfma(a1, b0, h[1][0]);
            h[1][1] = ab_mfma(a1, b1, h[1][1]);
            if (s + 1 < KS) stage_store<true>(w1s[cur ^ 1], tid, rb);
            __syncthreads();
        }

        // 2. a = rnd(relu(rnd(h + b1)) * keep * scale) -> LDS
#pragma unroll
        for (int tj = 0; tj < 2; ++tj) {
            const int col = j0 + 16 * tj + c;
            const float bj = P.b1[f0 + col];
#pragma unroll
            for (int ti = 0; ti < 2; ++ti)
#pragma unroll
                for (int v4 = 0; v4 < 4; ++v4) {
                    const int lr = i0 + 16 * ti + 4 * r + v4;
                    float v = fmaxf(bf_round(h[ti][tj][v4] + bj), 0.f);
                    if (P.thresh) {
                        const unsigned ctr = (unsigned)(m0 + lr) * (unsigned)F + (unsigned)(f0 + col);
                        v = at_hash(ctr + mix) >= P.thresh ? v * P.scale : 0.f;
                    }
                    as[lr * kFfARow + col] = f_bf(v);
                }
        }

        // 3. the second product, and the a chunk's way to memory
        store_w2(rw2);
        __syncthreads();
        load_w2(f0 + kBS, rw2);
        {
            const int row = tid >> 2, col = (tid & 3) * 16;
            if (m0 + row < M) {
                const uint4 lo = *reinterpret_cast<const uint4 *>(as + row * kFfARow + col);
                const uint4 hi = *reinterpret_cast<const uint4 *>(as + row * kFfARow + col + 8);
                uint16_t *dst = P.a + (long long)(m0 + row) * F + f0 + col;
                *reinterpret_cast<uint4 *>(dst) = lo;
                *reinterpret_cast<uint4 *>(dst + 8) = hi;
            }
        }
        y_step(0);
        __syncthreads();
        store_w2(rw2);
        __syncthreads();
        y_step(1);
    }

    // y = rnd(acc + b2) through the x panel's LDS (last read in step 1 of the last chunk, barriers since)
#pragma unroll
    for (int tj = 0; tj < NC; ++tj) {
        const int col = wave * (C / 4) + 16 * tj + c;
        const float bj = P.b2[col];
#pragma unroll
        for (int ti = 0; ti < 4; ++ti)
#pragma unroll
            for (int v4 = 0; v4 < 4; ++v4) xs[(16 * ti + 4 * r + v4) * XR + col] = f_bf(yacc[ti][tj][v4] + bj);
    }
    __syncthreads();
    for (int e = tid; e < kBT * (C / 8); e += kBBlock) {
        const int row = e / (C / 8), k = (e % (C / 8)) * 8;
        if (m0 + row < M)
            *reinterpret_cast<uint4 *>(P.y + (long long)(m0 + row) * C + k) = *reinterpret_cast<const uint4 *>(xs + row * XR + k);
    }
}

// ---- input gradients: out [M, N] = dy [M, K] (bf16) . rnd(W [K, N]) (fp32), 64 x 64 tiles -----------------------------------
// act != null (gh): out = rnd(acc * scale) under the ReLU mask of the saved bf16 activation, bf16; else (gx) acc as fp32, or
// rounded once to bf16.  bf16 tiles leave through LDS in 16-byte stores.
struct FfnDgradArgs {
    const uint16_t *dy;
    const float *w;
    const uint16_t *act;
    void *out;
    int out_bf16, M, K, N;
    float scale;
};

__global__ __launch_bounds__(kBBlock) void ffn_dgrad_bf16_kernel(FfnDgradArgs P)
{
    __shared__ __attribute__((aligned(16))) uint16_t As[2][kBLds];
    __shared__ __attribute__((aligned(16))) uint16_t Bs[2][kBLds];
    const int tiles_n = P.N / kBT, K = P.K, N = P.N, M = P.M, tid = threadIdx.x;
    const int m0 = ((int)blockIdx.x / tiles_n) * kBT, n0 = ((int)blockIdx.x % tiles_n) * kBT;
    const int m = m0 + slot_row<true>(tid), ka = slot_k<true>(tid);         // A = dy [row, k], K-major
    const int kb = slot_row<false>(tid), jn = n0 + slot_k<false>(tid);      // B = W [k, N], MN-major
    auto load = [&](int s, uint4 &ra, uint4 &rb) {
        ra = make_uint4(0u, 0u, 0u, 0u);
        if (m < M) ra = ld_row8(P.dy, (long long)m * K + s * kBS + ka, 1);
        rb = ld_row8(P.w, (long long)(s * kBS + kb) * N + jn, 0);
    };
    at_f4 acc[2][2];
    tile_loop<true, false>(As, Bs, K / kBS, load, NoStage(), acc);
    const int wave = tid >> 6, lane = tid & 63;
    const int i0 = (wave >> 1) * 32, j0 = (wave & 1) * 32, r = lane >> 4, c = lane & 15;
    if (!P.out_bf16) {
        float *out = static_cast<float *>(P.out);
#pragma unroll
        for (int tj = 0; tj < 2; ++tj)
#pragma unroll
            for (int ti = 0; ti < 2; ++ti)
#pragma unroll
                for (int v4 = 0; v4 < 4; ++v4) {
                    const int mo = m0 + i0 + 16 * ti + 4 * r + v4;
                    if (mo < M) out[(long long)mo * N + n0 + j0 + 16 * tj + c] = acc[ti][tj][v4];
                }
        return;
    }
    uint16_t *T = &As[0][0];                                                // [64][kFfARow]: every stage read is behind a barrier
#pragma unroll
    for (int tj = 0; tj < 2; ++tj)
#pragma unroll
        for (int ti = 0; ti < 2; ++ti)
#pragma unroll
            for (int v4 = 0; v4 < 4; ++v4)
                T[(i0 + 16 * ti + 4 * r + v4) * kFfARow + j0 + 16 * tj + c] = f_bf(acc[ti][tj][v4] * P.scale);
    __syncthreads();
    const int row = tid >> 2, col = (tid & 3) * 16;
    if (m0 + row < M) {
        uint4 lo = *reinterpret_cast<const uint4 *>(T + row * kFfARow + col);
        uint4 hi = *reinterpret_cast<const uint4 *>(T + row * kFfARow + col + 8);
        const long long e = (long long)(m0 + row) * N + n0 + col;
        if (P.act != nullptr) {
            lo = relu_mask8(lo, ld_row8(P.act, e, 1));
            hi = relu_mask8(hi, ld_row8(P.act, e + 8, 1));
        }
        uint16_t *dst = static_cast<uint16_t *>(P.out) + e;
        *reinterpret_cast<uint4 *>(dst) = lo;
        *reinterpret_cast<uint4 *>(dst + 8) = hi;
    }
}

inline int ferr(const char *msg) { return set_error(MSDA_ERR_ARGUMENT, msg); }
inline size_t up256(size_t n) { return (n + 255) & ~(size_t)255; }
inline bool al16(const void *p) { return aligned_to(p, 16); }

int ffn_check_sizes(long long M, int C, int F, double p)
{
    if (!ffn_bf16_supported(C, F))
        return ferr("msda_ffn_bf16: need C % 64 == 0, 64 <= C <= 256 and F % 64 == 0, 64 <= F <= 8192");
    if (M < 1) return ferr("msda_ffn_bf16: need M >= 1");
    if (M * (long long)F >= (1ll << 31)) return ferr("msda_ffn_bf16: tensors beyond 2^31 elements (M * F)");
    if (!(p >= 0.0 && p < 1.0)) return ferr("msda_ffn_bf16: need a dropout probability 0 <= p < 1");
    return MSDA_OK;
}

struct FfnWorkspace { size_t gh, ws2, ws1, total; };        // offsets of gh, gW2's and gW1's partials; bytes in all
FfnWorkspace ffn_workspace(long long M, int C, int F)
{
    FfnWorkspace w;
    w.gh = 0;
    w.ws2 = up256((size_t)M * F * sizeof(uint16_t));
    w.ws1 = w.ws2 + up256(linear_wgrad_workspace_bytes((int)M, C, F));
    w.total = w.ws1 + up256(linear_wgrad_workspace_bytes((int)M, F, C));
    return w;
}

}  // namespace

bool ffn_bf16_supported(int C, int F)
{
    return C % 64 == 0 && C >= kFfMinC && C <= kFfMaxC && F % 64 == 0 && F >= kFfMinF && F <= kFfMaxF;
}

size_t ffn_bf16_workspace_bytes(long long M, int C, int F)
{
    if (!ffn_bf16_supported(C, F) || M < 1 || M * (long long)F >= (1ll << 31)) return 0;
    return ffn_workspace(M, C, F).total;
}

int ffn_check_forward_bf16(long long M, int C, int F, const void *x, int x_is_bf16, const float *w1, const float *b1, const float *w2,
                           const float *b2, double p, const long long *seed, const uint16_t *xb, const uint16_t *a, const uint16_t *y)
{
    if (int rc = ffn_check_sizes(M, C, F, p)) return rc;
    if (!x || !w1 || !b1 || !w2 || !b2 || !a || !y || (!x_is_bf16 && !xb)) return ferr("msda_ffn_bf16: null pointer");
    if (p > 0.0 && seed == nullptr) return ferr("msda_ffn_bf16: dropout (p > 0) needs a device seed");
    if (!al16(x) || !al16(w1) || !al16(w2) || !al16(a) || !al16(y) || (!x_is_bf16 && !al16(xb)))
        return ferr("msda_ffn_bf16: x, xb, a, y and the weights must be 16-byte aligned");
    return MSDA_OK;
}

int launch_ffn_forward_bf16(long long M, int C, int F, const void *x, int x_is_bf16, const float *w1, const float *b1, const float *w2,
                            const float *b2, double p, const long long *seed, uint16_t *xb, uint16_t *a, uint16_t *y,
                            hipStream_t stream)
{
    FfnFwdArgs P;
    P.x = x; P.w1 = w1; P.b1 = b1; P.w2 = w2; P.b2 = b2;
    P.seed = reinterpret_cast<const unsigned long long *>(seed);
    P.xb = xb; P.a = a; P.y = y; P.x_bf16 = x_is_bf16 ? 1 : 0; P.M = (int)M; P.F = F;
    P.thresh = p > 0.0 ? (unsigned)fmin(4294967295.0, p * 4294967296.0) : 0u;
    P.scale = (float)(1.0 / (1.0 - p));
    const dim3 grid((unsigned)((M + kBT - 1) / kBT)), block(kBBlock);
    switch (C / 64) {
    case 1: hipLaunchKernelGGL(ffn_fwd_bf16_kernel<1>, grid, block, 0, stream, P); break;
    case 2: hipLaunchKernelGGL(ffn_fwd_bf16_kernel<2>, grid, block, 0, stream, P); break;
    case 3: hipLaunchKernelGGL(ffn_fwd_bf16_kernel<3>, grid, block, 0, stream, P); break;
    default: hipLaunchKernelGGL(ffn_fwd_bf16_kernel<4>, grid, block, 0, stream, P); break;
    }
    return check_launch("msda_ffn_bf16 forward");
}

int ffn_check_backward_bf16(long long M, int C, int F, const uint16_t *grad_out, const uint16_t *xb, const uint16_t *a, const float *w1,
                            const float *w2, double p, const void *grad_x, const float *grad_w1, const float *grad_b1,
                            const float *grad_w2, const float *grad_b2, const void *workspace, unsigned long long workspace_bytes)
{
    if (int rc = ffn_check_sizes(M, C, F, p)) return rc;
    if (!grad_out || !xb || !a || !w1 || !w2 || !workspace) return ferr("msda_ffn_bf16: null pointer");
    if ((grad_b1 && !grad_w1) || (grad_b2 && !grad_w2))
        return ferr("msda_ffn_bf16: a bias gradient comes with its weight gradient (null pointer)");
    if (!al16(grad_out) || !al16(xb) || !al16(a) || !al16(w1) || !al16(w2) || !al16(grad_x) || !al16(workspace))
        return ferr("msda_ffn_bf16: grad_out, xb, a, grad_x, the weights and the workspace must be 16-byte aligned");
    if (workspace_bytes < ffn_workspace(M, C, F).total)
        return ferr("msda_ffn_bf16: workspace smaller than msda_ffn_bf16_workspace_bytes");
    return MSDA_OK;
}

int launch_ffn_backward_bf16(long long M, int C, int F, const uint16_t *grad_out, const uint16_t *xb, const uint16_t *a, const float *w1,
                             const float *w2, double p, void *grad_x, int grad_x_is_bf16, float *grad_w1, float *grad_b1,
                             float *grad_w2, float *grad_b2, void *workspace, hipStream_t stream)
{
    const FfnWorkspace W = ffn_workspace(M, C, F);
    unsigned char *ws = static_cast<unsigned char *>(workspace);
    uint16_t *gh = reinterpret_cast<uint16_t *>(ws + W.gh);
    const unsigned tiles_m = (unsigned)((M + kBT - 1) / kBT);
    if (grad_x || grad_w1) {
        FfnDgradArgs g;
        g.dy = grad_out; g.w = w2; g.act = a; g.out = gh; g.out_bf16 = 1; g.M = (int)M; g.K = C; g.N = F;
        g.scale = (float)(1.0 / (1.0 - p));
        hipLaunchKernelGGL(ffn_dgrad_bf16_kernel, dim3(tiles_m * (unsigned)(F / kBT)), dim3(kBBlock), 0, stream, g);
        if (int rc = check_launch("msda_ffn_bf16 backward (gh)")) return rc;
    }
    if (grad_x) {
        FfnDgradArgs g;
        g.dy = gh; g.w = w1; g.act = nullptr; g.out = grad_x; g.out_bf16 = grad_x_is_bf16 ? 1 : 0; g.M = (int)M; g.K = F; g.N = C;
        g.scale = 1.f;
        hipLaunchKernelGGL(ffn_dgrad_bf16_kernel, dim3(tiles_m * (unsigned)(C / kBT)), dim3(kBBlock), 0, stream, g);
        if (int rc = check_launch("msda_ffn_bf16 backward (gx)")) return rc;
    }
    // gW2 = go^T . a, gW1 = gh^T . xb: bf16 operands, fp32 results, first stages back to back and one second stage
    const void *dy[2], *xo[2];
    float *dw[2], *db[2], *wsp[2];
    int bf[2], Ms[2], Ns[2], Ks[2], n = 0;
    if (grad_w2) {
        dy[n] = grad_out; xo[n] = a; dw[n] = grad_w2; db[n] = grad_b2; wsp[n] = reinterpret_cast<float *>(ws + W.ws2);
        bf[n] = 1; Ms[n] = (int)M; Ns[n] = C; Ks[n] = F; ++n;
    }
    if (grad_w1) {
        dy[n] = gh; xo[n] = xb; dw[n] = grad_w1; db[n] = grad_b1; wsp[n] = reinterpret_cast<float *>(ws + W.ws1);
        bf[n] = 1; Ms[n] = (int)M; Ns[n] = F; Ks[n] = C; ++n;
    }
    if (n == 0) return MSDA_OK;
    return launch_linear_wgrad_multi(n, dy, xo, bf, nullptr, Ms, Ns, Ks, dw, db, wsp, stream);
}

}  // namespace msda
