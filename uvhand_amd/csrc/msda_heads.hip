// The DeformableDETR prediction heads (UVHand models/actic_detr.py:245-287, models/assembly_detr.py:172-210) as grouped fp32
// GEMMs: every head of every decoder level in one launch per MLP depth forward, and in five launches backward.
//
// Rows are the flattened [L * M, .] space of the stacked tensors (M = B * Q rows per level): hs [L, M, C], the saved hidden
// activations [head][layer][L * M][C], the stacked outputs [L, M, n].  A problem covers the rows of one level (or of every
// level: the six shared ARCTIC Linears) and describes where its operands lie; one problem table per launch, by value.
//
//   forward   depth d: y = x . W^T + b  (NT), epilogue bias | bias + ReLU | keypoint (ARCTIC / AssemblyHands, below);
//             depth 1 also runs the class head and the six shared Linears (one problem, six column groups, each written
//             straight into its stacked output)
//   dgrad     dx = sum over segments (dy o mode) . W  (NN): depth 3, depth 2, then depth 1, whose reduction runs over the
//             concatenated outputs of every head that reads hs[l]; mode = sigmoid' from the saved s, or the ReLU mask of the
//             saved activation (threshold_backward's `out > 0`)
//   wgrad     partial dW[chunk] = (dy o mode)^T . x  over row chunks of kHeadsWgradChunk rows, the bias column sums beside them
//   reduce    dW = sum over chunks, in chunk order
//
// Kernel: fp32 MFMA (v_mfma_f32_32x32x2_f32), 64 x 64 output tile per 256-thread workgroup, 2 x 2 wavefronts of 32 x 32,
// reduction in stages of 32 through double-buffered LDS (one barrier per stage, next stage's global loads in flight during
// the MFMAs), the lane / register layout of msda_gemm.hip.  An operand is staged K-major ([64][32 + 4]) or MN-major
// ([32][64 + 4]) as it lies in memory; 16-byte loads where rows are C floats long (C % 4 == 0), 4-byte loads where they are
// a head's width (14, 42, 63 ...).  Fixed summation order everywhere: bitwise reproducible.
#include <cstdio>
#include <cstring>

#include "msda_common.h"
#include "msda_launch.h"

namespace msda {

namespace {

#include "msda_tile.h"
static_assert(kHBlock == kHeadsReduceBlock, "heads_reduce_kernel's block is what the bf16 form's plan counts with");

// the reference's inverse_sigmoid (util/misc.py:614-618)
__device__ __forceinline__ float inv_sigmoid(float x)
{
    x = fminf(fmaxf(x, 0.f), 1.f);
    const float x1 = fmaxf(x, 1e-5f), x2 = fmaxf(1.f - x, 1e-5f);
    return logf(x1 / x2);
}

__device__ __forceinline__ float apply_mode(float a, const float *aux, long long e, int mode)
{
    if (mode == kHeadsModeSigmoid) {
        const float s = aux[e];
        return (a * 2.f) * (1.f - s) * s;                   // MulBackward (out = 2 s - c), then sigmoid_backward
    }
    if (mode == kHeadsModeRelu) return aux[e] > 0.f ? a : 0.f;
    return a;
}

// ---- forward: y = x . W^T + b, one launch per depth ---------------------------------------------------------------------
__global__ __launch_bounds__(kHBlock) void heads_fwd_kernel(HeadsFwdArgs P)
{
    __shared__ __attribute__((aligned(16))) float As[2][kLds];
    __shared__ __attribute__((aligned(16))) float Bs[2][kLds];
    __shared__ float refoff[kHT][2];
    int pi = 0;
    while (pi + 1 < P.nprob && (int)blockIdx.x >= P.p[pi + 1].tile0) ++pi;
    const HeadsFwdProb &p = P.p[pi];
    const int tiles_n = (p.n + kHT - 1) / kHT;
    const int local = (int)blockIdx.x - p.tile0;
    if (local >= ((p.rows + kHT - 1) / kHT) * tiles_n) return;
    const int m0 = (local / tiles_n) * kHT, n0 = (local % tiles_n) * kHT;
    const int C = P.C, tid = threadIdx.x;
    const float *A = p.a + (long long)p.row0 * C;

    auto load = [&](int s, float (&ra)[8], float (&rb)[8]) {
        const int k = s * kHS + (tid % 8) * 4;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int m = m0 + tid / 8 + 32 * u, j = n0 + tid / 8 + 32 * u;
            float4 va = make_float4(0.f, 0.f, 0.f, 0.f), vb = va;
            if (m < p.rows && k < C) va = *reinterpret_cast<const float4 *>(A + (long long)m * C + k);
            if (j < p.n && k < C) {
                int gi = p.g0;
                while (gi + 1 < p.g0 + p.ng && j >= P.g[gi + 1].off) ++gi;
                vb = *reinterpret_cast<const float4 *>(P.g[gi].w + (long long)(j - P.g[gi].off) * C + k);
            }
            ra[4 * u] = va.x; ra[4 * u + 1] = va.y; ra[4 * u + 2] = va.z; ra[4 * u + 3] = va.w;
            rb[4 * u] = vb.x; rb[4 * u + 1] = vb.y; rb[4 * u + 2] = vb.z; rb[4 * u + 3] = vb.w;
        }
    };
    const f32x16 acc = tile_loop<true, true, true, true>(As, Bs, (C + kHS - 1) / kHS, load, NoStage());

    // AssemblyHands keypoints: the x / y offsets of each row of the tile (models/assembly_detr.py:172-199): the reference point
    // (2-d) or the means of the 21 x and 21 y values (42-d), after inverse_sigmoid; levels >= 1 map r -> (r + 0.5) / 2 first
    if (p.epi == kHeadsEpiAssembly) {
        if (tid < 2 * kHT) {
            const int row = tid >> 1, coord = tid & 1, gr = p.row0 + m0 + row;
            float v = 0.f;
            if (m0 + row < p.rows) {
                const bool first = gr < P.M;
                const float *ref = first ? P.init_ref + (long long)gr * P.R : P.inter_ref + (long long)(gr - P.M) * P.R;
                if (P.R == 2) {
                    const float r = ref[coord];
                    v = inv_sigmoid(first ? r : (r + 0.5f) / 2.f);
                } else {
                    float sum = 0.f;
                    for (int q = 0; q < P.R / 2; ++q) {
                        const float r = ref[2 * q + coord];
                        sum += inv_sigmoid(first ? r : (r + 0.5f) / 2.f);
                    }
                    v = sum / (float)(P.R / 2);
                }
            }
            refoff[row][coord] = v;
        }
        __syncthreads();
    }

    const int wave = tid >> 6, lane = tid & 63;
    const int i0 = (wave >> 1) * 32, g = lane >> 5, j = n0 + (wave & 1) * 32 + (lane & 31);
    if (j >= p.n) return;
    int gi = p.g0;
    while (gi + 1 < p.g0 + p.ng && j >= P.g[gi + 1].off) ++gi;
    const HeadsFwdGroup &G = P.g[gi];
    const int jj = j - G.off;
    const float bj = G.b[jj];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int m = m0 + i0 + acc_row(r, g);
        if (m >= p.rows) continue;
        const long long gr = (long long)p.row0 + m;
        float v = acc[r] + bj;
        if (p.epi == kHeadsEpiRelu) {
            v = fmaxf(v, 0.f);
        } else if (p.epi == kHeadsEpiArctic) {
            // (delta + inverse_sigmoid(reference)).sigmoid() * 2 - 1   (models/actic_detr.py:250-258)
            const float *ref = gr < P.M ? P.init_ref + gr * P.R : P.inter_ref + (gr - P.M) * P.R;
            const float s = 1.f / (1.f + expf(-(v + inv_sigmoid(ref[jj]))));
            p.sig[gr * G.n + jj] = s;
            v = s * 2.f - 1.f;
        } else if (p.epi == kHeadsEpiAssembly) {
            const int coord = jj % 3;
            if (coord < 2) v += refoff[i0 + acc_row(r, g)][coord];
            const float s = 1.f / (1.f + expf(-v));
            p.sig[gr * G.n + jj] = s;
            v = s * 2.f - 0.5f;
        }
        G.out[gr * G.n + jj] = v;
    }
}

// ---- input gradients: dx [rows, C] = sum over segments (dy o mode) . W -------------------------------------------------
__global__ __launch_bounds__(kHBlock) void heads_dgrad_kernel(HeadsDgradArgs P)
{
    __shared__ __attribute__((aligned(16))) float As[2][kLds];
    __shared__ __attribute__((aligned(16))) float Bs[2][kLds];
    int pi = 0;
    while (pi + 1 < P.nprob && (int)blockIdx.x >= P.p[pi + 1].tile0) ++pi;
    const HeadsDgradProb &p = P.p[pi];
    const int C = P.C, tiles_n = (C + kHT - 1) / kHT;
    const int local = (int)blockIdx.x - p.tile0;
    if (local >= ((p.rows + kHT - 1) / kHT) * tiles_n) return;
    const int m0 = (local / tiles_n) * kHT, n0 = (local % tiles_n) * kHT, tid = threadIdx.x;
    int nstages = 0;
    for (int s = p.s0; s < p.s0 + p.ns; ++s) nstages += (P.s[s].k + kHS - 1) / kHS;
    // stage -> (segment, k0): the cursor only moves forward, one stage per call
    int cseg = p.s0, ck0 = 0, cstage = 0;
    auto load = [&](int s, float (&ra)[8], float (&rb)[8]) {
        while (cstage < s) {
            ck0 += kHS;
            if (ck0 >= P.s[cseg].k) { ++cseg; ck0 = 0; }
            ++cstage;
        }
        const HeadsDgradSeg &S = P.s[cseg];
        // A = dy o mode [row, k]: 4-byte K-major
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int m = m0 + tid / 32 + 8 * u, k = ck0 + tid % 32;
            float v = 0.f;
            if (m < p.rows && k < S.k) {
                const long long e = ((long long)p.row0 + m) * S.k + k;
                v = apply_mode(S.a[e], S.aux, e, S.mode);
            }
            ra[u] = v;
        }
        // B = W [k, C]: 16-byte MN-major
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int k = ck0 + tid / 16 + 16 * u, jn = n0 + (tid % 16) * 4;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (k < S.k && jn < C) v = *reinterpret_cast<const float4 *>(S.w + (long long)k * C + jn);
            rb[4 * u] = v.x; rb[4 * u + 1] = v.y; rb[4 * u + 2] = v.z; rb[4 * u + 3] = v.w;
        }
    };
    const f32x16 acc = tile_loop<true, false, false, true>(As, Bs, nstages, load, NoStage());
    const int wave = tid >> 6, lane = tid & 63;
    const int i0 = (wave >> 1) * 32, g = lane >> 5, j = n0 + (wave & 1) * 32 + (lane & 31);
    if (j >= C) return;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int m = m0 + i0 + acc_row(r, g);
        if (m < p.rows) p.out[((long long)p.row0 + m) * C + j] = acc[r];
    }
}

// ---- weight gradients, per row chunk: part[chunk] [n, C] = (dy o mode)^T . x, bpart[chunk] [n] = column sums of dy o mode --
__global__ __launch_bounds__(kHBlock) void heads_wgrad_kernel(HeadsWgradArgs P)
{
    __shared__ __attribute__((aligned(16))) float As[2][kLds];
    __shared__ __attribute__((aligned(16))) float Bs[2][kLds];
    __shared__ float bred[4][kHT];
    int pi = 0;
    while (pi + 1 < P.nprob && (int)blockIdx.x >= P.p[pi + 1].tile0) ++pi;
    const HeadsWgradProb &p = P.p[pi];
    const int C = P.C, tiles_j = (C + kHT - 1) / kHT, tiles_i = (p.n + kHT - 1) / kHT;
    const int local = (int)blockIdx.x - p.tile0;
    if (local >= p.chunks * tiles_i * tiles_j) return;
    const int chunk = local / (tiles_i * tiles_j), rem = local % (tiles_i * tiles_j);
    const int i0t = (rem / tiles_j) * kHT, j0t = (rem % tiles_j) * kHT, tid = threadIdx.x;
    const int r0 = chunk * kHeadsWgradChunk;
    const int nrows = min(kHeadsWgradChunk, p.rows - r0);
    const long long base = (long long)p.row0 + r0;
    auto load = [&](int s, float (&ra)[8], float (&rb)[8]) {
        // A(i, m) = (dy o mode)[m, i]: 4-byte MN-major
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int m = s * kHS + tid / 64 + 4 * u, i = i0t + tid % 64;
            float v = 0.f;
            if (m < nrows && i < p.n) {
                const long long e = (base + m) * p.n + i;
                v = apply_mode(p.dy[e], p.aux, e, p.mode);
            }
            ra[u] = v;
        }
        // B(m, j) = x[m, j]: 16-byte MN-major
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int m = s * kHS + tid / 16 + 16 * u, jn = j0t + (tid % 16) * 4;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (m < nrows && jn < C) v = *reinterpret_cast<const float4 *>(p.x + (base + m) * C + jn);
            rb[4 * u] = v.x; rb[4 * u + 1] = v.y; rb[4 * u + 2] = v.z; rb[4 * u + 3] = v.w;
        }
    };
    // bias: the column tile 0 workgroups also sum their staged dy o mode, thread (q, i) over 8 rows of each stage
    float bsum = 0.f;
    const bool with_bias = j0t == 0;
    auto per_stage = [&](const float *S) {
        if (with_bias) {
            const int i = tid & 63, q = tid >> 6;
#pragma unroll
            for (int u = 0; u < 8; ++u) bsum += S[(8 * q + u) * kRowN + i];
        }
    };
    const f32x16 acc = tile_loop<false, false, false, true>(As, Bs, (nrows + kHS - 1) / kHS, load, per_stage);
    float *part = P.ws + p.part;
    if (with_bias) {                                                            // uniform per workgroup
        bred[tid >> 6][tid & 63] = bsum;
        __syncthreads();
        if (tid < kHT && i0t + tid < p.n)
            part[(long long)p.chunks * p.n * C + (long long)chunk * p.n + i0t + tid] =
                ((bred[0][tid] + bred[1][tid]) + bred[2][tid]) + bred[3][tid];
    }
    const int wave = tid >> 6, lane = tid & 63;
    const int i0 = (wave >> 1) * 32, g = lane >> 5, j = j0t + (wave & 1) * 32 + (lane & 31);
    if (j >= C) return;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int i = i0t + i0 + acc_row(r, g);
        if (i < p.n) part[((long long)chunk * p.n + i) * C + j] = acc[r];
    }
}

// ---- dW = sum of the chunk partials in chunk order; db likewise ------------------------------------------------------------
__global__ __launch_bounds__(kHBlock) void heads_reduce_kernel(HeadsReduceArgs P)
{
    int pi = 0;
    while (pi + 1 < P.nprob && (int)blockIdx.x >= P.p[pi + 1].blk0) ++pi;
    const HeadsReduceProb &p = P.p[pi];
    const long long nw = (long long)p.n * P.C;
    const long long e = (long long)((int)blockIdx.x - p.blk0) * kHBlock + threadIdx.x;
    if (e >= nw + p.n) return;
    const float *part = P.ws + p.part;
    float s = 0.f;
    if (e < nw) {
        for (int c = 0; c < p.chunks; ++c) s += part[c * nw + e];
        p.dw[e] = s;
    } else {
        const long long i = e - nw;
        for (int c = 0; c < p.chunks; ++c) s += part[p.chunks * nw + (long long)c * p.n + i];
        p.db[i] = s;
    }
}

}  // namespace

int launch_heads_forward(const HeadsFwdArgs &a, int tiles, hipStream_t stream)
{
    if (tiles == 0) return MSDA_OK;
    hipLaunchKernelGGL(heads_fwd_kernel, dim3((unsigned)tiles), dim3(kHBlock), 0, stream, a);
    return check_launch("heads_fwd_kernel");
}

int launch_heads_dgrad(const HeadsDgradArgs &a, int tiles, hipStream_t stream)
{
    if (tiles == 0) return MSDA_OK;
    hipLaunchKernelGGL(heads_dgrad_kernel, dim3((unsigned)tiles), dim3(kHBlock), 0, stream, a);
    return check_launch("heads_dgrad_kernel");
}

int launch_heads_wgrad(const HeadsWgradArgs &a, int tiles, hipStream_t stream)
{
    if (tiles == 0) return MSDA_OK;
    hipLaunchKernelGGL(heads_wgrad_kernel, dim3((unsigned)tiles), dim3(kHBlock), 0, stream, a);
    return check_launch("heads_wgrad_kernel");
}

int launch_heads_reduce(const HeadsReduceArgs &a, int blocks, hipStream_t stream)
{
    if (blocks == 0) return MSDA_OK;
    hipLaunchKernelGGL(heads_reduce_kernel, dim3((unsigned)blocks), dim3(kHBlock), 0, stream, a);
    return check_launch("heads_reduce_kernel");
}

// ---- host side: argument checks and problem tables ----------------------------------------------------------------------
static const int kSharedN[kHeadsShared] = {48, 10, 3, 3, 3, 1};   // mano pose, mano beta, hand cam, obj cam, obj rot, obj rad

static int heads_D(int kind) { return kind == MSDA_HEADS_ARCTIC ? 42 : 63; }
static int tiles_of(long long rows, int n) { return (int)(((rows + kHT - 1) / kHT) * ((n + kHT - 1) / kHT)); }
static int chunks_of(long long rows) { return (int)((rows + kHeadsWgradChunk - 1) / kHeadsWgradChunk); }

static int herr(const char *msg) { return set_error(MSDA_ERR_ARGUMENT, msg); }

int heads_check(const HeadsCall &c, bool backward)
{
    if (c.kind != MSDA_HEADS_ARCTIC && c.kind != MSDA_HEADS_ASSEMBLY)
        return herr("msda_heads: kind must be 0 (ARCTIC) or 1 (AssemblyHands)");
    if (c.L < 1 || c.L > kHeadsMaxLevels) return herr("msda_heads: need 1 <= L <= 8 levels");
    if (c.M < 1 || c.K < 1 || c.C < 4 || c.C > 4096 || c.C % 4 != 0)
        return herr("msda_heads: need M >= 1, K >= 1 and a hidden size C with C % 4 == 0, 4 <= C <= 4096");
    if ((c.flags & ~(unsigned)(MSDA_HEADS_SHARED_CLS | MSDA_HEADS_SHARED_MLP)) != 0) return herr("msda_heads: unknown flags");
    if (c.kind == MSDA_HEADS_ARCTIC ? (c.n_mlp != 0 && c.n_mlp != 2) : c.n_mlp != 1)
        return herr("msda_heads: n_mlp must be 0 or 2 (ARCTIC) or 1 (AssemblyHands)");
    if (c.n_mlp > 0 && !(c.kind == MSDA_HEADS_ARCTIC ? c.R == 42 : (c.R == 2 || c.R == 42)))
        return herr("msda_heads: reference width R must be 42 (ARCTIC) or 2 / 42 (AssemblyHands)");
    const long long LM = (long long)c.L * c.M;
    const int widest = c.C > c.K ? c.C : c.K;
    if (LM * widest >= (1LL << 31) || LM * (c.n_mlp > 0 ? c.R : 1) >= (1LL << 31))
        return herr("msda_heads: tensors beyond 2^31 elements");
    const int Lc = (c.flags & MSDA_HEADS_SHARED_CLS) ? 1 : c.L, Lw = (c.flags & MSDA_HEADS_SHARED_MLP) ? 1 : c.L;
    const bool arctic_shared = c.kind == MSDA_HEADS_ARCTIC;
    if (c.hs == nullptr || c.cls_w == nullptr || c.cls_b == nullptr) return herr("msda_heads: null pointer");
    for (int l = 0; l < Lc; ++l)
        if (c.cls_w[l] == nullptr || c.cls_b[l] == nullptr) return herr("msda_heads: null pointer");
    if (c.n_mlp > 0) {
        if (c.init_ref == nullptr || (c.L > 1 && c.inter_ref == nullptr) || c.mlp_w == nullptr || c.mlp_b == nullptr)
            return herr("msda_heads: null pointer");
        for (int i = 0; i < c.n_mlp * 3 * Lw; ++i)
            if (c.mlp_w[i] == nullptr || c.mlp_b[i] == nullptr) return herr("msda_heads: null pointer");
    }
    if (arctic_shared) {
        if (c.shared_w == nullptr || c.shared_b == nullptr) return herr("msda_heads: null pointer");
        for (int g = 0; g < kHeadsShared; ++g)
            if (c.shared_w[g] == nullptr || c.shared_b[g] == nullptr) return herr("msda_heads: null pointer");
    }
    if (c.n_mlp > 0 && (c.hidden == nullptr || c.sig == nullptr)) return herr("msda_heads: null pointer");
    if (!backward) {
        if (c.logits == nullptr || (c.n_mlp > 0 && c.kp_out == nullptr) || (arctic_shared && c.shared_out == nullptr))
            return herr("msda_heads: null pointer");
        for (int h = 0; h < c.n_mlp; ++h)
            if (c.kp_out[h] == nullptr) return herr("msda_heads: null pointer");
        for (int g = 0; arctic_shared && g < kHeadsShared; ++g)
            if (c.shared_out[g] == nullptr) return herr("msda_heads: null pointer");
        return MSDA_OK;
    }
    if (c.grad_logits == nullptr || c.grad_hs == nullptr || c.grad_cls_w == nullptr || c.grad_cls_b == nullptr
        || (c.n_mlp > 0 && (c.grad_kp == nullptr || c.grad_mlp_w == nullptr || c.grad_mlp_b == nullptr))
        || (arctic_shared && (c.grad_shared == nullptr || c.grad_shared_w == nullptr || c.grad_shared_b == nullptr)))
        return herr("msda_heads: null pointer");
    for (int l = 0; l < Lc; ++l)
        if (c.grad_cls_w[l] == nullptr || c.grad_cls_b[l] == nullptr) return herr("msda_heads: null pointer");
    for (int h = 0; h < c.n_mlp; ++h)
        if (c.grad_kp[h] == nullptr) return herr("msda_heads: null pointer");
    for (int i = 0; i < c.n_mlp * 3 * Lw; ++i)
        if (c.grad_mlp_w[i] == nullptr || c.grad_mlp_b[i] == nullptr) return herr("msda_heads: null pointer");
    for (int g = 0; arctic_shared && g < kHeadsShared; ++g)
        if (c.grad_shared[g] == nullptr || c.grad_shared_w[g] == nullptr || c.grad_shared_b[g] == nullptr)
            return herr("msda_heads: null pointer");
    if (c.ws == nullptr && c.ws_bytes > 0) return herr("msda_heads: null pointer");
    if (c.ws_bytes < heads_workspace_bytes(c.kind, c.L, c.M, c.C, c.K, c.n_mlp, c.flags))
        return herr("msda_heads: workspace smaller than msda_heads_workspace_bytes");
    return MSDA_OK;
}

// The weight problems of the backward, in one fixed order (the workspace layout follows it): class head(s), MLP layers
// (head, layer, level), the six shared Linears.  `emit(dy, aux, x, row0, rows, n, mode, dw, db)`.
template <class Emit>
static void heads_weight_problems(const HeadsCall &c, Emit emit)
{
    const long long LM = (long long)c.L * c.M;
    const int M = (int)c.M, C = c.C, D = heads_D(c.kind);
    const bool shc = (c.flags & MSDA_HEADS_SHARED_CLS) != 0, shm = (c.flags & MSDA_HEADS_SHARED_MLP) != 0;
    const int Lc = shc ? 1 : c.L, Lw = shm ? 1 : c.L;
    for (int l = 0; l < Lc; ++l)
        emit(c.grad_logits, (const float *)nullptr, c.hs, shc ? 0 : l * M, shc ? (int)LM : M, c.K, kHeadsModePlain,
             c.grad_cls_w ? c.grad_cls_w[l] : nullptr, c.grad_cls_b ? c.grad_cls_b[l] : nullptr);
    const float *dH = static_cast<const float *>(c.ws);                 // [n_mlp][2][LM][C]: dH1, dH2
    for (int h = 0; h < c.n_mlp; ++h)
        for (int layer = 0; layer < 3; ++layer)
            for (int l = 0; l < Lw; ++l) {
                const int wi = (h * 3 + layer) * Lw + l;
                const float *H1 = c.hidden + (long long)(h * 2) * LM * C, *H2 = H1 + LM * C;
                const float *dH1 = dH ? dH + (long long)(h * 2) * LM * C : nullptr, *dH2 = dH ? dH1 + LM * C : nullptr;
                const float *dy = layer == 0 ? dH1 : layer == 1 ? dH2 : (c.grad_kp ? c.grad_kp[h] : nullptr);
                const float *aux = layer == 0 ? H1 : layer == 1 ? H2 : c.sig + (long long)h * LM * D;
                const float *x = layer == 0 ? c.hs : layer == 1 ? H1 : H2;
                emit(dy, aux, x, shm ? 0 : l * M, shm ? (int)LM : M, layer == 2 ? D : C,
                     layer == 2 ? kHeadsModeSigmoid : kHeadsModeRelu, c.grad_mlp_w ? c.grad_mlp_w[wi] : nullptr,
                     c.grad_mlp_b ? c.grad_mlp_b[wi] : nullptr);
            }
    if (c.kind == MSDA_HEADS_ARCTIC)
        for (int g = 0; g < kHeadsShared; ++g)
            emit(c.grad_shared ? c.grad_shared[g] : nullptr, (const float *)nullptr, c.hs, 0, (int)LM, kSharedN[g],
                 kHeadsModePlain, c.grad_shared_w ? c.grad_shared_w[g] : nullptr,
                 c.grad_shared_b ? c.grad_shared_b[g] : nullptr);
}

unsigned long long heads_workspace_bytes(int kind, int L, long long M, int C, int K, int n_mlp, unsigned flags)
{
    HeadsCall c = {};
    c.kind = kind; c.L = L; c.M = M; c.C = C; c.K = K; c.n_mlp = n_mlp; c.flags = flags;
    const long long LM = (long long)L * M;
    unsigned long long floats = (unsigned long long)n_mlp * 2 * LM * C;
    heads_weight_problems(c, [&](const float *, const float *, const float *, int, int rows, int n, int, float *, float *) {
        floats += (unsigned long long)chunks_of(rows) * n * (C + 1);
    });
    return floats * sizeof(float);
}

int heads_plan_forward(const HeadsCall &c, HeadsFwdPlan &plan)
{
    int rc = heads_check(c, false);
    if (rc != MSDA_OK) return rc;
    std::memset(&plan, 0, sizeof(plan));
    const long long LM = (long long)c.L * c.M;
    const int M = (int)c.M, C = c.C, D = heads_D(c.kind);
    const bool shc = (c.flags & MSDA_HEADS_SHARED_CLS) != 0, shm = (c.flags & MSDA_HEADS_SHARED_MLP) != 0;
    const int Lw = shm ? 1 : c.L;
    for (int d = 0; d < 3; ++d) {
        HeadsFwdArgs &a = plan.a[d];
        a.init_ref = c.init_ref;
        a.inter_ref = c.inter_ref;
        a.M = M;
        a.C = C;
        a.R = c.R;
        int ng = 0, tiles = 0;
        auto add = [&](const float *x, int row0, int rows, int epi, float *sig) -> HeadsFwdProb & {
            HeadsFwdProb &p = a.p[a.nprob++];
            p.a = x; p.sig = sig; p.row0 = row0; p.rows = rows; p.epi = epi; p.g0 = ng; p.ng = 0; p.n = 0; p.tile0 = tiles;
            return p;
        };
        auto group = [&](HeadsFwdProb &p, const float *w, const float *b, float *out, int n) {
            HeadsFwdGroup &g = a.g[ng++];
            g.w = w; g.b = b; g.out = out; g.n = n; g.off = p.n;
            p.n += n;
            ++p.ng;
        };
        for (int l = 0; l < c.L; ++l) {
            if (d == 0) {
                HeadsFwdProb &p = add(c.hs, l * M, M, kHeadsEpiBias, nullptr);
                group(p, c.cls_w[shc ? 0 : l], c.cls_b[shc ? 0 : l], c.logits, c.K);
                tiles += tiles_of(M, p.n);
            }
            for (int h = 0; h < c.n_mlp; ++h) {
                const int wi = (h * 3 + d) * Lw + (shm ? 0 : l);
                float *H1 = c.hidden + (long long)(h * 2) * LM * C, *H2 = H1 + LM * C;
                const float *x = d == 0 ? c.hs : d == 1 ? H1 : H2;
                float *out = d == 0 ? H1 : d == 1 ? H2 : c.kp_out[h];
                const int epi = d < 2 ? kHeadsEpiRelu : c.kind == MSDA_HEADS_ARCTIC ? kHeadsEpiArctic : kHeadsEpiAssembly;
                HeadsFwdProb &p = add(x, l * M, M, epi, d == 2 ? c.sig + (long long)h * LM * D : nullptr);
                group(p, c.mlp_w[wi], c.mlp_b[wi], out, d < 2 ? C : D);
                tiles += tiles_of(M, p.n);
            }
        }
        if (d == 0 && c.kind == MSDA_HEADS_ARCTIC) {                    // the six shared Linears: ONE problem over L * M rows
            HeadsFwdProb &p = add(c.hs, 0, (int)LM, kHeadsEpiBias, nullptr);
            for (int g = 0; g < kHeadsShared; ++g) group(p, c.shared_w[g], c.shared_b[g], c.shared_out[g], kSharedN[g]);
            tiles += tiles_of(LM, p.n);
        }
        plan.tiles[d] = tiles;
    }
    return MSDA_OK;
}

int heads_plan_backward(const HeadsCall &c, HeadsBwdPlan &plan)
{
    int rc = heads_check(c, true);
    if (rc != MSDA_OK) return rc;
    std::memset(&plan, 0, sizeof(plan));
    const long long LM = (long long)c.L * c.M;
    const int M = (int)c.M, C = c.C, D = heads_D(c.kind);
    const bool shc = (c.flags & MSDA_HEADS_SHARED_CLS) != 0, shm = (c.flags & MSDA_HEADS_SHARED_MLP) != 0;
    const int Lw = shm ? 1 : c.L;
    float *dH = static_cast<float *>(c.ws);
    // input gradients: d[0] depth 3 -> dH2, d[1] depth 2 -> dH1, d[2] depth 1 -> grad_hs
    for (int step = 0; step < 3; ++step) {
        HeadsDgradArgs &a = plan.d[step];
        a.C = C;
        int ns = 0, tiles = 0;
        for (int l = 0; l < c.L; ++l) {
            auto seg = [&](const float *x, const float *aux, const float *w, int k, int mode) {
                HeadsDgradSeg &s = a.s[ns++];
                s.a = x; s.aux = aux; s.w = w; s.k = k; s.mode = mode;
            };
            auto prob = [&](float *out, int s0) {
                HeadsDgradProb &p = a.p[a.nprob++];
                p.out = out; p.row0 = l * M; p.rows = M; p.s0 = s0; p.ns = ns - s0; p.tile0 = tiles;
                tiles += tiles_of(M, C);
            };
            if (step < 2) {
                for (int h = 0; h < c.n_mlp; ++h) {
                    const float *H1 = c.hidden + (long long)(h * 2) * LM * C, *H2 = H1 + LM * C;
                    float *dH1 = dH + (long long)(h * 2) * LM * C, *dH2 = dH1 + LM * C;
                    const int layer = 2 - step, wi = (h * 3 + layer) * Lw + (shm ? 0 : l);
                    const int s0 = ns;
                    if (step == 0) seg(c.grad_kp[h], c.sig + (long long)h * LM * D, c.mlp_w[wi], D, kHeadsModeSigmoid);
                    else seg(dH2, H2, c.mlp_w[wi], C, kHeadsModeRelu);
                    prob(step == 0 ? dH2 : dH1, s0);
                }
            } else {
                const int s0 = ns;
                seg(c.grad_logits, nullptr, c.cls_w[shc ? 0 : l], c.K, kHeadsModePlain);
                for (int h = 0; h < c.n_mlp; ++h) {
                    const float *H1 = c.hidden + (long long)(h * 2) * LM * C;
                    seg(dH + (long long)(h * 2) * LM * C, H1, c.mlp_w[(h * 3) * Lw + (shm ? 0 : l)], C, kHeadsModeRelu);
                }
                if (c.kind == MSDA_HEADS_ARCTIC)
                    for (int g = 0; g < kHeadsShared; ++g) seg(c.grad_shared[g], nullptr, c.shared_w[g], kSharedN[g], kHeadsModePlain);
                prob(c.grad_hs, s0);
            }
        }
        plan.dtiles[step] = tiles;
    }
    // weight gradients: partials per chunk, then the chunk-ordered sums
    long long off = (long long)c.n_mlp * 2 * LM * C;
    plan.w.ws = dH;
    plan.w.C = C;
    plan.r.ws = dH;
    plan.r.C = C;
    int wt = 0, rb = 0;
    heads_weight_problems(c, [&](const float *dy, const float *aux, const float *x, int row0, int rows, int n, int mode, float *dw,
                                 float *db) {
        HeadsWgradProb &p = plan.w.p[plan.w.nprob++];
        p.dy = dy; p.aux = aux; p.x = x; p.part = off; p.row0 = row0; p.rows = rows; p.n = n; p.mode = mode;
        p.chunks = chunks_of(rows); p.tile0 = wt;
        wt += p.chunks * ((n + kHT - 1) / kHT) * ((C + kHT - 1) / kHT);
        HeadsReduceProb &r = plan.r.p[plan.r.nprob++];
        r.part = off; r.dw = dw; r.db = db; r.n = n; r.chunks = p.chunks; r.blk0 = rb;
        rb += (int)(((long long)n * (C + 1) + kHBlock - 1) / kHBlock);
        off += (long long)p.chunks * n * (C + 1);
    });
    plan.wtiles = wt;
    plan.rblocks = rb;
    return MSDA_OK;
}

int heads_run_forward(const HeadsFwdPlan &plan, hipStream_t stream)
{
    for (int d = 0; d < 3; ++d) {
        const int rc = launch_heads_forward(plan.a[d], plan.tiles[d], stream);
        if (rc != MSDA_OK) return rc;
    }
    return MSDA_OK;
}

int heads_run_backward(const HeadsBwdPlan &plan, hipStream_t stream)
{
    for (int s = 0; s < 3; ++s) {
        const int rc = launch_heads_dgrad(plan.d[s], plan.dtiles[s], stream);
        if (rc != MSDA_OK) return rc;
    }
    int rc = launch_heads_wgrad(plan.w, plan.wtiles, stream);
    if (rc != MSDA_OK) return rc;
    return launch_heads_reduce(plan.r, plan.rblocks, stream);
}

}  // namespace msda
