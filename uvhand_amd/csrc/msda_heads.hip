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
//   wgrad     partial dW[chunk] = (dy o mode)^T . x  over row chunks of kHeadsWgradChunk rows, the bias column sums beside them;
//             a chunk's rows are summed 32 at a time (one stage of the tile loop) from zero and the stage sums added to a
//             second accumulator, and the bias column sums are kept in fp64 until the chunk's one rounding: these are sums
//             over hundreds of rows whose terms cancel, and one running fp32 sum missed the fp64 rule there (DESIGN.md §4.32,
//             "The weight gradient's summation order")
//   reduce    dW = sum over chunks, in chunk order
//
// Kernel: fp32 MFMA (v_mfma_f32_32x32x2_f32), 64 x 64 output tile per 256-thread workgroup, 2 x 2 wavefronts of 32 x 32,
// reduction in stages of 32 through double-buffered LDS (one barrier per stage, next stage's global loads in flight during
// the MFMAs), the lane / register layout of msda_gemm.hip.  An operand is staged K-major ([64][32 + 4]) or MN-major
// ([32][64 + 4]) as it lies in memory; 16-byte loads where rows are C floats long (C % 4 == 0), 4-byte loads where they are
// a head's width (14, 42, 63 ...).  Fixed summation order everywhere: bitwise reproducible.
//
// The host side below is the planner of BOTH forms, this one and the bf16-autocast one (kernels: msda_heads_bf16.hip): one
// argument check, one enumeration of the problems, one workspace layout, one set of tables (msda_launch.h) whose dtype flags
// come from a form's description (Form); heads_run_* launch a plan on its form's kernels.  The fp32 kernels here read the
// same tables and ignore the flags.
#include <cstdio>
#include <cstring>

#include "msda_heads_common.h"

namespace msda {

namespace {

#include "msda_tile.h"
static_assert(kHBlock == kHeadsReduceBlock && kHT == kHeadsTile, "what the planner counts workgroups with");

// this form's operands are all fp32: the tables' dtype flags are not read
__device__ __forceinline__ const float *f32(const void *p) { return static_cast<const float *>(p); }
__device__ __forceinline__ float *f32(void *p) { return static_cast<float *>(p); }

__device__ __forceinline__ float apply_mode(float a, const void *aux, long long e, int mode)
{
    if (mode == kHeadsModeSigmoid) {
        const float s = f32(aux)[e];
        return (a * 2.f) * (1.f - s) * s;                   // MulBackward (out = 2 s - c), then sigmoid_backward
    }
    if (mode == kHeadsModeRelu) return f32(aux)[e] > 0.f ? a : 0.f;
    return a;
}

// ---- forward: y = x . W^T + b, one launch per depth ---------------------------------------------------------------------
__global__ __launch_bounds__(kHBlock) void heads_fwd_kernel(HeadsFwdArgs P)
{
    __shared__ __attribute__((aligned(16))) float As[2][kLds];
    __shared__ __attribute__((aligned(16))) float Bs[2][kLds];
    __shared__ float refoff[kHT][2];
    const HeadsFwdProb &p = P.p[heads_problem(P)];
    const int tiles_n = (p.n + kHT - 1) / kHT;
    const int local = (int)blockIdx.x - p.tile0;
    if (local >= ((p.rows + kHT - 1) / kHT) * tiles_n) return;
    const int m0 = (local / tiles_n) * kHT, n0 = (local % tiles_n) * kHT;
    const int C = P.C, tid = threadIdx.x;
    const float *A = f32(p.a) + (long long)p.row0 * C;

    auto load = [&](int s, float (&ra)[8], float (&rb)[8]) {
        const int k = s * kHS + (tid % 8) * 4;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int m = m0 + tid / 8 + 32 * u, j = n0 + tid / 8 + 32 * u;
            float4 va = make_float4(0.f, 0.f, 0.f, 0.f), vb = va;
            if (m < p.rows && k < C) va = *reinterpret_cast<const float4 *>(A + (long long)m * C + k);
            if (j < p.n && k < C) {
                const HeadsFwdGroup &G = P.g[heads_group(P, p, j)];
                vb = *reinterpret_cast<const float4 *>(G.w + (long long)(j - G.off) * C + k);
            }
            ra[4 * u] = va.x; ra[4 * u + 1] = va.y; ra[4 * u + 2] = va.z; ra[4 * u + 3] = va.w;
            rb[4 * u] = vb.x; rb[4 * u + 1] = vb.y; rb[4 * u + 2] = vb.z; rb[4 * u + 3] = vb.w;
        }
    };
    const f32x16 acc = tile_loop<true, true, true, true>(As, Bs, (C + kHS - 1) / kHS, load, NoStage());

    if (p.epi == kHeadsEpiAssembly) heads_refoff(P, p, m0, refoff);

    const int wave = tid >> 6, lane = tid & 63;
    const int i0 = (wave >> 1) * 32, g = lane >> 5, j = n0 + (wave & 1) * 32 + (lane & 31);
    if (j >= p.n) return;
    const HeadsFwdGroup &G = P.g[heads_group(P, p, j)];
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
        f32(G.out)[gr * G.n + jj] = v;
    }
}

// ---- input gradients: dx [rows, C] = sum over segments (dy o mode) . W -------------------------------------------------
__global__ __launch_bounds__(kHBlock) void heads_dgrad_kernel(HeadsDgradArgs P)
{
    __shared__ __attribute__((aligned(16))) float As[2][kLds];
    __shared__ __attribute__((aligned(16))) float Bs[2][kLds];
    const HeadsDgradProb &p = P.p[heads_problem(P)];
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
                v = apply_mode(f32(S.a)[e], S.aux, e, S.mode);
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
        if (m < p.rows) f32(p.out)[((long long)p.row0 + m) * C + j] = acc[r];
    }
}

// ---- weight gradients, per row chunk: part[chunk] [n, C] = (dy o mode)^T . x, bpart[chunk] [n] = column sums of dy o mode --
__global__ __launch_bounds__(kHBlock) void heads_wgrad_kernel(HeadsWgradArgs P)
{
    __shared__ __attribute__((aligned(16))) float As[2][kLds];
    __shared__ __attribute__((aligned(16))) float Bs[2][kLds];
    __shared__ double bred[4][kHT];
    const HeadsWgradProb &p = P.p[heads_problem(P)];
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
                v = apply_mode(f32(p.dy)[e], p.aux, e, p.mode);
            }
            ra[u] = v;
        }
        // B(m, j) = x[m, j]: 16-byte MN-major
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int m = s * kHS + tid / 16 + 16 * u, jn = j0t + (tid % 16) * 4;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (m < nrows && jn < C) v = *reinterpret_cast<const float4 *>(f32(p.x) + (base + m) * C + jn);
            rb[4 * u] = v.x; rb[4 * u + 1] = v.y; rb[4 * u + 2] = v.z; rb[4 * u + 3] = v.w;
        }
    };
    // bias: the column tile 0 workgroups also sum their staged dy o mode, thread (q, i) over 8 rows of each stage; in fp64, so
    // that a chunk's column sum is rounded once (a bias gradient is often a single element whose terms cancel)
    double bsum = 0.0;
    const bool with_bias = j0t == 0;
    auto per_stage = [&](const float *S) {
        if (with_bias) {
            const int i = tid & 63, q = tid >> 6;
#pragma unroll
            for (int u = 0; u < 8; ++u) bsum += S[(8 * q + u) * kRowN + i];
        }
    };
    // the rows are summed stage by stage (32 rows) and the stage sums added up: see tile_loop_impl
    const f32x16 acc = tile_loop_impl<false, false, false, true, true>(As, Bs, (nrows + kHS - 1) / kHS, load, per_stage);
    float *part = P.ws + p.part;
    if (with_bias) {                                                            // uniform per workgroup
        bred[tid >> 6][tid & 63] = bsum;
        __syncthreads();
        if (tid < kHT && i0t + tid < p.n)
            part[(long long)p.chunks * p.n * C + (long long)chunk * p.n + i0t + tid] =
                (float)(((bred[0][tid] + bred[1][tid]) + bred[2][tid]) + bred[3][tid]);
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
    const HeadsReduceProb &p = P.p[heads_problem(P)];
    const long long nw = (long long)p.n * P.C;
    const long long e = (long long)((int)blockIdx.x - p.tile0) * kHBlock + threadIdx.x;
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

// ---- reference gradient of the ARCTIC keypoint epilogue (DINO: models/dino/dino.py:333-334 with references that carry a gradient)
// The flat space is that of the stacked tensors, [L * M * R] with R = D = 42: level 0 reads init_ref, levels >= 1 inter_ref.
// A thread moves groups of W consecutive elements, [e0 + W * i, e0 + W * (i + 1)); the host picks W from the flat element index
// (M * R and every base are multiples of W), so no group crosses from init_ref into inter_ref and every access is W * 4 bytes.
// Per element: the two heads' depth-3 operands in apply_mode's order and grouping, summed head 0 then head 1, times what
// autograd makes of inverse_sigmoid's three clamps and its log (torch's clamp passes the gradient at its bounds).
__device__ __forceinline__ float ref_dinv(float x)
{
    const float eps = 1e-5f, y = 1.f - x;
    const float d = (x >= eps ? 1.f / fmaxf(x, eps) : 0.f) + (y >= eps ? 1.f / fmaxf(y, eps) : 0.f);
    return x >= 0.f && x <= 1.f ? d : 0.f;
}

template <int W>
__global__ __launch_bounds__(kHBlock) void heads_ref_bwd_kernel(HeadsRefBwdArgs P)
{
#pragma clang fp contract(off)     // every width rounds each product and sum on its own: the same bits whichever width serves a call
    struct __attribute__((aligned(W * 4))) Vec { float v[W]; };
    const long long stride = (long long)gridDim.x * kHBlock;
    for (long long i = (long long)blockIdx.x * kHBlock + threadIdx.x; i < P.groups; i += stride) {
        const long long e = P.e0 + i * W;
        const bool first = e < P.MR;
        const Vec x = *reinterpret_cast<const Vec *>(first ? P.init_ref + e : P.inter_ref + (e - P.MR));
        const Vec g0 = *reinterpret_cast<const Vec *>(P.grad_kp[0] + e), g1 = *reinterpret_cast<const Vec *>(P.grad_kp[1] + e);
        const Vec s0 = *reinterpret_cast<const Vec *>(P.sig + e), s1 = *reinterpret_cast<const Vec *>(P.sig + P.LMR + e);
        Vec out;
#pragma unroll
        for (int u = 0; u < W; ++u) {
            // each head's term rounded as the depth-3 operand is, then one rounded add
            const float t = (g0.v[u] * 2.f) * (1.f - s0.v[u]) * s0.v[u] + (g1.v[u] * 2.f) * (1.f - s1.v[u]) * s1.v[u];
            const float d = ref_dinv(x.v[u]);
            out.v[u] = d != 0.f ? d * t : 0.f;                  // outside [0, 1]: exactly zero, whatever t holds
        }
        *reinterpret_cast<Vec *>(first ? P.grad_init_ref + e : P.grad_inter_ref + (e - P.MR)) = out;
    }
}

// ---- host side, both forms: argument checks, problem tables, workspace layout ----------------------------------------------
const int kSharedN[kHeadsShared] = {48, 10, 3, 3, 3, 1};   // mano pose, mano beta, hand cam, obj cam, obj rot, obj rad

// What a form is, beyond the operands that are fp32 in both (hs, weights, references, sig, parameter gradients): nothing else
// may differ between the forms.
struct Form {
    int hidden_bf16;            // hidden, the hidden gradients, the six shared outputs and their gradients
    int out_bf16[2];            // logits, keypoints and their gradients, by kind
    int width;                  // C % width == 0, width <= C <= 4096
    bool aligned;               // hs, hidden, every weight and the (required) workspace are 16-byte aligned
    const char *width_msg;      // the form's own width test comes before every other check; null: the shared check's
    const char *ws_msg;         // a workspace smaller than the form's entry asks for
};
const Form kForms[2] = {
    {0, {0, 0}, 4, false, nullptr, "msda_heads: workspace smaller than msda_heads_workspace_bytes"},
    {1, {0, 1}, 8, true, "msda_heads_bf16: need a hidden size C with C % 8 == 0, 8 <= C <= 4096",
     "msda_heads_bf16: workspace smaller than msda_heads_bf16_workspace_bytes"},
};

int heads_D(int kind) { return kind == MSDA_HEADS_ARCTIC ? 42 : 63; }
int tiles_of(long long rows, int n) { return (int)(((rows + kHT - 1) / kHT) * ((n + kHT - 1) / kHT)); }
int chunks_of(long long rows) { return (int)((rows + kHeadsWgradChunk - 1) / kHeadsWgradChunk); }
bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
int herr(const char *msg) { return set_error(MSDA_ERR_ARGUMENT, msg); }
// dy rows of width n can be staged 8 elements per load: whole groups, aligned rows (fp32 rows: two 16-byte loads each)
int vec_ok(const void *dy, const void *aux, int n, int mode)
{
    return n % 8 == 0 && mode != kHeadsModeSigmoid && aligned16(dy) && (mode != kHeadsModeRelu || aligned16(aux)) ? 1 : 0;
}

// Where the tensors stacked behind one pointer lie, in the form's element types: the saved hidden activations
// [head][layer][L * M][C], the hidden gradients that open the workspace in the same layout, sig [head][L * M][D].  A null
// base (heads_workspace_bytes has no operands) stays null.
struct Stacked {
    long long LM;
    int C, D, es;               // es: bytes per hidden element
    Stacked(const HeadsCall &c)
        : LM((long long)c.L * c.M), C(c.C), D(heads_D(c.kind)), es(kForms[c.form].hidden_bf16 ? 2 : 4) {}
    void *hidden(void *base, int h, int layer) const
    {
        return base ? static_cast<char *>(base) + ((long long)(h * 2 + layer) * LM * C) * es : nullptr;
    }
    float *sig(float *base, int h) const { return base ? base + (long long)h * LM * D : nullptr; }
};

int heads_check(const HeadsCall &c, bool backward)
{
    const Form &f = kForms[c.form];
    if (f.width_msg != nullptr && !heads_supported(c.form, c.C)) return herr(f.width_msg);
    if (c.kind != MSDA_HEADS_ARCTIC && c.kind != MSDA_HEADS_ASSEMBLY)
        return herr("msda_heads: kind must be 0 (ARCTIC) or 1 (AssemblyHands)");
    if (c.L < 1 || c.L > kHeadsMaxLevels) return herr("msda_heads: need 1 <= L <= 8 levels");
    if (c.M < 1 || c.K < 1 || !heads_supported(kHeadsF32, c.C))
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
    const int n_shared = c.kind == MSDA_HEADS_ARCTIC ? kHeadsShared : 0, n_w = c.n_mlp * 3 * Lw;
    // every array of n pointers that the call reads, and the single pointers beside them
    auto all = [](auto a, int n) {
        bool ok = n == 0 || a != nullptr;
        for (int i = 0; ok && i < n; ++i) ok = a[i] != nullptr;
        return ok;
    };
    bool ok = c.hs != nullptr && all(c.cls_w, Lc) && all(c.cls_b, Lc) && all(c.mlp_w, n_w) && all(c.mlp_b, n_w)
              && all(c.shared_w, n_shared) && all(c.shared_b, n_shared);
    if (c.n_mlp > 0)
        ok = ok && c.init_ref != nullptr && (c.L == 1 || c.inter_ref != nullptr) && c.hidden != nullptr && c.sig != nullptr;
    if (!backward)
        ok = ok && c.logits != nullptr && all(c.kp_out, c.n_mlp) && all(c.shared_out, n_shared);
    else
        ok = ok && c.grad_logits != nullptr && c.grad_hs != nullptr && all(c.grad_cls_w, Lc) && all(c.grad_cls_b, Lc)
             && all(c.grad_kp, c.n_mlp) && all(c.grad_mlp_w, n_w) && all(c.grad_mlp_b, n_w) && all(c.grad_shared, n_shared)
             && all(c.grad_shared_w, n_shared) && all(c.grad_shared_b, n_shared)
             && (c.ws != nullptr || (!f.aligned && c.ws_bytes == 0));           // the fp32 form's workspace may be empty
    if (!ok) return herr("msda_heads: null pointer");
    if (f.aligned) {
        ok = aligned16(c.hs) && (c.n_mlp == 0 || aligned16(c.hidden));
        for (int l = 0; l < Lc; ++l) ok = ok && aligned16(c.cls_w[l]);
        for (int i = 0; i < n_w; ++i) ok = ok && aligned16(c.mlp_w[i]);
        for (int g = 0; g < n_shared; ++g) ok = ok && aligned16(c.shared_w[g]);
        if (!ok) return herr("msda_heads_bf16: hs, hidden and the weights must be 16-byte aligned");
        if (backward && !aligned16(c.ws)) return herr("msda_heads_bf16: the workspace must be 16-byte aligned");
    }
    if (backward && c.ws_bytes < heads_workspace_bytes(c.form, c.kind, c.L, c.M, c.C, c.K, c.n_mlp, c.flags)) return herr(f.ws_msg);
    return MSDA_OK;
}

// The weight problems of the backward, in one fixed order (the workspace layout follows it): class head(s), MLP layers
// (head, layer, level), the six shared Linears.  Operands the call does not carry (heads_workspace_bytes) come out null.
struct WeightProblem {
    const void *dy, *aux, *x;
    int dy_bf16, x_bf16, row0, rows, n, mode;
    float *dw, *db;
};
template <class Emit>
void weight_problems(const HeadsCall &c, Emit emit)
{
    const Form &f = kForms[c.form];
    const Stacked at(c);
    const int M = (int)c.M, LM = (int)at.LM, hb = f.hidden_bf16, ob = f.out_bf16[c.kind == MSDA_HEADS_ASSEMBLY];
    const bool shc = (c.flags & MSDA_HEADS_SHARED_CLS) != 0, shm = (c.flags & MSDA_HEADS_SHARED_MLP) != 0;
    const int Lc = shc ? 1 : c.L, Lw = shm ? 1 : c.L;
    auto of = [](float *const *a, int i) { return a ? a[i] : nullptr; };
    for (int l = 0; l < Lc; ++l)
        emit(WeightProblem{c.grad_logits, nullptr, c.hs, ob, 0, shc ? 0 : l * M, shc ? LM : M, c.K, kHeadsModePlain,
                           of(c.grad_cls_w, l), of(c.grad_cls_b, l)});
    for (int h = 0; h < c.n_mlp; ++h)
        for (int layer = 0; layer < 3; ++layer)
            for (int l = 0; l < Lw; ++l) {
                const int wi = (h * 3 + layer) * Lw + l;
                const void *dy = layer < 2 ? at.hidden(c.ws, h, layer) : c.grad_kp ? c.grad_kp[h] : nullptr;
                const void *aux = layer < 2 ? at.hidden(c.hidden, h, layer) : at.sig(c.sig, h);
                const void *x = layer == 0 ? c.hs : at.hidden(c.hidden, h, layer - 1);
                emit(WeightProblem{dy, aux, x, layer < 2 ? hb : ob, layer == 0 ? 0 : hb, shm ? 0 : l * M, shm ? LM : M,
                                   layer == 2 ? at.D : c.C, layer == 2 ? kHeadsModeSigmoid : kHeadsModeRelu, of(c.grad_mlp_w, wi),
                                   of(c.grad_mlp_b, wi)});
            }
    if (c.kind == MSDA_HEADS_ARCTIC)
        for (int g = 0; g < kHeadsShared; ++g)
            emit(WeightProblem{c.grad_shared ? c.grad_shared[g] : nullptr, nullptr, c.hs, hb, 0, 0, LM, kSharedN[g], kHeadsModePlain,
                               of(c.grad_shared_w, g), of(c.grad_shared_b, g)});
}

// the float offset of the first weight-gradient partial: behind the hidden gradients [n_mlp][2][L * M][C] (bf16: an even count)
long long partials_offset(const HeadsCall &c) { return (long long)c.n_mlp * 2 * c.L * c.M * c.C * Stacked(c).es / 4; }

}  // namespace

bool heads_supported(int form, int C) { return C >= kForms[form].width && C <= 4096 && C % kForms[form].width == 0; }

// The workspace: hidden gradients [n_mlp][2][L * M][C] in the form's hidden type, then per weight problem, in enumeration
// order, fp32 partials [chunks][n][C] and [chunks][n].
unsigned long long heads_workspace_bytes(int form, int kind, int L, long long M, int C, int K, int n_mlp, unsigned flags)
{
    HeadsCall c = {};
    c.form = form; c.kind = kind; c.L = L; c.M = M; c.C = C; c.K = K; c.n_mlp = n_mlp; c.flags = flags;
    unsigned long long floats = (unsigned long long)partials_offset(c);
    weight_problems(c, [&](const WeightProblem &w) { floats += (unsigned long long)chunks_of(w.rows) * w.n * (C + 1); });
    return floats * sizeof(float);
}

int heads_plan_forward(const HeadsCall &c, HeadsFwdPlan &plan)
{
    int rc = heads_check(c, false);
    if (rc != MSDA_OK) return rc;
    std::memset(&plan, 0, sizeof(plan));
    plan.form = c.form;
    const Form &f = kForms[c.form];
    const Stacked at(c);
    const int M = (int)c.M, LM = (int)at.LM, C = c.C, hb = f.hidden_bf16, ob = f.out_bf16[c.kind == MSDA_HEADS_ASSEMBLY];
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
        auto add = [&](const void *x, int x_bf16, int row0, int rows, int epi, float *sig) -> HeadsFwdProb & {
            HeadsFwdProb &p = a.p[a.nprob++];
            p.a = x; p.a_bf16 = x_bf16; p.sig = sig; p.row0 = row0; p.rows = rows; p.epi = epi; p.g0 = ng; p.ng = 0; p.n = 0;
            p.tile0 = tiles;
            return p;
        };
        auto group = [&](HeadsFwdProb &p, const float *w, const float *b, void *out, int out_bf16, int n) {
            HeadsFwdGroup &g = a.g[ng++];
            g.w = w; g.b = b; g.out = out; g.out_bf16 = out_bf16; g.n = n; g.off = p.n;
            p.n += n;
            ++p.ng;
        };
        for (int l = 0; l < c.L; ++l) {
            if (d == 0) {
                HeadsFwdProb &p = add(c.hs, 0, l * M, M, kHeadsEpiBias, nullptr);
                group(p, c.cls_w[shc ? 0 : l], c.cls_b[shc ? 0 : l], c.logits, ob, c.K);
                tiles += tiles_of(M, p.n);
            }
            for (int h = 0; h < c.n_mlp; ++h) {
                const int wi = (h * 3 + d) * Lw + (shm ? 0 : l);
                const void *x = d == 0 ? c.hs : at.hidden(c.hidden, h, d - 1);
                void *out = d < 2 ? at.hidden(c.hidden, h, d) : c.kp_out[h];
                const int epi = d < 2 ? kHeadsEpiRelu : c.kind == MSDA_HEADS_ARCTIC ? kHeadsEpiArctic : kHeadsEpiAssembly;
                HeadsFwdProb &p = add(x, d == 0 ? 0 : hb, l * M, M, epi, d == 2 ? at.sig(c.sig, h) : nullptr);
                group(p, c.mlp_w[wi], c.mlp_b[wi], out, d < 2 ? hb : ob, d < 2 ? C : at.D);
                tiles += tiles_of(M, p.n);
            }
        }
        if (d == 0 && c.kind == MSDA_HEADS_ARCTIC) {                    // the six shared Linears: ONE problem over L * M rows
            HeadsFwdProb &p = add(c.hs, 0, 0, LM, kHeadsEpiBias, nullptr);
            for (int g = 0; g < kHeadsShared; ++g) group(p, c.shared_w[g], c.shared_b[g], c.shared_out[g], hb, kSharedN[g]);
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
    plan.form = c.form;
    const Form &f = kForms[c.form];
    const Stacked at(c);
    const int M = (int)c.M, C = c.C, hb = f.hidden_bf16, ob = f.out_bf16[c.kind == MSDA_HEADS_ASSEMBLY];
    const bool shc = (c.flags & MSDA_HEADS_SHARED_CLS) != 0, shm = (c.flags & MSDA_HEADS_SHARED_MLP) != 0;
    const int Lw = shm ? 1 : c.L;
    // input gradients: d[0] depth 3 -> dH2, d[1] depth 2 -> dH1 (the workspace's hidden gradients), d[2] depth 1 -> fp32 grad_hs
    for (int step = 0; step < 3; ++step) {
        HeadsDgradArgs &a = plan.d[step];
        a.C = C;
        int ns = 0, tiles = 0;
        for (int l = 0; l < c.L; ++l) {
            auto seg = [&](const void *x, int x_bf16, const void *aux, const float *w, int k, int mode) {
                HeadsDgradSeg &s = a.s[ns++];
                s.a = x; s.a_bf16 = x_bf16; s.aux = aux; s.w = w; s.k = k; s.mode = mode;
                s.vec = vec_ok(x, aux, k, mode);
            };
            auto prob = [&](void *out, int out_bf16, int s0) {
                HeadsDgradProb &p = a.p[a.nprob++];
                p.out = out; p.out_bf16 = out_bf16; p.row0 = l * M; p.rows = M; p.s0 = s0; p.ns = ns - s0; p.tile0 = tiles;
                tiles += tiles_of(M, C);
            };
            if (step < 2) {
                for (int h = 0; h < c.n_mlp; ++h) {
                    const int layer = 2 - step, wi = (h * 3 + layer) * Lw + (shm ? 0 : l);
                    const int s0 = ns;
                    if (step == 0) seg(c.grad_kp[h], ob, at.sig(c.sig, h), c.mlp_w[wi], at.D, kHeadsModeSigmoid);
                    else seg(at.hidden(c.ws, h, 1), hb, at.hidden(c.hidden, h, 1), c.mlp_w[wi], C, kHeadsModeRelu);
                    prob(at.hidden(c.ws, h, 1 - step), hb, s0);
                }
            } else {
                const int s0 = ns;
                seg(c.grad_logits, ob, nullptr, c.cls_w[shc ? 0 : l], c.K, kHeadsModePlain);
                for (int h = 0; h < c.n_mlp; ++h)
                    seg(at.hidden(c.ws, h, 0), hb, at.hidden(c.hidden, h, 0), c.mlp_w[(h * 3) * Lw + (shm ? 0 : l)], C, kHeadsModeRelu);
                if (c.kind == MSDA_HEADS_ARCTIC)
                    for (int g = 0; g < kHeadsShared; ++g) seg(c.grad_shared[g], hb, nullptr, c.shared_w[g], kSharedN[g], kHeadsModePlain);
                prob(c.grad_hs, 0, s0);
            }
        }
        plan.dtiles[step] = tiles;
    }
    // weight gradients: fp32 partials per chunk behind the hidden gradients, then the chunk-ordered sums
    long long off = partials_offset(c);
    plan.w.ws = static_cast<float *>(c.ws);
    plan.w.C = C;
    plan.r.ws = plan.w.ws;
    plan.r.C = C;
    int wt = 0, rb = 0;
    weight_problems(c, [&](const WeightProblem &w) {
        HeadsWgradProb &p = plan.w.p[plan.w.nprob++];
        p.dy = w.dy; p.aux = w.aux; p.x = w.x; p.x_bf16 = w.x_bf16; p.part = off; p.row0 = w.row0; p.rows = w.rows; p.n = w.n;
        p.dy_flags = (w.dy_bf16 ? kHeadsSrcBf16 : 0) | (vec_ok(w.dy, w.aux, w.n, w.mode) ? kHeadsSrcVec : 0);
        p.mode = w.mode; p.chunks = chunks_of(w.rows); p.tile0 = wt;
        wt += p.chunks * tiles_of(w.n, C);
        HeadsReduceProb &r = plan.r.p[plan.r.nprob++];
        r.part = off; r.dw = w.dw; r.db = w.db; r.n = w.n; r.chunks = p.chunks; r.tile0 = rb;
        rb += (int)(((long long)w.n * (C + 1) + kHBlock - 1) / kHBlock);
        off += (long long)p.chunks * w.n * (C + 1);
    });
    plan.wtiles = wt;
    plan.rblocks = rb;
    return MSDA_OK;
}

int heads_run_forward(const HeadsFwdPlan &plan, hipStream_t stream)
{
    for (int d = 0; d < 3; ++d) {
        const int rc = plan.form == kHeadsBf16 ? launch_heads_forward_bf16(plan.a[d], plan.tiles[d], stream)
                                               : heads_launch(heads_fwd_kernel, "heads_fwd_kernel", plan.a[d], plan.tiles[d], stream);
        if (rc != MSDA_OK) return rc;
    }
    return MSDA_OK;
}

int heads_run_backward(const HeadsBwdPlan &plan, hipStream_t stream)
{
    const bool bf = plan.form == kHeadsBf16;
    for (int s = 0; s < 3; ++s) {
        const int rc = bf ? launch_heads_dgrad_bf16(plan.d[s], plan.dtiles[s], stream)
                          : heads_launch(heads_dgrad_kernel, "heads_dgrad_kernel", plan.d[s], plan.dtiles[s], stream);
        if (rc != MSDA_OK) return rc;
    }
    const int rc = bf ? launch_heads_wgrad_bf16(plan.w, plan.wtiles, stream)
                      : heads_launch(heads_wgrad_kernel, "heads_wgrad_kernel", plan.w, plan.wtiles, stream);
    if (rc != MSDA_OK) return rc;
    return heads_launch(heads_reduce_kernel, "heads_reduce_kernel", plan.r, plan.rblocks, stream);
}

// The reference gradient beside the backward above: one launch over the levels whose output is given, none when both are null.
int heads_plan_ref_backward(int L, long long M, int n_mlp, int R, const float *init_ref, const float *inter_ref, const float *sig,
                            const float *const *grad_kp, float *grad_init_ref, float *grad_inter_ref, HeadsRefBwdPlan &plan)
{
    plan.blocks = 0;
    plan.width = 1;
    if (L < 1 || L > kHeadsMaxLevels) return herr("msda_heads_ref_backward: need 1 <= L <= 8 levels");
    if (M < 1) return herr("msda_heads_ref_backward: need M >= 1");
    if (n_mlp != 2) return herr("msda_heads_ref_backward: n_mlp must be 2 (key_embed, obj_key_embed)");
    if (R != 42) return herr("msda_heads_ref_backward: reference width R must be 42");
    if (M >= (1LL << 31) || (long long)L * M * R >= (1LL << 31)) return herr("msda_heads_ref_backward: tensors beyond 2^31 elements");
    const bool want0 = grad_init_ref != nullptr, want1 = grad_inter_ref != nullptr && L > 1;
    if (sig == nullptr || grad_kp == nullptr || grad_kp[0] == nullptr || grad_kp[1] == nullptr || (want0 && init_ref == nullptr)
        || (want1 && inter_ref == nullptr))
        return herr("msda_heads_ref_backward: null pointer");
    if (!want0 && !want1) return MSDA_OK;
    HeadsRefBwdArgs &a = plan.a;
    a.init_ref = init_ref; a.inter_ref = inter_ref; a.sig = sig; a.grad_kp[0] = grad_kp[0]; a.grad_kp[1] = grad_kp[1];
    a.grad_init_ref = grad_init_ref; a.grad_inter_ref = grad_inter_ref;
    a.MR = M * R; a.LMR = (long long)L * a.MR;
    a.e0 = want0 ? 0 : a.MR;
    const long long n = (want1 ? a.LMR : a.MR) - a.e0;
    // the access width: M * R is even, and a multiple of 4 when M is; every base must be as aligned as the width it is read with
    int W = M % 2 == 0 ? 4 : 2;
    // (the pointers of a level that is not wanted are not read and do not count)
    for (const void *p : {(const void *)(want0 ? init_ref : nullptr), (const void *)(want1 ? inter_ref : nullptr), (const void *)sig,
                          (const void *)grad_kp[0], (const void *)grad_kp[1], (const void *)(want0 ? grad_init_ref : nullptr),
                          (const void *)(want1 ? grad_inter_ref : nullptr)})
        while (W > 1 && (reinterpret_cast<uintptr_t>(p) & (uintptr_t)(W * 4 - 1)) != 0) W /= 2;
    a.groups = n / W;                                                           // n is a multiple of M * R, so of W
    const long long blocks = (a.groups + kHBlock - 1) / kHBlock;
    plan.blocks = (int)(blocks < 2048 ? blocks : 2048);                         // the kernel strides over the rest
    plan.width = W;
    return MSDA_OK;
}

int heads_run_ref_backward(const HeadsRefBwdPlan &plan, hipStream_t stream)
{
    if (plan.width == 4) return heads_launch(heads_ref_bwd_kernel<4>, "heads_ref_bwd_kernel", plan.a, plan.blocks, stream);
    if (plan.width == 2) return heads_launch(heads_ref_bwd_kernel<2>, "heads_ref_bwd_kernel", plan.a, plan.blocks, stream);
    return heads_launch(heads_ref_bwd_kernel<1>, "heads_ref_bwd_kernel", plan.a, plan.blocks, stream);
}

}  // namespace msda
