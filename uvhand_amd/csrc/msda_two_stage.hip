// Two-stage query selection of UVHand's DeformableTransformer (models/arctic_transformer.py:23-259):
//
//   proposals   gen_encoder_output_proposals (:106-142) forward in one pass over the rows: per level the valid extent read
//               off the padding mask exactly as :113-114 do (first column / first row, so masks that are not a clean
//               rectangle give the reference's numbers), the 42-d proposal (pixel centre / valid extent, then the 20 learned
//               or constant (x, y) offsets), its logit with +inf at padded rows and at rows outside (0.01, 0.99), a copy of
//               `memory` with those rows zeroed and a byte mask of the zeroed rows (the backward zeroes the same rows of the
//               incoming gradient with msda_zero_masked_rows_f32).
//   select      the query selection (:208-232): per frame the row max / argmax over the K class logits, the top Q rows by
//               that max (descending; ties -> lower row index first; NaN ranks above every number), the 42 coordinates
//               gathered from the hand / object / proposal source by the class rule, and sigmoid * 2 - 1 of them.  One
//               workgroup per frame, one launch, no host round trip (the reference's boolean-mask assignment is a nonzero
//               and a device -> host sync; this is capturable in a graph).  The ordering is a bitonic sort of 64-bit keys
//               (order-preserving image of the max, inverted, above the row index) in LDS: S <= 8192 rows per frame.
//   pe          get_proposal_pos_embed (:91-104): PE[m, c*128 + 2i + s] = s ? cos(u) : sin(u),
//               u = (sigmoid(r[m, c]) * 2 pi) / dim_t[2i], dim_t the 64-entry table torch computes (:96-97), given by the host.
//   pe_linear   relu(PE(r) @ W1^T + b1) — pos_trans[0] and its ReLU — on fp32 MFMA with the A operand generated per K stage
//               from the 42 numbers of the row into LDS, so the [M, 5376] table never exists in memory.
//
// sin / cos: sincosf (the device library's full-range form — the same function torch's sin / cos kernels reach), sigmoid as
// torch writes it, 1 / (1 + exp(-x)); both in plain fp32 without fast-math.
#include "msda_common.h"
#include "msda_launch.h"

namespace msda {

constexpr int kTsBlock = 256;
constexpr int kPeWidth = 5376;                 // 42 coordinates x 128 features
constexpr float kTwoPi = 6.283185307179586f;   // 2 * math.pi as torch casts it to the tensor's fp32

__device__ __forceinline__ float sigmoid_ref(float x) { return 1.f / (1.f + expf(-x)); }

// ---- proposals --------------------------------------------------------------------------------------------------------
struct LevelTable {
    int L;
    int H[kMaxLevels], W[kMaxLevels], start[kMaxLevels];
};

// grid (ceil(S / 256), N); one thread per row for the proposal, the workgroup together for the memory copy.
__global__ __launch_bounds__(kTsBlock) void proposals_kernel(
    const float *__restrict__ memory, const uint8_t *__restrict__ pad, LevelTable lv, const float *__restrict__ learnedxy,
    int S, int C, float *__restrict__ proposals, float *__restrict__ memory_out, uint8_t *__restrict__ row_mask)
{
    __shared__ int vh[kMaxLevels], vw[kMaxLevels];
    __shared__ float xy[kMaxLevels][40];
    __shared__ int xy_ok[kMaxLevels];
    __shared__ uint8_t dead[kTsBlock];
    const int n = blockIdx.y, tid = threadIdx.x;
    const uint8_t *pm = pad + (long long)n * S;
    if (tid < kMaxLevels) { vh[tid] = 0; vw[tid] = 0; xy_ok[tid] = 1; }
    __syncthreads();
    // valid_H = number of unpadded rows in the first column, valid_W = unpadded columns in the first row (:113-114)
    for (int l = 0; l < lv.L; ++l) {
        int ch = 0, cw = 0;
        for (int h = tid; h < lv.H[l]; h += kTsBlock) ch += pm[lv.start[l] + h * lv.W[l]] == 0;
        for (int w = tid; w < lv.W[l]; w += kTsBlock) cw += pm[lv.start[l] + w] == 0;
        if (ch) atomicAdd(&vh[l], ch);
        if (cw) atomicAdd(&vw[l], cw);
    }
    // the 40 level-constant columns: sigmoid(learnedxy) * 2^lvl, or 0.05 * 2^lvl
    for (int e = tid; e < lv.L * 40; e += kTsBlock) {
        const int l = e / 40, j = e % 40;
        const float base = learnedxy != nullptr ? sigmoid_ref(learnedxy[j]) : 0.05f;
        xy[l][j] = base * (float)(1 << l);
    }
    __syncthreads();
    for (int e = tid; e < lv.L * 40; e += kTsBlock) {
        const int l = e / 40, j = e % 40;
        const float p = xy[l][j];
        if (!(p > 0.01f && p < 0.99f)) xy_ok[l] = 0;                 // benign race: every writer writes 0
    }
    __syncthreads();
    const int s = blockIdx.x * kTsBlock + tid;
    bool zero = false;
    if (s < S) {
        int l = 0;
        while (l + 1 < lv.L && s >= lv.start[l + 1]) ++l;
        const int local = s - lv.start[l], h = local / lv.W[l], w = local % lv.W[l];
        const float px = ((float)w + 0.5f) / (float)vw[l];
        const float py = ((float)h + 0.5f) / (float)vh[l];
        const bool valid = px > 0.01f && px < 0.99f && py > 0.01f && py < 0.99f && xy_ok[l];
        zero = pm[s] != 0 || !valid;
        float *out = proposals + ((long long)n * S + s) * 42;
        const float inf = __builtin_inff();
        out[0] = zero ? inf : logf(px / (1.f - px));
        out[1] = zero ? inf : logf(py / (1.f - py));
        for (int j = 0; j < 40; ++j) {
            const float p = xy[l][j];
            out[2 + j] = zero ? inf : logf(p / (1.f - p));
        }
        row_mask[(long long)n * S + s] = zero ? 1 : 0;
    }
    dead[tid] = zero ? 1 : 0;
    __syncthreads();
    // memory_out rows of this workgroup: C / 4 float4 per row
    const int rows = min(kTsBlock, S - (int)blockIdx.x * kTsBlock);
    const int per_row = C / 4;
    const long long row0 = (long long)n * S + (long long)blockIdx.x * kTsBlock;
    const float4 *src4 = reinterpret_cast<const float4 *>(memory + row0 * C);
    float4 *dst4 = reinterpret_cast<float4 *>(memory_out + row0 * C);
    for (int e = tid; e < rows * per_row; e += kTsBlock) {
        const int r = e / per_row;
        dst4[e] = dead[r] ? make_float4(0.f, 0.f, 0.f, 0.f) : src4[e];
    }
}

int launch_two_stage_proposals(const float *memory, const uint8_t *pad, int N, int S, int C, int L, const int *heights,
                               const int *widths, const float *learnedxy, float *proposals, float *memory_out, uint8_t *row_mask,
                               hipStream_t stream)
{
    LevelTable lv{};
    lv.L = L;
    int start = 0;
    for (int l = 0; l < L; ++l) {
        lv.H[l] = heights[l];
        lv.W[l] = widths[l];
        lv.start[l] = start;
        start += heights[l] * widths[l];
    }
    if (N == 0 || S == 0) return MSDA_OK;
    hipLaunchKernelGGL(proposals_kernel, dim3((unsigned)((S + kTsBlock - 1) / kTsBlock), (unsigned)N), dim3(kTsBlock), 0, stream,
                       memory, pad, lv, learnedxy, S, C, proposals, memory_out, row_mask);
    return check_launch("proposals_kernel");
}

// ---- query selection --------------------------------------------------------------------------------------------------
constexpr int kSelBlock = 1024;

// order-preserving image of a float as an unsigned integer; NaN above +inf, -0 == +0
__device__ __forceinline__ uint32_t float_order(float x)
{
    if (x != x) return 0xffffffffu;
    if (x == 0.f) x = 0.f;
    const uint32_t b = __float_as_uint(x);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// max / argmax over k logits as torch.max(-1) / argmax(-1): NaN wins, first occurrence of the maximum
__device__ __forceinline__ void row_max(const float *p, int K, float &mx, int &arg)
{
    mx = p[0];
    arg = 0;
    for (int k = 1; k < K; ++k) {
        const float v = p[k];
        if (mx != mx) break;
        if (v != v || v > mx) { mx = v; arg = k; }
    }
}

__global__ __launch_bounds__(kSelBlock) void select_kernel(
    const float *__restrict__ cls, const float *__restrict__ hand, const float *__restrict__ obj, const float *__restrict__ prop,
    int S, int K, int Q, int P, int hand0, int hand1, int64_t *__restrict__ topk, float *__restrict__ unsig,
    float *__restrict__ refp)
{
    __shared__ unsigned long long key[kSelMaxRows];
    const int n = blockIdx.x, tid = threadIdx.x;
    const float *c = cls + (long long)n * S * K;
    for (int s = tid; s < P; s += kSelBlock) {
        unsigned long long k = ~0ull;                                   // padding sorts last
        if (s < S) {
            float mx;
            int arg;
            row_max(c + (long long)s * K, K, mx, arg);
            k = ((unsigned long long)(~float_order(mx)) << 32) | (unsigned)s;
        }
        key[s] = k;
    }
    __syncthreads();
    // bitonic sort, ascending: descending max, then ascending row index
    for (int k = 2; k <= P; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < P / 2; t += kSelBlock) {
                const int i = 2 * t - (t & (j - 1)), ixj = i + j;
                const unsigned long long a = key[i], b = key[ixj];
                const bool up = (i & k) == 0;
                if ((a > b) == up) { key[i] = b; key[ixj] = a; }
            }
            __syncthreads();
        }
    }
    const long long base = (long long)n * S;
    for (int e = tid; e < Q * 42; e += kSelBlock) {
        const int q = e / 42, col = e % 42;
        const int s = (int)(key[q] & 0xffffffffu);
        float mx;
        int cl;
        row_max(c + (long long)s * K, K, mx, cl);
        const bool is_hand = cl == hand0 || cl == hand1, is_obj = !is_hand && cl != 0;
        const float *src = is_hand ? hand : (is_obj ? obj : prop);
        const float v = src[(base + s) * 42 + col];
        const long long o = ((long long)n * Q + q) * 42 + col;
        unsig[o] = v;
        refp[o] = sigmoid_ref(v) * 2.f - 1.f;
        if (col == 0 && topk != nullptr) topk[(long long)n * Q + q] = s;
    }
}

int launch_two_stage_select(const float *cls, const float *hand, const float *obj, const float *prop, int N, int S, int K, int Q,
                            int hand0, int hand1, int64_t *topk, float *unsig, float *refp, hipStream_t stream)
{
    if (N == 0 || Q == 0) return MSDA_OK;
    int P = 2;
    while (P < S) P <<= 1;
    hipLaunchKernelGGL(select_kernel, dim3((unsigned)N), dim3(kSelBlock), 0, stream, cls, hand, obj, prop, S, K, Q, P, hand0, hand1,
                       topk, unsig, refp);
    return check_launch("select_kernel");
}

// ---- proposal embedding -----------------------------------------------------------------------------------------------
// (sin u_i, cos u_i, sin u_{i+1}, cos u_{i+1}) of row coordinate a = sigmoid(r) * 2 pi: PE columns 4q .. 4q+3 of one coordinate
__device__ __forceinline__ float4 pe_quad(float a, float d0, float d1)
{
    float4 v;
    sincosf(a / d0, &v.x, &v.y);
    sincosf(a / d1, &v.z, &v.w);
    return v;
}

// one thread per (row, coordinate, pair of features): 4 consecutive floats of the table
__global__ __launch_bounds__(kTsBlock) void pe_kernel(const float *__restrict__ r, const float *__restrict__ dim_t, long long M,
                                                      float *__restrict__ pe)
{
    const long long e = (long long)blockIdx.x * kTsBlock + threadIdx.x;        // float4 index in [0, M * 1344)
    if (e >= M * (kPeWidth / 4)) return;
    const long long m = e / (kPeWidth / 4);
    const int q = (int)(e % (kPeWidth / 4)), col = q >> 5, i = (q & 31) * 2;
    const float a = sigmoid_ref(r[m * 42 + col]) * kTwoPi;
    reinterpret_cast<float4 *>(pe)[e] = pe_quad(a, dim_t[i], dim_t[i + 1]);
}

int launch_pe(const float *r, const float *dim_t, long long M, float *pe, hipStream_t stream)
{
    if (M == 0) return MSDA_OK;
    const long long n4 = M * (kPeWidth / 4);
    hipLaunchKernelGGL(pe_kernel, dim3((unsigned)((n4 + kTsBlock - 1) / kTsBlock)), dim3(kTsBlock), 0, stream, r, dim_t, M, pe);
    return check_launch("pe_kernel");
}

// ---- PE(r) @ W1^T + b1, ReLU ------------------------------------------------------------------------------------------
// 64 x 128 outputs per 256-thread workgroup: 4 wavefronts as 2 x 2 blocks of 32 rows x 64 columns, each two 32 x 32
// v_mfma_f32_32x32x2_f32 accumulators; reduction in stages of 32 columns of PE (a quarter of one coordinate's 128).  The
// B operand (W1, [out, 5376] K-major) is staged from memory as msda_gemm.hip's linear_rows_kernel stages it; the A operand
// is generated: each thread computes its 2 x 4 PE values of the stage (4 sincosf) two stages ahead, while the MFMAs of the
// current stage run, and stores them to LDS where the global loads would have landed.  Every PE element is generated
// Nc / 128 times (8 at Nc = 1024).  The sum of an output is two-level: MFMA chains of kPlFlush = 256 columns, added into a
// total in order.  Fixed summation order: bitwise reproducible.
constexpr int kPlM = 64, kPlN = 128, kPlStage = 32, kPlRow = kPlStage + 4;
constexpr int kPlFlush = 256;                  // columns per MFMA chain
static_assert(kPeWidth % kPlFlush == 0 && (kPlFlush & (kPlFlush - 1)) == 0 && kPlFlush % kPlStage == 0, "chains tile the reduction");

__global__ __launch_bounds__(kTsBlock) __attribute__((amdgpu_waves_per_eu(2, 2))) void pe_linear_relu_kernel(
    const float *__restrict__ R, const float *__restrict__ dim_t, const float *__restrict__ B, const float *__restrict__ bias,
    float *__restrict__ C, long long M, int Nc, int tiles_n, long long tiles)
{
    constexpr int G = 2, NI = kPlStage / (4 * G);             // 32x32x2: two lane groups; 4 float4 fragment reads per stage
    constexpr int kPerRow = kPlStage / 4, kStep = kTsBlock / kPerRow;
    constexpr int kLdA = kPlM / kStep, kLdB = kPlN / kStep;   // 2 and 4 float4 per thread and stage
    using Acc = __attribute__((ext_vector_type(16))) float;
    __shared__ __attribute__((aligned(16))) float As[2][kPlM * kPlRow];
    __shared__ __attribute__((aligned(16))) float Bs[2][kPlN * kPlRow];
    __shared__ float dt[64];
    const long long per = (tiles + 7) >> 3;
    const long long logical = (long long)(blockIdx.x & 7) * per + (blockIdx.x >> 3);
    if ((long long)(blockIdx.x >> 3) >= per || logical >= tiles) return;
    const long long m0 = (logical / tiles_n) * kPlM;
    const int n0 = (int)(logical % tiles_n) * kPlN;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int i0 = (wave >> 1) * 32, j0 = (wave & 1) * 64, g = lane >> 5, c = lane & 31;
    if (tid < 64) dt[tid] = dim_t[tid];
    const int krow = tid / kPerRow, kcol = (tid % kPerRow) * 4;
    // the sigmoid-scaled coordinate of this thread's rows changes every 4 stages (128 / 32): kept in registers
    float ang[kLdA];
    int ang_col = -1;
    float4 ra[kLdA], rb[kLdB];
    __syncthreads();                                           // dt visible
#define TS_GEN(k0_)                                                                                                     \
    do {                                                                                                                \
        const int col_ = (k0_) >> 7, i_ = ((k0_) & 127) / 2 + kcol / 2;                                                 \
        if (col_ != ang_col) {                                                                                          \
            ang_col = col_;                                                                                             \
            _Pragma("unroll") for (int r = 0; r < kLdA; ++r) {                                                          \
                const long long m = m0 + krow + kStep * r;                                                              \
                ang[r] = m < M ? sigmoid_ref(R[m * 42 + col_]) * kTwoPi : 0.f;                                          \
            }                                                                                                           \
        }                                                                                                               \
        const float d0_ = dt[i_], d1_ = dt[i_ + 1];                                                                     \
        _Pragma("unroll") for (int r = 0; r < kLdA; ++r) ra[r] = pe_quad(ang[r], d0_, d1_);   /* rows >= M: never stored */ \
    } while (0)
#define TS_LOAD_B(k0_)                                                                                                  \
    do {                                                                                                                \
        _Pragma("unroll") for (int r = 0; r < kLdB; ++r) {                                                              \
            const int n = n0 + krow + kStep * r;                                                                        \
            rb[r] = make_float4(0.f, 0.f, 0.f, 0.f);                                                                    \
            if (n < Nc) rb[r] = *reinterpret_cast<const float4 *>(B + (long long)n * kPeWidth + (k0_) + kcol);          \
        }                                                                                                               \
    } while (0)
#define TS_STORE(buf_)                                                                                                  \
    do {                                                                                                                \
        _Pragma("unroll") for (int r = 0; r < kLdA; ++r)                                                                \
            *reinterpret_cast<float4 *>(&As[buf_][(krow + kStep * r) * kPlRow + kcol]) = ra[r];                         \
        _Pragma("unroll") for (int r = 0; r < kLdB; ++r)                                                                \
            *reinterpret_cast<float4 *>(&Bs[buf_][(krow + kStep * r) * kPlRow + kcol]) = rb[r];                         \
    } while (0)
#define TS_FRAGS(buf_, a_, b0_, b1_)                                                                                    \
    do {                                                                                                                \
        _Pragma("unroll") for (int i = 0; i < NI; ++i) {                                                                \
            a_[i] = *reinterpret_cast<const float4 *>(&As[buf_][(i0 + c) * kPlRow + 4 * G * i + 4 * g]);                \
            b0_[i] = *reinterpret_cast<const float4 *>(&Bs[buf_][(j0 + c) * kPlRow + 4 * G * i + 4 * g]);               \
            b1_[i] = *reinterpret_cast<const float4 *>(&Bs[buf_][(j0 + 32 + c) * kPlRow + 4 * G * i + 4 * g]);          \
        }                                                                                                               \
    } while (0)
#define TS_MMA(from_, to_)                                                                                              \
    do {                                                                                                                \
        _Pragma("unroll") for (int i = (from_); i < (to_); ++i) {                                                       \
            acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(av[i].x, bv0[i].x, acc0, 0, 0, 0);                              \
            acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(av[i].x, bv1[i].x, acc1, 0, 0, 0);                              \
            acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(av[i].y, bv0[i].y, acc0, 0, 0, 0);                              \
            acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(av[i].y, bv1[i].y, acc1, 0, 0, 0);                              \
            acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(av[i].z, bv0[i].z, acc0, 0, 0, 0);                              \
            acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(av[i].z, bv1[i].z, acc1, 0, 0, 0);                              \
            acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(av[i].w, bv0[i].w, acc0, 0, 0, 0);                              \
            acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(av[i].w, bv1[i].w, acc1, 0, 0, 0);                              \
        }                                                                                                               \
    } while (0)
    float4 av[NI], bv0[NI], bv1[NI], avn[NI], bvn0[NI], bvn1[NI];
    // two-level sum: the MFMA chain runs over kPlFlush columns (two coordinates, 128 MFMAs), then goes into the total.  One
    // chain over all 5376 columns rounds 2688 times at the magnitude of the whole sum: 2.1e-6 of max |y| against 4e-7 for
    // torch's blocked fp32 GEMM (tests/test_two_stage_envelope_gpu.py); 128 + 21 roundings leave a third of that.
    Acc acc0, acc1, tot0, tot1;
#pragma unroll
    for (int r = 0; r < 16; ++r) { acc0[r] = 0.f; acc1[r] = 0.f; tot0[r] = 0.f; tot1[r] = 0.f; }
    TS_GEN(0);
    TS_LOAD_B(0);
    TS_STORE(0);
    TS_GEN(kPlStage);
    TS_LOAD_B(kPlStage);
    __syncthreads();
    TS_FRAGS(0, av, bv0, bv1);
    // software pipeline as linear_rows_kernel: at the start of stage s the registers of stage s+1 go to the other buffer and
    // stage s+2 is generated / loaded; half the MFMAs; one barrier; the fragments of stage s+1; the other half
    int cur = 0;
    for (int k0 = 0; k0 < kPeWidth; k0 += kPlStage) {
        const bool more = k0 + kPlStage < kPeWidth;
        if (more) {
            TS_STORE(cur ^ 1);
            if (k0 + 2 * kPlStage < kPeWidth) {
                TS_LOAD_B(k0 + 2 * kPlStage);
                TS_GEN(k0 + 2 * kPlStage);
            }
        }
        TS_MMA(0, NI / 2);
        if (more) {
            __syncthreads();
            TS_FRAGS(cur ^ 1, avn, bvn0, bvn1);
        }
        TS_MMA(NI / 2, NI);
        if (more) {
#pragma unroll
            for (int i = 0; i < NI; ++i) { av[i] = avn[i]; bv0[i] = bvn0[i]; bv1[i] = bvn1[i]; }
        }
        if ((k0 & (kPlFlush - 1)) == kPlFlush - kPlStage) {     // the last stage of a chain (and of the loop)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                tot0[r] += acc0[r];
                tot1[r] += acc1[r];
                acc0[r] = 0.f;
                acc1[r] = 0.f;
            }
        }
        cur ^= 1;
    }
#undef TS_GEN
#undef TS_LOAD_B
#undef TS_STORE
#undef TS_FRAGS
#undef TS_MMA
    // C/D layout of 32x32x2: column c, row (r & 3) + 8 (r >> 2) + 4 g; ReLU keeps NaN (torch.relu does)
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        const int j = n0 + j0 + 32 * half + c;
        if (j >= Nc) continue;
        const float bj = bias != nullptr ? bias[j] : 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const long long i = m0 + i0 + (r & 3) + 8 * (r >> 2) + 4 * g;
            if (i < M) {
                const float v = (half ? tot1[r] : tot0[r]) + bj;
                C[i * Nc + j] = v < 0.f ? 0.f : v;
            }
        }
    }
}

int launch_pe_linear_relu(const float *r, const float *dim_t, const float *w, const float *bias, long long M, int Nc, float *y,
                          hipStream_t stream)
{
    if (M == 0) return MSDA_OK;
    const int tiles_n = (Nc + kPlN - 1) / kPlN;
    const long long tiles = ((M + kPlM - 1) / kPlM) * tiles_n;
    const long long grid = 8 * ((tiles + 7) / 8);
    if (grid * kTsBlock > 0xffffffffLL) return set_error(MSDA_ERR_ARGUMENT, "pe_linear: too many rows for one launch");
    hipLaunchKernelGGL(pe_linear_relu_kernel, dim3((unsigned)grid), dim3(kTsBlock), 0, stream, r, dim_t, w, bias, y, M, Nc, tiles_n,
                       tiles);
    return check_launch("pe_linear_relu_kernel");
}

}  // namespace msda
