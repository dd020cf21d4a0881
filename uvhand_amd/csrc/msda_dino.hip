// The DINO decoder's query positions and reference-point refinement (models/dino/deformable_transformer.py:730-746, :781-798;
// models/dino/utils.py:138-165):
//
//   sine_embed  gen_sineembed_for_position of reference_points * valid_ratios[level 0]: per row the means of the x and of the y
//               columns (1 or 21 of each), times 2 pi, divided by torch's 64-entry table, sin / cos interleaved, the y half first
//               (the reference's cat((pos_y, pos_x))).  Rows are sequence-first: row m belongs to frame m % N.
//   query_pos   ref_point_head (256 -> 256 -> 256, ReLU between) of that table in ONE launch: a workgroup owns a panel of 64 rows,
//               generates the panel's [64, 256] table straight into LDS as the A operand of the first product, keeps the panel's
//               h = relu(. @ W1^T + b1) in the same LDS buffer as the A operand of the second, and writes h to memory once (the
//               backward saves it).  fp32 MFMA (v_mfma_f32_32x32x2_f32), the lane / register layout of msda_gemm.hip.
//   refine      the layer's refinement: code = class rule of the row (2 hand, 1 object, 0 stays), u = inverse_sigmoid(ref) plus
//               the hand or the object head's delta, out = sigmoid(u) * 2 - 1; the reference's two boolean-mask adds (a nonzero
//               and a host synchronisation each) as one launch.  Backward: g_u = g_out * (1 - out^2) / 2 routed by the code.
//
// sin / cos: sincosf (the device library's full-range form, as pe_kernel of msda_two_stage.hip); sigmoid as torch writes it,
// 1 / (1 + exp(-x)); inverse_sigmoid is util/misc.py:614-618 with torch's NaN-propagating clamp; plain fp32, no fast-math.  The
// mean multiplies the sum by the fp32 reciprocal of the count, as torch's mean does.  No atomics, fixed summation order:
// bitwise reproducible.
#include "msda_common.h"
#include "msda_launch.h"

namespace msda {

namespace {

constexpr int kDnBlock = 256;
constexpr int kDnWidth = 256;                  // columns of the sine table = in = hidden = out features of ref_point_head
constexpr float kDnTwoPi = 6.283185307179586f; // 2 * math.pi as torch casts it to the tensor's fp32

__device__ __forceinline__ float dn_sigmoid(float x) { return 1.f / (1.f + expf(-x)); }

// (sin, cos) of a / d0 and of a / d1: table columns 4q .. 4q+3 of one axis
__device__ __forceinline__ float4 dn_quad(float a, float d0, float d1)
{
    float4 v;
    sincosf(a / d0, &v.x, &v.y);
    sincosf(a / d1, &v.z, &v.w);
    return v;
}

// 2 pi * mean_k(ref[m, 2k + axis] * valid[frame, axis]) of one row; axis 0 = x, 1 = y
__device__ __forceinline__ float dn_axis_embed(const float *__restrict__ ref, int W, const float *__restrict__ valid_xy, int N,
                                               long long m, int axis)
{
    const float vr = valid_xy != nullptr ? valid_xy[(m % N) * 2 + axis] : 1.f;
    const float *r = ref + m * W + axis;
    if (W == 2) return r[0] * vr * kDnTwoPi;
    float s = 0.f;
    for (int k = 0; k < 21; ++k) s += r[2 * k] * vr;
    return s * (1.f / 21.f) * kDnTwoPi;
}

// ---- the table ----------------------------------------------------------------------------------------------------------
// 4 rows per 256-thread workgroup: one thread per 4 consecutive floats of the table
__global__ __launch_bounds__(kDnBlock) void dino_sine_embed_kernel(const float *__restrict__ ref, int W,
                                                                   const float *__restrict__ valid_xy, int N, long long M,
                                                                   const float *__restrict__ dim_t, float *__restrict__ pe)
{
    __shared__ float e[4][2];
    const int tid = threadIdx.x;
    const long long m0 = (long long)blockIdx.x * 4;
    if (tid < 8) {
        const long long m = m0 + (tid >> 1);
        e[tid >> 1][tid & 1] = m < M ? dn_axis_embed(ref, W, valid_xy, N, m, tid & 1) : 0.f;
    }
    __syncthreads();
    const int row = tid >> 6, q = tid & 63, i = (q & 31) * 2;
    const long long m = m0 + row;
    if (m >= M) return;
    const float a = e[row][q < 32 ? 1 : 0];                         // y first
    reinterpret_cast<float4 *>(pe)[m * (kDnWidth / 4) + q] = dn_quad(a, dim_t[i], dim_t[i + 1]);
}

// ---- table -> Linear -> ReLU -> Linear in one launch ----------------------------------------------------------------------
// 512 threads = 8 wavefronts as 2 (rows of 32) x 4 (columns of 64); a wavefront holds two 32 x 32 accumulators.  LDS: the
// panel [64][256 + 4] (66 560 B: the table, then h) and the double-buffered stage of a weight, [2][256][32 + 4] (73 728 B): one
// workgroup per CU.  The 16 stages of 32 reduction columns (8 of W1, 8 of W2) run as one stream: the loads of stage s + 1 are
// in flight during the MFMAs of stage s, one barrier per stage.  Row strides 260 and 36 floats: 16-byte aligned and odd in
// units of 4 banks, so the 16-byte fragment reads of a half wavefront do not collide (msda_gemm.hip).
constexpr int kQpBlock = 512, kQpRows = 64, kQpStage = 32;
constexpr int kQpRowP = kDnWidth + 4, kQpRowB = kQpStage + 4;
constexpr int kQpStages = kDnWidth / kQpStage;
using f32x16 = __attribute__((ext_vector_type(16))) float;

__global__ __launch_bounds__(kQpBlock) void dino_query_pos_kernel(
    const float *__restrict__ ref, int W, const float *__restrict__ valid_xy, int N, long long M, const float *__restrict__ dim_t,
    const float *__restrict__ w1, const float *__restrict__ b1, const float *__restrict__ w2, const float *__restrict__ b2,
    float *__restrict__ h, float *__restrict__ y)
{
    __shared__ __attribute__((aligned(16))) float P[kQpRows * kQpRowP];
    __shared__ __attribute__((aligned(16))) float Bs[2][kDnWidth * kQpRowB];
    __shared__ float e[kQpRows][2];
    __shared__ float dt[64];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int i0 = (wave >> 2) * 32, j0 = (wave & 3) * 64, g = lane >> 5, c = lane & 31;
    const long long m0 = (long long)blockIdx.x * kQpRows;
    // staging of a weight stage: 256 rows x 8 float4, 4 per thread
    const int krow = tid >> 3, kcol = (tid & 7) * 4;
    float4 rb0, rb1, rb2, rb3;
#define DN_LOAD_B(s_)                                                                                               \
    do {                                                                                                            \
        const float *wsrc = ((s_) < kQpStages ? w1 : w2) + krow * kDnWidth + ((s_) & (kQpStages - 1)) * kQpStage + kcol; \
        rb0 = *reinterpret_cast<const float4 *>(wsrc);                                                              \
        rb1 = *reinterpret_cast<const float4 *>(wsrc + 64 * kDnWidth);                                              \
        rb2 = *reinterpret_cast<const float4 *>(wsrc + 128 * kDnWidth);                                             \
        rb3 = *reinterpret_cast<const float4 *>(wsrc + 192 * kDnWidth);                                             \
    } while (0)
#define DN_STORE_B(buf_)                                                                                            \
    do {                                                                                                            \
        float *bdst = &Bs[buf_][krow * kQpRowB + kcol];                                                             \
        *reinterpret_cast<float4 *>(bdst) = rb0;                                                                    \
        *reinterpret_cast<float4 *>(bdst + 64 * kQpRowB) = rb1;                                                     \
        *reinterpret_cast<float4 *>(bdst + 128 * kQpRowB) = rb2;                                                    \
        *reinterpret_cast<float4 *>(bdst + 192 * kQpRowB) = rb3;                                                    \
    } while (0)
    DN_LOAD_B(0);
    if (tid < 64) dt[tid] = dim_t[tid];
    if (tid < 2 * kQpRows) {
        const long long m = m0 + (tid >> 1);
        e[tid >> 1][tid & 1] = m < M ? dn_axis_embed(ref, W, valid_xy, N, m, tid & 1) : 0.f;   // rows >= M: never stored
    }
    __syncthreads();
    // the panel's table: 64 rows x 64 quads, 8 per thread
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        const int idx = tid + kQpBlock * u, row = idx >> 6, q = idx & 63, i = (q & 31) * 2;
        *reinterpret_cast<float4 *>(&P[row * kQpRowP + 4 * q]) = dn_quad(e[row][q < 32 ? 1 : 0], dt[i], dt[i + 1]);
    }
    DN_STORE_B(0);
    __syncthreads();

    f32x16 acc0, acc1;
#pragma unroll
    for (int r = 0; r < 16; ++r) { acc0[r] = 0.f; acc1[r] = 0.f; }
    int cur = 0;
    for (int s = 0; s < 2 * kQpStages; ++s) {
        const bool more = s + 1 < 2 * kQpStages;                    // uniform
        if (more) DN_LOAD_B(s + 1);
        if (s == kQpStages) {
            // every wavefront is past the barrier of stage 7: nobody reads the table any more.  h = relu(acc + b1) replaces
            // it (C/D layout of 32x32x2: column c, row (r & 3) + 8 (r >> 2) + 4 g; ReLU keeps NaN as torch.relu does) and
            // goes to memory, its only write.
#pragma unroll
            for (int half = 0; half < 2; ++half) {
                const int j = j0 + 32 * half + c;
                const float bj = b1[j];
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = i0 + (r & 3) + 8 * (r >> 2) + 4 * g;
                    float v = (half ? acc1[r] : acc0[r]) + bj;
                    v = v < 0.f ? 0.f : v;
                    P[row * kQpRowP + j] = v;
                    if (m0 + row < M) h[(m0 + row) * kDnWidth + j] = v;
                }
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) { acc0[r] = 0.f; acc1[r] = 0.f; }
            __syncthreads();
        }
        const int k0 = (s & (kQpStages - 1)) * kQpStage;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            // lane (c, g) owns reduction indices 8 i + 4 g + t of the stage, t = 0..3 feeding 4 MFMAs per accumulator
            const float4 a = *reinterpret_cast<const float4 *>(&P[(i0 + c) * kQpRowP + k0 + 8 * i + 4 * g]);
            const float4 p = *reinterpret_cast<const float4 *>(&Bs[cur][(j0 + c) * kQpRowB + 8 * i + 4 * g]);
            const float4 q = *reinterpret_cast<const float4 *>(&Bs[cur][(j0 + 32 + c) * kQpRowB + 8 * i + 4 * g]);
            acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, p.x, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, q.x, acc1, 0, 0, 0);
            acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, p.y, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, q.y, acc1, 0, 0, 0);
            acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, p.z, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, q.z, acc1, 0, 0, 0);
            acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, p.w, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, q.w, acc1, 0, 0, 0);
        }
        if (more) DN_STORE_B(cur ^ 1);                               // its readers are behind the barrier of stage s - 1
        __syncthreads();
        cur ^= 1;
    }
#undef DN_LOAD_B
#undef DN_STORE_B
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        const int j = j0 + 32 * half + c;
        const float bj = b2[j];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const long long i = m0 + i0 + (r & 3) + 8 * (r >> 2) + 4 * g;
            if (i < M) y[i * kDnWidth + j] = (half ? acc1[r] : acc0[r]) + bj;
        }
    }
}

// ---- refinement -----------------------------------------------------------------------------------------------------------
// torch.argmax over K contiguous logits: first maximum, the first NaN above every number (msda_two_stage_select_f32)
__device__ __forceinline__ int dn_argmax(const float *p, int K)
{
    float mx = p[0];
    int arg = 0;
    for (int k = 1; k < K && mx == mx; ++k) {
        const float v = p[k];
        if (v != v || v > mx) { mx = v; arg = k; }
    }
    return arg;
}

// 256 rows per workgroup: a thread classifies one row, then the workgroup walks the rows' 42 columns in memory order
__global__ __launch_bounds__(kDnBlock) void dino_refine_fwd_kernel(
    const float *__restrict__ ref, const float *__restrict__ cls, int K, const float *__restrict__ dkey,
    const float *__restrict__ dobj, int hand0, int hand1, long long M, float *__restrict__ out, uint8_t *__restrict__ code)
{
    __shared__ uint8_t cd[kDnBlock];
    const int tid = threadIdx.x;
    const long long r0 = (long long)blockIdx.x * kDnBlock;
    const int rows = (int)((M - r0) < kDnBlock ? (M - r0) : kDnBlock);
    if (tid < rows) {
        const int cl = dn_argmax(cls + (r0 + tid) * K, K);
        const uint8_t v = (cl == hand0 || cl == hand1) ? 2 : (cl != 0 ? 1 : 0);
        cd[tid] = v;
        code[r0 + tid] = v;
    }
    __syncthreads();
    for (int t = tid; t < rows * 42; t += kDnBlock) {
        const long long o = r0 * 42 + t;
        const int k = cd[t / 42];
        float u = inverse_sigmoid_f32(ref[o]);
        if (k == 1) u += dobj[o];
        if (k == 2) u += dkey[o];
        out[o] = dn_sigmoid(u) * 2.f - 1.f;
    }
}

__global__ __launch_bounds__(kDnBlock) void dino_refine_bwd_kernel(
    const float *__restrict__ gout, const float *__restrict__ out, const uint8_t *__restrict__ code, long long total,
    float *__restrict__ gkey, float *__restrict__ gobj)
{
    const long long o = (long long)blockIdx.x * kDnBlock + threadIdx.x;
    if (o >= total) return;
    const int k = code[o / 42];
    const float v = out[o];
    const float gu = gout[o] * (1.f - v * v) / 2.f;
    if (gkey != nullptr) gkey[o] = k == 2 ? gu : 0.f;
    if (gobj != nullptr) gobj[o] = k == 1 ? gu : 0.f;
}

}  // namespace

int launch_dino_sine_embed(const float *ref, int width, const float *valid_xy, int N, long long M, const float *dim_t, float *pe,
                           hipStream_t stream)
{
    if (M == 0) return MSDA_OK;
    hipLaunchKernelGGL(dino_sine_embed_kernel, dim3((unsigned)((M + 3) / 4)), dim3(kDnBlock), 0, stream, ref, width, valid_xy, N, M,
                       dim_t, pe);
    return check_launch("dino_sine_embed_kernel");
}

int launch_dino_query_pos(const float *ref, int width, const float *valid_xy, int N, long long M, const float *dim_t, const float *w1,
                          const float *b1, const float *w2, const float *b2, float *h, float *y, hipStream_t stream)
{
    if (M == 0) return MSDA_OK;
    hipLaunchKernelGGL(dino_query_pos_kernel, dim3((unsigned)((M + kQpRows - 1) / kQpRows)), dim3(kQpBlock), 0, stream, ref, width,
                       valid_xy, N, M, dim_t, w1, b1, w2, b2, h, y);
    return check_launch("dino_query_pos_kernel");
}

int launch_dino_refine_fwd(const float *ref, const float *cls, int K, const float *dkey, const float *dobj, int hand0, int hand1,
                           long long M, float *out, uint8_t *code, hipStream_t stream)
{
    if (M == 0) return MSDA_OK;
    hipLaunchKernelGGL(dino_refine_fwd_kernel, dim3((unsigned)((M + kDnBlock - 1) / kDnBlock)), dim3(kDnBlock), 0, stream, ref, cls, K,
                       dkey, dobj, hand0, hand1, M, out, code);
    return check_launch("dino_refine_fwd_kernel");
}

int launch_dino_refine_bwd(const float *gout, const float *out, const uint8_t *code, long long M, float *gkey, float *gobj,
                           hipStream_t stream)
{
    if (M == 0 || (gkey == nullptr && gobj == nullptr)) return MSDA_OK;
    const long long total = M * 42;
    hipLaunchKernelGGL(dino_refine_bwd_kernel, dim3((unsigned)((total + kDnBlock - 1) / kDnBlock)), dim3(kDnBlock), 0, stream, gout, out,
                       code, total, gkey, gobj);
    return check_launch("dino_refine_bwd_kernel");
}

}  // namespace msda
