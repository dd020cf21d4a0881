// The SmoothNet stage's query selection, get_arctic_item (UVHand arctic_tools/process.py:20-70): per frame, the object query
// (the sequential rule over the object classes 1 .. hand_idx[0] - 1: best_score starts at 0, a class replaces it when
// best_score < its max probability, strictly) and the two hand queries (argmax of their class probability), then the nine
// gathered rows.  One workgroup per frame forward; one backward launch that writes every element of the six source gradients
// (a row picked by both hands receives both gradients, left first).
//
// Probabilities are torch's sigmoid, 1 / (1 + exp(-x)) in fp32: they saturate to 1.0f for logits above about 17, so the
// argmax compares probabilities, not logits, and ties go to the lowest query index (torch.max / argmax).  A NaN probability
// wins the argmax (the first NaN); as an object score it never passes `best_score < score`.  No atomics: deterministic.
//
// The grouped entries (msda_arctic_item_many_*) run the same two device functions for up to kAiMaxSets prediction sets in one
// launch, grid (bs, n_sets), on fp32 or bf16 sources (ST = float / uint16_t bits).  bf16 rows are 3, 3, 48, 10, 1 and 3 values
// wide, so only 2-byte aligned: every source access is one element.  Outputs are fp32 (bf16 widened exactly); a bf16 source
// gradient is the fp32 sum of its row's gradients rounded once, to nearest even.
#include <cmath>
#include <cstdint>

#include "msda_common.h"
#include "msda_launch.h"

namespace msda {

namespace {

constexpr int kAiBlock = 256, kAiSources = 6, kAiOutputs = 9, kAiMaxSets = 8;
// source tensors [bs, Q, w]: hand_cam, obj_cam, mano_pose, mano_shape, obj_rad, obj_rot
constexpr int kAiWidth[kAiSources] = {3, 3, 48, 10, 1, 3};
// outputs in the reference's order: root_l, root_r, root_o, pose_l, pose_r, shape_l, shape_r, obj_rot, obj_rad; their source
// and the query they take (0 left hand, 1 right hand, 2 object)
constexpr int kAiOutSrc[kAiOutputs] = {0, 0, 1, 2, 2, 3, 3, 5, 4};
constexpr int kAiOutWho[kAiOutputs] = {0, 1, 2, 0, 1, 0, 1, 2, 2};

struct AiFwdArgs {
    const float *logits;
    const float *src[kAiSources];
    float *out[kAiOutputs];
    int64_t *idx;                   // [bs, 3]: left, right, object
    int Q, K, obj_end, hand_l, hand_r;
};
struct AiBwdArgs {
    const int64_t *idx;
    const float *gout[kAiOutputs];  // null: no gradient
    float *gsrc[kAiSources];
    int Q;
};
// the grouped launch: set s owns logits[s], src[6 s ..], out[9 s ..], idx[s * bs * 3 ..], gout[9 s ..], gsrc[6 s ..]
struct AiManyFwdArgs {
    const float *logits[kAiMaxSets];
    const void *src[kAiMaxSets * kAiSources];
    float *out[kAiMaxSets * kAiOutputs];
    int64_t *idx;                   // [n_sets, bs, 3]
    int bs, Q, K, obj_end, hand_l, hand_r;
};
struct AiManyBwdArgs {
    const int64_t *idx;
    const float *gout[kAiMaxSets * kAiOutputs];   // null: no gradient
    void *gsrc[kAiMaxSets * kAiSources];
    int bs, Q;
};
static_assert(sizeof(AiManyFwdArgs) <= 2000 && sizeof(AiManyBwdArgs) <= 2000, "kernel argument tables");

__device__ __forceinline__ float ai_load(const float *p, long long e) { return p[e]; }
__device__ __forceinline__ float ai_load(const uint16_t *p, long long e) { return __uint_as_float((unsigned)p[e] << 16); }
__device__ __forceinline__ void ai_store(float *p, long long e, float v) { p[e] = v; }
__device__ __forceinline__ void ai_store(uint16_t *p, long long e, float v) { p[e] = __builtin_bit_cast(uint16_t, (__bf16)v); }

// (value, index) pairs ordered as torch's max reduction orders them: NaN first, then larger, then lower index
__device__ __forceinline__ bool ai_better(float va, int ia, float vb, int ib)
{
    const bool na = va != va, nb = vb != vb;
    if (na != nb) return na;
    if (!na && va != vb) return va > vb;
    return ia < ib;
}

// One frame of one set: frame b's logits lg [Q, K], the six sources [bs, Q, w] of type ST, the nine fp32 outputs [bs, w] and
// the frame's idx [3].  The whole workgroup calls it.
template <typename ST>
__device__ __forceinline__ void ai_forward_frame(const float *lg, const ST *const *src, float *const *out, int64_t *idx, int b,
                                                 int Q, int K, int obj_end, int hand_l, int hand_r)
{
    __shared__ float sv[kAiBlock];
    __shared__ int si[kAiBlock];
    __shared__ int pick[3];
    const int tid = threadIdx.x;
    float best_score = 0.f;
    int obj = 0;
    for (int k = 1; k < obj_end + 2; ++k) {
        const int cls = k < obj_end ? k : (k == obj_end ? hand_l : hand_r);
        float v = 0.f;
        int vi = 0x7fffffff;
        for (int q = tid; q < Q; q += kAiBlock) {
            const float p = 1.f / (1.f + expf(-lg[(long long)q * K + cls]));
            if (vi == 0x7fffffff || ai_better(p, q, v, vi)) { v = p; vi = q; }
        }
        sv[tid] = v;
        si[tid] = vi;
        __syncthreads();
        for (int h = kAiBlock / 2; h > 0; h >>= 1) {
            if (tid < h && si[tid + h] != 0x7fffffff && (si[tid] == 0x7fffffff || ai_better(sv[tid + h], si[tid + h], sv[tid], si[tid]))) {
                sv[tid] = sv[tid + h];
                si[tid] = si[tid + h];
            }
            __syncthreads();
        }
        if (tid == 0) {
            if (k < obj_end) {
                if (best_score < sv[0]) { obj = si[0]; best_score = sv[0]; }
            } else {
                pick[k - obj_end] = si[0];
            }
        }
        __syncthreads();
    }
    if (tid == 0) {
        pick[2] = obj;
        idx[0] = pick[0];
        idx[1] = pick[1];
        idx[2] = obj;
    }
    __syncthreads();
    for (int o = 0; o < kAiOutputs; ++o) {
        const int w = kAiWidth[kAiOutSrc[o]];
        if (tid < w) out[o][(long long)b * w + tid] = ai_load(src[kAiOutSrc[o]], ((long long)b * Q + pick[kAiOutWho[o]]) * w + tid);
    }
}

// Frame b of one set's six source gradients [bs, Q, w] of type ST from the nine fp32 output gradients (null: none): every
// element written; the sum runs in fp32 in output order (left hand first) and is stored once.
template <typename ST>
__device__ __forceinline__ void ai_backward_frame(const int64_t *idx, const float *const *gout, ST *const *gsrc, int b, int Q)
{
    const int tid = threadIdx.x;
    for (int s = 0; s < kAiSources; ++s) {
        const int w = kAiWidth[s];
        for (int e = tid; e < Q * w; e += kAiBlock) {
            const int q = e / w, c = e - q * w;
            float v = 0.f;
            for (int o = 0; o < kAiOutputs; ++o)
                if (kAiOutSrc[o] == s && gout[o] != nullptr && idx[kAiOutWho[o]] == q) v += gout[o][(long long)b * w + c];
            ai_store(gsrc[s], (long long)b * Q * w + e, v);
        }
    }
}

__global__ __launch_bounds__(kAiBlock) void arctic_item_fwd_kernel(AiFwdArgs a)
{
    const int b = blockIdx.x;
    ai_forward_frame<float>(a.logits + (long long)b * a.Q * a.K, a.src, a.out, a.idx + 3 * b, b, a.Q, a.K, a.obj_end, a.hand_l,
                            a.hand_r);
}

__global__ __launch_bounds__(kAiBlock) void arctic_item_bwd_kernel(AiBwdArgs a)
{
    const int b = blockIdx.x;
    ai_backward_frame<float>(a.idx + 3 * b, a.gout, a.gsrc, b, a.Q);
}

template <typename ST>
__global__ __launch_bounds__(kAiBlock) void arctic_item_many_fwd_kernel(AiManyFwdArgs a)
{
    const int b = blockIdx.x, s = blockIdx.y;
    ai_forward_frame<ST>(a.logits[s] + (long long)b * a.Q * a.K, reinterpret_cast<const ST *const *>(a.src + s * kAiSources),
                         a.out + s * kAiOutputs, a.idx + 3 * ((long long)s * a.bs + b), b, a.Q, a.K, a.obj_end, a.hand_l, a.hand_r);
}

template <typename ST>
__global__ __launch_bounds__(kAiBlock) void arctic_item_many_bwd_kernel(AiManyBwdArgs a)
{
    const int b = blockIdx.x, s = blockIdx.y;
    ai_backward_frame<ST>(a.idx + 3 * ((long long)s * a.bs + b), a.gout + s * kAiOutputs,
                          reinterpret_cast<ST *const *>(a.gsrc + s * kAiSources), b, a.Q);
}

void ai_begin()
{
    set_error(MSDA_OK, "");
    (void)hipGetLastError();
}

}  // namespace

}  // namespace msda

using namespace msda;

extern "C" {

int msda_arctic_item_forward_f32(int bs, int Q, int K, int obj_end, int hand_l, int hand_r, const float *logits,
                                 const float *const *sources, float *const *out, int64_t *idx, msda_stream_t stream)
{
    if (bs < 1 || Q < 1 || K < 1 || obj_end < 1 || obj_end > K || hand_l < 0 || hand_l >= K || hand_r < 0 || hand_r >= K
        || (long long)bs * Q * (K > 48 ? K : 48) >= (1LL << 31) || bs > 65535 * 1024)
        return set_error(MSDA_ERR_ARGUMENT, "msda_arctic_item_forward_f32: need bs, Q, K >= 1, 1 <= hand_idx[0] <= K, hand classes "
                                            "< K, bs * Q * max(K, 48) < 2^31");
    if (logits == nullptr || sources == nullptr || out == nullptr || idx == nullptr)
        return set_error(MSDA_ERR_ARGUMENT, "msda_arctic_item_forward_f32: null pointer");
    AiFwdArgs a{};
    a.logits = logits; a.idx = idx; a.Q = Q; a.K = K; a.obj_end = obj_end; a.hand_l = hand_l; a.hand_r = hand_r;
    for (int s = 0; s < kAiSources; ++s) {
        if (sources[s] == nullptr) return set_error(MSDA_ERR_ARGUMENT, "msda_arctic_item_forward_f32: null pointer");
        a.src[s] = sources[s];
    }
    for (int o = 0; o < kAiOutputs; ++o) {
        if (out[o] == nullptr) return set_error(MSDA_ERR_ARGUMENT, "msda_arctic_item_forward_f32: null pointer");
        a.out[o] = out[o];
    }
    ai_begin();
    hipLaunchKernelGGL(arctic_item_fwd_kernel, dim3((unsigned)bs), dim3(kAiBlock), 0, (hipStream_t)stream, a);
    return check_launch("arctic_item_fwd_kernel");
}

int msda_arctic_item_backward_f32(int bs, int Q, const int64_t *idx, const float *const *grad_out, float *const *grad_sources,
                                  msda_stream_t stream)
{
    if (bs < 1 || Q < 1 || (long long)bs * Q * 48 >= (1LL << 31))
        return set_error(MSDA_ERR_ARGUMENT, "msda_arctic_item_backward_f32: need bs, Q >= 1, bs * Q * 48 < 2^31");
    if (idx == nullptr || grad_out == nullptr || grad_sources == nullptr)
        return set_error(MSDA_ERR_ARGUMENT, "msda_arctic_item_backward_f32: null pointer");
    AiBwdArgs a{};
    a.idx = idx; a.Q = Q;
    for (int o = 0; o < kAiOutputs; ++o) a.gout[o] = grad_out[o];
    for (int s = 0; s < kAiSources; ++s) {
        if (grad_sources[s] == nullptr) return set_error(MSDA_ERR_ARGUMENT, "msda_arctic_item_backward_f32: null pointer");
        a.gsrc[s] = grad_sources[s];
    }
    ai_begin();
    hipLaunchKernelGGL(arctic_item_bwd_kernel, dim3((unsigned)bs), dim3(kAiBlock), 0, (hipStream_t)stream, a);
    return check_launch("arctic_item_bwd_kernel");
}

int msda_arctic_item_many_forward(int n_sets, int bs, int Q, int K, int obj_end, int hand_l, int hand_r, int src_bf16,
                                  const float *const *logits, const void *const *sources, float *const *out, int64_t *idx,
                                  msda_stream_t stream)
{
    if (n_sets < 1 || n_sets > kAiMaxSets)
        return set_error(MSDA_ERR_ARGUMENT, "msda_arctic_item_many_forward: need 1 <= n_sets <= 8");
    if (bs < 1 || Q < 1 || K < 1 || obj_end < 1 || obj_end > K || hand_l < 0 || hand_l >= K || hand_r < 0 || hand_r >= K
        || (long long)bs * Q * (K > 48 ? K : 48) >= (1LL << 31) || bs > 65535 * 1024)
        return set_error(MSDA_ERR_ARGUMENT, "msda_arctic_item_many_forward: need bs, Q, K >= 1, 1 <= hand_idx[0] <= K, hand classes "
                                            "< K, bs * Q * max(K, 48) < 2^31");
    if (logits == nullptr || sources == nullptr || out == nullptr || idx == nullptr)
        return set_error(MSDA_ERR_ARGUMENT, "msda_arctic_item_many_forward: null pointer");
    AiManyFwdArgs a{};
    a.idx = idx; a.bs = bs; a.Q = Q; a.K = K; a.obj_end = obj_end; a.hand_l = hand_l; a.hand_r = hand_r;
    for (int s = 0; s < n_sets; ++s) {
        if (logits[s] == nullptr) return set_error(MSDA_ERR_ARGUMENT, "msda_arctic_item_many_forward: null pointer");
        a.logits[s] = logits[s];
    }
    for (int i = 0; i < n_sets * kAiSources; ++i) {
        if (sources[i] == nullptr) return set_error(MSDA_ERR_ARGUMENT, "msda_arctic_item_many_forward: null pointer");
        a.src[i] = sources[i];
    }
    for (int i = 0; i < n_sets * kAiOutputs; ++i) {
        if (out[i] == nullptr) return set_error(MSDA_ERR_ARGUMENT, "msda_arctic_item_many_forward: null pointer");
        a.out[i] = out[i];
    }
    ai_begin();
    const dim3 grid((unsigned)bs, (unsigned)n_sets);
    if (src_bf16)
        hipLaunchKernelGGL(arctic_item_many_fwd_kernel<uint16_t>, grid, dim3(kAiBlock), 0, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL(arctic_item_many_fwd_kernel<float>, grid, dim3(kAiBlock), 0, (hipStream_t)stream, a);
    return check_launch("arctic_item_many_fwd_kernel");
}

int msda_arctic_item_many_backward(int n_sets, int bs, int Q, int src_bf16, const int64_t *idx, const float *const *grad_out,
                                   void *const *grad_sources, msda_stream_t stream)
{
    if (n_sets < 1 || n_sets > kAiMaxSets)
        return set_error(MSDA_ERR_ARGUMENT, "msda_arctic_item_many_backward: need 1 <= n_sets <= 8");
    if (bs < 1 || Q < 1 || (long long)bs * Q * 48 >= (1LL << 31) || bs > 65535 * 1024)
        return set_error(MSDA_ERR_ARGUMENT, "msda_arctic_item_many_backward: need bs, Q >= 1, bs * Q * 48 < 2^31");
    if (idx == nullptr || grad_out == nullptr || grad_sources == nullptr)
        return set_error(MSDA_ERR_ARGUMENT, "msda_arctic_item_many_backward: null pointer");
    AiManyBwdArgs a{};
    a.idx = idx; a.bs = bs; a.Q = Q;
    for (int i = 0; i < n_sets * kAiOutputs; ++i) a.gout[i] = grad_out[i];
    for (int i = 0; i < n_sets * kAiSources; ++i) {
        if (grad_sources[i] == nullptr) return set_error(MSDA_ERR_ARGUMENT, "msda_arctic_item_many_backward: null pointer");
        a.gsrc[i] = grad_sources[i];
    }
    ai_begin();
    const dim3 grid((unsigned)bs, (unsigned)n_sets);
    if (src_bf16)
        hipLaunchKernelGGL(arctic_item_many_bwd_kernel<uint16_t>, grid, dim3(kAiBlock), 0, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL(arctic_item_many_bwd_kernel<float>, grid, dim3(kAiBlock), 0, (hipStream_t)stream, a);
    return check_launch("arctic_item_many_bwd_kernel");
}

}  // extern "C"
