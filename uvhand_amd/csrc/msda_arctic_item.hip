// The SmoothNet stage's query selection, get_arctic_item (UVHand arctic_tools/process.py:20-70): per frame, the object query
// (the sequential rule over the object classes 1 .. hand_idx[0] - 1: best_score starts at 0, a class replaces it when
// best_score < its max probability, strictly) and the two hand queries (argmax of their class probability), then the nine
// gathered rows.  One workgroup per frame forward; one backward launch that writes every element of the six source gradients
// (a row picked by both hands receives both gradients, left first).
//
// Probabilities are torch's sigmoid, 1 / (1 + exp(-x)) in fp32: they saturate to 1.0f for logits above about 17, so the
// argmax compares probabilities, not logits, and ties go to the lowest query index (torch.max / argmax).  A NaN probability
// wins the argmax (the first NaN); as an object score it never passes `best_score < score`.  No atomics: deterministic.
#include <cmath>
#include <cstdint>

#include "msda_common.h"
#include "msda_launch.h"

namespace msda {

namespace {

constexpr int kAiBlock = 256, kAiSources = 6, kAiOutputs = 9;
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

// (value, index) pairs ordered as torch's max reduction orders them: NaN first, then larger, then lower index
__device__ __forceinline__ bool ai_better(float va, int ia, float vb, int ib)
{
    const bool na = va != va, nb = vb != vb;
    if (na != nb) return na;
    if (!na && va != vb) return va > vb;
    return ia < ib;
}

__global__ __launch_bounds__(kAiBlock) void arctic_item_fwd_kernel(AiFwdArgs a)
{
    __shared__ float sv[kAiBlock];
    __shared__ int si[kAiBlock];
    __shared__ int pick[3];
    const int b = blockIdx.x, tid = threadIdx.x;
    const float *lg = a.logits + (long long)b * a.Q * a.K;
    float best_score = 0.f;
    int obj = 0;
    for (int k = 1; k < a.obj_end + 2; ++k) {
        const int cls = k < a.obj_end ? k : (k == a.obj_end ? a.hand_l : a.hand_r);
        float v = 0.f;
        int vi = 0x7fffffff;
        for (int q = tid; q < a.Q; q += kAiBlock) {
            const float p = 1.f / (1.f + expf(-lg[(long long)q * a.K + cls]));
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
            if (k < a.obj_end) {
                if (best_score < sv[0]) { obj = si[0]; best_score = sv[0]; }
            } else {
                pick[k - a.obj_end] = si[0];
            }
        }
        __syncthreads();
    }
    if (tid == 0) {
        pick[2] = obj;
        a.idx[3 * b] = pick[0];
        a.idx[3 * b + 1] = pick[1];
        a.idx[3 * b + 2] = obj;
    }
    __syncthreads();
    for (int o = 0; o < kAiOutputs; ++o) {
        const int w = kAiWidth[kAiOutSrc[o]];
        if (tid < w) a.out[o][(long long)b * w + tid] = a.src[kAiOutSrc[o]][((long long)b * a.Q + pick[kAiOutWho[o]]) * w + tid];
    }
}

__global__ __launch_bounds__(kAiBlock) void arctic_item_bwd_kernel(AiBwdArgs a)
{
    const int b = blockIdx.x, tid = threadIdx.x;
    const int64_t *idx = a.idx + 3 * b;
    for (int s = 0; s < kAiSources; ++s) {
        const int w = kAiWidth[s];
        for (int e = tid; e < a.Q * w; e += kAiBlock) {
            const int q = e / w, c = e - q * w;
            float v = 0.f;
            for (int o = 0; o < kAiOutputs; ++o)
                if (kAiOutSrc[o] == s && a.gout[o] != nullptr && idx[kAiOutWho[o]] == q) v += a.gout[o][(long long)b * w + c];
            a.gsrc[s][(long long)b * a.Q * w + e] = v;
        }
    }
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

}  // extern "C"
