// The AssemblyHands DeformableTransformer (UVHand models/assembly_transformer.py:23-251, :387-465): the arithmetic that the
// reference writes with boolean-mask indexing (a nonzero, hence a device -> host sync, per use), as plain launches:
//
//   refine      the decoder's keypoint refinement (:407-465), one thread per query: hand = argmax(cls) != 0 (first maximum;
//               NaN ranks highest); base = inverse_sigmoid(r) for 2-d refpoints, inverse_sigmoid(((mean x, mean y) + 0.5) / 2)
//               for 42-d ones (means over the 21 even / odd columns); hand rows add the (x, y) of each of the 21 (x, y, z)
//               triples of the keypoint head; out = sigmoid(.) * 2 - 0.5, [N, Q, 42].  One launch per decoder layer.
//   proposals   gen_encoder_output_proposals (:106-141) on ONE level (the forward passes the last, :184): valid extent off
//               the mask's first column / first row, the 2-d proposal (pixel centre / valid extent), its logit with +inf at
//               padded rows and rows outside (0.01, 0.99), memory with those rows zeroed and a byte mask of them.  Reads the
//               level's rows in place from the full [N, S, C] tensors (frame strides given), so the slice is never copied.
//   select      the two-stage selection (:202-226), one workgroup per frame: per class the torch.max over rows; the object
//               row by the reference's loop (best 0, index 0; classes obj_first..obj_last in order; update on best < score
//               only); left / right = argmax of their class columns; reference_points [N, 3, 2] = the means of sigmoid over
//               the x and y columns of the three gathered 63-d rows (left and right from the hand head, the object from
//               the object head).
//
// The proposal logits take logf of the fp32 ratio (within an ulp of torch.log's on the device, see the kernel).
// inverse_sigmoid is util/misc.py:614-618 (clamp to [0, 1], both sides floored at 1e-5, log of the ratio) with torch's
// NaN-propagating clamp; sigmoid is torch's 1 / (1 + exp(-x)); plain fp32, no fast-math.  Means multiply the sum by the
// fp32 reciprocal of the count, as torch's mean does.
#include "msda_common.h"
#include "msda_launch.h"

namespace msda {

constexpr int kAsBlock = 256;
constexpr int kKeypoints = 21;

__device__ __forceinline__ float as_sigmoid(float x) { return 1.f / (1.f + expf(-x)); }

__device__ __forceinline__ float as_clamp(float x, float lo, float hi)
{
    return x != x ? x : fminf(fmaxf(x, lo), hi);
}

__device__ __forceinline__ float as_inverse_sigmoid(float x)
{
    x = as_clamp(x, 0.f, 1.f);
    const float x1 = x != x ? x : fmaxf(x, 1e-5f);
    const float one_minus = 1.f - x;
    const float x2 = one_minus != one_minus ? one_minus : fmaxf(one_minus, 1e-5f);
    return logf(x1 / x2);
}

// torch.argmax over k contiguous logits: first maximum, the first NaN above every number
__device__ __forceinline__ int as_argmax(const float *p, int K)
{
    float mx = p[0];
    int arg = 0;
    for (int k = 1; k < K && mx == mx; ++k) {
        const float v = p[k];
        if (v != v || v > mx) { mx = v; arg = k; }
    }
    return arg;
}

// ---- refinement -------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kAsBlock) void refine_kernel(const float *__restrict__ ref, int W, const float *__restrict__ cls,
                                                          int K, const float *__restrict__ kp, long long M,
                                                          float *__restrict__ out)
{
    const long long m = (long long)blockIdx.x * kAsBlock + threadIdx.x;
    if (m >= M) return;
    const bool hand = as_argmax(cls + m * K, K) != 0;
    const float *r = ref + m * W;
    float bx, by;
    if (W == 2) {
        bx = as_inverse_sigmoid(r[0]);
        by = as_inverse_sigmoid(r[1]);
    } else {
        float sx = 0.f, sy = 0.f;
        for (int j = 0; j < kKeypoints; ++j) { sx += r[2 * j]; sy += r[2 * j + 1]; }
        const float inv = 1.f / (float)kKeypoints;
        bx = as_inverse_sigmoid((sx * inv + 0.5f) / 2.f);
        by = as_inverse_sigmoid((sy * inv + 0.5f) / 2.f);
    }
    const float *t = kp + m * (3 * kKeypoints);
    float *o = out + m * (2 * kKeypoints);
    for (int j = 0; j < kKeypoints; ++j) {
        const float x = hand ? bx + t[3 * j] : bx;
        const float y = hand ? by + t[3 * j + 1] : by;
        o[2 * j] = as_sigmoid(x) * 2.f - 0.5f;
        o[2 * j + 1] = as_sigmoid(y) * 2.f - 0.5f;
    }
}

int launch_assembly_refine(const float *ref, int width, const float *cls, int K, const float *kp, long long M, float *out,
                           hipStream_t stream)
{
    if (M == 0) return MSDA_OK;
    hipLaunchKernelGGL(refine_kernel, dim3((unsigned)((M + kAsBlock - 1) / kAsBlock)), dim3(kAsBlock), 0, stream, ref, width, cls,
                       K, kp, M, out);
    return check_launch("assembly_refine_kernel");
}

// ---- proposals of one level -------------------------------------------------------------------------------------------
// grid (ceil(H*W / 256), N); one thread per row for the proposal, the workgroup together for the memory copy.
__global__ __launch_bounds__(kAsBlock) void level_proposals_kernel(
    const float *__restrict__ memory, long long mem_frame_stride, const uint8_t *__restrict__ pad, long long pad_frame_stride,
    int H, int W, int C, float *__restrict__ proposals, float *__restrict__ memory_out, uint8_t *__restrict__ row_mask)
{
    __shared__ int vh, vw;
    __shared__ uint8_t dead[kAsBlock];
    const int n = blockIdx.y, tid = threadIdx.x, S = H * W;
    const uint8_t *pm = pad + (long long)n * pad_frame_stride;
    if (tid == 0) { vh = 0; vw = 0; }
    __syncthreads();
    // valid_H = unpadded rows of the first column, valid_W = unpadded columns of the first row (:118-119)
    int ch = 0, cw = 0;
    for (int h = tid; h < H; h += kAsBlock) ch += pm[h * W] == 0;
    for (int w = tid; w < W; w += kAsBlock) cw += pm[w] == 0;
    if (ch) atomicAdd(&vh, ch);
    if (cw) atomicAdd(&vw, cw);
    __syncthreads();
    const int s = blockIdx.x * kAsBlock + tid;
    bool zero = false;
    if (s < S) {
        const int h = s / W, w = s % W;
        const float px = ((float)w + 0.5f) / (float)vw;
        const float py = ((float)h + 0.5f) / (float)vh;
        const bool valid = px > 0.01f && px < 0.99f && py > 0.01f && py < 0.99f;
        zero = pm[s] != 0 || !valid;
        float *out = proposals + ((long long)n * S + s) * 2;
        const float inf = __builtin_inff();
        // the fp32 ratio as torch forms it and logf, as msda_two_stage.hip's proposals take it.  Over every ratio of the valid
        // extents 1 .. 599 logf is within one ulp of torch.log on the device (equal on 67 %); the correctly rounded log of the
        // ratio, which this kernel wrote before, is two ulps from torch's on 1.4 % of them (none below an extent of 13)
        out[0] = zero ? inf : logf(px / (1.f - px));
        out[1] = zero ? inf : logf(py / (1.f - py));
        row_mask[(long long)n * S + s] = zero ? 1 : 0;
    }
    dead[tid] = zero ? 1 : 0;
    __syncthreads();
    const int rows = min(kAsBlock, S - (int)blockIdx.x * kAsBlock);
    const int per_row = C / 4;
    const long long r0 = (long long)blockIdx.x * kAsBlock;
    const float4 *src4 = reinterpret_cast<const float4 *>(memory + (long long)n * mem_frame_stride + r0 * C);
    float4 *dst4 = reinterpret_cast<float4 *>(memory_out + ((long long)n * S + r0) * C);
    for (int e = tid; e < rows * per_row; e += kAsBlock) {
        const int r = e / per_row;
        dst4[e] = dead[r] ? make_float4(0.f, 0.f, 0.f, 0.f) : src4[e];
    }
}

int launch_assembly_level_proposals(const float *memory, long long mem_frame_stride, const uint8_t *pad, long long pad_frame_stride,
                                    int N, int H, int W, int C, float *proposals, float *memory_out, uint8_t *row_mask,
                                    hipStream_t stream)
{
    if (N == 0) return MSDA_OK;
    const int S = H * W;
    hipLaunchKernelGGL(level_proposals_kernel, dim3((unsigned)((S + kAsBlock - 1) / kAsBlock), (unsigned)N), dim3(kAsBlock), 0, stream,
                       memory, mem_frame_stride, pad, pad_frame_stride, H, W, C, proposals, memory_out, row_mask);
    return check_launch("assembly_level_proposals_kernel");
}

// ---- selection --------------------------------------------------------------------------------------------------------
constexpr int kAsSelClasses = kAssemblySelMaxObj + 2;   // classes a selection reduces over: obj_first..obj_last, left, right

// (a, ia) ranks above (b, ib) as torch.max / argmax over rows decides: NaN first, then the larger value, then the lower row
__device__ __forceinline__ bool as_better(float a, int ia, float b, int ib)
{
    const bool na = a != a, nb = b != b;
    if (na || nb) return na && (!nb || ia < ib);
    return a > b || (a == b && ia < ib);
}

__global__ __launch_bounds__(kAsBlock) void assembly_select_kernel(
    const float *__restrict__ cls, const float *__restrict__ hand, const float *__restrict__ obj, int S, int K, int obj_first,
    int obj_last, int left, int right, int64_t *__restrict__ indices, float *__restrict__ refp)
{
    __shared__ float sv[kAsBlock];
    __shared__ int si[kAsBlock];
    __shared__ float best_v[kAsSelClasses];
    __shared__ int best_i[kAsSelClasses];
    __shared__ int picked[3];
    const int n = blockIdx.x, tid = threadIdx.x;
    const int n_obj = obj_last - obj_first + 1, n_cls = n_obj + 2;
    const float *c = cls + (long long)n * S * K;
    for (int j = 0; j < n_cls; ++j) {
        const int k = j < n_obj ? obj_first + j : (j == n_obj ? left : right);
        float v = 0.f;
        int iv = -1;                                           // no row yet
        for (int s = tid; s < S; s += kAsBlock) {
            const float x = c[(long long)s * K + k];
            if (iv < 0 || as_better(x, s, v, iv)) { v = x; iv = s; }
        }
        sv[tid] = v;
        si[tid] = iv;
        __syncthreads();
        for (int half = kAsBlock / 2; half > 0; half >>= 1) {
            if (tid < half) {
                const float b = sv[tid + half];
                const int ib = si[tid + half];
                if (ib >= 0 && (si[tid] < 0 || as_better(b, ib, sv[tid], si[tid]))) { sv[tid] = b; si[tid] = ib; }
            }
            __syncthreads();
        }
        if (tid == 0) { best_v[j] = sv[0]; best_i[j] = si[0]; }
        __syncthreads();
    }
    if (tid == 0) {
        float best = 0.f;
        int oi = 0;
        for (int j = 0; j < n_obj; ++j)
            if (best < best_v[j]) { best = best_v[j]; oi = best_i[j]; }
        picked[0] = best_i[n_obj];
        picked[1] = best_i[n_obj + 1];
        picked[2] = oi;
        if (indices != nullptr)
            for (int q = 0; q < 3; ++q) indices[(long long)n * 3 + q] = picked[q];
    }
    __syncthreads();
    if (tid < 6) {                                              // (query, axis): mean of sigmoid over the 21 keypoints
        const int q = tid >> 1, axis = tid & 1;
        const float *row = (q == 2 ? obj : hand) + ((long long)n * S + picked[q]) * (3 * kKeypoints);
        float sum = 0.f;
        for (int j = 0; j < kKeypoints; ++j) sum += as_sigmoid(row[3 * j + axis]);
        refp[((long long)n * 3 + q) * 2 + axis] = sum * (1.f / (float)kKeypoints);
    }
}

int launch_assembly_select(const float *cls, const float *hand, const float *obj, int N, int S, int K, int obj_first, int obj_last,
                           int left, int right, int64_t *indices, float *refp, hipStream_t stream)
{
    if (N == 0) return MSDA_OK;
    hipLaunchKernelGGL(assembly_select_kernel, dim3((unsigned)N), dim3(kAsBlock), 0, stream, cls, hand, obj, S, K, obj_first, obj_last,
                       left, right, indices, refp);
    return check_launch("assembly_select_kernel");
}

}  // namespace msda
