// The input-projection neck of DeformableDETR.forward (UVHand models/actic_detr.py:191-225, models/assembly_detr.py:145-171):
// per feature level  GroupNorm(groups, C)(conv(x) + bias) * (uniform > 0.3),  every level of a call in ONE launch forward and
// one launch plus a small reduce backward.  The convolution itself stays with the caller: the kernels take its output y
// WITHOUT the bias and add bias[c] on the way in, so that the bias gradient comes out of the same backward launch.
//
// Layout.  In NCHW one (frame, group) of GroupNorm is one contiguous run of (C / groups) * H * W floats.  One workgroup of
// four wavefronts owns it; wavefront w takes the group's channels w, w + 4, ... whole, so bias / gamma / beta are
// wave-uniform, no index is ever divided, and the per-channel sums of the backward are wave reductions.
//
// Forward, three passes over the group: (1) x = y + bias[c], its sum, and — when the group fits kNeckLdsFloats — a copy of x
// in LDS; (2) sum of (x - mean) and of (x - mean)^2, from LDS or, for a larger group, from y again (an L2 hit: the group was
// read a moment ago by the same workgroup); (3) the output.  The variance is the centred one, never E[x^2] - mean^2; the
// first-order sum corrects the fp32 rounding of the mean (mean += sum(x - mean) / n, var -= that^2), which makes the mean of
// a constant group exact: x - mean is then 0, not rounding noise times eps^-1/2.
//
// Reduction order (fixed, no atomics): a lane adds its elements in index order, the 64 lanes combine in a xor butterfly,
// the four wavefronts' totals add as (w0 + w1) + (w2 + w3).  Backward the same, and the sums over frames run in index
// order in neck_reduce_kernel.  Every result is bitwise reproducible.
//
// The mask is kept as one byte per element (1 = kept); the backward reads it instead of the uniforms.
#include <cstring>
#include <initializer_list>

#include "msda_common.h"
#include "msda_launch.h"

namespace msda {

constexpr int kNeckBlock = 256;
constexpr int kNeckWaves = kNeckBlock / kWave;
constexpr int kNeckLdsFloats = 8192;                 // 32 KiB: five workgroups per CU beside it
constexpr float kNeckThreshold = 0.3f;               // models/actic_detr.py:200,219

namespace {

template <int W> __device__ __forceinline__ void ldv(const float *p, float (&v)[W])
{
    if constexpr (W == 4) { const float4 t = *reinterpret_cast<const float4 *>(p); v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w; }
    else v[0] = *p;
}
template <int W> __device__ __forceinline__ void stv(float *p, const float (&v)[W])
{
    if constexpr (W == 4) *reinterpret_cast<float4 *>(p) = make_float4(v[0], v[1], v[2], v[3]);
    else *p = v[0];
}
// the mask bytes of W elements as factors 0.f / 1.f
template <int W> __device__ __forceinline__ void ldm(const unsigned char *p, float (&m)[W])
{
    if constexpr (W == 4) {
        const uint32_t t = *reinterpret_cast<const uint32_t *>(p);
#pragma unroll
        for (int k = 0; k < 4; ++k) m[k] = ((t >> (8 * k)) & 0xffu) ? 1.f : 0.f;
    } else m[0] = *p ? 1.f : 0.f;
}
template <int W> __device__ __forceinline__ void stm(unsigned char *p, const float (&m)[W])
{
    if constexpr (W == 4) {
        uint32_t t = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) t |= (m[k] != 0.f ? 1u : 0u) << (8 * k);
        *reinterpret_cast<uint32_t *>(p) = t;
    } else *p = m[0] != 0.f ? 1 : 0;
}

// Totals of two per-lane values over the workgroup, to every thread: butterfly inside a wavefront, then the four wavefronts
// through `red` in a fixed order.  Each call site has its own slot of `red`, so one barrier per call is enough.
__device__ __forceinline__ void block_sum2(float &a, float &b, float (*red)[2], int wave, int lane)
{
    a = wave_sum(a); b = wave_sum(b);
    if (lane == 0) { red[wave][0] = a; red[wave][1] = b; }
    __syncthreads();
    a = (red[0][0] + red[1][0]) + (red[2][0] + red[3][0]);
    b = (red[0][1] + red[1][1]) + (red[2][1] + red[3][1]);
}

// block -> (level, frame, group) from the prefix table (uniform)
__device__ __forceinline__ int level_of(const int *first_block, int L)
{
    int l = 0;
    while (l + 1 < L && (int)blockIdx.x >= first_block[l + 1]) ++l;
    return l;
}

template <int W>
__device__ __forceinline__ void neck_fwd_group(const NeckFwdPlan &plan, int l, int n, int g, int C, int groups, float eps,
                                               float *sx, float (*red)[kNeckWaves][2])
{
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int HW = plan.hw[l], cpg = C / groups, c0 = g * cpg, nv = HW / W;
    const long long base = ((long long)n * C + c0) * HW;
    const float *yb = plan.y[l] + base;
    const float *bias = plan.bias[l];
    const long long len = (long long)cpg * HW;
    const bool staged = len <= kNeckLdsFloats;
    const float inv_len = 1.f / (float)len;

    float s = 0.f, unused = 0.f;
    for (int cc = wave; cc < cpg; cc += kNeckWaves) {
        const float b = bias ? bias[c0 + cc] : 0.f;
        const float *yc = yb + (long long)cc * HW;
        for (int p = lane; p < nv; p += kWave) {
            float v[W];
            ldv<W>(yc + p * W, v);
#pragma unroll
            for (int k = 0; k < W; ++k) { v[k] += b; s += v[k]; }
            if (staged) stv<W>(sx + cc * HW + p * W, v);        // read back by this same lane only
        }
    }
    block_sum2(s, unused, red[0], wave, lane);
    float mean = s * inv_len;

    float d1 = 0.f, d2 = 0.f;
    for (int cc = wave; cc < cpg; cc += kNeckWaves) {
        const float b = bias ? bias[c0 + cc] : 0.f;
        const float *yc = yb + (long long)cc * HW;
        for (int p = lane; p < nv; p += kWave) {
            float v[W];
            if (staged) ldv<W>(sx + cc * HW + p * W, v);
            else {
                ldv<W>(yc + p * W, v);
#pragma unroll
                for (int k = 0; k < W; ++k) v[k] += b;
            }
#pragma unroll
            for (int k = 0; k < W; ++k) { const float d = v[k] - mean; d1 += d; d2 += d * d; }
        }
    }
    block_sum2(d1, d2, red[1], wave, lane);
    const float delta = d1 * inv_len;
    mean += delta;
    const float var = fmaxf(d2 * inv_len - delta * delta, 0.f);
    const float rstd = 1.f / sqrtf(var + eps);
    if (tid == 0) {
        plan.mean[l][(long long)n * groups + g] = mean;
        plan.rstd[l][(long long)n * groups + g] = rstd;
    }

    const float *ub = plan.u[l] ? plan.u[l] + base : nullptr;
    unsigned char *mb = plan.u[l] ? plan.mask[l] + base : nullptr;
    float *ob = plan.out[l] + base;
    for (int cc = wave; cc < cpg; cc += kNeckWaves) {
        const float b = bias ? bias[c0 + cc] : 0.f;
        const float ga = plan.gamma[l][c0 + cc], be = plan.beta[l][c0 + cc];
        const long long off = (long long)cc * HW;
        for (int p = lane; p < nv; p += kWave) {
            float v[W], o[W];
            if (staged) ldv<W>(sx + cc * HW + p * W, v);
            else {
                ldv<W>(yb + off + p * W, v);
#pragma unroll
                for (int k = 0; k < W; ++k) v[k] += b;
            }
#pragma unroll
            for (int k = 0; k < W; ++k) o[k] = (v[k] - mean) * rstd * ga + be;
            if (ub) {
                float u[W], m[W];
                ldv<W>(ub + off + p * W, u);
#pragma unroll
                for (int k = 0; k < W; ++k) { m[k] = u[k] > kNeckThreshold ? 1.f : 0.f; o[k] *= m[k]; }
                stm<W>(mb + off + p * W, m);
            }
            stv<W>(ob + off + p * W, o);
        }
    }
}

template <int W>
__device__ __forceinline__ void neck_bwd_group(const NeckBwdPlan &plan, int l, int n, int g, int N, int C, int groups,
                                               float (*red)[kNeckWaves][2])
{
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int HW = plan.hw[l], cpg = C / groups, c0 = g * cpg, nv = HW / W;
    const long long base = ((long long)n * C + c0) * HW;
    const float *yb = plan.y[l] + base, *gb = plan.grad_out[l] + base;
    const unsigned char *mb = plan.mask[l] ? plan.mask[l] + base : nullptr;
    const float *bias = plan.bias[l];
    float *dyb = plan.grad_y[l] + base;
    const float mean = plan.mean[l][(long long)n * groups + g], rstd = plan.rstd[l][(long long)n * groups + g];
    const float inv_len = 1.f / (float)((long long)cpg * HW);
    // per-(frame, channel) partial sums of this level: g' x^ (dgamma), g' (dbeta), dy (conv bias)
    float *part = plan.partial[l];
    const long long NC = (long long)N * C;

    float s1 = 0.f, s2 = 0.f;                                   // wave-uniform: sum over this wavefront's channels
    for (int cc = wave; cc < cpg; cc += kNeckWaves) {
        const float b = bias ? bias[c0 + cc] : 0.f;
        const long long off = (long long)cc * HW;
        float a = 0.f, t = 0.f;
        for (int p = lane; p < nv; p += kWave) {
            float v[W], go[W];
            ldv<W>(yb + off + p * W, v);
            ldv<W>(gb + off + p * W, go);
            if (mb) {
                float m[W];
                ldm<W>(mb + off + p * W, m);
#pragma unroll
                for (int k = 0; k < W; ++k) go[k] *= m[k];
            }
#pragma unroll
            for (int k = 0; k < W; ++k) { a += go[k] * ((v[k] + b - mean) * rstd); t += go[k]; }
        }
        a = wave_sum(a); t = wave_sum(t);
        if (lane == 0) {
            part[(long long)n * C + c0 + cc] = a;
            part[NC + (long long)n * C + c0 + cc] = t;
        }
        const float ga = plan.gamma[l][c0 + cc];
        s1 += ga * t; s2 += ga * a;
    }
    if (lane == 0) { red[0][wave][0] = s1; red[0][wave][1] = s2; }
    __syncthreads();
    const float m1 = ((red[0][0][0] + red[0][1][0]) + (red[0][2][0] + red[0][3][0])) * inv_len;
    const float m2 = ((red[0][0][1] + red[0][1][1]) + (red[0][2][1] + red[0][3][1])) * inv_len;

    for (int cc = wave; cc < cpg; cc += kNeckWaves) {
        const float b = bias ? bias[c0 + cc] : 0.f;
        const float ga = plan.gamma[l][c0 + cc];
        const long long off = (long long)cc * HW;
        float dsum = 0.f;
        for (int p = lane; p < nv; p += kWave) {
            float v[W], go[W], dy[W];
            ldv<W>(yb + off + p * W, v);
            ldv<W>(gb + off + p * W, go);
            if (mb) {
                float m[W];
                ldm<W>(mb + off + p * W, m);
#pragma unroll
                for (int k = 0; k < W; ++k) go[k] *= m[k];
            }
#pragma unroll
            for (int k = 0; k < W; ++k) {
                const float xh = (v[k] + b - mean) * rstd;
                dy[k] = rstd * (go[k] * ga - m1 - xh * m2);
                dsum += dy[k];
            }
            stv<W>(dyb + off + p * W, dy);
        }
        dsum = wave_sum(dsum);
        if (lane == 0) part[2 * NC + (long long)n * C + c0 + cc] = dsum;
    }
}

__global__ __launch_bounds__(kNeckBlock) void neck_fwd_kernel(const NeckFwdPlan plan, int N, int C, int groups, float eps)
{
    __shared__ __attribute__((aligned(16))) float sx[kNeckLdsFloats];
    __shared__ float red[2][kNeckWaves][2];
    const int l = level_of(plan.first_block, plan.L);
    const int rest = (int)blockIdx.x - plan.first_block[l];
    const int n = rest / groups, g = rest % groups;
    if (plan.vec[l]) neck_fwd_group<4>(plan, l, n, g, C, groups, eps, sx, red);
    else neck_fwd_group<1>(plan, l, n, g, C, groups, eps, sx, red);
}

__global__ __launch_bounds__(kNeckBlock) void neck_bwd_kernel(const NeckBwdPlan plan, int N, int C, int groups)
{
    __shared__ float red[1][kNeckWaves][2];
    const int l = level_of(plan.first_block, plan.L);
    const int rest = (int)blockIdx.x - plan.first_block[l];
    const int n = rest / groups, g = rest % groups;
    if (plan.vec[l]) neck_bwd_group<4>(plan, l, n, g, N, C, groups, red);
    else neck_bwd_group<1>(plan, l, n, g, N, C, groups, red);
}

// dgamma, dbeta, dbias of every level: the [N, C] partials summed over frames in index order.  grid = (C / 256 rounded up, L).
__global__ __launch_bounds__(256) void neck_reduce_kernel(const NeckBwdPlan plan, int N, int C)
{
    const int l = (int)blockIdx.y, c = (int)(blockIdx.x * 256 + threadIdx.x);
    if (c >= C) return;
    const float *part = plan.partial[l];
    const long long NC = (long long)N * C;
    float a = 0.f, b = 0.f, d = 0.f;
    for (int n = 0; n < N; ++n) {
        a += part[(long long)n * C + c];
        b += part[NC + (long long)n * C + c];
        d += part[2 * NC + (long long)n * C + c];
    }
    if (plan.grad_gamma[l]) plan.grad_gamma[l][c] = a;
    if (plan.grad_beta[l]) plan.grad_beta[l][c] = b;
    if (plan.grad_bias[l]) plan.grad_bias[l][c] = d;
}

template <typename Plan>
long long neck_blocks(Plan &plan, int N, int groups)
{
    long long blocks = 0;
    for (int l = 0; l < plan.L; ++l) {
        plan.first_block[l] = (int)blocks;
        blocks += (long long)N * groups;
        if (blocks > 0x7fffffffLL) return -1;
    }
    return blocks;
}

}  // namespace

bool neck_supported(int L, int N, int C, int groups, const int *heights, const int *widths)
{
    if (L < 1 || L > kNeckMaxLevels || N < 0 || C < 1 || groups < 1 || C % groups != 0 || heights == nullptr || widths == nullptr)
        return false;
    if ((long long)N * C > 0x3fffffffLL || (long long)N * groups * L > 0x7fffffffLL) return false;
    for (int l = 0; l < L; ++l) {
        if (heights[l] < 1 || widths[l] < 1) return false;
        // a group's element index stays an int (LDS offsets; the global offsets are 64-bit)
        if ((long long)heights[l] * widths[l] * (C / groups) > 0x3fffffffLL) return false;
    }
    return true;
}

size_t neck_workspace_bytes(int L, int N, int C) { return (size_t)L * 3 * (size_t)N * (size_t)C * sizeof(float); }

int launch_neck_forward(const NeckFwdPlan &plan_in, int N, int C, int groups, float eps, hipStream_t stream)
{
    NeckFwdPlan plan = plan_in;
    const long long blocks = neck_blocks(plan, N, groups);
    if (blocks < 0) return set_error(MSDA_ERR_ARGUMENT, "msda neck: too many (level, frame, group) blocks");
    if (blocks == 0) return MSDA_OK;
    hipLaunchKernelGGL(neck_fwd_kernel, dim3((unsigned)blocks), dim3(kNeckBlock), 0, stream, plan, N, C, groups, eps);
    return check_launch("msda neck forward");
}

int launch_neck_backward(const NeckBwdPlan &plan_in, int N, int C, int groups, hipStream_t stream)
{
    NeckBwdPlan plan = plan_in;
    const long long blocks = neck_blocks(plan, N, groups);
    if (blocks < 0) return set_error(MSDA_ERR_ARGUMENT, "msda neck: too many (level, frame, group) blocks");
    if (blocks == 0) return MSDA_OK;
    hipLaunchKernelGGL(neck_bwd_kernel, dim3((unsigned)blocks), dim3(kNeckBlock), 0, stream, plan, N, C, groups);
    if (int rc = check_launch("msda neck backward")) return rc;
    hipLaunchKernelGGL(neck_reduce_kernel, dim3((unsigned)((C + 255) / 256), (unsigned)plan.L), dim3(256), 0, stream, plan, N, C);
    return check_launch("msda neck parameter gradients");
}

}  // namespace msda

using namespace msda;

static int neck_err(const char *msg) { return set_error(MSDA_ERR_ARGUMENT, msg); }

static bool neck_aligned(const void *p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

int msda_neck_supported(int L, int N, int C, int groups, const int *heights, const int *widths)
{
    return neck_supported(L, N, C, groups, heights, widths) ? 1 : 0;
}

unsigned long long msda_neck_workspace_bytes(int L, int N, int C)
{
    if (L < 1 || L > kNeckMaxLevels || N < 0 || C < 1) return 0;
    return neck_workspace_bytes(L, N, C);
}

int msda_neck_forward_f32(int L, const float *const *y, const float *const *bias, const float *const *gamma,
                          const float *const *beta, const float *const *uniform, const int *heights, const int *widths, int N, int C,
                          int groups, float eps, float *const *out, float *const *mean, float *const *rstd,
                          unsigned char *const *mask, msda_stream_t stream)
{
    if (!neck_supported(L, N, C, groups, heights, widths))
        return neck_err("msda_neck_forward_f32: unsupported geometry (msda_neck_supported)");
    if (!(eps > 0.f)) return neck_err("msda_neck_forward_f32: eps must be positive");
    if (!y || !gamma || !beta || !out || !mean || !rstd || (uniform && !mask)) return neck_err("msda_neck_forward_f32: null table");
    NeckFwdPlan plan;
    memset(&plan, 0, sizeof(plan));
    plan.L = L;
    for (int l = 0; l < L; ++l) {
        plan.y[l] = y[l]; plan.bias[l] = bias ? bias[l] : nullptr; plan.gamma[l] = gamma[l]; plan.beta[l] = beta[l];
        plan.u[l] = uniform ? uniform[l] : nullptr; plan.mask[l] = uniform ? mask[l] : nullptr;
        plan.out[l] = out[l]; plan.mean[l] = mean[l]; plan.rstd[l] = rstd[l];
        plan.hw[l] = heights[l] * widths[l];
        if (N > 0 && (!plan.y[l] || !plan.gamma[l] || !plan.beta[l] || !plan.out[l] || !plan.mean[l] || !plan.rstd[l]
                      || (uniform && (!plan.u[l] || !plan.mask[l]))))
            return neck_err("msda_neck_forward_f32: null level pointer");
        if (!neck_aligned(plan.y[l], 4) || !neck_aligned(plan.out[l], 4) || !neck_aligned(plan.u[l], 4))
            return neck_err("msda_neck_forward_f32: tensors must be 4-byte aligned");
        plan.vec[l] = (plan.hw[l] & 3) == 0 && neck_aligned(plan.y[l], 16) && neck_aligned(plan.out[l], 16)
                      && neck_aligned(plan.u[l], 16) && neck_aligned(plan.mask[l], 4);
    }
    set_error(MSDA_OK, "");
    (void)hipGetLastError();
    if (N == 0) return MSDA_OK;
    return launch_neck_forward(plan, N, C, groups, eps, (hipStream_t)stream);
}

int msda_neck_backward_f32(int L, const float *const *grad_out, const float *const *y, const float *const *bias,
                           const float *const *gamma, const float *const *mean, const float *const *rstd,
                           const unsigned char *const *mask, const int *heights, const int *widths, int N, int C, int groups,
                           float *const *grad_y, float *const *grad_gamma, float *const *grad_beta, float *const *grad_bias,
                           void *workspace, unsigned long long workspace_bytes, msda_stream_t stream)
{
    if (!neck_supported(L, N, C, groups, heights, widths))
        return neck_err("msda_neck_backward_f32: unsupported geometry (msda_neck_supported)");
    if (!grad_out || !y || !gamma || !mean || !rstd || !grad_y) return neck_err("msda_neck_backward_f32: null table");
    if (N > 0 && (workspace == nullptr || workspace_bytes < neck_workspace_bytes(L, N, C) || !neck_aligned(workspace, 4)))
        return neck_err("msda_neck_backward_f32: workspace smaller than msda_neck_workspace_bytes");
    NeckBwdPlan plan;
    memset(&plan, 0, sizeof(plan));
    plan.L = L;
    for (int l = 0; l < L; ++l) {
        plan.grad_out[l] = grad_out[l]; plan.y[l] = y[l]; plan.bias[l] = bias ? bias[l] : nullptr; plan.gamma[l] = gamma[l];
        plan.mean[l] = mean[l]; plan.rstd[l] = rstd[l]; plan.mask[l] = mask ? mask[l] : nullptr;
        plan.grad_y[l] = grad_y[l];
        plan.grad_gamma[l] = grad_gamma ? grad_gamma[l] : nullptr;
        plan.grad_beta[l] = grad_beta ? grad_beta[l] : nullptr;
        plan.grad_bias[l] = grad_bias ? grad_bias[l] : nullptr;
        plan.partial[l] = static_cast<float *>(workspace) + (size_t)l * 3 * (size_t)N * (size_t)C;
        plan.hw[l] = heights[l] * widths[l];
        if (N > 0 && (!plan.grad_out[l] || !plan.y[l] || !plan.gamma[l] || !plan.mean[l] || !plan.rstd[l] || !plan.grad_y[l]))
            return neck_err("msda_neck_backward_f32: null level pointer");
        if (!neck_aligned(plan.y[l], 4) || !neck_aligned(plan.grad_out[l], 4) || !neck_aligned(plan.grad_y[l], 4))
            return neck_err("msda_neck_backward_f32: tensors must be 4-byte aligned");
        plan.vec[l] = (plan.hw[l] & 3) == 0 && neck_aligned(plan.y[l], 16) && neck_aligned(plan.grad_out[l], 16)
                      && neck_aligned(plan.grad_y[l], 16) && neck_aligned(plan.mask[l], 4);
    }
    set_error(MSDA_OK, "");
    (void)hipGetLastError();
    if (N == 0) {
        for (int l = 0; l < L; ++l)
            for (float *p : {plan.grad_gamma[l], plan.grad_beta[l], plan.grad_bias[l]})
                if (p && hipMemsetAsync(p, 0, sizeof(float) * (size_t)C, (hipStream_t)stream) != hipSuccess)
                    return set_error(MSDA_ERR_LAUNCH, "msda_neck_backward_f32: hipMemsetAsync failed");
        return MSDA_OK;
    }
    return launch_neck_backward(plan, N, C, groups, (hipStream_t)stream);
}
