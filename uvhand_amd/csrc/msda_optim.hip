// The tail of the training step (engine.py:644-648: clip_grad_norm_ then optimizer.step(); util/settings.py:434: AdamW over
// three parameter groups; util/misc.py get_total_grad_norm: the norm alone when max_norm <= 0) as multi-tensor launches whose
// number does not grow with the number of tensors.
//
// Work decomposition.  Every tensor is cut into chunks of kChunk elements; one workgroup takes one chunk, a chunk never spans
//   two tensors.  The tensors are described by device-resident tables the caller owns: pointers to p, g, exp_avg and
//   exp_avg_sq, numel, chunk_start [n + 1] (msda_optim_chunks fills it on the host), group index and step offset.  A workgroup
//   finds its tensor by a binary search over chunk_start with its block index: wave-uniform, scalar loads.
//
// Alignment.  A tensor may be only 4-byte aligned (a view into a merged parameter buffer or a gradient bucket).  A chunk
//   moves 16-byte vectors only when every base it touches is 16-byte aligned (a chunk's offset in its tensor is a multiple
//   of 16 bytes); otherwise the same thread moves the same four elements one by one, so that the element a thread owns,
//   and with it the order of every sum, does not depend on the alignment.  Tails are element-wise.
//
// grad_sumsq_kernel   one fp32 partial per chunk: a thread sums the squares of its elements in index order (fmaf), the
//                     workgroup adds its threads in a fixed tree order.  No atomics.
// norm_finish_kernel  one workgroup adds the partials in a fixed order (fp64, rounded once), out[0] = sqrt of the sum,
//                     out[1] = the clip coefficient as torch forms it: clamp(reciprocal(norm + 1e-6) * max_norm, max = 1);
//                     a NaN norm gives a NaN coefficient, max_norm <= 0 gives 1.
// grad_scale_kernel   g *= coef in place (clip_grad_norm_ on its own).
// adamw_step_kernel   torch.optim.AdamW's single-tensor update in its operation order, with the clipped gradient g * coef
//                     formed in registers: g is read, never written.  The bias corrections 1 - beta^t are fp64 (t: the
//                     launch's global_step minus the tensor's step offset; beta^t by repeated squaring, at most 126 fp64
//                     products, an error below 1e-14 of beta^t), lr / bc1 and sqrt(bc2) are fp64 rounded to fp32 once, as
//                     torch's Python scalars are.  sqrtf and the divisions are correctly rounded, no fast intrinsic; every
//                     fused multiply-add is written out and contraction is off, so the arithmetic is the text below.
//
// The device-state forms (torch.optim.AdamW(capturable=True): every tensor's step is a 0-d fp32 DEVICE tensor, reached through a
// table of pointers; the groups' lr, weight_decay, beta1, beta2, eps are a DEVICE table of doubles) take nothing from the host
// that changes from step to step, so a captured launch replays with the values of the replay (util/settings.py:434-440: OneCycleLR
// moves lr and beta1 after every step):
// optim_advance_kernel    *step[i] += 1 for every tensor: the unclipped step's first launch.
// norm_finish_dev_kernel  norm_finish_kernel, then status[0] = skipped = skip_nonfinite && !isfinite(norm), status[1] += skipped
//                         and, unless skipped, *step[i] += 1 for every tensor (its threads loop over i).
// adamw_step_dev_kernel   adamw_step_kernel with t = *step[tensor] (already advanced) and the per-group scalars formed on the
//                         device by the fp64 expressions of launch_adamw_step, each rounded to fp32 once: the same bits.  A
//                         non-zero *skip ends the workgroup before it touches anything.
#include <cmath>
#include <cstdio>
#include <cstring>

#include "msda_common.h"
#include "msda_launch.h"

#pragma clang fp contract(off)

namespace msda {

namespace {

constexpr int kBlock = 256, kIters = 8, kChunk = kBlock * 4 * kIters;      // 8192 elements: 32 KB of each tensor per workgroup
constexpr int kFinishBlock = 1024;
constexpr int kMaxTensors = 1 << 20;

static_assert(kChunk == kOptimChunk, "msda_launch.h");

struct ChunkRef {
    int tensor;
    long long base;      // first element of the chunk inside its tensor
    int count;           // 1 .. kChunk
};

// chunk_start is non-decreasing with chunk_start[0] = 0 and chunk_start[n] = the grid size; an empty tensor owns no chunk.
__device__ __forceinline__ ChunkRef find_chunk(const long long *chunk_start, const long long *numel, int n)
{
    const long long c = blockIdx.x;
    int lo = 0, hi = n;                       // the answer is the last i in [0, n) with chunk_start[i] <= c
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (chunk_start[mid] <= c) lo = mid; else hi = mid;
    }
    ChunkRef r;
    r.tensor = lo;
    r.base = (c - chunk_start[lo]) * (long long)kChunk;
    const long long left = numel[lo] - r.base;
    r.count = (int)(left < (long long)kChunk ? (left > 0 ? left : 0) : (long long)kChunk);
    return r;
}

// The tensors' addresses come out of the tables, so the compiler cannot know that they are global memory: say so (flat
// accesses would also wait on the LDS counter).
typedef __attribute__((address_space(1))) float gfloat;
typedef float f4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) f4 gf4;

__device__ __forceinline__ gfloat *as_global(float *p) { return (gfloat *)p; }
__device__ __forceinline__ const gfloat *as_global(const float *p) { return (const gfloat *)p; }

__device__ __forceinline__ bool aligned16(const gfloat *p) { return ((uintptr_t)p & 15) == 0; }

// the four elements at e .. e + 3 of a chunk of `count`: a vector when VEC and all four exist, else one by one (missing: 0)
template <bool VEC>
__device__ __forceinline__ f4 load_quad(const gfloat *x, int e, int count)
{
    if (VEC && e + 4 <= count) return *(const gf4 *)(x + e);
    f4 v = {0.f, 0.f, 0.f, 0.f};
    if (e < count) v.x = x[e];
    if (e + 1 < count) v.y = x[e + 1];
    if (e + 2 < count) v.z = x[e + 2];
    if (e + 3 < count) v.w = x[e + 3];
    return v;
}

template <bool VEC>
__device__ __forceinline__ void store_quad(gfloat *x, int e, int count, f4 v)
{
    if (VEC && e + 4 <= count) { *(gf4 *)(x + e) = v; return; }
    if (e < count) x[e] = v.x;
    if (e + 1 < count) x[e + 1] = v.y;
    if (e + 2 < count) x[e + 2] = v.z;
    if (e + 3 < count) x[e + 3] = v.w;
}

template <bool VEC>
__device__ __forceinline__ float sumsq_chunk(const gfloat *g, int count)
{
    float acc = 0.f;
#pragma unroll
    for (int it = 0; it < kIters; ++it) {
        const int e = (it * kBlock + (int)threadIdx.x) * 4;
        const f4 v = load_quad<VEC>(g, e, count);              // a missing element adds +0
        acc = __builtin_fmaf(v.x, v.x, acc);
        acc = __builtin_fmaf(v.y, v.y, acc);
        acc = __builtin_fmaf(v.z, v.z, acc);
        acc = __builtin_fmaf(v.w, v.w, acc);
    }
    return acc;
}

__global__ void __launch_bounds__(kBlock) grad_sumsq_kernel(const float *const *g, const long long *numel,
                                                            const long long *chunk_start, int n, float *partials)
{
    __shared__ float red[1][kBlock];
    const ChunkRef c = find_chunk(chunk_start, numel, n);
    const gfloat *x = as_global(g[c.tensor]) + c.base;
    const float v[1] = {aligned16(x) ? sumsq_chunk<true>(x, c.count) : sumsq_chunk<false>(x, c.count)};
    block_reduce(red, v);
    if (threadIdx.x == 0) partials[blockIdx.x] = red[0][0];
}

__global__ void __launch_bounds__(kFinishBlock) norm_finish_kernel(const float *partials, long long n_chunks, float max_norm,
                                                                   float *out)
{
    __shared__ double red[kFinishBlock];
    const int tid = threadIdx.x;
    double s = 0.0;
    for (long long i = tid; i < n_chunks; i += kFinishBlock) s += (double)partials[i];
    red[tid] = s;
    __syncthreads();
    for (int w = kFinishBlock / 2; w > 0; w >>= 1) {
        if (tid < w) red[tid] += red[tid + w];
        __syncthreads();
    }
    if (tid == 0) {
        const float norm = (float)sqrt(red[0]);
        float coef = 1.f;
        if (max_norm > 0.f) {
            // torch: clamp(max_norm / (total_norm + 1e-6), max = 1), where float / Tensor is reciprocal() * float
            const float c = (1.f / (norm + 1e-6f)) * max_norm;
            coef = c > 1.f ? 1.f : c;                      // a NaN stays a NaN, as in torch.clamp
        }
        out[0] = norm;
        out[1] = coef;
    }
}

template <bool VEC>
__device__ __forceinline__ void scale_chunk(gfloat *g, int count, float coef)
{
#pragma unroll
    for (int it = 0; it < kIters; ++it) {
        const int e = (it * kBlock + (int)threadIdx.x) * 4;
        if (e >= count) break;
        f4 v = load_quad<VEC>(g, e, count);
        v.x *= coef; v.y *= coef; v.z *= coef; v.w *= coef;
        store_quad<VEC>(g, e, count, v);
    }
}

__global__ void __launch_bounds__(kBlock) grad_scale_kernel(float *const *g, const long long *numel, const long long *chunk_start,
                                                            int n, const float *coef)
{
    const ChunkRef c = find_chunk(chunk_start, numel, n);
    gfloat *x = as_global(g[c.tensor]) + c.base;
    const float k = *coef;
    if (aligned16(x)) scale_chunk<true>(x, c.count, k); else scale_chunk<false>(x, c.count, k);
}

struct AdamGroups {
    double lr[kOptimMaxGroups], beta1[kOptimMaxGroups], beta2[kOptimMaxGroups];
    float decay[kOptimMaxGroups];        // 1 - lr * weight_decay, fp64 rounded once
    float w1[kOptimMaxGroups];           // 1 - beta1
    float b2[kOptimMaxGroups];           // beta2
    float w2[kOptimMaxGroups];           // 1 - beta2
    float eps[kOptimMaxGroups];
    int n;
};

struct AdamScalars { float decay, w1, b2, w2, eps, step_size, bc2_sqrt, coef; };

// beta^t for an integer t >= 1 by repeated squaring (wave-uniform)
__device__ __forceinline__ double powi(double b, long long t)
{
    double r = 1.0;
    while (t > 0) {
        if (t & 1) r *= b;
        b *= b;
        t >>= 1;
    }
    return r;
}

__device__ __forceinline__ void adamw_one(float &p, float g, float &m, float &v, const AdamScalars &s)
{
    g = g * s.coef;                                        // the clipped gradient, rounded once
    p = p * s.decay;                                       // param.mul_(1 - lr * weight_decay)
    m = __builtin_fmaf(g - m, s.w1, m);                    // exp_avg.lerp_(grad, 1 - beta1)
    v = __builtin_fmaf(g * g, s.w2, v * s.b2);             // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value = 1 - beta2)
    const float denom = sqrtf(v) / s.bc2_sqrt + s.eps;     // (exp_avg_sq.sqrt() / sqrt(bc2)).add_(eps)
    p = __builtin_fmaf(-s.step_size, m / denom, p);        // param.addcdiv_(exp_avg, denom, value = -lr / bc1)
}

template <bool VEC>
__device__ __forceinline__ void adamw_chunk(gfloat *p, const gfloat *g, gfloat *m, gfloat *v, int count, const AdamScalars &s)
{
#pragma unroll 2
    for (int it = 0; it < kIters; ++it) {
        const int e = (it * kBlock + (int)threadIdx.x) * 4;
        if (e >= count) break;
        f4 P = load_quad<VEC>(p, e, count), M = load_quad<VEC>(m, e, count), V = load_quad<VEC>(v, e, count);
        const f4 G = load_quad<VEC>(g, e, count);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float pj = P[j], mj = M[j], vj = V[j];
            adamw_one(pj, G[j], mj, vj, s);
            P[j] = pj; M[j] = mj; V[j] = vj;
        }
        store_quad<VEC>(p, e, count, P);
        store_quad<VEC>(m, e, count, M);
        store_quad<VEC>(v, e, count, V);
    }
}

__global__ void __launch_bounds__(kBlock) adamw_step_kernel(float *const *p, const float *const *g, float *const *m, float *const *v,
                                                            const long long *numel, const long long *chunk_start, const int *group,
                                                            const long long *step_offset, int n, AdamGroups hp,
                                                            long long global_step, const float *coef)
{
    const ChunkRef c = find_chunk(chunk_start, numel, n);
    int gi = group[c.tensor];
    gi = gi < 0 ? 0 : (gi >= hp.n ? hp.n - 1 : gi);        // a bad table entry never indexes past the argument arrays
    long long t = global_step - step_offset[c.tensor];
    if (t < 1) t = 1;
    AdamScalars s;
    s.decay = hp.decay[gi]; s.w1 = hp.w1[gi]; s.b2 = hp.b2[gi]; s.w2 = hp.w2[gi]; s.eps = hp.eps[gi];
    const double bc1 = 1.0 - powi(hp.beta1[gi], t), bc2 = 1.0 - powi(hp.beta2[gi], t);
    s.step_size = (float)(hp.lr[gi] / bc1);
    s.bc2_sqrt = (float)sqrt(bc2);
    s.coef = coef ? *coef : 1.f;
    gfloat *pp = as_global(p[c.tensor]) + c.base, *mm = as_global(m[c.tensor]) + c.base, *vv = as_global(v[c.tensor]) + c.base;
    const gfloat *gg = as_global(g[c.tensor]) + c.base;
    if (aligned16(pp) && aligned16(gg) && aligned16(mm) && aligned16(vv)) adamw_chunk<true>(pp, gg, mm, vv, c.count, s);
    else adamw_chunk<false>(pp, gg, mm, vv, c.count, s);
}

__global__ void __launch_bounds__(kBlock) optim_advance_kernel(float *const *step, int n)
{
    const int i = (int)blockIdx.x * kBlock + (int)threadIdx.x;
    if (i < n) *step[i] += 1.f;                            // every tensor has a step of its own: no two threads meet
}

// What the device-state kernels share with their host-state twins above (norm_finish_kernel, adamw_step_kernel), one copy each.
// The twins keep their own text for now; they are to call these too, so that a fix reaches both.

// The total norm and the clip coefficient out of the chunks' sums of squares, by one workgroup of kFinishBlock threads: the
// reduction and the expressions of norm_finish_kernel.  Writes out[0] = norm, out[1] = coef; the norm is returned to thread 0 only.
__device__ __forceinline__ float finish_norm_and_coef(const float *partials, long long n_chunks, float max_norm, float *out,
                                                      double *red)
{
    const int tid = threadIdx.x;
    double s = 0.0;
    for (long long i = tid; i < n_chunks; i += kFinishBlock) s += (double)partials[i];
    red[tid] = s;
    __syncthreads();
    for (int w = kFinishBlock / 2; w > 0; w >>= 1) {
        if (tid < w) red[tid] += red[tid + w];
        __syncthreads();
    }
    if (tid != 0) return 0.f;
    const float norm = (float)sqrt(red[0]);
    float coef = 1.f;
    if (max_norm > 0.f) {
        // torch: clamp(max_norm / (total_norm + 1e-6), max = 1), where float / Tensor is reciprocal() * float
        const float c = (1.f / (norm + 1e-6f)) * max_norm;
        coef = c > 1.f ? 1.f : c;                          // a NaN stays a NaN, as in torch.clamp
    }
    out[0] = norm;
    out[1] = coef;
    return norm;
}

// step_size = lr / bc1 and sqrt(bc2) of a tensor at step t >= 1: fp64, each rounded to fp32 once
__device__ __forceinline__ void set_bias_corrections(AdamScalars &s, double lr, double beta1, double beta2, long long t)
{
    const double bc1 = 1.0 - powi(beta1, t), bc2 = 1.0 - powi(beta2, t);
    s.step_size = (float)(lr / bc1);
    s.bc2_sqrt = (float)sqrt(bc2);
}

// the update of chunk c of its tensor: vector accesses when all four addresses are 16-byte aligned, else element by element
__device__ __forceinline__ void adamw_update_chunk(float *const *p, const float *const *g, float *const *m, float *const *v,
                                                   const ChunkRef &c, const AdamScalars &s)
{
    gfloat *pp = as_global(p[c.tensor]) + c.base, *mm = as_global(m[c.tensor]) + c.base, *vv = as_global(v[c.tensor]) + c.base;
    const gfloat *gg = as_global(g[c.tensor]) + c.base;
    if (aligned16(pp) && aligned16(gg) && aligned16(mm) && aligned16(vv)) adamw_chunk<true>(pp, gg, mm, vv, c.count, s);
    else adamw_chunk<false>(pp, gg, mm, vv, c.count, s);
}

__global__ void __launch_bounds__(kFinishBlock) norm_finish_dev_kernel(const float *partials, long long n_chunks, float max_norm,
                                                                       float *out, float *const *step, int n_tensors,
                                                                       int skip_nonfinite, int *status)
{
    __shared__ double red[kFinishBlock];
    __shared__ int skip_all;
    const int tid = threadIdx.x;
    const float norm = finish_norm_and_coef(partials, n_chunks, max_norm, out, red);
    if (tid == 0) {
        const int skipped = (skip_nonfinite && !std::isfinite(norm)) ? 1 : 0;
        if (status) {
            status[0] = skipped;
            status[1] += skipped;
        }
        skip_all = skipped;
    }
    __syncthreads();
    if (skip_all) return;
    for (int i = tid; i < n_tensors; i += kFinishBlock) *step[i] += 1.f;
}

__global__ void __launch_bounds__(kBlock) adamw_step_dev_kernel(float *const *p, const float *const *g, float *const *m,
                                                                float *const *v, const long long *numel,
                                                                const long long *chunk_start, const int *group,
                                                                const float *const *step, int n, const double *hyper, int n_groups,
                                                                const float *coef, const int *skip)
{
    if (skip && *skip != 0) return;                        // a skipped step: nothing is read or written
    const ChunkRef c = find_chunk(chunk_start, numel, n);
    int gi = group[c.tensor];
    gi = gi < 0 ? 0 : (gi >= n_groups ? n_groups - 1 : gi);   // a bad table entry never indexes past the hyper table
    long long t = (long long)*step[c.tensor];              // advanced by this step's earlier launch
    if (t < 1) t = 1;
    const double *h = hyper + 5 * gi;
    const double lr = h[0], weight_decay = h[1], beta1 = h[2], beta2 = h[3], eps = h[4];
    AdamScalars s;                                         // launch_adamw_step's expressions, on the device
    s.decay = (float)(1.0 - lr * weight_decay);
    s.w1 = (float)(1.0 - beta1);
    s.b2 = (float)beta2;
    s.w2 = (float)(1.0 - beta2);
    s.eps = (float)eps;
    set_bias_corrections(s, lr, beta1, beta2, t);
    s.coef = coef ? *coef : 1.f;
    adamw_update_chunk(p, g, m, v, c, s);
}

int perr(const char *msg) { return set_error(MSDA_ERR_ARGUMENT, msg); }

// the checks every entry shares; *launch: whether there is anything to launch
int check_tables(const char *who, int n, long long n_chunks, bool tables_ok, bool *launch)
{
    char buf[160];
    *launch = false;
    if (n < 0 || n > kMaxTensors || n_chunks < 0 || n_chunks > 0x7fffffffLL) {
        std::snprintf(buf, sizeof(buf), "%s: tensor count 0 .. %d and chunk count 0 .. 2^31 - 1 (msda_optim_supported)", who, kMaxTensors);
        return perr(buf);
    }
    if (n == 0 || n_chunks == 0) return MSDA_OK;
    if (!tables_ok) {
        std::snprintf(buf, sizeof(buf), "%s: null table", who);
        return perr(buf);
    }
    *launch = true;
    return MSDA_OK;
}

}  // namespace

bool optim_supported(long long n_tensors, int n_groups)
{
    return n_tensors >= 0 && n_tensors <= kMaxTensors && n_groups >= 1 && n_groups <= kOptimMaxGroups;
}

long long optim_chunks(int n, const long long *numel, long long *chunk_start)
{
    if (n < 0 || n > kMaxTensors) { perr("msda_optim_chunks: tensor count 0 .. 2^20 (msda_optim_supported)"); return -1; }
    if (chunk_start == nullptr || (n > 0 && numel == nullptr)) { perr("msda_optim_chunks: null pointer"); return -1; }
    long long total = 0;
    for (int i = 0; i < n; ++i) {
        if (numel[i] < 0 || numel[i] > (1LL << 46)) { perr("msda_optim_chunks: numel must be 0 .. 2^46"); return -1; }
        total += (numel[i] + kChunk - 1) / kChunk;
        if (total > 0x7fffffffLL) { perr("msda_optim_chunks: more than 2^31 - 1 chunks"); return -1; }
    }
    set_error(MSDA_OK, "");
    total = 0;
    for (int i = 0; i < n; ++i) {
        chunk_start[i] = total;
        total += (numel[i] + kChunk - 1) / kChunk;
    }
    chunk_start[n] = total;
    return total;
}

int launch_grad_sumsq(int n, long long n_chunks, const float *const *g, const long long *numel, const long long *chunk_start,
                      float *partials, hipStream_t stream)
{
    bool launch;
    if (int rc = check_tables("msda_grad_sumsq", n, n_chunks, g && numel && chunk_start && partials, &launch)) return rc;
    if (!launch) return MSDA_OK;
    hipLaunchKernelGGL(grad_sumsq_kernel, dim3((unsigned)n_chunks), dim3(kBlock), 0, stream, g, numel, chunk_start, n, partials);
    return check_launch("grad_sumsq_kernel");
}

int launch_grad_norm_finish(long long n_chunks, const float *partials, float max_norm, float *out, hipStream_t stream)
{
    if (n_chunks < 0 || n_chunks > 0x7fffffffLL) return perr("msda_grad_norm_finish: chunk count 0 .. 2^31 - 1");
    if (std::isnan(max_norm)) return perr("msda_grad_norm_finish: max_norm is NaN");
    if (n_chunks == 0) return MSDA_OK;
    if (partials == nullptr || out == nullptr) return perr("msda_grad_norm_finish: null pointer");
    hipLaunchKernelGGL(norm_finish_kernel, dim3(1), dim3(kFinishBlock), 0, stream, partials, n_chunks, max_norm, out);
    return check_launch("norm_finish_kernel");
}

int launch_grad_scale(int n, long long n_chunks, float *const *g, const long long *numel, const long long *chunk_start,
                      const float *coef, hipStream_t stream)
{
    bool launch;
    if (int rc = check_tables("msda_grad_scale", n, n_chunks, g && numel && chunk_start && coef, &launch)) return rc;
    if (!launch) return MSDA_OK;
    hipLaunchKernelGGL(grad_scale_kernel, dim3((unsigned)n_chunks), dim3(kBlock), 0, stream, g, numel, chunk_start, n, coef);
    return check_launch("grad_scale_kernel");
}

int launch_adamw_step(const OptimTables &t, int n_groups, const double *lr, const double *weight_decay, const double *beta1,
                      const double *beta2, const double *eps, long long global_step, const float *coef, hipStream_t stream)
{
    if (!optim_supported(t.n, n_groups)) return perr("msda_adamw_step: 0 .. 2^20 tensors in 1 .. 8 groups (msda_optim_supported)");
    if (!lr || !weight_decay || !beta1 || !beta2 || !eps) return perr("msda_adamw_step: null hyperparameter array");
    if (global_step < 1) return perr("msda_adamw_step: global_step must be at least 1");
    AdamGroups hp;
    memset(&hp, 0, sizeof(hp));
    hp.n = n_groups;
    for (int k = 0; k < n_groups; ++k) {
        if (!(beta1[k] >= 0.0 && beta1[k] < 1.0) || !(beta2[k] >= 0.0 && beta2[k] < 1.0))
            return perr("msda_adamw_step: betas must be in [0, 1)");
        if (!std::isfinite(lr[k]) || !std::isfinite(eps[k]) || !std::isfinite(weight_decay[k]))
            return perr("msda_adamw_step: lr, eps and weight_decay must be finite");
        hp.lr[k] = lr[k]; hp.beta1[k] = beta1[k]; hp.beta2[k] = beta2[k];
        hp.decay[k] = (float)(1.0 - lr[k] * weight_decay[k]);
        hp.w1[k] = (float)(1.0 - beta1[k]);
        hp.b2[k] = (float)beta2[k];
        hp.w2[k] = (float)(1.0 - beta2[k]);
        hp.eps[k] = (float)eps[k];
    }
    bool launch;
    const bool ok = t.p && t.g && t.exp_avg && t.exp_avg_sq && t.numel && t.chunk_start && t.group && t.step_offset;
    if (int rc = check_tables("msda_adamw_step", t.n, t.n_chunks, ok, &launch)) return rc;
    if (!launch) return MSDA_OK;
    hipLaunchKernelGGL(adamw_step_kernel, dim3((unsigned)t.n_chunks), dim3(kBlock), 0, stream, t.p, t.g, t.exp_avg, t.exp_avg_sq,
                       t.numel, t.chunk_start, t.group, t.step_offset, t.n, hp, global_step, coef);
    return check_launch("adamw_step_kernel");
}

int launch_optim_advance(int n, float *const *step, hipStream_t stream)
{
    if (n < 0 || n > kMaxTensors) return perr("msda_optim_advance: tensor count 0 .. 2^20 (msda_optim_supported)");
    if (n == 0) return MSDA_OK;
    if (step == nullptr) return perr("msda_optim_advance: null step table");
    hipLaunchKernelGGL(optim_advance_kernel, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, stream, step, n);
    return check_launch("optim_advance_kernel");
}

int launch_grad_norm_finish_dev(long long n_chunks, const float *partials, float max_norm, float *out, int n, float *const *step,
                                int skip_nonfinite, int *status, hipStream_t stream)
{
    if (n < 0 || n > kMaxTensors || n_chunks < 0 || n_chunks > 0x7fffffffLL)
        return perr("msda_grad_norm_finish_dev: tensor count 0 .. 2^20 and chunk count 0 .. 2^31 - 1 (msda_optim_supported)");
    if (std::isnan(max_norm)) return perr("msda_grad_norm_finish_dev: max_norm is NaN");
    if (skip_nonfinite && status == nullptr) return perr("msda_grad_norm_finish_dev: skip_nonfinite needs a status array");
    if (n == 0 || n_chunks == 0) return MSDA_OK;
    if (partials == nullptr || out == nullptr) return perr("msda_grad_norm_finish_dev: null pointer");
    if (step == nullptr) return perr("msda_grad_norm_finish_dev: null step table");
    hipLaunchKernelGGL(norm_finish_dev_kernel, dim3(1), dim3(kFinishBlock), 0, stream, partials, n_chunks, max_norm, out, step, n,
                       skip_nonfinite ? 1 : 0, status);
    return check_launch("norm_finish_dev_kernel");
}

int launch_adamw_step_dev(const OptimTables &t, const float *const *step, int n_groups, const double *hyper, const float *coef,
                          const int *skip, hipStream_t stream)
{
    if (!optim_supported(t.n, n_groups)) return perr("msda_adamw_step_dev: 0 .. 2^20 tensors in 1 .. 8 groups (msda_optim_supported)");
    if (hyper == nullptr) return perr("msda_adamw_step_dev: null hyper table");
    bool launch;
    const bool ok = t.p && t.g && t.exp_avg && t.exp_avg_sq && t.numel && t.chunk_start && t.group;
    if (int rc = check_tables("msda_adamw_step_dev", t.n, t.n_chunks, ok, &launch)) return rc;
    if (!launch) return MSDA_OK;
    if (step == nullptr) return perr("msda_adamw_step_dev: null step table");
    hipLaunchKernelGGL(adamw_step_dev_kernel, dim3((unsigned)t.n_chunks), dim3(kBlock), 0, stream, t.p, t.g, t.exp_avg, t.exp_avg_sq,
                       t.numel, t.chunk_start, t.group, step, t.n, hyper, n_groups, coef, skip);
    return check_launch("adamw_step_dev_kernel");
}

}  // namespace msda
