// The memory-bound glue of a Swin block around the window attention and the MLP (models/swin_transformer.py:209-245 the block's
// norm1 / residual + drop_path / norm2 / residual + drop_path, :263-287 PatchMerging's pad, 2x2 gather, concatenation and norm),
// for MI355X (gfx950).  Opt-in from Python (MSDA_SWIN_GLUE=1); C entries msda_swin_glue_*.
//
// X is the type of the residual stream (x, y, their gradients and the rows the backward re-reads), T the type of the branch a,
// of the per-sample drop-path scale keep, of the normalised output z and of their gradients: float, or uint16_t holding bf16
// bits.  X = float is the stream outside autocast and of stage 0 under bf16 autocast; X = bf16 (the _sbf16 entries) is the
// stream from the first PatchMerging on under bf16 autocast, with T = bf16, or T = float for the per-stage output norms.
//
//   norm        z = LN(x) gamma + beta                                            -> z (T), mean, rstd
//   add_norm    y = x + rnd_T(a keep[row / rows_per_sample]);  z = LN(y) ...      -> y (fp32), z (T), mean, rstd   one launch
//   add         y = x + rnd_T(a keep[..])                                          (no LayerNorm follows inside the checkpoint)
//   merge_norm  z = LN(cat(x[2i,2j], x[2i+1,2j], x[2i,2j+1], x[2i+1,2j+1])), zeros where an odd H or W is padded
//
// rnd_T rounds to bf16 (nearest even) for bf16 and is the identity for fp32: the product a * keep is a tensor of type T in
// torch before type promotion widens it for the add, so y is bit for bit torch's.  keep null means 1 (no product, no rounding).
// Nothing here is contracted into an fma (the pragma below): torch runs the product and the add as separate kernels.
//
// A bf16 stream rounds (rnd_X, nearest even) wherever torch's bf16 arithmetic under autocast materialises a bf16 tensor:
//   forward   y = rnd_X(x + rnd_T(a keep)), and z normalises that ROUNDED y (the LayerNorm reads the stored tensor);
//   backward  grad_x = rnd_X(grad_y + rnd_X(LN'(grad_z))): the cast's backward rounds, then autograd's accumulation rounds;
//             grad_a = rnd_T(grad_x keep) from the rounded grad_x; without keep grad_a is grad_x and is not written.
// rnd_X is the identity for X = float, so the fp32-stream instantiations compute what they computed before X existed.
//
// Conventions of msda_layernorm.hip: one wavefront per row, 4 rows in flight per workgroup, lane i holds channels 4i..4i+3
// (+256k) as float4 (16-byte fp32 / 8-byte bf16 accesses), two-pass moments in fp32 over registers; the backward's gamma / beta
// gradients are per-workgroup partial column sums combined by a fixed-order second stage: no float atomics, bitwise reproducible.
// Widths up to 3072 (12 float4 per lane).  Up to 1024 the backward keeps its column sums in registers; above, each wavefront
// keeps them in its own LDS region (only the lane that owns a column touches it), so that the kernel does not spill.
#include <initializer_list>
#include <stdio.h>

#include "msda_common.h"
#include "msda_launch.h"

#pragma clang fp contract(off)

namespace msda {
namespace {

constexpr int kGlBlock = 256;                     // 4 wavefronts = 4 rows in flight per workgroup
constexpr int kGlWaves = kGlBlock / kWave;
constexpr int kGlMaxWidth = 3072;                 // 12 float4 per lane
constexpr int kGlRegVec = 4;                      // up to this many float4 per lane the backward sums columns in registers
constexpr int kNorm = 0, kAddNorm = 1, kMerge = 2;

typedef __attribute__((ext_vector_type(4))) __bf16 bf4;

__device__ __forceinline__ void st4(float *p, float4 v) { *reinterpret_cast<float4 *>(p) = v; }
__device__ __forceinline__ void st4(uint16_t *p, float4 v)
{
    *reinterpret_cast<bf4 *>(p) = bf4{(__bf16)v.x, (__bf16)v.y, (__bf16)v.z, (__bf16)v.w};
}
__device__ __forceinline__ float ld1(const float *p) { return *p; }
__device__ __forceinline__ float ld1(const uint16_t *p) { return __uint_as_float((unsigned)*p << 16); }

template <typename T>
__device__ __forceinline__ float rnd(float v)
{
    if (sizeof(T) == 2) return (float)(__bf16)v;
    return v;
}
template <typename T>
__device__ __forceinline__ float4 rnd4(float4 v) { return make_float4(rnd<T>(v.x), rnd<T>(v.y), rnd<T>(v.z), rnd<T>(v.w)); }
// rnd_T(v * keep): a tensor of type T in torch
template <typename T>
__device__ __forceinline__ float4 scale4(float4 v, float keep)
{
    return make_float4(rnd<T>(v.x * keep), rnd<T>(v.y * keep), rnd<T>(v.z * keep), rnd<T>(v.w * keep));
}

// PatchMerging: merged row -> (image, i, j) once per row; channel c of the 4C-wide row -> the float offset of its source in
// x [B, H, W, C], or -1 for a padded position.  Channel blocks in the reference's order (0,0), (1,0), (0,1), (1,1).
struct MergeGeo { int H, W, H2, W2, C; };
struct MergeRow { long long base; int h, w; };
__device__ __forceinline__ MergeRow merge_row(const MergeGeo &g, long long row)
{
    const long long per = (long long)g.H2 * g.W2, b = row / per;
    const int t = (int)(row - b * per), i = t / g.W2, j = t - i * g.W2;
    return MergeRow{b * g.H * g.W, 2 * i, 2 * j};
}
__device__ __forceinline__ long long merge_off(const MergeGeo &g, const MergeRow &r, int c)
{
    const int q = c / g.C, cc = c - q * g.C;
    const int h = r.h + (q & 1), w = r.w + (q >> 1);
    if (h >= g.H || w >= g.W) return -1;
    return (r.base + (long long)h * g.W + w) * g.C + cc;
}

template <int NV, typename X, typename T, int MODE>
__global__ __launch_bounds__(kGlBlock) void glue_fwd_kernel(
    const X *__restrict__ x, const T *__restrict__ a, const T *__restrict__ keep, long long rows, long long rows_per_sample,
    int d, MergeGeo geo, const float *__restrict__ gamma, const float *__restrict__ beta, float eps, X *__restrict__ y,
    T *__restrict__ z, float *__restrict__ mean_out, float *__restrict__ rstd_out)
{
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    const long long row = (long long)blockIdx.x * kGlWaves + wave;
    if (row >= rows) return;                                             // whole wavefront leaves together
    const bool scaled = MODE == kAddNorm && keep != nullptr;
    const float kp = scaled ? ld1(keep + row / rows_per_sample) : 1.f;
    MergeRow mr{0, 0, 0};
    if (MODE == kMerge) mr = merge_row(geo, row);
    float4 v[NV];
    float sum = 0.f;
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        const int c = (k * kWave + lane) * 4;
        v[k] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (c < d) {
            if (MODE == kMerge) {
                const long long off = merge_off(geo, mr, c);
                if (off >= 0) v[k] = ld4(x + off);
            } else {
                v[k] = ld4(x + row * d + c);
            }
            if (MODE == kAddNorm) {
                float4 t = ld4(a + row * d + c);
                if (scaled) t = scale4<T>(t, kp);
                v[k].x += t.x; v[k].y += t.y; v[k].z += t.z; v[k].w += t.w;
                v[k] = rnd4<X>(v[k]);                                    // the LayerNorm reads the stored y
                st4(y + row * d + c, v[k]);
            }
            sum += (v[k].x + v[k].y) + (v[k].z + v[k].w);
        }
    }
    const float mean = wave_sum(sum) / (float)d;
    float sq = 0.f;
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        const int c = (k * kWave + lane) * 4;
        if (c < d) {
            const float p = v[k].x - mean, q = v[k].y - mean, r = v[k].z - mean, s = v[k].w - mean;
            sq += (p * p + q * q) + (r * r + s * s);
        }
    }
    const float rstd = rsqrtf(wave_sum(sq) / (float)d + eps);
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        const int c = (k * kWave + lane) * 4;
        if (c < d) {
            const float4 g = ld4(gamma + c), b = ld4(beta + c);
            float4 o;
            o.x = (v[k].x - mean) * rstd * g.x + b.x; o.y = (v[k].y - mean) * rstd * g.y + b.y;
            o.z = (v[k].z - mean) * rstd * g.z + b.z; o.w = (v[k].w - mean) * rstd * g.w + b.w;
            st4(z + row * d + c, o);
        }
    }
    if (lane == 0) { mean_out[row] = mean; rstd_out[row] = rstd; }
}

// Workgroup w owns the rows [w * rows_per_wg, (w+1) * rows_per_wg); its 4 wavefronts take them round-robin.  src: the rows the
// forward normalised (norm, merge_norm: x; add_norm: the saved y).  add_norm adds grad_y and writes the sum as grad_x, and
// grad_a = rnd_T(rnd_T(grad_x) keep) (the two roundings of torch's autograd; one product for fp32) unless ga is null.
// A bf16 stream rounds LN'(grad_z) before the sum and the sum again (the file comment); grad_a then starts from that grad_x.
// partial[w][2][d]: the workgroup's dgamma / dbeta column sums.
template <int NV, typename X, typename T, int MODE>
__global__ __launch_bounds__(kGlBlock) void glue_bwd_kernel(
    const X *__restrict__ gy, const T *__restrict__ gz, const X *__restrict__ src, const T *__restrict__ keep,
    const float *__restrict__ gamma, const float *__restrict__ mean_in, const float *__restrict__ rstd_in, long long rows,
    long long rows_per_sample, int d, MergeGeo geo, int rows_per_wg, X *__restrict__ gx, T *__restrict__ ga,
    float *__restrict__ partial)
{
    constexpr bool kLds = NV > kGlRegVec;                                // column sums in LDS instead of registers
    constexpr int kW = NV * kWave * 4;
    __shared__ __attribute__((aligned(16))) float red[kGlWaves][2][kW];
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    const long long r0 = (long long)blockIdx.x * rows_per_wg;
    const long long r1 = r0 + rows_per_wg < rows ? r0 + rows_per_wg : rows;
    const bool scaled = MODE == kAddNorm && keep != nullptr;
    float4 gm[kLds ? 1 : NV], dg[kLds ? 1 : NV], db[kLds ? 1 : NV];
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        const int c = (k * kWave + lane) * 4;
        if (kLds) {
            st4(&red[wave][0][c], make_float4(0.f, 0.f, 0.f, 0.f));
            st4(&red[wave][1][c], make_float4(0.f, 0.f, 0.f, 0.f));
        } else {
            gm[k] = c < d ? ld4(gamma + c) : make_float4(0.f, 0.f, 0.f, 0.f);
            dg[k] = db[k] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
    }
    for (long long row = r0 + wave; row < r1; row += kGlWaves) {
        const float mean = mean_in[row], rstd = rstd_in[row];
        const float kp = scaled ? ld1(keep + row / rows_per_sample) : 1.f;
        MergeRow mr{0, 0, 0};
        if (MODE == kMerge) mr = merge_row(geo, row);
        float4 xh[NV], g[NV];
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int k = 0; k < NV; ++k) {
            const int c = (k * kWave + lane) * 4;
            xh[k] = g[k] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (c < d) {
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (MODE == kMerge) {
                    const long long off = merge_off(geo, mr, c);
                    if (off >= 0) v = ld4(src + off);
                } else {
                    v = ld4(src + row * d + c);
                }
                const float4 o = ld4(gz + row * d + c);
                const float4 gmk = kLds ? ld4(gamma + c) : gm[kLds ? 0 : k];
                xh[k] = make_float4((v.x - mean) * rstd, (v.y - mean) * rstd, (v.z - mean) * rstd, (v.w - mean) * rstd);
                g[k] = make_float4(o.x * gmk.x, o.y * gmk.y, o.z * gmk.z, o.w * gmk.w);
                s1 += (g[k].x + g[k].y) + (g[k].z + g[k].w);
                s2 += (g[k].x * xh[k].x + g[k].y * xh[k].y) + (g[k].z * xh[k].z + g[k].w * xh[k].w);
                if (kLds) {
                    float4 t = ld4(&red[wave][0][c]), u = ld4(&red[wave][1][c]);
                    t.x += o.x * xh[k].x; t.y += o.y * xh[k].y; t.z += o.z * xh[k].z; t.w += o.w * xh[k].w;
                    u.x += o.x; u.y += o.y; u.z += o.z; u.w += o.w;
                    st4(&red[wave][0][c], t);
                    st4(&red[wave][1][c], u);
                } else {
                    float4 &t = dg[kLds ? 0 : k], &u = db[kLds ? 0 : k];
                    t.x += o.x * xh[k].x; t.y += o.y * xh[k].y; t.z += o.z * xh[k].z; t.w += o.w * xh[k].w;
                    u.x += o.x; u.y += o.y; u.z += o.z; u.w += o.w;
                }
            }
        }
        const float c1 = wave_sum(s1) / (float)d, c2 = wave_sum(s2) / (float)d;
#pragma unroll
        for (int k = 0; k < NV; ++k) {
            const int c = (k * kWave + lane) * 4;
            if (c < d) {
                float4 o;
                o.x = rstd * (g[k].x - c1 - xh[k].x * c2); o.y = rstd * (g[k].y - c1 - xh[k].y * c2);
                o.z = rstd * (g[k].z - c1 - xh[k].z * c2); o.w = rstd * (g[k].w - c1 - xh[k].w * c2);
                if (MODE == kMerge) {
                    const long long off = merge_off(geo, mr, c);
                    if (off >= 0) st4(gx + off, o);                      // every real token belongs to exactly one merged row
                } else {
                    if (MODE == kAddNorm) {
                        const float4 t = ld4(gy + row * d + c);
                        o = rnd4<X>(o);
                        o.x += t.x; o.y += t.y; o.z += t.z; o.w += t.w;
                        o = rnd4<X>(o);
                    }
                    st4(gx + row * d + c, o);
                    if (MODE == kAddNorm && ga) {
                        float4 t = rnd4<T>(o);
                        if (scaled) t = scale4<T>(t, kp);
                        st4(ga + row * d + c, t);
                    }
                }
            }
        }
    }
    // the 4 wavefronts' column sums, combined in a fixed order
    if (!kLds) {
#pragma unroll
        for (int k = 0; k < NV; ++k) {
            st4(&red[wave][0][(k * kWave + lane) * 4], dg[kLds ? 0 : k]);
            st4(&red[wave][1][(k * kWave + lane) * 4], db[kLds ? 0 : k]);
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 2 * d; i += kGlBlock) {
        const int which = i >= d, c = which ? i - d : i;
        float t = red[0][which][c];
#pragma unroll
        for (int w = 1; w < kGlWaves; ++w) t += red[w][which][c];
        partial[((long long)blockIdx.x * 2 + which) * d + c] = t;
    }
}

// y = rnd_X(x + rnd_T(a keep[row / rows_per_sample])) (the store rounds): one wavefront per row, so the sample index is found
// once per row
template <typename X, typename T>
__global__ __launch_bounds__(kGlBlock) void glue_add_fwd_kernel(const X *__restrict__ x, const T *__restrict__ a,
                                                                const T *__restrict__ keep, long long rows,
                                                                long long rows_per_sample, int d, X *__restrict__ y)
{
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    const long long row = (long long)blockIdx.x * kGlWaves + wave;
    if (row >= rows) return;
    const float kp = keep ? ld1(keep + row / rows_per_sample) : 1.f;
    for (int c = lane * 4; c < d; c += kWave * 4) {
        float4 v = ld4(x + row * d + c), t = ld4(a + row * d + c);
        if (keep) t = scale4<T>(t, kp);
        v.x += t.x; v.y += t.y; v.z += t.z; v.w += t.w;
        st4(y + row * d + c, v);
    }
}

// grad_a = rnd_T(rnd_T(grad_y) keep[..]) (keep null: rnd_T(grad_y)); grad_x is grad_y itself
template <typename X, typename T>
__global__ __launch_bounds__(kGlBlock) void glue_add_bwd_kernel(const X *__restrict__ gy, const T *__restrict__ keep,
                                                                long long rows, long long rows_per_sample, int d,
                                                                T *__restrict__ ga)
{
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    const long long row = (long long)blockIdx.x * kGlWaves + wave;
    if (row >= rows) return;
    const float kp = keep ? ld1(keep + row / rows_per_sample) : 1.f;
    for (int c = lane * 4; c < d; c += kWave * 4) {
        float4 t = rnd4<T>(ld4(gy + row * d + c));
        if (keep) t = scale4<T>(t, kp);
        st4(ga + row * d + c, t);
    }
}

// dgamma[c] / dbeta[c] = sum over the workgroups' partials: a 256-thread workgroup takes 16 columns, 16 threads per column each
// summing every 16th partial (independent load chains), combined through LDS in a fixed order (as msda_layernorm.hip's).
__global__ __launch_bounds__(256) void glue_param_reduce_kernel(const float *__restrict__ partial, int nwg, int d,
                                                                float *__restrict__ dgamma, float *__restrict__ dbeta)
{
    __shared__ float red[16][17];
    const int cl = (int)threadIdx.x & 15, part = (int)threadIdx.x >> 4;
    const int col = (int)blockIdx.x * 16 + cl, which = (int)blockIdx.y;
    float t0 = 0.f, t1 = 0.f;
    if (col < d) {
        int w = part;
        for (; w + 16 < nwg; w += 32) {
            t0 += partial[((long long)w * 2 + which) * d + col];
            t1 += partial[((long long)(w + 16) * 2 + which) * d + col];
        }
        if (w < nwg) t0 += partial[((long long)w * 2 + which) * d + col];
    }
    red[part][cl] = t0 + t1;
    __syncthreads();
    if (part == 0 && col < d) {
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < 16; ++k) s += red[k][cl];
        (which ? dbeta : dgamma)[col] = s;
    }
}

int glue_wgs(long long rows)
{
    long long w = (rows + 15) / 16;                   // at least ~16 rows per workgroup
    if (w > 1024) w = 1024;
    return (int)(w < 1 ? 1 : w);
}

constexpr long long kGlMaxRows = 1LL << 32;           // one wavefront per row, 4 per workgroup: the grid stays below 2^31

struct Ptr { const void *p; size_t align; bool optional; };

int glue_check(const char *who, long long rows, long long rows_per_sample, int d, std::initializer_list<Ptr> ptrs)
{
    char buf[200];
    if (!swin_glue_supported(d)) {
        snprintf(buf, sizeof buf, "%s: need a width C with C %% 4 == 0 and 0 < C <= %d (msda_swin_glue_supported)", who, kGlMaxWidth);
        return set_error(MSDA_ERR_ARGUMENT, buf);
    }
    if (rows < 0 || rows > kGlMaxRows) {
        snprintf(buf, sizeof buf, "%s: need 0 <= rows <= 2^32", who);
        return set_error(MSDA_ERR_ARGUMENT, buf);
    }
    if (rows_per_sample <= 0) {
        snprintf(buf, sizeof buf, "%s: rows_per_sample must be positive", who);
        return set_error(MSDA_ERR_ARGUMENT, buf);
    }
    for (const Ptr &q : ptrs) {
        if (!q.p && !q.optional) {
            snprintf(buf, sizeof buf, "%s: null device pointer", who);
            return set_error(MSDA_ERR_ARGUMENT, buf);
        }
    }
    for (const Ptr &q : ptrs) {
        if (q.p && !aligned_to(q.p, q.align)) {
            snprintf(buf, sizeof buf, "%s: operands must be aligned (fp32 rows and parameters 16 bytes, bf16 rows 8 bytes)", who);
            return set_error(MSDA_ERR_ARGUMENT, buf);
        }
    }
    return MSDA_OK;
}

int glue_check_workspace(const char *who, long long rows, int d, const void *workspace, unsigned long long bytes)
{
    char buf[200];
    if (!workspace || !aligned_to(workspace, 16)) {
        snprintf(buf, sizeof buf, "%s: null or not 16-byte aligned workspace", who);
        return set_error(MSDA_ERR_ARGUMENT, buf);
    }
    if (bytes < swin_glue_workspace_bytes(rows, d)) {
        snprintf(buf, sizeof buf, "%s: workspace smaller than msda_swin_glue_workspace_bytes", who);
        return set_error(MSDA_ERR_ARGUMENT, buf);
    }
    return MSDA_OK;
}

int merge_check(const char *who, int B, int H, int W, int C)
{
    char buf[200];
    if (B < 0 || H <= 0 || W <= 0 || !swin_glue_supported(C) || 4 * C > kGlMaxWidth) {
        snprintf(buf, sizeof buf, "%s: need B >= 0, H, W > 0 and a width C with C %% 4 == 0 and 0 < 4 C <= %d", who, kGlMaxWidth);
        return set_error(MSDA_ERR_ARGUMENT, buf);
    }
    return MSDA_OK;
}

MergeGeo merge_geo(int H, int W, int C) { return MergeGeo{H, W, (H + 1) / 2, (W + 1) / 2, C}; }

#define MSDA_GLUE_NV(d, F)                                                                                                       \
    do {                                                                                                                         \
        if (d <= 256) F(1); else if (d <= 512) F(2); else if (d <= 768) F(3); else if (d <= 1024) F(4);                          \
        else if (d <= 1536) F(6); else if (d <= 2048) F(8); else F(12);                                                          \
    } while (0)

template <typename X, typename T, int MODE>
int glue_fwd(const void *x, const void *a, const void *keep, long long rows, long long rps, int d, MergeGeo geo,
             const float *gamma, const float *beta, float eps, void *y, void *z, float *mean, float *rstd, hipStream_t stream)
{
    if (rows == 0) return MSDA_OK;
    const dim3 grid((unsigned)((rows + kGlWaves - 1) / kGlWaves)), block(kGlBlock);
#define MSDA_GLUE_F(NV)                                                                                                          \
    hipLaunchKernelGGL((glue_fwd_kernel<NV, X, T, MODE>), grid, block, 0, stream, (const X *)x, (const T *)a, (const T *)keep,   \
                       rows, rps, d, geo, gamma, beta, eps, (X *)y, (T *)z, mean, rstd)
    MSDA_GLUE_NV(d, MSDA_GLUE_F);
#undef MSDA_GLUE_F
    return check_launch("msda swin glue forward");
}

template <typename X, typename T, int MODE>
int glue_bwd(const void *gy, const void *gz, const void *src, const void *keep, const float *gamma, const float *mean,
             const float *rstd, long long rows, long long rps, int d, MergeGeo geo, void *gx, void *ga, float *dgamma,
             float *dbeta, float *workspace, hipStream_t stream)
{
    // rows == 0: no partials; the reduce below then writes zeros from one empty workgroup's sums
    const int nwg = glue_wgs(rows);
    const int rows_per_wg = (int)((rows + nwg - 1) / nwg);
#define MSDA_GLUE_B(NV)                                                                                                          \
    hipLaunchKernelGGL((glue_bwd_kernel<NV, X, T, MODE>), dim3(nwg), dim3(kGlBlock), 0, stream, (const X *)gy, (const T *)gz,    \
                       (const X *)src, (const T *)keep, gamma, mean, rstd, rows, rps, d, geo, rows_per_wg, (X *)gx, (T *)ga,    \
                       workspace)
    MSDA_GLUE_NV(d, MSDA_GLUE_B);
#undef MSDA_GLUE_B
    if (int rc = check_launch("msda swin glue backward")) return rc;
    hipLaunchKernelGGL(glue_param_reduce_kernel, dim3((d + 15) / 16, 2), dim3(256), 0, stream, workspace, nwg, d, dgamma, dbeta);
    return check_launch("msda swin glue parameter gradients");
}

// The instantiations: a bf16 stream has a bf16 branch, and fp32 normalised rows for norm alone (the per-stage output norms).
#define MSDA_GLUE_PICK(sbf16, bf16, CALL) ((sbf16) ? CALL(uint16_t, uint16_t) : (bf16) ? CALL(float, uint16_t) : CALL(float, float))
#define MSDA_GLUE_PICK_NORM(sbf16, bf16, CALL) ((sbf16) && !(bf16) ? CALL(uint16_t, float) : MSDA_GLUE_PICK(sbf16, bf16, CALL))

inline size_t row_align(bool bf16) { return bf16 ? 8 : 16; }
inline size_t elem_align(bool bf16) { return bf16 ? 2 : 4; }

// "msda_swin_glue_<op>_<T>[_sbf16]"
const char *entry_name(bool sbf16, bool bf16, const char *const (&names)[4]) { return names[(sbf16 ? 2 : 0) + (bf16 ? 1 : 0)]; }
#define MSDA_GLUE_NAMES(op)                                                                                                      \
    {"msda_swin_glue_" op "_f32", "msda_swin_glue_" op "_bf16", "msda_swin_glue_" op "_f32_sbf16",                               \
     "msda_swin_glue_" op "_bf16_sbf16"}

}  // namespace

bool swin_glue_supported(int C) { return C > 0 && C % 4 == 0 && C <= kGlMaxWidth; }

unsigned long long swin_glue_workspace_bytes(long long rows, int C)
{
    if (!swin_glue_supported(C) || rows < 0 || rows > kGlMaxRows) return 0;
    return (unsigned long long)glue_wgs(rows) * 2 * C * sizeof(float);
}

int swin_glue_norm_forward(bool sbf16, bool bf16, const void *x, const float *gamma, const float *beta, long long rows, int C,
                           float eps, void *z, float *mean, float *rstd, hipStream_t stream)
{
    const char *who = entry_name(sbf16, bf16, MSDA_GLUE_NAMES("norm_forward"));
    if (int rc = glue_check(who, rows, 1, C, {{x, row_align(sbf16), false}, {gamma, 16, false}, {beta, 16, false},
                                             {z, row_align(bf16), false}, {mean, 4, false}, {rstd, 4, false}}))
        return rc;
    const MergeGeo geo{};
#define MSDA_GLUE_CALL(X, T) glue_fwd<X, T, kNorm>(x, nullptr, nullptr, rows, 1, C, geo, gamma, beta, eps, nullptr, z, mean, rstd, stream)
    return MSDA_GLUE_PICK_NORM(sbf16, bf16, MSDA_GLUE_CALL);
#undef MSDA_GLUE_CALL
}

int swin_glue_norm_backward(bool sbf16, bool bf16, const void *grad_z, const void *x, const float *gamma, const float *mean,
                            const float *rstd, long long rows, int C, void *grad_x, float *grad_gamma, float *grad_beta,
                            void *workspace, unsigned long long workspace_bytes, hipStream_t stream)
{
    const char *who = entry_name(sbf16, bf16, MSDA_GLUE_NAMES("norm_backward"));
    if (int rc = glue_check(who, rows, 1, C, {{grad_z, row_align(bf16), false}, {x, row_align(sbf16), false},
                                             {gamma, 16, false}, {mean, 4, false}, {rstd, 4, false},
                                             {grad_x, row_align(sbf16), false}, {grad_gamma, 4, false}, {grad_beta, 4, false}}))
        return rc;
    if (int rc = glue_check_workspace(who, rows, C, workspace, workspace_bytes)) return rc;
    const MergeGeo geo{};
#define MSDA_GLUE_CALL(X, T)                                                                                                     \
    glue_bwd<X, T, kNorm>(nullptr, grad_z, x, nullptr, gamma, mean, rstd, rows, 1, C, geo, grad_x, nullptr, grad_gamma,          \
                          grad_beta, (float *)workspace, stream)
    return MSDA_GLUE_PICK_NORM(sbf16, bf16, MSDA_GLUE_CALL);
#undef MSDA_GLUE_CALL
}

int swin_glue_add_norm_forward(bool sbf16, bool bf16, const void *x, const void *a, const void *keep, long long rows,
                               long long rows_per_sample, int C, const float *gamma, const float *beta, float eps, void *y,
                               void *z, float *mean, float *rstd, hipStream_t stream)
{
    const char *who = entry_name(sbf16, bf16, MSDA_GLUE_NAMES("add_norm_forward"));
    if (int rc = glue_check(who, rows, rows_per_sample, C,
                            {{x, row_align(sbf16), false}, {a, row_align(bf16), false}, {keep, elem_align(bf16), true},
                             {gamma, 16, false}, {beta, 16, false}, {y, row_align(sbf16), false}, {z, row_align(bf16), false},
                             {mean, 4, false}, {rstd, 4, false}}))
        return rc;
    const MergeGeo geo{};
#define MSDA_GLUE_CALL(X, T)                                                                                                     \
    glue_fwd<X, T, kAddNorm>(x, a, keep, rows, rows_per_sample, C, geo, gamma, beta, eps, y, z, mean, rstd, stream)
    return MSDA_GLUE_PICK(sbf16, bf16, MSDA_GLUE_CALL);
#undef MSDA_GLUE_CALL
}

int swin_glue_add_norm_backward(bool sbf16, bool bf16, const void *grad_y, const void *grad_z, const void *y, const void *keep,
                                const float *gamma, const float *mean, const float *rstd, long long rows,
                                long long rows_per_sample, int C, void *grad_x, void *grad_a, float *grad_gamma,
                                float *grad_beta, void *workspace, unsigned long long workspace_bytes, hipStream_t stream)
{
    const char *who = entry_name(sbf16, bf16, MSDA_GLUE_NAMES("add_norm_backward"));
    // grad_a may be null only where it would equal grad_x bit for bit: a branch of the stream's type without a keep vector
    if (int rc = glue_check(who, rows, rows_per_sample, C,
                            {{grad_y, row_align(sbf16), false}, {grad_z, row_align(bf16), false}, {y, row_align(sbf16), false},
                             {keep, elem_align(bf16), true}, {gamma, 16, false}, {mean, 4, false}, {rstd, 4, false},
                             {grad_x, row_align(sbf16), false}, {grad_a, row_align(bf16), sbf16 == bf16 && !keep},
                             {grad_gamma, 4, false}, {grad_beta, 4, false}}))
        return rc;
    if (int rc = glue_check_workspace(who, rows, C, workspace, workspace_bytes)) return rc;
    const MergeGeo geo{};
#define MSDA_GLUE_CALL(X, T)                                                                                                     \
    glue_bwd<X, T, kAddNorm>(grad_y, grad_z, y, keep, gamma, mean, rstd, rows, rows_per_sample, C, geo, grad_x, grad_a,          \
                             grad_gamma, grad_beta, (float *)workspace, stream)
    return MSDA_GLUE_PICK(sbf16, bf16, MSDA_GLUE_CALL);
#undef MSDA_GLUE_CALL
}

int swin_glue_add_forward(bool sbf16, bool bf16, const void *x, const void *a, const void *keep, long long rows,
                          long long rows_per_sample, int C, void *y, hipStream_t stream)
{
    const char *who = entry_name(sbf16, bf16, MSDA_GLUE_NAMES("add_forward"));
    if (int rc = glue_check(who, rows, rows_per_sample, C, {{x, row_align(sbf16), false}, {a, row_align(bf16), false},
                                                           {keep, elem_align(bf16), true}, {y, row_align(sbf16), false}}))
        return rc;
    if (rows == 0) return MSDA_OK;
    const dim3 grid((unsigned)((rows + kGlWaves - 1) / kGlWaves)), block(kGlBlock);
#define MSDA_GLUE_CALL(X, T)                                                                                                     \
    hipLaunchKernelGGL((glue_add_fwd_kernel<X, T>), grid, block, 0, stream, (const X *)x, (const T *)a, (const T *)keep, rows,   \
                       rows_per_sample, C, (X *)y)
    if (sbf16) MSDA_GLUE_CALL(uint16_t, uint16_t); else if (bf16) MSDA_GLUE_CALL(float, uint16_t); else MSDA_GLUE_CALL(float, float);
#undef MSDA_GLUE_CALL
    return check_launch("msda swin glue add forward");
}

int swin_glue_add_backward(bool sbf16, bool bf16, const void *grad_y, const void *keep, long long rows,
                           long long rows_per_sample, int C, void *grad_a, hipStream_t stream)
{
    const char *who = entry_name(sbf16, bf16, MSDA_GLUE_NAMES("add_backward"));
    // a bf16 stream without keep: grad_a is grad_y itself, there is nothing to compute
    if (int rc = glue_check(who, rows, rows_per_sample, C, {{grad_y, row_align(sbf16), false}, {keep, elem_align(bf16), !sbf16},
                                                           {grad_a, row_align(bf16), false}}))
        return rc;
    if (rows == 0) return MSDA_OK;
    const dim3 grid((unsigned)((rows + kGlWaves - 1) / kGlWaves)), block(kGlBlock);
#define MSDA_GLUE_CALL(X, T)                                                                                                     \
    hipLaunchKernelGGL((glue_add_bwd_kernel<X, T>), grid, block, 0, stream, (const X *)grad_y, (const T *)keep, rows,            \
                       rows_per_sample, C, (T *)grad_a)
    if (sbf16) MSDA_GLUE_CALL(uint16_t, uint16_t); else if (bf16) MSDA_GLUE_CALL(float, uint16_t); else MSDA_GLUE_CALL(float, float);
#undef MSDA_GLUE_CALL
    return check_launch("msda swin glue add backward");
}

int swin_glue_merge_norm_forward(bool sbf16, bool bf16, const void *x, int B, int H, int W, int C, const float *gamma,
                                 const float *beta, float eps, void *z, float *mean, float *rstd, hipStream_t stream)
{
    const char *who = entry_name(sbf16, bf16, MSDA_GLUE_NAMES("merge_norm_forward"));
    if (int rc = merge_check(who, B, H, W, C)) return rc;
    const MergeGeo geo = merge_geo(H, W, C);
    const long long rows = (long long)B * geo.H2 * geo.W2;
    if (int rc = glue_check(who, rows, 1, 4 * C, {{x, row_align(sbf16), false}, {gamma, 16, false}, {beta, 16, false},
                                                 {z, row_align(bf16), false}, {mean, 4, false}, {rstd, 4, false}}))
        return rc;
#define MSDA_GLUE_CALL(X, T)                                                                                                     \
    glue_fwd<X, T, kMerge>(x, nullptr, nullptr, rows, 1, 4 * C, geo, gamma, beta, eps, nullptr, z, mean, rstd, stream)
    return MSDA_GLUE_PICK(sbf16, bf16, MSDA_GLUE_CALL);
#undef MSDA_GLUE_CALL
}

int swin_glue_merge_norm_backward(bool sbf16, bool bf16, const void *grad_z, const void *x, const float *gamma,
                                  const float *mean, const float *rstd, int B, int H, int W, int C, void *grad_x,
                                  float *grad_gamma, float *grad_beta, void *workspace, unsigned long long workspace_bytes,
                                  hipStream_t stream)
{
    const char *who = entry_name(sbf16, bf16, MSDA_GLUE_NAMES("merge_norm_backward"));
    if (int rc = merge_check(who, B, H, W, C)) return rc;
    const MergeGeo geo = merge_geo(H, W, C);
    const long long rows = (long long)B * geo.H2 * geo.W2;
    if (int rc = glue_check(who, rows, 1, 4 * C, {{grad_z, row_align(bf16), false}, {x, row_align(sbf16), false},
                                                 {gamma, 16, false}, {mean, 4, false}, {rstd, 4, false},
                                                 {grad_x, row_align(sbf16), false}, {grad_gamma, 4, false},
                                                 {grad_beta, 4, false}}))
        return rc;
    if (int rc = glue_check_workspace(who, rows, 4 * C, workspace, workspace_bytes)) return rc;
#define MSDA_GLUE_CALL(X, T)                                                                                                     \
    glue_bwd<X, T, kMerge>(nullptr, grad_z, x, nullptr, gamma, mean, rstd, rows, 1, 4 * C, geo, grad_x, nullptr, grad_gamma,     \
                           grad_beta, (float *)workspace, stream)
    return MSDA_GLUE_PICK(sbf16, bf16, MSDA_GLUE_CALL);
#undef MSDA_GLUE_CALL
}

}  // namespace msda
