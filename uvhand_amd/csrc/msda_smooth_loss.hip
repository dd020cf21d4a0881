// The SmoothNet criterion (arctic_tools/src/callbacks/loss/loss_arctic_sf.py compute_smoothnet_loss): the contact deviation
// `loss/cd` (src/utils/loss_modules.py compute_contact_devi_loss) and the acceleration errors `acc/h`, `acc/o`
// (src/utils/eval_modules.py eval_acc_pose, compute_error_accel) of N = B * T frames, without host syncs.
//
// Per frame: hand vertices [NV, 3] and joints [J, 3] (row 0 = the root) of r and l, object vertices [L, 3] (padded), for the
// prediction and the ground truth; dist / idx [NV] per hand, the three validity flags; parts_ids [N, L] of which ROW 0 decides
// the bottom columns of every frame (parts_ids[0] == 2), as the reference does.
//   forward   3 launches whatever the data holds.  (1) one workgroup per (frame, pred | gt): the object root, the mean of the
//             bottom columns, summed and kept in fp64.  (2) one workgroup per (frame, body r | l | o): the centre frame's acceleration error, the mean over
//             all columns of |a_pred - a_gt| with a = (x[t-1] - 2 x[t] + x[t+1]) fps^2 on root-relative vertices, and for the
//             hands the frame's contact sum and count.  (3) one workgroup: the convolve validity (the three flags around t sum to 3
//             after truncation to int64, in fp64), every nanmean over frames, the "any non-NaN" gates, nan_to_num, and the
//             per-frame weights the backward reads.
//   backward  1 launch, one workgroup per frame: each (frame, vertex) recomputes the unit vectors of its up to three centre
//             frames and writes its gradient once; the root's gradient is the negated sum of the frame, reduced in the
//             workgroup: joints row 0 for a hand, 1 / nb onto each bottom column for the object (second phase, after the
//             barrier).  The contact gradient onto object rows is added by the first contact of each row, which sums all
//             contacts of that row in (hand, vertex) order, as msda_small_loss.hip does; the contacts are sorted by (row, item)
//             in LDS first, so that finding a row's contacts is no search.  acc_grad = 0 skips the acceleration
//             part: only the contact gradient is written.
// A zero difference vector has a zero acceleration gradient (torch's norm); a zero contact displacement divides by zero as
// torch's sqrt backward does.  Fixed summation order everywhere, no atomics: bitwise reproducible.  Everything is fp32 but the
// object roots, which are summed, stored (workspace) and subtracted in fp64, and the validity sum.
#include <cmath>
#include <cstring>

#include "msda_common.h"
#include "msda_launch.h"

namespace msda {

namespace {

constexpr int kBlock = 256, kBwdBlock = 512;
constexpr int kMaxN = 8192, kMaxNV = 1024, kMaxJ = 64, kMaxLen = 65536;
constexpr int kFloats = 15, kLongs = 3, kGrads = 5;
constexpr float kContact = 3e-3f;
constexpr int kItemBits = 11;                        // 2 kMaxNV items; a padded object row takes 17 bits above them
constexpr unsigned kNoKey = 0xffffffffu;
static_assert(2 * kMaxNV <= (1 << kItemBits) && kMaxLen <= (1 << (32 - kItemBits - 1)), "contact keys");

// floats table
enum { F_VR, F_VL, F_JR, F_JL, F_VO, F_GVR, F_GVL, F_GJR, F_GJL, F_GVO, F_DIST_RO, F_DIST_LO, F_IS_VALID, F_LEFT_VALID, F_RIGHT_VALID };
// longs table
enum { G_IDX_RO, G_IDX_LO, G_PARTS };
// gradient table
enum { D_VR, D_VL, D_JR, D_JL, D_VO };

struct SMArgs {
    int N, NV, J, L, acc_grad;
    float fps2;
    const float *f[kFloats];
    const long long *g[kLongs];
    float *grad[kGrads];
    const float *glosses;
    float *losses, *frames;
    // workspace: object roots [2][N][3] in fp64, then fp32: err [3][N], contact sum and count [2][N] each, weights [3][N],
    // coefficients [4]
    double *root;
    float *err, *cds, *cdn, *wt, *coef;
};

// body 0 = r, 1 = l, 2 = o: vertices, rows per frame and the per-frame roots of the prediction (which = 0) or the gt (1)
struct Body {
    const float *v, *root;          // root: a hand's joints (row 0 of a frame), null for the object
    const double *rootd;            // the object's roots [N][3]
    int rows;
    long long root_stride;
};

__device__ __forceinline__ Body body_of(const SMArgs &a, int body, int which)
{
    Body b;
    if (body < 2) {
        b.v = a.f[(which ? F_GVR : F_VR) + body];
        b.root = a.f[(which ? F_GJR : F_JR) + body];
        b.rootd = nullptr;
        b.rows = a.NV;
        b.root_stride = (long long)a.J * 3;
    } else {
        b.v = a.f[which ? F_GVO : F_VO];
        b.root = nullptr;
        b.rootd = a.root + (long long)which * a.N * 3;
        b.rows = a.L;
        b.root_stride = 3;
    }
    return b;
}

// the acceleration of vertex v at centre frame c on root-relative coordinates: ((x[c-1] - 2 x[c]) + x[c+1]) fps^2.  The
// object's root is a mean of coordinates near z = 12 m: it is kept in fp64 and subtracted in fp64, so that x - root, of the
// object's size, is rounded to fp32 once instead of carrying the mean's fp32 rounding, which the stencil multiplies by 900.
__device__ __forceinline__ void accel(const Body &b, int c, int v, float fps2, float out[3])
{
    const long long fs = (long long)b.rows * 3;
    const float *x = b.v + (long long)(c - 1) * fs + 3LL * v;
    for (int q = 0; q < 3; ++q) {
        float x0, x1, x2;
        if (b.rootd) {
            const double *r = b.rootd + (long long)(c - 1) * 3;
            x0 = (float)((double)x[q] - r[q]); x1 = (float)((double)x[fs + q] - r[3 + q]); x2 = (float)((double)x[2 * fs + q] - r[6 + q]);
        } else {
            const float *r = b.root + (long long)(c - 1) * b.root_stride;
            x0 = x[q] - r[q]; x1 = x[fs + q] - r[b.root_stride + q]; x2 = x[2 * fs + q] - r[2 * b.root_stride + q];
        }
        out[q] = ((x0 - 2.f * x1) + x2) * fps2;
    }
}

// forward launch 1: the object root of (frame, pred | gt), summed in fp64 (strided partials, then a fixed-order tree)
__global__ void __launch_bounds__(kBlock) sm_root_kernel(SMArgs a)
{
    __shared__ double red[4][kBlock];
    const int t = blockIdx.x, which = blockIdx.y, tid = threadIdx.x;
    const float *v = a.f[which ? F_GVO : F_VO] + (long long)t * a.L * 3;
    const long long *parts = a.g[G_PARTS];
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (int i = tid; i < a.L; i += kBlock)
        if (parts[i] == 2) {
            acc[0] += v[3 * i]; acc[1] += v[3 * i + 1]; acc[2] += v[3 * i + 2];
            acc[3] += 1.0;
        }
    for (int k = 0; k < 4; ++k) red[k][tid] = acc[k];
    __syncthreads();
    for (int w = kBlock / 2; w > 0; w >>= 1) {
        if (tid < w)
            for (int k = 0; k < 4; ++k) red[k][tid] += red[k][tid + w];
        __syncthreads();
    }
    if (tid < 3) a.root[((long long)which * a.N + t) * 3 + tid] = red[tid][0] / red[3][0];      // no bottom column: NaN, as torch
    if (tid == 0 && t == 0 && which == 0) a.coef[2] = (float)red[3][0];
}

__device__ __forceinline__ float hand_flag(const SMArgs &a, int body, int t)
{
    const float iv = a.f[F_IS_VALID][t];
    return body == 0 ? a.f[F_RIGHT_VALID][t] * iv : (body == 1 ? a.f[F_LEFT_VALID][t] * iv : iv);
}

// contact of (hand, frame t, vertex k): the displacement object row - hand vertex; false when the pair does not count
__device__ __forceinline__ bool contact(const SMArgs &a, int h, int t, int k, float d[3], float &dn, long long &oi)
{
    if (hand_flag(a, h, t) != 1.f) return false;                         // (1 - valid) != 0
    const long long e = (long long)t * a.NV + k;
    if (a.f[F_DIST_RO + h][e] > kContact) return false;
    oi = a.g[G_IDX_RO + h][e];
    if (oi < 0 || oi >= a.L) return false;
    const float *vo = a.f[F_VO] + ((long long)t * a.L + oi) * 3, *vh = a.f[F_VR + h] + e * 3;
    float d2 = 0.f;
    for (int q = 0; q < 3; ++q) { d[q] = vo[q] - vh[q]; d2 += d[q] * d[q]; }
    dn = sqrtf(d2);
    return !isnan(dn);                                                   // nanmean leaves a NaN distance out
}

// forward launch 2: per (frame, body) the acceleration error of the centre frame and the hand's contact partials
__global__ void __launch_bounds__(kBlock) sm_part_kernel(SMArgs a)
{
    __shared__ float red[3][kBlock];
    const int t = blockIdx.x, body = blockIdx.y, tid = threadIdx.x;
    float acc[3] = {0.f, 0.f, 0.f};
    if (t >= 1 && t <= a.N - 2) {
        const Body p = body_of(a, body, 0), g = body_of(a, body, 1);
        for (int v = tid; v < p.rows; v += kBlock) {
            float ap[3], ag[3], n2 = 0.f;
            accel(p, t, v, a.fps2, ap);
            accel(g, t, v, a.fps2, ag);
            for (int q = 0; q < 3; ++q) { const float e = ap[q] - ag[q]; n2 += e * e; }
            acc[0] += sqrtf(n2);
        }
    }
    if (body < 2)
        for (int k = tid; k < a.NV; k += kBlock) {
            float d[3], dn;
            long long oi;
            if (contact(a, body, t, k, d, dn, oi)) { acc[1] += dn; acc[2] += 1.f; }
        }
    block_reduce<3, kBlock>(red, acc);
    if (tid == 0) {
        a.err[(long long)body * a.N + t] = red[0][0] / (float)(body < 2 ? a.NV : a.L);
        if (body < 2) {
            a.cds[(long long)body * a.N + t] = red[1][0];
            a.cdn[(long long)body * a.N + t] = red[2][0];
        }
    }
}

// np.convolve(valid, ones(3), 'valid').astype(int64) == 3 at centre frame c
__device__ __forceinline__ bool centre_valid(const SMArgs &a, int body, int c)
{
    const double s = (double)hand_flag(a, body, c - 1) + (double)hand_flag(a, body, c) + (double)hand_flag(a, body, c + 1);
    return s == s && fabs(s) < 9e18 && (long long)s == 3;                // a NaN or infinite flag never counts (numpy: INT64_MIN)
}

__device__ __forceinline__ float nan_to_num(float v)
{
    if (isnan(v)) return 0.f;
    if (isinf(v)) return v > 0.f ? 3.4028234663852886e38f : -3.4028234663852886e38f;
    return v;
}

// forward launch 3: one workgroup.  Per-thread strided partials, then the fixed-order tree: (sum, count) of acc/h, of acc/o and
// of each hand's per-frame contact means.
__global__ void __launch_bounds__(kBlock) sm_final_kernel(SMArgs a)
{
    __shared__ float red[8][kBlock];
    const int N = a.N, tid = threadIdx.x;
    const float nan = NAN;
    float acc[8];
    for (int k = 0; k < 8; ++k) acc[k] = 0.f;
    // acc/h: per centre frame the nanmean of (r, l), then the nanmean over frames; acc/o
    for (int c = 1 + tid; c <= N - 2; c += kBlock) {
        float e[3];
        bool ok[3];
        for (int b = 0; b < 3; ++b) {
            e[b] = a.err[(long long)b * N + c];
            ok[b] = centre_valid(a, b, c) && !isnan(e[b]);
        }
        const int k = (ok[0] ? 1 : 0) + (ok[1] ? 1 : 0);
        const float h = k ? ((ok[0] ? e[0] : 0.f) + (ok[1] ? e[1] : 0.f)) / (float)k : nan;
        if (k) { acc[0] += h; acc[1] += 1.f; }
        if (ok[2]) { acc[2] += e[2]; acc[3] += 1.f; }
        // weights of the backward, still to be divided by the number of counted frames
        a.wt[c] = ok[0] ? 1.f / (float)k : 0.f;
        a.wt[N + c] = ok[1] ? 1.f / (float)k : 0.f;
        a.wt[2 * N + c] = ok[2] ? 1.f : 0.f;
        if (a.frames) { a.frames[c] = h; a.frames[N + c - 1] = ok[2] ? e[2] : nan; }
    }
    // loss/cd: per frame the nanmean over the contacts, then the nanmean over frames
    for (int t = tid; t < N; t += kBlock)
        for (int h = 0; h < 2; ++h) {
            const float cnt = a.cdn[(long long)h * N + t];
            if (cnt > 0.f) { acc[4 + 2 * h] += a.cds[(long long)h * N + t] / cnt; acc[5 + 2 * h] += 1.f; }
        }
    block_reduce<8, kBlock>(red, acc);
    const float n_h = red[1][0], n_o = red[3][0];
    for (int c = 1 + tid; c <= N - 2; c += kBlock)                       // the thread that wrote them
        for (int b = 0; b < 3; ++b)
            if (a.wt[(long long)b * N + c] != 0.f) a.wt[(long long)b * N + c] /= b < 2 ? n_h : n_o;
    if (tid != 0) return;
    for (int b = 0; b < 3; ++b) {
        a.wt[(long long)b * N] = 0.f;
        a.wt[(long long)b * N + N - 1] = 0.f;
    }
    if (a.frames) {
        a.frames[0] = nan;
        a.frames[N - 1] = nan;
        if (N >= 2) { a.frames[N + N - 2] = nan; a.frames[N + N - 1] = nan; }
    }
    float cd = 0.f;                                                      // nan_to_num, r then l
    for (int h = 0; h < 2; ++h) {
        const float nf = red[5 + 2 * h][0];
        a.coef[h] = nf > 0.f ? 1.f / nf : 0.f;
        if (nf > 0.f) cd += nan_to_num(red[4 + 2 * h][0] / nf);
    }
    a.losses[0] = cd;
    a.losses[1] = n_h > 0.f ? red[0][0] / n_h : 0.f;
    a.losses[2] = n_o > 0.f ? red[2][0] / n_o : 0.f;
}

// d (acc loss) / d x[t, v] of one body on root-relative coordinates: over the centre frames c = t-1, t, t+1 that count,
// weight(c) * stencil(c) * fps^2 / rows * e / |e|
__device__ __forceinline__ void accel_grad(const SMArgs &a, const Body &p, const Body &g, const float *wt, float up, int t, int v,
                                           float out[3])
{
    out[0] = out[1] = out[2] = 0.f;
    for (int c = t - 1; c <= t + 1; ++c) {
        if (c < 1 || c > a.N - 2) continue;
        const float w = wt[c];
        if (w == 0.f) continue;
        float ap[3], ag[3], e[3], n2 = 0.f;
        accel(p, c, v, a.fps2, ap);
        accel(g, c, v, a.fps2, ag);
        for (int q = 0; q < 3; ++q) { e[q] = ap[q] - ag[q]; n2 += e[q] * e[q]; }
        const float n = sqrtf(n2);
        if (!(n > 0.f)) continue;                                        // zero vector (or NaN): no gradient
        const float s = (c == t ? -2.f : 1.f) * (up * w) * a.fps2 / (float)p.rows / n;
        for (int q = 0; q < 3; ++q) out[q] += s * e[q];
    }
}

// backward: one workgroup of kBwdBlock threads per frame (the frame's loops are short and serial: more threads, fewer rounds)
__global__ void __launch_bounds__(kBwdBlock) sm_bwd_kernel(SMArgs a)
{
    __shared__ float red[9][kBwdBlock];
    __shared__ float sgd[2 * kMaxNV][3];
    __shared__ unsigned skey[2 * kMaxNV];                                // (object row << 11) | item, kNoKey: no contact
    const int t = blockIdx.x, tid = threadIdx.x, N = a.N, NV = a.NV, L = a.L;
    int P = 1;                                                           // the sort's length: a power of two >= 2 NV
    while (P < 2 * NV) P <<= 1;
    for (int it = 2 * NV + tid; it < P; it += kBwdBlock) skey[it] = kNoKey;
    const float g_cd = a.glosses[0], g_h = a.glosses[1], g_o = a.glosses[2];
    float rs[9];
    for (int k = 0; k < 9; ++k) rs[k] = 0.f;
    float *gvo = a.grad[D_VO] + (long long)t * L * 3;
    // hands: the acceleration gradient, then the contact gradient of the same vertex
    for (int it = tid; it < 2 * NV; it += kBwdBlock) {
        const int h = it / NV, k = it % NV;
        float gv[3] = {0.f, 0.f, 0.f};
        if (a.acc_grad && g_h != 0.f) {
            accel_grad(a, body_of(a, h, 0), body_of(a, h, 1), a.wt + (long long)h * N, g_h, t, k, gv);
            for (int q = 0; q < 3; ++q) { rs[q] += h == 0 ? gv[q] : 0.f; rs[3 + q] += h == 1 ? gv[q] : 0.f; }   // static indices
        }
        float d[3], dn;
        long long oi;
        skey[it] = kNoKey;
        const float cnt = a.cdn[(long long)h * N + t], c = a.coef[h];
        if (c != 0.f && cnt > 0.f && contact(a, h, t, k, d, dn, oi)) {
            const float w = g_cd * c / cnt / dn;
            for (int q = 0; q < 3; ++q) {
                const float gq = w * d[q];
                gv[q] -= gq;
                sgd[it][q] = gq;
            }
            skey[it] = ((unsigned)oi << kItemBits) | (unsigned)it;
        }
        float *gh = a.grad[D_VR + h] + ((long long)t * NV + k) * 3;
        gh[0] = gv[0]; gh[1] = gv[1]; gh[2] = gv[2];
    }
    // object: the acceleration gradient (or zeros)
    {
        const Body p = body_of(a, 2, 0), g = body_of(a, 2, 1);
        for (int v = tid; v < L; v += kBwdBlock) {
            float gv[3] = {0.f, 0.f, 0.f};
            if (a.acc_grad && g_o != 0.f) {
                accel_grad(a, p, g, a.wt + 2LL * N, g_o, t, v, gv);
                for (int q = 0; q < 3; ++q) rs[6 + q] += gv[q];
            }
            gvo[3 * v] = gv[0]; gvo[3 * v + 1] = gv[1]; gvo[3 * v + 2] = gv[2];
        }
    }
    block_reduce<9, kBwdBlock>(red, rs);
    if (a.acc_grad) {
        // the roots: joints row 0 of each hand (the other rows have no gradient), 1 / nb onto the object's bottom columns
        for (int e = tid; e < 2 * a.J * 3; e += kBwdBlock) {
            const int h = e / (a.J * 3), r = e % (a.J * 3);
            a.grad[D_JR + h][(long long)t * a.J * 3 + r] = r < 3 ? -red[3 * h + r][0] : 0.f;
        }
        const float nb = a.coef[2];
        const long long *parts = a.g[G_PARTS];
        if (g_o != 0.f)
            for (int v = tid; v < L; v += kBwdBlock)
                if (parts[v] == 2)
                    for (int q = 0; q < 3; ++q) gvo[3 * v + q] += -red[6 + q][0] / nb;
    }
    __syncthreads();
    // sort the contacts by (object row, item) in LDS (bitonic), so that the contacts of a row are neighbours in (hand, vertex)
    // order; the first of each row then adds them all, one after the other
    for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < P; i += kBwdBlock) {
                const int x = i ^ j;
                if (x > i) {
                    const unsigned u = skey[i], w = skey[x];
                    if ((u > w) == ((i & k) == 0)) { skey[i] = w; skey[x] = u; }
                }
            }
            __syncthreads();
        }
    for (int i = tid; i < P; i += kBwdBlock) {
        const unsigned key = skey[i];
        if (key == kNoKey) continue;
        const unsigned d = key >> kItemBits;
        if (i > 0 && (skey[i - 1] >> kItemBits) == d) continue;
        float acc[3] = {gvo[3 * d], gvo[3 * d + 1], gvo[3 * d + 2]};
        for (int p = i; p < P && (skey[p] >> kItemBits) == d; ++p) {
            const unsigned it = skey[p] & ((1u << kItemBits) - 1u);
            acc[0] += sgd[it][0]; acc[1] += sgd[it][1]; acc[2] += sgd[it][2];
        }
        gvo[3 * d] = acc[0]; gvo[3 * d + 1] = acc[1]; gvo[3 * d + 2] = acc[2];
    }
}

// ---- host side ----------------------------------------------------------------------------------------------------------------
void begin_entry()
{
    set_error(MSDA_OK, "");
    (void)hipGetLastError();
}

int serr(const char *msg) { return set_error(MSDA_ERR_ARGUMENT, msg); }

bool dims_ok(int N, int NV, int J, int L)
{
    // N L 3 stays below 2^31 at these limits; the kernels index with 64-bit offsets all the same
    return N >= 1 && N <= kMaxN && NV >= 1 && NV <= kMaxNV && J >= 1 && J <= kMaxJ && L >= 1 && L <= kMaxLen;
}

unsigned long long ws_floats(int N) { return 22ULL * N + 4; }      // 6 N doubles, then 10 N + 4 floats

int setup(SMArgs &a, const int *dims, float fps, const float *const *floats, const long long *const *longs, void *workspace,
          unsigned long long workspace_bytes)
{
    memset(&a, 0, sizeof(a));
    if (dims == nullptr || floats == nullptr || longs == nullptr) return serr("msda_smooth_loss: null pointer");
    if (!dims_ok(dims[0], dims[1], dims[2], dims[3])) return serr("msda_smooth_loss: unsupported geometry");
    if (!(fps > 0.f)) return serr("msda_smooth_loss: fps must be positive");
    a.N = dims[0]; a.NV = dims[1]; a.J = dims[2]; a.L = dims[3];
    a.fps2 = fps * fps;
    for (int k = 0; k < kFloats; ++k) {
        a.f[k] = floats[k];
        if (a.f[k] == nullptr) return serr("msda_smooth_loss: null float tensor");
    }
    for (int k = 0; k < kLongs; ++k) {
        a.g[k] = longs[k];
        if (a.g[k] == nullptr) return serr("msda_smooth_loss: null int64 tensor");
    }
    if (workspace == nullptr || workspace_bytes < ws_floats(a.N) * sizeof(float))
        return serr("msda_smooth_loss: workspace smaller than msda_smooth_loss_workspace_bytes");
    if (((uintptr_t)workspace & 7) != 0) return serr("msda_smooth_loss: workspace must be 8-byte aligned");
    const long long N = a.N;
    a.root = static_cast<double *>(workspace);                // 6 N doubles = 12 N floats
    float *w = static_cast<float *>(workspace) + 12 * N;      // the fp32 part
    a.err = w; a.cds = w + 3 * N; a.cdn = w + 5 * N; a.wt = w + 7 * N; a.coef = w + 10 * N;
    return MSDA_OK;
}

}  // namespace

}  // namespace msda

using namespace msda;

int msda_smooth_loss_supported(int N, int NV, int J, int L) { return dims_ok(N, NV, J, L) ? 1 : 0; }

unsigned long long msda_smooth_loss_workspace_bytes(int N, int NV, int J, int L)
{
    return dims_ok(N, NV, J, L) ? ws_floats(N) * sizeof(float) : 0;
}

int msda_smooth_loss_forward_f32(const int *dims, float fps, const float *const *floats, const long long *const *longs,
                                 float *losses, float *frames, void *workspace, unsigned long long workspace_bytes,
                                 msda_stream_t stream)
{
    SMArgs a;
    int rc = setup(a, dims, fps, floats, longs, workspace, workspace_bytes);
    if (rc != MSDA_OK) return rc;
    if (losses == nullptr) return serr("msda_smooth_loss: null losses");
    a.losses = losses;
    a.frames = frames;
    begin_entry();
    hipLaunchKernelGGL(sm_root_kernel, dim3((unsigned)a.N, 2), dim3(kBlock), 0, (hipStream_t)stream, a);
    rc = check_launch("sm_root_kernel");
    if (rc != MSDA_OK) return rc;
    hipLaunchKernelGGL(sm_part_kernel, dim3((unsigned)a.N, 3), dim3(kBlock), 0, (hipStream_t)stream, a);
    rc = check_launch("sm_part_kernel");
    if (rc != MSDA_OK) return rc;
    hipLaunchKernelGGL(sm_final_kernel, dim3(1), dim3(kBlock), 0, (hipStream_t)stream, a);
    return check_launch("sm_final_kernel");
}

int msda_smooth_loss_backward_f32(const int *dims, float fps, const float *const *floats, const long long *const *longs,
                                  const float *grad_losses, int acc_grad, float *const *grads, const void *workspace,
                                  unsigned long long workspace_bytes, msda_stream_t stream)
{
    SMArgs a;
    int rc = setup(a, dims, fps, floats, longs, const_cast<void *>(workspace), workspace_bytes);
    if (rc != MSDA_OK) return rc;
    if (grad_losses == nullptr || grads == nullptr) return serr("msda_smooth_loss: null pointer");
    a.acc_grad = acc_grad ? 1 : 0;
    a.glosses = grad_losses;
    for (int k = 0; k < kGrads; ++k) {
        a.grad[k] = grads[k];
        const bool joints = k == D_JR || k == D_JL;
        if (a.grad[k] == nullptr && (!joints || a.acc_grad)) return serr("msda_smooth_loss: null gradient");
    }
    begin_entry();
    hipLaunchKernelGGL(sm_bwd_kernel, dim3((unsigned)a.N), dim3(kBwdBlock), 0, (hipStream_t)stream, a);
    return check_launch("sm_bwd_kernel");
}
