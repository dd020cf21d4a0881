// ARCTIC evaluation step (arctic_tools/process.py prepare_data / measure_error, src/utils/eval_modules.py, common/metrics.py,
// engine.py test_pose's per-key means) without host syncs: the nearest-neighbour search that stands where pytorch3d's
// knn_points stands in src/utils/loss_modules.py get_NN, and the six default evaluation metrics of a step.
//
// Nearest neighbour.  A pair is src [B, N1, 3], trg [B, N2, 3]; the pairs of a launch share B and N1 (the two hands of a step).
//   forward   one launch, grid (ceil(N1 / 256), B, pairs): the N2 target points of one (pair, frame) staged once in LDS as
//             three planes (padded to a multiple of 4 with NaN, read as float4: every lane reads the same words, a broadcast);
//             one source point per thread scans them.  d = dx dx + dy dy + dz dz summed in coordinate order; the running
//             minimum is replaced only on strict <, so the lowest index wins a tie and a NaN distance never wins (no
//             finite candidate: distance +inf, index 0).
//   backward  one launch, grid (ceil(N1 / 256) + ceil(N2 / 256), B, pairs).  The first blocks write grad_src[i] =
//             2 g_i (a_i - b_idx[i]).  The others own one target per thread: the frame's idx is staged in LDS (16-bit, N2 <=
//             1024) and every thread walks it in source order, adding -2 g_i (a_i - b_j) where idx[i] == j: a fixed order
//             and no atomics, so two runs are bitwise equal.
//
// Metrics.  One launch, one workgroup per frame, two fixed-order block reductions: the object root (mean of the rows below
// v_len whose part id is 2) of gt and pred, then the v2v success count and the contact deviations; thread 0 finishes the
// six rows (aae, mpjpe/ra/h, mrrpe/r/l, mrrpe/r/o, success_rate/0.05, cdev/ho) in the reference's units with NaN where the
// reference has NaN.  A second one-block launch adds each key's mean over the step's non-NaN frames to device totals
// (engine.py:784-794 + MetricLogger.update: a key that is all NaN in a step is dropped for that step).
#include <cmath>
#include <cstdio>
#include <cstring>

#include "msda_common.h"
#include "msda_launch.h"

namespace msda {

namespace {

constexpr int kBlock = 256;
constexpr int kNNMaxPairs = 8, kNNMaxN1 = 8192, kNNMaxN2 = 1024;
constexpr int kEvMaxJ = 32, kEvMaxNV = 1024, kEvMaxLen = 65536;
constexpr int kMetrics = 6;
constexpr float kContact = 3e-3f, kAlpha = 0.05f, kPi = 3.14159265358979323846f;

enum { M_AAE, M_MPJPE, M_MRRPE_RL, M_MRRPE_RO, M_SUCCESS, M_CDEV };

struct NNPair {
    const float *src, *trg;
    float *dist;
    long long *idx;                 // forward: written; backward: read
    const float *gdist;
    float *gsrc, *gtrg;
};
struct NNArgs {
    NNPair p[kNNMaxPairs];
    int pairs, B, N1, N2, nsb;      // nsb: source blocks per frame of the backward grid
};

__global__ void __launch_bounds__(kBlock) nn_fwd_kernel(NNArgs a)
{
    __shared__ float4 tx[kNNMaxN2 / 4], ty[kNNMaxN2 / 4], tz[kNNMaxN2 / 4];
    const NNPair &P = a.p[blockIdx.z];
    const int b = blockIdx.y, tid = threadIdx.x, N2 = a.N2;
    const int n4 = (N2 + 3) / 4;
    const float *trg = P.trg + (long long)b * N2 * 3;
    for (int j = tid; j < n4 * 4; j += kBlock) {
        const bool in = j < N2;
        ((float *)tx)[j] = in ? trg[3 * j] : NAN;
        ((float *)ty)[j] = in ? trg[3 * j + 1] : NAN;
        ((float *)tz)[j] = in ? trg[3 * j + 2] : NAN;
    }
    __syncthreads();
    const int i = blockIdx.x * kBlock + tid;
    if (i >= a.N1) return;
    const float *s = P.src + ((long long)b * a.N1 + i) * 3;
    const float sx = s[0], sy = s[1], sz = s[2];
    float best = INFINITY;
    int bi = 0;
    for (int q = 0; q < n4; ++q) {
        const float4 X = tx[q], Y = ty[q], Z = tz[q];
        const float xs[4] = {X.x, X.y, X.z, X.w}, ys[4] = {Y.x, Y.y, Y.z, Y.w}, zs[4] = {Z.x, Z.y, Z.z, Z.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float dx = sx - xs[k], dy = sy - ys[k], dz = sz - zs[k];
            float d = dx * dx;
            d += dy * dy;
            d += dz * dz;
            if (d < best) { best = d; bi = 4 * q + k; }
        }
    }
    P.dist[(long long)b * a.N1 + i] = best;
    P.idx[(long long)b * a.N1 + i] = bi;
}

__global__ void __launch_bounds__(kBlock) nn_bwd_kernel(NNArgs a)
{
    __shared__ unsigned short sidx[kNNMaxN1];
    const NNPair &P = a.p[blockIdx.z];
    const int b = blockIdx.y, tid = threadIdx.x, N1 = a.N1, N2 = a.N2;
    const float *src = P.src + (long long)b * N1 * 3, *trg = P.trg + (long long)b * N2 * 3;
    const float *g = P.gdist + (long long)b * N1;
    const long long *idx = P.idx + (long long)b * N1;
    if ((int)blockIdx.x < a.nsb) {
        if (P.gsrc == nullptr) return;
        const int i = blockIdx.x * kBlock + tid;
        if (i >= N1) return;
        const long long j = idx[i];
        float *o = P.gsrc + ((long long)b * N1 + i) * 3;
        if (j < 0 || j >= N2) { o[0] = o[1] = o[2] = 0.f; return; }   // never from the forward; no read out of bounds
        const float w = 2.f * g[i];
        for (int c = 0; c < 3; ++c) o[c] = w * (src[3 * i + c] - trg[3 * j + c]);
        return;
    }
    if (P.gtrg == nullptr) return;
    for (int i = tid; i < N1; i += kBlock) {
        const long long j = idx[i];
        sidx[i] = (j < 0 || j >= N2) ? (unsigned short)0xffff : (unsigned short)j;
    }
    __syncthreads();
    const int j = ((int)blockIdx.x - a.nsb) * kBlock + tid;
    if (j >= N2) return;
    const float bx = trg[3 * j], by = trg[3 * j + 1], bz = trg[3 * j + 2];
    float acc[3] = {0.f, 0.f, 0.f};
    for (int i = 0; i < N1; ++i) {
        if (sidx[i] != (unsigned short)j) continue;
        const float w = 2.f * g[i];
        acc[0] -= w * (src[3 * i] - bx);
        acc[1] -= w * (src[3 * i + 1] - by);
        acc[2] -= w * (src[3 * i + 2] - bz);
    }
    float *o = P.gtrg + ((long long)b * N2 + j) * 3;
    o[0] = acc[0]; o[1] = acc[1]; o[2] = acc[2];
}

// ---- metrics ------------------------------------------------------------------------------------------------------------------
enum { E_RAD_P, E_RAD_G, E_J3D_R_P, E_J3D_L_P, E_J3D_R_G, E_J3D_L_G, E_OBJ_P, E_OBJ_G, E_DIAM, E_IS_VALID, E_LEFT_VALID,
       E_RIGHT_VALID, E_V3D_R_P, E_V3D_L_P, E_DIST_RO, E_DIST_LO, kEvFloats };
enum { E_VLEN, E_PARTS, E_IDX_RO, E_IDX_LO, kEvLongs };

struct EvArgs {
    const float *f[kEvFloats];
    const long long *l[kEvLongs];
    float *out;                     // [6, B]
    int B, J, NV, Lp, Lg, Lparts;   // rows of pred object.v.cam, gt object.v.cam and part_ids per frame
};

__device__ __forceinline__ bool invalid_long(float v) { return (long long)(1.f - v) != 0; }   // (1 - v).long() != 0

// nanmean of two values (torch_utils.nanmean over dim 1 of a [B, 2] stack): 0 / 0 = NaN when both are NaN
__device__ __forceinline__ float nanmean2(float a, float b)
{
    const float n = (isnan(a) ? 0.f : 1.f) + (isnan(b) ? 0.f : 1.f);
    return ((isnan(a) ? 0.f : a) + (isnan(b) ? 0.f : b)) / n;
}

__global__ void __launch_bounds__(kBlock) arctic_metrics_kernel(EvArgs a)
{
    __shared__ float red[7][kBlock];
    __shared__ float jd[2][kEvMaxJ];
    __shared__ float root[6];
    const int b = blockIdx.x, tid = threadIdx.x, J = a.J, NV = a.NV;
    const int Lmin = a.Lp < a.Lg ? a.Lp : a.Lg;
    long long vl = a.l[E_VLEN][b];
    const int vlen = (int)(vl < 0 ? 0 : (vl > Lmin ? Lmin : vl));
    const float *vp = a.f[E_OBJ_P] + (long long)b * a.Lp * 3, *vg = a.f[E_OBJ_G] + (long long)b * a.Lg * 3;
    const long long *parts = a.l[E_PARTS] + (long long)b * a.Lparts;
    const float iv = a.f[E_IS_VALID][b], lv = a.f[E_LEFT_VALID][b] * iv, rv = a.f[E_RIGHT_VALID][b] * iv;

    // object roots: rows below v_len of the bottom part (id 2)
    {
        float acc[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        const int n = vlen < a.Lparts ? vlen : a.Lparts;
        for (int r = tid; r < n; r += kBlock) {
            if (parts[r] != 2) continue;
            for (int c = 0; c < 3; ++c) { acc[c] += vg[3 * r + c]; acc[3 + c] += vp[3 * r + c]; }
            acc[6] += 1.f;
        }
        block_reduce<7>(red, acc);
        if (tid < 6) root[tid] = red[tid][0] / red[6][0];
    }
    // root-relative joint errors, item = (hand, joint); hand 0 = r, 1 = l
    for (int it = tid; it < 2 * J; it += kBlock) {
        const int h = it / J, j = it % J;
        const float *p = a.f[E_J3D_R_P + h] + (long long)b * J * 3, *g = a.f[E_J3D_R_G + h] + (long long)b * J * 3;
        float e = 0.f;
        for (int c = 0; c < 3; ++c) e += sq((g[3 * j + c] - g[c]) - (p[3 * j + c] - p[c]));
        jd[h][j] = sqrtf(e);
    }
    __syncthreads();
    // v2v success count over the real rows, contact deviation over (hand, vertex); hand 0 = r (idx.ro), 1 = l
    float acc[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
    {
        const float thr = a.f[E_DIAM][b] * kAlpha;
        for (int r = tid; r < vlen; r += kBlock) {
            float e = 0.f;
            for (int c = 0; c < 3; ++c) e += sq((vg[3 * r + c] - root[c]) - (vp[3 * r + c] - root[3 + c]));
            if (sqrtf(e) < thr) acc[0] += 1.f;
        }
        for (int it = tid; it < 2 * NV; it += kBlock) {
            const int h = it / NV, k = it % NV;
            if ((1.f - (h ? lv : rv)) != 0.f) continue;                 // contact_deviation: (1 - valid).nonzero(), no .long()
            if (a.f[E_DIST_RO + h][(long long)b * NV + k] > kContact) continue;
            const long long oi = a.l[E_IDX_RO + h][(long long)b * NV + k];
            if (oi < 0 || oi >= a.Lp) continue;                         // the reference's gather would raise
            const float *vh = a.f[E_V3D_R_P + h] + ((long long)b * NV + k) * 3;
            float e = 0.f;
            for (int c = 0; c < 3; ++c) e += sq(vp[3 * oi + c] - vh[c]);
            const float d = sqrtf(e);
            if (isnan(d)) continue;
            acc[1 + 2 * h] += d;
            acc[2 + 2 * h] += 1.f;
        }
    }
    block_reduce<5>(red, acc);
    if (tid != 0) return;
    float *out = a.out;
    const int B = a.B;
    {
        const float e = fabsf(a.f[E_RAD_P][b] / kPi * 180.f - a.f[E_RAD_G][b] / kPi * 180.f);
        out[M_AAE * B + b] = invalid_long(iv) ? NAN : e;
    }
    {
        float m[2];
        for (int h = 0; h < 2; ++h) {
            float s = 0.f;
            for (int j = 0; j < J; ++j) s += jd[h][j];
            m[h] = invalid_long(h ? lv : rv) ? NAN : s / (float)J;
        }
        out[M_MPJPE * B + b] = nanmean2(m[0], m[1]) * 1000.f;
    }
    {
        const float *rp = a.f[E_J3D_R_P] + (long long)b * J * 3, *lp = a.f[E_J3D_L_P] + (long long)b * J * 3;
        const float *rg = a.f[E_J3D_R_G] + (long long)b * J * 3, *lg = a.f[E_J3D_L_G] + (long long)b * J * 3;
        float e_rl = 0.f, e_ro = 0.f;
        for (int c = 0; c < 3; ++c) {
            e_rl += sq((lp[c] - rp[c]) - (lg[c] - rg[c]));
            e_ro += sq((root[3 + c] - rp[c]) - (root[c] - rg[c]));
        }
        out[M_MRRPE_RL * B + b] = (invalid_long(lv * rv) ? NAN : sqrtf(e_rl)) * 1000.f;
        out[M_MRRPE_RO * B + b] = (invalid_long(rv * iv) ? NAN : sqrtf(e_ro)) * 1000.f;
    }
    out[M_SUCCESS * B + b] = iv != 0.f ? red[0][0] / (float)vlen * 100.f : NAN;
    out[M_CDEV * B + b] = nanmean2(red[1][0] / red[2][0], red[3][0] / red[4][0]) * 1000.f;
}

// per key: the mean over this step's non-NaN frames, added to total with 1 to count when there is one
__global__ void arctic_metrics_accumulate_kernel(const float *vals, int B, double *total, double *count)
{
    const int k = threadIdx.x;
    if (k >= kMetrics) return;
    double s = 0.0;
    int n = 0;
    for (int b = 0; b < B; ++b) {
        const float v = vals[k * B + b];
        if (!isnan(v)) { s += (double)v; ++n; }
    }
    if (n > 0) { total[k] += s / (double)n; count[k] += 1.0; }
}

void begin_entry()
{
    set_error(MSDA_OK, "");
    (void)hipGetLastError();
}

int eerr(const char *msg) { return set_error(MSDA_ERR_ARGUMENT, msg); }

bool nn_dims_ok(int B, int N1, int N2)
{
    return B >= 0 && B <= 65535 && N1 >= 1 && N1 <= kNNMaxN1 && N2 >= 1 && N2 <= kNNMaxN2;
}

bool ev_dims_ok(int B, int J, int NV, int Lp, int Lg, int Lparts)
{
    return B >= 0 && (long long)B * kMetrics < (1LL << 31) && J >= 1 && J <= kEvMaxJ && NV >= 1 && NV <= kEvMaxNV && Lp >= 1
           && Lp <= kEvMaxLen && Lg >= 1 && Lg <= kEvMaxLen && Lparts >= 1 && Lparts <= kEvMaxLen;
}

int nn_setup(NNArgs &a, int n_pairs, int B, int N1, int N2, const float *const *src, const float *const *trg)
{
    memset(&a, 0, sizeof(a));
    if (n_pairs < 1 || n_pairs > kNNMaxPairs) return eerr("msda_nn: 1 .. 8 pairs");
    if (!nn_dims_ok(B, N1, N2)) return eerr("msda_nn: unsupported geometry (msda_nn_supported)");
    if (src == nullptr || trg == nullptr) return eerr("msda_nn: null pointer");
    a.pairs = n_pairs; a.B = B; a.N1 = N1; a.N2 = N2;
    for (int i = 0; i < n_pairs; ++i) {
        a.p[i].src = src[i]; a.p[i].trg = trg[i];
        if (B > 0 && (!src[i] || !trg[i])) return eerr("msda_nn: null pointer");
    }
    return MSDA_OK;
}

}  // namespace

}  // namespace msda

using namespace msda;

int msda_nn_supported(int B, int N1, int N2) { return nn_dims_ok(B, N1, N2) ? 1 : 0; }

int msda_nn_forward_f32(int n_pairs, int B, int N1, int N2, const float *const *src, const float *const *trg, float *const *dists,
                        long long *const *idx, msda_stream_t stream)
{
    NNArgs a;
    int rc = nn_setup(a, n_pairs, B, N1, N2, src, trg);
    if (rc != MSDA_OK) return rc;
    if (dists == nullptr || idx == nullptr) return eerr("msda_nn: null pointer");
    for (int i = 0; i < n_pairs; ++i) {
        a.p[i].dist = dists[i]; a.p[i].idx = idx[i];
        if (B > 0 && (!dists[i] || !idx[i])) return eerr("msda_nn: null output");
    }
    begin_entry();
    if (B == 0) return MSDA_OK;
    hipLaunchKernelGGL(nn_fwd_kernel, dim3((unsigned)((N1 + kBlock - 1) / kBlock), (unsigned)B, (unsigned)n_pairs), dim3(kBlock), 0,
                       (hipStream_t)stream, a);
    return check_launch("nn_fwd_kernel");
}

int msda_nn_backward_f32(int n_pairs, int B, int N1, int N2, const float *const *src, const float *const *trg,
                         const long long *const *idx, const float *const *grad_dists, float *const *grad_src,
                         float *const *grad_trg, msda_stream_t stream)
{
    NNArgs a;
    int rc = nn_setup(a, n_pairs, B, N1, N2, src, trg);
    if (rc != MSDA_OK) return rc;
    if (idx == nullptr || grad_dists == nullptr || grad_src == nullptr || grad_trg == nullptr) return eerr("msda_nn: null pointer");
    for (int i = 0; i < n_pairs; ++i) {
        a.p[i].idx = const_cast<long long *>(idx[i]); a.p[i].gdist = grad_dists[i];
        a.p[i].gsrc = grad_src[i]; a.p[i].gtrg = grad_trg[i];
        if (B > 0 && (!idx[i] || !grad_dists[i])) return eerr("msda_nn: null pointer");
    }
    begin_entry();
    if (B == 0) return MSDA_OK;
    a.nsb = (N1 + kBlock - 1) / kBlock;
    hipLaunchKernelGGL(nn_bwd_kernel, dim3((unsigned)(a.nsb + (N2 + kBlock - 1) / kBlock), (unsigned)B, (unsigned)n_pairs),
                       dim3(kBlock), 0, (hipStream_t)stream, a);
    return check_launch("nn_bwd_kernel");
}

int msda_arctic_metrics_supported(int B, int J, int NV, int L_pred, int L_gt, int L_parts)
{
    return ev_dims_ok(B, J, NV, L_pred, L_gt, L_parts) ? 1 : 0;
}

int msda_arctic_metrics_f32(const int *dims, const float *const *floats, const long long *const *longs, float *out,
                            msda_stream_t stream)
{
    if (dims == nullptr || floats == nullptr || longs == nullptr || out == nullptr) return eerr("msda_arctic_metrics: null pointer");
    if (!ev_dims_ok(dims[0], dims[1], dims[2], dims[3], dims[4], dims[5]))
        return eerr("msda_arctic_metrics: unsupported geometry (msda_arctic_metrics_supported)");
    EvArgs a;
    memset(&a, 0, sizeof(a));
    a.B = dims[0]; a.J = dims[1]; a.NV = dims[2]; a.Lp = dims[3]; a.Lg = dims[4]; a.Lparts = dims[5];
    for (int k = 0; k < kEvFloats; ++k) {
        a.f[k] = floats[k];
        if (a.B > 0 && a.f[k] == nullptr) return eerr("msda_arctic_metrics: null input");
    }
    for (int k = 0; k < kEvLongs; ++k) {
        a.l[k] = longs[k];
        if (a.B > 0 && a.l[k] == nullptr) return eerr("msda_arctic_metrics: null input");
    }
    a.out = out;
    begin_entry();
    if (a.B == 0) return MSDA_OK;
    hipLaunchKernelGGL(arctic_metrics_kernel, dim3((unsigned)a.B), dim3(kBlock), 0, (hipStream_t)stream, a);
    return check_launch("arctic_metrics_kernel");
}

int msda_arctic_metrics_accumulate_f32(const float *values, int B, double *total, double *count, msda_stream_t stream)
{
    if (values == nullptr || total == nullptr || count == nullptr) return eerr("msda_arctic_metrics_accumulate: null pointer");
    if (B < 0 || (long long)B * kMetrics >= (1LL << 31)) return eerr("msda_arctic_metrics_accumulate: bad frame count");
    begin_entry();
    if (B == 0) return MSDA_OK;
    hipLaunchKernelGGL(arctic_metrics_accumulate_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, values, B, total, count);
    return check_launch("arctic_metrics_accumulate_kernel");
}
