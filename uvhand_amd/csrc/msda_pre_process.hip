// ARCTIC target preparation (arctic_tools/process.py arctic_pre_process over src/callbacks/process/process_arctic.py
// process_data) without host syncs: the two pieces that are neither the MANO layer, the object layer nor a translation.
//
// Target fit.  One launch, one wavefront per frame.  The lanes stage the frame's keypoints, intrinsics and joints in LDS and
//   test them for non-finite values; lane 0 runs the fp64 algebra of msda_pre_fit.h in a fixed order (centroids, H, the
//   rotation of Arun's method, T0, the 3 x 3 normal equations of estimate_translation_k_np); the lanes then move the joints
//   (j0 = R0 j_full + T0, one joint per lane), lanes 0 .. 5 sum j0 - j_cano over the joints in joint order, and every output
//   is rounded to fp32 once.  Stands where batch_solve_rigid_tf's and estimate_translation_k's host round trips stand.
//
// Distance fields.  One launch, grid (B, 2 ceil(NV / 256) + 2 ceil(L / 256)): the blocks of a frame are four jobs, hand r
//   -> object, hand l -> object, object -> hand r, object -> hand l (interfield.py compute_dist_mano_to_obj /
//   compute_dist_obj_to_mano, i.e. knn_points with K = 1 and lengths on the object).  A block owns 256 sources and walks
//   its target in LDS chunks of kChunk points (three planes padded with NaN to a multiple of 4, read as float4 broadcasts),
//   up to v_len[b] rows when the target is the object.  nn_fwd_kernel's conventions (msda_arctic_eval.hip): d = dx dx + dy dy
//   + dz dz in that order, strict < (lowest index on a tie, a NaN distance never wins); the value is clamp(sqrt(d), dist_min,
//   dist_max).  Object rows at or beyond v_len are never candidates and, as sources, get 0 before the clamp and index 0;
//   with v_len = 0 every hand vertex gets the same.
#include <cmath>
#include <cstdio>
#include <cstring>

#include "msda_common.h"
#include "msda_launch.h"
#include "msda_pre_fit.h"

namespace msda {

namespace {

constexpr int kFitBlock = 64, kFitMaxNK = 64, kFitMaxJ = 32;
constexpr int kDfBlock = 256, kChunk = 1024, kDfMaxNV = 1024, kDfMaxL = 65536;

enum { F_KP_FULL, F_KP_CANO, F_KP2D, F_K, F_JFULL_R, F_JFULL_L, F_JCANO_R, F_JCANO_L, kFitInputs };
enum { O_R0, O_T0, O_TRANSL, O_J3D_R, O_J3D_L, O_CAMT_R, O_CAMT_L, O_WP_R, O_WP_L, O_WP_O, O_OFF_R, O_OFF_L, kFitOutputs };

struct FitArgs {
    const float *in[kFitInputs];
    float *out[kFitOutputs];
    int *status;
    int B, NK, J;
    float img_res;
};

__device__ __forceinline__ bool finite3(const float *p, int n)
{
    bool ok = true;
    for (int i = 0; i < n; ++i) ok = ok && isfinite(p[i]);
    return ok;
}

__global__ void __launch_bounds__(kFitBlock) pre_fit_kernel(FitArgs a)
{
    __shared__ float kf[kFitMaxNK * 3], kc[kFitMaxNK * 3], k2[kFitMaxNK * 2], Km[9];
    __shared__ double sR[9], sT0[3], st[3], dj[2][kFitMaxJ][3];
    __shared__ int sbad;
    const int b = blockIdx.x, tid = threadIdx.x, NK = a.NK, J = a.J;
    const long long kb = (long long)b * NK, jb = (long long)b * J * 3;
    if (tid == 0) sbad = 0;
    __syncthreads();
    bool ok = true;
    if (tid < NK) {
        for (int c = 0; c < 3; ++c) {
            kf[3 * tid + c] = a.in[F_KP_FULL][(kb + tid) * 3 + c];
            kc[3 * tid + c] = a.in[F_KP_CANO][(kb + tid) * 3 + c];
        }
        for (int c = 0; c < 2; ++c) k2[2 * tid + c] = a.in[F_KP2D][(kb + tid) * 2 + c];
        ok = finite3(kf + 3 * tid, 3) && finite3(kc + 3 * tid, 3) && finite3(k2 + 2 * tid, 2);
    }
    if (tid < 9) {
        Km[tid] = a.in[F_K][(long long)b * 9 + tid];
        ok = ok && isfinite(Km[tid]);
    }
    // item = (hand, joint): its full-space and canonical joint; hand 0 = r, 1 = l
    double jf[3] = {0.0, 0.0, 0.0}, jc[3] = {0.0, 0.0, 0.0};
    const int h = tid / J, j = tid % J;          // J <= 32: 2 J items fit the 64 lanes
    const bool item = tid < 2 * J;
    if (item) {
        for (int c = 0; c < 3; ++c) {
            const float f = a.in[F_JFULL_R + h][jb + 3 * j + c], cn = a.in[F_JCANO_R + h][jb + 3 * j + c];
            ok = ok && isfinite(f) && isfinite(cn);
            jf[c] = (double)f; jc[c] = (double)cn;
        }
    }
    if (!ok) sbad = 1;                            // every writer stores the same value
    __syncthreads();
    if (tid == 0) {
        int status;
        if (sbad) {
            status = kFitNonFinite;
            for (int i = 0; i < 9; ++i) sR[i] = NAN;
            for (int i = 0; i < 3; ++i) { sT0[i] = NAN; st[i] = NAN; }
        } else {
            status = fit_frame(kf, kc, k2, Km, NK, (double)a.img_res, sR, sT0, st);
        }
        a.status[b] = status;
    }
    __syncthreads();
    if (tid < 9) a.out[O_R0][(long long)b * 9 + tid] = (float)sR[tid];
    if (tid < 3) {
        a.out[O_T0][(long long)b * 3 + tid] = (float)sT0[tid];
        a.out[O_TRANSL][(long long)b * 3 + tid] = (float)st[tid];
    }
    const double fbar = ((double)Km[0] + (double)Km[4]) / 2.0, res = (double)a.img_res;
    if (tid == 0) {
        float *wp = a.out[O_WP_O] + (long long)b * 3;
        wp[0] = (float)(2.0 * fbar / (res * st[2] + 1e-9)); wp[1] = (float)st[0]; wp[2] = (float)st[1];
    }
    if (item) {
        double j0[3];
        for (int i = 0; i < 3; ++i) {
            j0[i] = sR[3 * i] * jf[0] + sR[3 * i + 1] * jf[1] + sR[3 * i + 2] * jf[2] + sT0[i];
            dj[h][j][i] = j0[i] - jc[i];
            a.out[O_J3D_R + h][jb + 3 * j + i] = (float)(j0[i] + st[i]);
        }
        if (j == 0) {
            const double ct[3] = {j0[0] + st[0] - jc[0], j0[1] + st[1] - jc[1], j0[2] + st[2] - jc[2]};
            float *o = a.out[O_CAMT_R + h] + (long long)b * 3, *wp = a.out[O_WP_R + h] + (long long)b * 3;
            for (int i = 0; i < 3; ++i) o[i] = (float)ct[i];
            wp[0] = (float)(2.0 * fbar / (res * ct[2] + 1e-9)); wp[1] = (float)ct[0]; wp[2] = (float)ct[1];
        }
    }
    __syncthreads();
    if (tid < 6) {
        const int hh = tid / 3, c = tid % 3;
        double s = 0.0;
        for (int q = 0; q < J; ++q) s += dj[hh][q][c];
        a.out[O_OFF_R + hh][(long long)b * 3 + c] = (float)(s / (double)J + st[c]);
    }
}

// ---- distance fields ----------------------------------------------------------------------------------------------------------
struct DfArgs {
    const float *hand[2], *obj;      // hand 0 = r, 1 = l
    const long long *v_len;
    float *dist[4];                  // ro, lo, or, ol
    long long *idx[4];
    int B, NV, L, nbh, nbo;          // nbh / nbo: blocks of a hand -> object / object -> hand job
    float dmin, dmax;
};

__global__ void __launch_bounds__(kDfBlock) dist_fields_kernel(DfArgs a)
{
    __shared__ float4 tx[kChunk / 4], ty[kChunk / 4], tz[kChunk / 4];
    const int b = blockIdx.x, tid = threadIdx.x, NV = a.NV, L = a.L;
    int blk = blockIdx.y, job;
    if (blk < 2 * a.nbh) { job = blk / a.nbh; blk -= job * a.nbh; }
    else { blk -= 2 * a.nbh; job = 2 + blk / a.nbo; blk -= (job - 2) * a.nbo; }
    const int hnd = job & 1;
    const bool to_obj = job < 2;
    long long vl = a.v_len[b];
    const int vlen = (int)(vl < 0 ? 0 : (vl > L ? L : vl));
    const float *hand = a.hand[hnd] + (long long)b * NV * 3, *obj = a.obj + (long long)b * L * 3;
    const float *src = to_obj ? hand : obj, *trg = to_obj ? obj : hand;
    const int nsrc = to_obj ? NV : L;
    const int ntrg = to_obj ? vlen : (blk * kDfBlock < vlen ? NV : 0);     // a block of padded rows scans nothing
    const int i = blk * kDfBlock + tid;
    // a source that searches: a hand vertex with a non-empty object, or an object row below v_len
    const bool active = i < nsrc && (to_obj ? vlen > 0 : i < vlen);
    float sx = 0.f, sy = 0.f, sz = 0.f;
    if (active) { sx = src[3 * i]; sy = src[3 * i + 1]; sz = src[3 * i + 2]; }
    float best = INFINITY;
    int bi = 0;
    for (int c0 = 0; c0 < ntrg; c0 += kChunk) {          // ntrg is the same for every thread of the block
        const int n = ntrg - c0 < kChunk ? ntrg - c0 : kChunk, n4 = (n + 3) / 4;
        __syncthreads();
        for (int q = tid; q < n4 * 4; q += kDfBlock) {
            const bool in = q < n;
            ((float *)tx)[q] = in ? trg[3 * (c0 + q)] : NAN;
            ((float *)ty)[q] = in ? trg[3 * (c0 + q) + 1] : NAN;
            ((float *)tz)[q] = in ? trg[3 * (c0 + q) + 2] : NAN;
        }
        __syncthreads();
        if (!active) continue;
        for (int q = 0; q < n4; ++q) {
            const float4 X = tx[q], Y = ty[q], Z = tz[q];
            const float xs[4] = {X.x, X.y, X.z, X.w}, ys[4] = {Y.x, Y.y, Y.z, Y.w}, zs[4] = {Z.x, Z.y, Z.z, Z.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float dx = sx - xs[k], dy = sy - ys[k], dz = sz - zs[k];
                float d = dx * dx;
                d += dy * dy;
                d += dz * dz;
                if (d < best) { best = d; bi = c0 + 4 * q + k; }
            }
        }
    }
    if (i >= nsrc) return;
    const float v = active ? sqrtf(best) : 0.f;
    a.dist[job][(long long)b * nsrc + i] = fminf(fmaxf(v, a.dmin), a.dmax);
    a.idx[job][(long long)b * nsrc + i] = active ? bi : 0;
}

void begin_entry()
{
    set_error(MSDA_OK, "");
    (void)hipGetLastError();
}

int perr(const char *msg) { return set_error(MSDA_ERR_ARGUMENT, msg); }

bool fit_dims_ok(int B, int NK, int J) { return B >= 0 && NK >= 3 && NK <= kFitMaxNK && J >= 1 && J <= kFitMaxJ; }

bool df_dims_ok(int B, int NV, int L) { return B >= 0 && NV >= 1 && NV <= kDfMaxNV && L >= 1 && L <= kDfMaxL; }

}  // namespace

}  // namespace msda

using namespace msda;

int msda_pre_fit_supported(int B, int NK, int J) { return fit_dims_ok(B, NK, J) ? 1 : 0; }

int msda_pre_fit_f32(int B, int NK, int J, float img_res, const float *const *inputs, float *const *outputs, int *status,
                     msda_stream_t stream)
{
    if (!fit_dims_ok(B, NK, J)) return perr("msda_pre_fit: unsupported geometry (msda_pre_fit_supported)");
    if (inputs == nullptr || outputs == nullptr) return perr("msda_pre_fit: null pointer");
    if (!(img_res > 0.f)) return perr("msda_pre_fit: img_res must be positive");
    FitArgs a;
    memset(&a, 0, sizeof(a));
    a.B = B; a.NK = NK; a.J = J; a.img_res = img_res; a.status = status;
    for (int k = 0; k < kFitInputs; ++k) {
        a.in[k] = inputs[k];
        if (B > 0 && a.in[k] == nullptr) return perr("msda_pre_fit: null input");
    }
    for (int k = 0; k < kFitOutputs; ++k) {
        a.out[k] = outputs[k];
        if (B > 0 && a.out[k] == nullptr) return perr("msda_pre_fit: null output");
    }
    if (B > 0 && status == nullptr) return perr("msda_pre_fit: null output");
    begin_entry();
    if (B == 0) return MSDA_OK;
    hipLaunchKernelGGL(pre_fit_kernel, dim3((unsigned)B), dim3(kFitBlock), 0, (hipStream_t)stream, a);
    return check_launch("pre_fit_kernel");
}

int msda_dist_fields_supported(int B, int NV, int L) { return df_dims_ok(B, NV, L) ? 1 : 0; }

int msda_dist_fields_f32(int B, int NV, int L, const float *hand_r, const float *hand_l, const float *obj, const long long *v_len,
                         float dist_min, float dist_max, float *const *dists, long long *const *idx, msda_stream_t stream)
{
    if (!df_dims_ok(B, NV, L)) return perr("msda_dist_fields: unsupported geometry (msda_dist_fields_supported)");
    if (dists == nullptr || idx == nullptr) return perr("msda_dist_fields: null pointer");
    if (!(dist_min <= dist_max)) return perr("msda_dist_fields: dist_min must not exceed dist_max");
    DfArgs a;
    memset(&a, 0, sizeof(a));
    a.B = B; a.NV = NV; a.L = L; a.dmin = dist_min; a.dmax = dist_max;
    a.hand[0] = hand_r; a.hand[1] = hand_l; a.obj = obj; a.v_len = v_len;
    if (B > 0 && (!hand_r || !hand_l || !obj || !v_len)) return perr("msda_dist_fields: null input");
    for (int k = 0; k < 4; ++k) {
        a.dist[k] = dists[k]; a.idx[k] = idx[k];
        if (B > 0 && (!dists[k] || !idx[k])) return perr("msda_dist_fields: null output");
    }
    begin_entry();
    if (B == 0) return MSDA_OK;
    a.nbh = (NV + kDfBlock - 1) / kDfBlock;
    a.nbo = (L + kDfBlock - 1) / kDfBlock;
    hipLaunchKernelGGL(dist_fields_kernel, dim3((unsigned)B, (unsigned)(2 * a.nbh + 2 * a.nbo)), dim3(kDfBlock), 0,
                       (hipStream_t)stream, a);
    return check_launch("dist_fields_kernel");
}
