// ARCTIC object layer (arctic_tools/common/object_tensors.py ObjectTensors.forward_7d_batch) and the per-set MANO / object
// small losses (src/callbacks/loss/loss_arctic_sf.py compute_small_loss) for every set of a step, without host syncs.
//
// Object layer.  A model holds N padded objects: v [N, Lm, 3] with parts_ids [N, Lm] (1 = top part), v_sub [N, NS, 3] with
// parts_sub_ids [N, NS], bbox_top / bbox_bottom [N, NBt | NBb, 3], kp_top / kp_bottom [N, NKt | NKb, 3].  A group is B frames:
// obj_idx [B] (int64), angles [B], global_orient [B, 3], transl [B, 3] or none, a host row count `len` <= Lm.  Each output row
// is R_g (top ? R_a p : p) + t, with R_q p = Im(q (0, p) q*), q_a = aa2q((0, 0, -angle)), q_g = aa2q(global_orient) (pytorch3d's
// axis_angle_to_quaternion: sin(theta/2)/theta, or 1/2 - theta^2/48 below 1e-6, not renormalised).
//   forward   one launch: one thread per output row (v, v_sub, bbox3d, kp3d) of every frame of every group.
//   backward  one launch: one workgroup per frame sums the rows' quaternion gradients in a fixed order (per-thread strided
//             partials, then an LDS tree), then the axis-angle backward with the same polynomial below 1e-6.
//
// Small losses.  A set is one decoder output: the nine get_arctic_item tensors, the MANO vertices / joints of both hands
// (without camera translation) and the object's v / kp3d.  The targets are shared by all sets.
//   forward   launch 1, one workgroup per (set, frame): 22 per-frame partial sums (squared errors, L1 smoothing, contact
//             distances and counts).  Launch 2, one thread per set: sums the partials over frames in frame order, evaluates
//             the reference's gates and masks on the device and writes the 19 terms plus the coefficients of the backward.
//   backward  one launch, one workgroup per (set, frame): every input gradient of that frame.  The contact-deviation gradient
//             into object vertices is added by the first (hand) index of each object vertex, which sums all contributions to
//             that vertex in hand-vertex order.
// Fixed summation order everywhere, no atomics: bitwise reproducible.
#include <cmath>
#include <cstdio>
#include <cstring>

#include "msda_common.h"
#include "msda_launch.h"
#include "msda_pose.h"

namespace msda {

namespace {

constexpr int kBlock = 256;
constexpr int kObjMaxGroups = 16, kObjMaxObjects = 64, kObjMaxLen = 65536, kObjMaxSub = 4096, kObjMaxBox = 64, kObjMaxKp = 256;
constexpr int kSLMaxSets = 8, kSLMaxJ = 32, kSLMaxNV = 1024, kSLMaxKO = 64, kSLMaxNB = 16, kSLMaxLen = 65536;
constexpr int kTerms = 19, kParts = 22, kCoef = 20;
constexpr float kContact = 3e-3f, kMinS = 0.1f;

// term order (= the reference's dict insertion order)
enum {
    T_KP2D_L, T_POSE_L, T_BETA_L, T_CAMT_L, T_KP3D_L,
    T_KP2D_R, T_POSE_R, T_BETA_R, T_CAMT_R, T_KP3D_R, T_OTRANSL,
    T_TRANSL_L,
    T_OKP2D, T_OCAMT, T_OKP3D, T_RAD, T_ROT, T_SMOOTH,
    T_CD
};
// partials: the 18 sums of the terms before T_CD, then contact (sum, count) for r and l
enum { P_CD_R = 18, P_CN_R, P_CD_L, P_CN_L };
// coefficients: one per term before T_CD, then cd r and cd l (1 / number of frames in contact, 0 when gated)
enum { C_CD_R = 18, C_CD_L };


// ---- object layer -------------------------------------------------------------------------------------------------------------
struct ObjModel {
    const float *v, *v_sub, *bb_top, *bb_bot, *kp_top, *kp_bot;
    const long long *parts, *parts_sub;
    int n_obj, Lm, NS, NBt, NBb, NKt, NKb;
};
struct ObjGroup {
    const long long *idx;
    const float *angles, *go, *transl;
    float *v, *v_sub, *bbox, *kp;
    const float *gv, *gv_sub, *gbbox, *gkp;
    float *gang, *ggo, *gtransl;
    int B, len, f0;
};
struct ObjArgs {
    ObjModel m;
    ObjGroup g[kObjMaxGroups + 1];              // g[ngroups].f0 = total frames
    int ngroups;
};
static_assert(sizeof(ObjArgs) <= 4000, "kernel argument table");

__device__ __forceinline__ int obj_group_of(const ObjArgs &a, int f)
{
    int gi = 0;
    while (gi + 1 < a.ngroups && f >= a.g[gi + 1].f0) ++gi;
    return gi;
}

__device__ __forceinline__ int obj_rows(const ObjModel &m, int len) { return len + m.NS + m.NBt + m.NBb + m.NKt + m.NKb; }

// template point, top flag, output row pointer and gradient row pointer of row r of frame b
__device__ __forceinline__ void obj_row(const ObjModel &m, const ObjGroup &g, int b, long long oi, int r, float p[3], bool &top,
                                        float **out, const float **gout)
{
    const float *src;
    long long orow;
    if (r < g.len) {
        src = m.v + (oi * m.Lm + r) * 3; top = m.parts[oi * m.Lm + r] == 1; orow = (long long)b * g.len + r;
        if (out) *out = g.v + orow * 3;
        if (gout) *gout = g.gv ? g.gv + orow * 3 : nullptr;
    } else if ((r -= g.len) < m.NS) {
        src = m.v_sub + (oi * m.NS + r) * 3; top = m.parts_sub[oi * m.NS + r] == 1; orow = (long long)b * m.NS + r;
        if (out) *out = g.v_sub + orow * 3;
        if (gout) *gout = g.gv_sub ? g.gv_sub + orow * 3 : nullptr;
    } else if ((r -= m.NS) < m.NBt + m.NBb) {
        top = r < m.NBt;
        src = top ? m.bb_top + (oi * m.NBt + r) * 3 : m.bb_bot + (oi * m.NBb + r - m.NBt) * 3;
        orow = (long long)b * (m.NBt + m.NBb) + r;
        if (out) *out = g.bbox + orow * 3;
        if (gout) *gout = g.gbbox ? g.gbbox + orow * 3 : nullptr;
    } else {
        r -= m.NBt + m.NBb;
        top = r < m.NKt;
        src = top ? m.kp_top + (oi * m.NKt + r) * 3 : m.kp_bot + (oi * m.NKb + r - m.NKt) * 3;
        orow = (long long)b * (m.NKt + m.NKb) + r;
        if (out) *out = g.kp + orow * 3;
        if (gout) *gout = g.gkp ? g.gkp + orow * 3 : nullptr;
    }
    p[0] = src[0]; p[1] = src[1]; p[2] = src[2];
}

__global__ void __launch_bounds__(kBlock) obj_fwd_kernel(ObjArgs a)
{
    const int f = blockIdx.x;
    const ObjGroup &g = a.g[obj_group_of(a, f)];
    const int b = f - g.f0;
    const int R = obj_rows(a.m, g.len);
    const long long oi_raw = g.idx[b];
    const bool bad = oi_raw < 0 || oi_raw >= a.m.n_obj;       // out of range: NaN rows (the reference raises)
    const long long oi = bad ? 0 : oi_raw;
    const Q qa = aa2q(0.f, 0.f, -g.angles[b]);
    const Q qg = aa2q(g.go[3 * b], g.go[3 * b + 1], g.go[3 * b + 2]);
    float t[3] = {0.f, 0.f, 0.f};
    if (g.transl) { t[0] = g.transl[3 * b]; t[1] = g.transl[3 * b + 1]; t[2] = g.transl[3 * b + 2]; }
    for (int r = blockIdx.y * kBlock + threadIdx.x; r < R; r += gridDim.y * kBlock) {
        float p[3], y[3], o[3];
        bool top;
        float *out;
        obj_row(a.m, g, b, oi, r, p, top, &out, nullptr);
        if (bad) p[0] = p[1] = p[2] = NAN;
        if (top) qapply(qa, p, y); else { y[0] = p[0]; y[1] = p[1]; y[2] = p[2]; }
        qapply(qg, y, o);
        out[0] = o[0] + t[0]; out[1] = o[1] + t[1]; out[2] = o[2] + t[2];
    }
}


__global__ void __launch_bounds__(kBlock) obj_bwd_kernel(ObjArgs a)
{
    __shared__ float red[11][kBlock];
    const int f = blockIdx.x;
    const ObjGroup &g = a.g[obj_group_of(a, f)];
    const int b = f - g.f0;
    const int R = obj_rows(a.m, g.len);
    const long long oi_raw = g.idx[b];
    const bool bad = oi_raw < 0 || oi_raw >= a.m.n_obj;
    const long long oi = bad ? 0 : oi_raw;
    const float ang = g.angles[b];
    const Q qa = aa2q(0.f, 0.f, -ang);
    const float gx = g.go[3 * b], gy = g.go[3 * b + 1], gz = g.go[3 * b + 2];
    const Q qg = aa2q(gx, gy, gz);
    Q gqa = {0.f, 0.f, 0.f, 0.f}, gqg = {0.f, 0.f, 0.f, 0.f};
    float gt[3] = {0.f, 0.f, 0.f};
    for (int r = threadIdx.x; r < R; r += kBlock) {
        float p[3], y[3], gy3[3], gp[3];
        bool top;
        const float *go;
        obj_row(a.m, g, b, oi, r, p, top, nullptr, &go);
        if (go == nullptr) continue;
        if (bad) p[0] = p[1] = p[2] = NAN;
        const float gr[3] = {go[0], go[1], go[2]};
        gt[0] += gr[0]; gt[1] += gr[1]; gt[2] += gr[2];
        if (top) qapply(qa, p, y); else { y[0] = p[0]; y[1] = p[1]; y[2] = p[2]; }
        qapply_bwd(qg, y, gr, gqg, gy3);
        if (top) qapply_bwd(qa, p, gy3, gqa, gp);
    }
    const float v[11] = {gqa.w, gqa.x, gqa.y, gqa.z, gqg.w, gqg.x, gqg.y, gqg.z, gt[0], gt[1], gt[2]};
    block_reduce<11>(red, v);
    if (threadIdx.x == 0) {
        float ga[3];
        aa2q_bwd(0.f, 0.f, -ang, {red[0][0], red[1][0], red[2][0], red[3][0]}, ga);
        if (g.gang) g.gang[b] = -ga[2];
        aa2q_bwd(gx, gy, gz, {red[4][0], red[5][0], red[6][0], red[7][0]}, ga);
        if (g.ggo) { g.ggo[3 * b] = ga[0]; g.ggo[3 * b + 1] = ga[1]; g.ggo[3 * b + 2] = ga[2]; }
        if (g.gtransl) { g.gtransl[3 * b] = red[8][0]; g.gtransl[3 * b + 1] = red[9][0]; g.gtransl[3 * b + 2] = red[10][0]; }
    }
}

// ---- small losses -------------------------------------------------------------------------------------------------------------
enum { I_ROOT_L, I_ROOT_R, I_ROOT_O, I_POSE_L, I_POSE_R, I_BETA_L, I_BETA_R, I_ROT, I_RAD,
       I_VERT_L, I_VERT_R, I_JNT_L, I_JNT_R, I_OBJ_V, I_OBJ_KP, kInputs };
enum { G_POSE_L, G_POSE_R, G_BETA_L, G_BETA_R, G_J3D_L, G_J3D_R, G_KP3D_O, G_J2D_L, G_J2D_R, G_KP2D_O, G_ROT, G_RAD,
       G_CAMT_L, G_CAMT_R, G_CAMT_O, G_IS_VALID, G_LEFT_VALID, G_RIGHT_VALID, G_JV_L, G_JV_R, G_DIST_RO, G_DIST_LO, G_K,
       kTargets };

struct SLSet {
    const float *in[kInputs];
    float *grad[kInputs];
};
struct SLArgs {
    SLSet s[kSLMaxSets];
    const float *t[kTargets];
    const long long *idx_ro, *idx_lo;
    float *losses;                              // [S, 19]
    const float *glosses;                       // [S, 19]
    float *part;                                // [S, B, kParts]
    float *coef;                                // [S, kCoef]
    int S, B, J, NV, KO, NB, L;
    float img_res;
};
static_assert(sizeof(SLArgs) <= 4000, "kernel argument table");

__device__ __forceinline__ bool trunc_valid(float m) { return (long long)m != 0; }     // is_valid.long().bool()

// weak perspective (s, tx, ty) -> (tx, ty, 2 f / (img_res s' + 1e-9)), s' = max(s, 0.1); f = (K00 + K11) / 2
__device__ __forceinline__ void cam_t(const float *root, const float *K, float img_res, float ct[3])
{
    const float f = (K[0] + K[4]) / 2.0f;
    const float s = fmaxf(root[0], kMinS);
    ct[0] = root[1]; ct[1] = root[2]; ct[2] = 2.f * f / (img_res * s + 1e-9f);
}


__device__ __forceinline__ float sgn(float x) { return x > 0.f ? 1.f : (x < 0.f ? -1.f : 0.f); }

// forward launch 1: per (set, frame) partial sums
__global__ void __launch_bounds__(kBlock) sl_part_kernel(SLArgs a)
{
    __shared__ float red[kParts][kBlock];
    const int s = blockIdx.x / a.B, b = blockIdx.x % a.B, tid = threadIdx.x;
    const SLSet &S = a.s[s];
    const int J = a.J, NV = a.NV, KO = a.KO, NB = a.NB, L = a.L;
    const float *K = a.t[G_K] + 9 * b;
    float ct[3][3];
    for (int h = 0; h < 3; ++h) cam_t(S.in[I_ROOT_L + h] + 3 * b, K, a.img_res, ct[h]);
    float acc[kParts];
    for (int k = 0; k < kParts; ++k) acc[k] = 0.f;

    // hand joints: kp2d (joints_loss) and root-relative kp3d, item = (hand, joint)
    for (int it = tid; it < 2 * J; it += kBlock) {
        const int h = it / J, j = it % J;
        const float *jp = S.in[I_JNT_L + h] + ((long long)b * J) * 3;
        const float *gj = a.t[G_J3D_L + h] + ((long long)b * J) * 3;
        const float jv = a.t[G_JV_L + h][b * J + j];
        float x[3], x0[3], n[2], ph[3];
        for (int c = 0; c < 3; ++c) { x[c] = jp[3 * j + c] + ct[h][c]; x0[c] = jp[c] + ct[h][c]; }
        project(K, x, a.img_res, n, ph);
        const float *g2 = a.t[G_J2D_L + h] + ((long long)b * J + j) * 2;
        acc[h ? T_KP2D_R : T_KP2D_L] += (sq(n[0] - g2[0]) + sq(n[1] - g2[1])) * jv;
        float e3 = 0.f;
        for (int c = 0; c < 3; ++c) e3 += sq((x[c] - x0[c]) - (gj[3 * j + c] - gj[c]));
        acc[h ? T_KP3D_R : T_KP3D_L] += e3 * jv;
    }
    // pose matrices, item = (hand, joint)
    for (int it = tid; it < 32; it += kBlock) {
        const int h = it / 16, j = it % 16;
        const float *pp = S.in[I_POSE_L + h] + b * 48 + 3 * j, *gp = a.t[G_POSE_L + h] + b * 48 + 3 * j;
        float Mp[9], Mg[9];
        q2m(aa2q(pp[0], pp[1], pp[2]), Mp);
        q2m(aa2q(gp[0], gp[1], gp[2]), Mg);
        float e = 0.f;
        for (int m = 0; m < 9; ++m) e += sq(Mp[m] - Mg[m]);
        acc[h ? T_POSE_R : T_POSE_L] += e;
    }
    if (tid == 0) {
        for (int h = 0; h < 2; ++h) {
            const float *bp = S.in[I_BETA_L + h] + b * NB, *bg = a.t[G_BETA_L + h] + b * NB;
            float e = 0.f;
            for (int m = 0; m < NB; ++m) e += sq(bp[m] - bg[m]);
            acc[h ? T_BETA_R : T_BETA_L] = e;
        }
        const float *rl = S.in[I_ROOT_L] + 3 * b, *rr = S.in[I_ROOT_R] + 3 * b, *ro = S.in[I_ROOT_O] + 3 * b;
        const float *gl = a.t[G_CAMT_L] + 3 * b, *gr = a.t[G_CAMT_R] + 3 * b, *go = a.t[G_CAMT_O] + 3 * b;
        for (int c = 0; c < 3; ++c) {
            acc[T_CAMT_L] += sq(rl[c] - gl[c]);
            acc[T_CAMT_R] += sq(rr[c] - gr[c]);
            acc[T_OTRANSL] += sq((ro[c] - rr[c]) - (go[c] - gr[c]));
            acc[T_TRANSL_L] += sq((rl[c] - rr[c]) - (gl[c] - gr[c]));
            acc[T_OCAMT] += sq(ro[c] - go[c]);
            acc[T_ROT] += sq(S.in[I_ROT][3 * b + c] - a.t[G_ROT][3 * b + c]);
        }
        acc[T_RAD] = sq(S.in[I_RAD][b] - a.t[G_RAD][b]);
    }
    // object keypoints: kp2d and kp3d relative to keypoint KO / 2
    {
        const float *kp = S.in[I_OBJ_KP] + (long long)b * KO * 3, *gk = a.t[G_KP3D_O] + (long long)b * KO * 3;
        const int root = KO / 2;
        for (int k = tid; k < KO; k += kBlock) {
            float x[3], xr[3], n[2], ph[3];
            for (int c = 0; c < 3; ++c) { x[c] = kp[3 * k + c] + ct[2][c]; xr[c] = kp[3 * root + c] + ct[2][c]; }
            project(K, x, a.img_res, n, ph);
            const float *g2 = a.t[G_KP2D_O] + ((long long)b * KO + k) * 2;
            acc[T_OKP2D] += sq(n[0] - g2[0]) + sq(n[1] - g2[1]);
            for (int c = 0; c < 3; ++c) acc[T_OKP3D] += sq((x[c] - xr[c]) - (gk[3 * k + c] - gk[3 * root + c]));
        }
    }
    // v3d smoothing: |v[b] + ct[b] - v[b + 1] - ct[b + 1]|
    if (b + 1 < a.B) {
        float cn[3];
        cam_t(S.in[I_ROOT_O] + 3 * (b + 1), a.t[G_K] + 9 * (b + 1), a.img_res, cn);
        const float *v0 = S.in[I_OBJ_V] + (long long)b * L * 3, *v1 = v0 + (long long)L * 3;
        for (int e = tid; e < 3 * L; e += kBlock) {
            const int c = e % 3;
            acc[T_SMOOTH] += fabsf((v0[e] + ct[2][c]) - (v1[e] + cn[c]));
        }
    }
    // contact deviation, item = (hand, vertex); hand 0 = r (idx.ro), hand 1 = l (idx.lo)
    {
        const float iv = a.t[G_IS_VALID][b];
        const float *vo = S.in[I_OBJ_V] + (long long)b * L * 3;
        for (int it = tid; it < 2 * NV; it += kBlock) {
            const int h = it / NV, k = it % NV;
            const int hs = h ? 0 : 1;                                    // 0 = left, 1 = right for the inputs
            const bool fv = a.t[G_LEFT_VALID + hs][b] * iv == 1.f;
            const float dist = (h ? a.t[G_DIST_LO] : a.t[G_DIST_RO])[(long long)b * NV + k];
            if (!fv || dist > kContact) continue;
            const long long oi = (h ? a.idx_lo : a.idx_ro)[(long long)b * NV + k];
            const float *vh = S.in[I_VERT_L + hs] + ((long long)b * NV + k) * 3;
            float d2 = 0.f;
            if (oi < 0 || oi >= L) d2 = NAN;
            else
                for (int c = 0; c < 3; ++c) d2 += sq((vo[3 * oi + c] + ct[2][c]) - (vh[c] + ct[hs][c]));
            acc[h ? P_CD_L : P_CD_R] += sqrtf(d2);
            acc[h ? P_CN_L : P_CN_R] += 1.f;
        }
    }
    block_reduce<kParts>(red, acc);
    if (tid < kParts) a.part[((long long)s * a.B + b) * kParts + tid] = red[tid][0];
}

// vector_loss's denominators: 0 when mask.sum() == 0 (the reference returns zeros(1)), else the number of frames that
// .long().bool() keeps
struct MaskStat { bool any; int n; };

__device__ MaskStat mask_stat(const SLArgs &a, int m0, int m1)
{
    float sum = 0.f;
    int n = 0;
    for (int b = 0; b < a.B; ++b) {
        const float m = a.t[m0][b] * (m1 >= 0 ? a.t[m1][b] : 1.f);
        sum += m;
        n += trunc_valid(m);
    }
    return {sum != 0.f, n};
}

__device__ __forceinline__ bool frame_ok(const SLArgs &a, int m0, int m1, int b)
{
    return trunc_valid(a.t[m0][b] * (m1 >= 0 ? a.t[m1][b] : 1.f));
}

// forward launch 2: one thread per set
__global__ void sl_final_kernel(SLArgs a)
{
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= a.S) return;
    const float *P = a.part + (long long)s * a.B * kParts;
    // vector_loss terms sum their mask's frames only (the reference's dist[is_valid.long().bool()])
    float sum[kParts];
    for (int k = 0; k < kParts; ++k) sum[k] = 0.f;
    for (int b = 0; b < a.B; ++b) {
        const bool v_l = frame_ok(a, G_LEFT_VALID, -1, b), v_r = frame_ok(a, G_RIGHT_VALID, -1, b);
        const bool v_i = frame_ok(a, G_IS_VALID, -1, b), v_ri = frame_ok(a, G_RIGHT_VALID, G_IS_VALID, b);
        const bool v_rl = frame_ok(a, G_RIGHT_VALID, G_LEFT_VALID, b);
        for (int k = 0; k < kParts; ++k) {
            bool on;
            switch (k) {
            case T_POSE_L: case T_BETA_L: case T_CAMT_L: on = v_l; break;
            case T_POSE_R: case T_BETA_R: case T_CAMT_R: on = v_r; break;
            case T_OTRANSL: on = v_ri; break;
            case T_TRANSL_L: on = v_rl; break;
            case T_OKP2D: case T_OCAMT: case T_OKP3D: case T_RAD: case T_ROT: on = v_i; break;
            default: on = true;
            }
            if (on) sum[k] += P[b * kParts + k];
        }
    }
    // gates: Python's sum(is_valid * hand_valid) != 0, in frame order
    float gl = 0.f, gr = 0.f;
    for (int b = 0; b < a.B; ++b) {
        gl = gl + a.t[G_IS_VALID][b] * a.t[G_LEFT_VALID][b];
        gr = gr + a.t[G_IS_VALID][b] * a.t[G_RIGHT_VALID][b];
    }
    const bool gate_l = gl != 0.f, gate_r = gr != 0.f;
    const float B = (float)a.B;
    float c[kCoef];
    auto vec = [&](MaskStat m, float inner, bool gate) { return gate && m.any ? 1.f / ((float)m.n * inner) : 0.f; };
    const MaskStat ml = mask_stat(a, G_LEFT_VALID, -1), mr = mask_stat(a, G_RIGHT_VALID, -1);
    const MaskStat mi = mask_stat(a, G_IS_VALID, -1), mri = mask_stat(a, G_RIGHT_VALID, G_IS_VALID);
    const MaskStat mrl = mask_stat(a, G_RIGHT_VALID, G_LEFT_VALID);
    c[T_KP2D_L] = gate_l ? 1.f / (B * a.J * 2) : 0.f;
    c[T_POSE_L] = vec(ml, 144.f, gate_l);
    c[T_BETA_L] = vec(ml, (float)a.NB, gate_l);
    c[T_CAMT_L] = vec(ml, 3.f, gate_l);
    c[T_KP3D_L] = gate_l ? 1.f / (B * a.J * 3) : 0.f;
    c[T_KP2D_R] = gate_r ? 1.f / (B * a.J * 2) : 0.f;
    c[T_POSE_R] = vec(mr, 144.f, gate_r);
    c[T_BETA_R] = vec(mr, (float)a.NB, gate_r);
    c[T_CAMT_R] = vec(mr, 3.f, gate_r);
    c[T_KP3D_R] = gate_r ? 1.f / (B * a.J * 3) : 0.f;
    c[T_OTRANSL] = vec(mri, 3.f, gate_r);
    c[T_TRANSL_L] = vec(mrl, 3.f, gate_l && gate_r);
    c[T_OKP2D] = vec(mi, (float)a.KO * 2, true);
    c[T_OCAMT] = vec(mi, 3.f, true);
    c[T_OKP3D] = vec(mi, (float)a.KO * 3, true);
    c[T_RAD] = vec(mi, 1.f, true);
    c[T_ROT] = vec(mi, 3.f, true);
    c[T_SMOOTH] = 1.f;
    float *L = a.losses + (long long)s * kTerms;
    for (int k = 0; k < T_CD; ++k) {
        bool on;
        switch (k) {
        case T_KP2D_L: case T_KP3D_L: case T_POSE_L: case T_BETA_L: case T_CAMT_L: on = gate_l; break;
        case T_KP2D_R: case T_KP3D_R: case T_POSE_R: case T_BETA_R: case T_CAMT_R: case T_OTRANSL: on = gate_r; break;
        case T_TRANSL_L: on = gate_l && gate_r; break;
        default: on = true;
        }
        const MaskStat *m = nullptr;
        switch (k) {
        case T_POSE_L: case T_BETA_L: case T_CAMT_L: m = &ml; break;
        case T_POSE_R: case T_BETA_R: case T_CAMT_R: m = &mr; break;
        case T_OTRANSL: m = &mri; break;
        case T_TRANSL_L: m = &mrl; break;
        case T_OKP2D: case T_OCAMT: case T_OKP3D: case T_RAD: case T_ROT: m = &mi; break;
        default: break;
        }
        float inner = 1.f;
        switch (k) {
        case T_POSE_L: case T_POSE_R: inner = 144.f; break;
        case T_BETA_L: case T_BETA_R: inner = (float)a.NB; break;
        case T_OKP2D: inner = (float)a.KO * 2; break;
        case T_OKP3D: inner = (float)a.KO * 3; break;
        case T_RAD: inner = 1.f; break;
        case T_KP2D_L: case T_KP2D_R: inner = (float)a.J * 2; break;
        case T_KP3D_L: case T_KP3D_R: inner = (float)a.J * 3; break;
        default: inner = 3.f;
        }
        if (k == T_SMOOTH) L[k] = sum[k];
        else if (!on || (m && !m->any)) L[k] = 0.f;
        else L[k] = sum[k] / ((m ? (float)m->n : B) * inner);
    }
    // contact deviation: per-frame nanmean, nanmean over frames, nan_to_num; a gated hand adds nothing
    float cd = 0.f;
    for (int h = 0; h < 2; ++h) {
        const bool gate = h ? gate_l : gate_r;
        float tot = 0.f;
        int nf = 0;
        for (int b = 0; b < a.B; ++b) {
            const float cnt = P[b * kParts + (h ? P_CN_L : P_CN_R)];
            if (cnt > 0.f) { tot += P[b * kParts + (h ? P_CD_L : P_CD_R)] / cnt; ++nf; }
        }
        c[h ? C_CD_L : C_CD_R] = gate && nf > 0 ? 1.f / (float)nf : 0.f;
        if (gate && nf > 0) {
            float v = tot / (float)nf;
            if (isnan(v)) v = 0.f;
            else if (isinf(v)) v = v > 0.f ? 3.4028234663852886e38f : -3.4028234663852886e38f;
            cd += v;
        }
    }
    L[T_CD] = cd;
    for (int k = 0; k < kCoef; ++k) a.coef[(long long)s * kCoef + k] = c[k];
}

// backward: one workgroup per (set, frame)
__global__ void __launch_bounds__(kBlock) sl_bwd_kernel(SLArgs a)
{
    __shared__ float red[9][kBlock];
    __shared__ float sgd[2 * kSLMaxNV][3];
    __shared__ int sidx[2 * kSLMaxNV];
    const int s = blockIdx.x / a.B, b = blockIdx.x % a.B, tid = threadIdx.x;
    const SLSet &S = a.s[s];
    const int J = a.J, NV = a.NV, KO = a.KO, NB = a.NB, L = a.L, B = a.B;
    const float *K = a.t[G_K] + 9 * b;
    const float *cf = a.coef + (long long)s * kCoef, *gL = a.glosses + (long long)s * kTerms;
    auto G = [&](int k) { return cf[k] != 0.f ? gL[k] * cf[k] : 0.f; };
    float ct[3][3];
    for (int h = 0; h < 3; ++h) cam_t(S.in[I_ROOT_L + h] + 3 * b, K, a.img_res, ct[h]);
    float gct[9];                                       // d loss / d cam_t of l, r, o
    for (int k = 0; k < 9; ++k) gct[k] = 0.f;
    const bool v_l = frame_ok(a, G_LEFT_VALID, -1, b), v_r = frame_ok(a, G_RIGHT_VALID, -1, b);
    const bool v_i = frame_ok(a, G_IS_VALID, -1, b), v_ri = frame_ok(a, G_RIGHT_VALID, G_IS_VALID, b);
    const bool v_rl = frame_ok(a, G_RIGHT_VALID, G_LEFT_VALID, b);

    // hand joints: one thread per hand, joints in order (the root row takes minus the others' kp3d gradient)
    if (tid < 2) {
        const int h = tid;
        const float *jp = S.in[I_JNT_L + h] + (long long)b * J * 3, *gj = a.t[G_J3D_L + h] + (long long)b * J * 3;
        float *gout = S.grad[I_JNT_L + h] + (long long)b * J * 3;
        const float g2 = G(h ? T_KP2D_R : T_KP2D_L), g3 = G(h ? T_KP3D_R : T_KP3D_L);
        float groot[3] = {0.f, 0.f, 0.f};
        for (int j = 0; j < J; ++j) {
            const float jv = a.t[G_JV_L + h][b * J + j];
            float x[3], x0[3], n[2], ph[3], gx[3];
            for (int c = 0; c < 3; ++c) { x[c] = jp[3 * j + c] + ct[h][c]; x0[c] = jp[c] + ct[h][c]; }
            project(K, x, a.img_res, n, ph);
            const float *t2 = a.t[G_J2D_L + h] + ((long long)b * J + j) * 2;
            const float gn[2] = {g2 != 0.f ? g2 * jv * 2.f * (n[0] - t2[0]) : 0.f, g2 != 0.f ? g2 * jv * 2.f * (n[1] - t2[1]) : 0.f};
            project_bwd(K, ph, a.img_res, gn, gx);
            for (int c = 0; c < 3; ++c) {
                gct[3 * h + c] += gx[c];
                const float e = (x[c] - x0[c]) - (gj[3 * j + c] - gj[c]);
                const float g = (j > 0 && g3 != 0.f) ? g3 * jv * 2.f * e : 0.f;
                groot[c] -= g;
                gout[3 * j + c] = gx[c] + g;
            }
        }
        for (int c = 0; c < 3; ++c) gout[c] += groot[c];
    } else if (tid == 2) {
        // object keypoints, in order (keypoint KO / 2 takes minus the others' kp3d gradient)
        const float *kp = S.in[I_OBJ_KP] + (long long)b * KO * 3, *gk = a.t[G_KP3D_O] + (long long)b * KO * 3;
        float *gout = S.grad[I_OBJ_KP] + (long long)b * KO * 3;
        const float g2 = v_i ? G(T_OKP2D) : 0.f, g3 = v_i ? G(T_OKP3D) : 0.f;
        const int root = KO / 2;
        float groot[3] = {0.f, 0.f, 0.f};
        for (int k = 0; k < KO; ++k) {
            float x[3], xr[3], n[2], ph[3], gx[3];
            for (int c = 0; c < 3; ++c) { x[c] = kp[3 * k + c] + ct[2][c]; xr[c] = kp[3 * root + c] + ct[2][c]; }
            project(K, x, a.img_res, n, ph);
            const float *t2 = a.t[G_KP2D_O] + ((long long)b * KO + k) * 2;
            const float gn[2] = {g2 != 0.f ? g2 * 2.f * (n[0] - t2[0]) : 0.f, g2 != 0.f ? g2 * 2.f * (n[1] - t2[1]) : 0.f};
            project_bwd(K, ph, a.img_res, gn, gx);
            for (int c = 0; c < 3; ++c) {
                gct[6 + c] += gx[c];
                const float e = (x[c] - xr[c]) - (gk[3 * k + c] - gk[3 * root + c]);
                const float g = (k != root && g3 != 0.f) ? g3 * 2.f * e : 0.f;
                groot[c] -= g;
                gout[3 * k + c] = gx[c] + g;
            }
        }
        for (int c = 0; c < 3; ++c) gout[3 * root + c] += groot[c];
    } else if (tid == 3) {
        // betas, rotation, radian
        for (int h = 0; h < 2; ++h) {
            const float g = (h ? v_r : v_l) ? G(h ? T_BETA_R : T_BETA_L) : 0.f;
            const float *bp = S.in[I_BETA_L + h] + b * NB, *bg = a.t[G_BETA_L + h] + b * NB;
            float *gout = S.grad[I_BETA_L + h] + b * NB;
            for (int m = 0; m < NB; ++m) gout[m] = g != 0.f ? g * 2.f * (bp[m] - bg[m]) : 0.f;
        }
        const float gr = v_i ? G(T_ROT) : 0.f, ga = v_i ? G(T_RAD) : 0.f;
        for (int c = 0; c < 3; ++c)
            S.grad[I_ROT][3 * b + c] = gr != 0.f ? gr * 2.f * (S.in[I_ROT][3 * b + c] - a.t[G_ROT][3 * b + c]) : 0.f;
        S.grad[I_RAD][b] = ga != 0.f ? ga * 2.f * (S.in[I_RAD][b] - a.t[G_RAD][b]) : 0.f;
    }
    // pose: item = (hand, joint)
    for (int it = tid; it < 32; it += kBlock) {
        const int h = it / 16, j = it % 16;
        const float g = (h ? v_r : v_l) ? G(h ? T_POSE_R : T_POSE_L) : 0.f;
        const float *pp = S.in[I_POSE_L + h] + b * 48 + 3 * j, *gp = a.t[G_POSE_L + h] + b * 48 + 3 * j;
        float *gout = S.grad[I_POSE_L + h] + b * 48 + 3 * j;
        if (g == 0.f) { gout[0] = gout[1] = gout[2] = 0.f; continue; }
        const Q qp = aa2q(pp[0], pp[1], pp[2]);
        float Mp[9], Mg[9], GM[9], ga[3];
        q2m(qp, Mp);
        q2m(aa2q(gp[0], gp[1], gp[2]), Mg);
        for (int m = 0; m < 9; ++m) GM[m] = g * 2.f * (Mp[m] - Mg[m]);
        aa2q_bwd(pp[0], pp[1], pp[2], q2m_bwd(qp, GM), ga);
        gout[0] = ga[0]; gout[1] = ga[1]; gout[2] = ga[2];
    }
    // v3d smoothing into the object vertices and cam_t_o
    {
        const float gs = G(T_SMOOTH);
        float cp[3], cn[3];
        if (b > 0) cam_t(S.in[I_ROOT_O] + 3 * (b - 1), a.t[G_K] + 9 * (b - 1), a.img_res, cp);
        if (b + 1 < B) cam_t(S.in[I_ROOT_O] + 3 * (b + 1), a.t[G_K] + 9 * (b + 1), a.img_res, cn);
        const float *v = S.in[I_OBJ_V] + (long long)b * L * 3;
        float *gv = S.grad[I_OBJ_V] + (long long)b * L * 3;
        for (int e = tid; e < 3 * L; e += kBlock) {
            const int c = e % 3;
            const float x = v[e] + ct[2][c];
            float g = 0.f;
            if (b + 1 < B) g += sgn(x - (v[e + 3 * L] + cn[c]));
            if (b > 0) g -= sgn((v[e - 3 * L] + cp[c]) - x);
            g = gs != 0.f ? gs * g : 0.f;
            gv[e] = g;
            gct[6 + c] += g;
        }
    }
    // contact deviation: hand vertex gradients, cam_t, and the per-contact object gradients staged in LDS
    {
        const float iv = a.t[G_IS_VALID][b];
        const float *vo = S.in[I_OBJ_V] + (long long)b * L * 3;
        const float *P = a.part + ((long long)s * B + b) * kParts;
        for (int it = tid; it < 2 * NV; it += kBlock) {
            const int h = it / NV, k = it % NV;
            const int hs = h ? 0 : 1;
            float *gh = S.grad[I_VERT_L + hs] + ((long long)b * NV + k) * 3;
            const bool fv = a.t[G_LEFT_VALID + hs][b] * iv == 1.f;
            const float dist = (h ? a.t[G_DIST_LO] : a.t[G_DIST_RO])[(long long)b * NV + k];
            const float cnt = P[h ? P_CN_L : P_CN_R];
            const float c = cf[h ? C_CD_L : C_CD_R];
            const long long oi = (h ? a.idx_lo : a.idx_ro)[(long long)b * NV + k];
            sidx[it] = -1;
            if (!fv || dist > kContact || c == 0.f || cnt <= 0.f || oi < 0 || oi >= L) {
                gh[0] = gh[1] = gh[2] = 0.f;
                continue;
            }
            const float *vh = S.in[I_VERT_L + hs] + ((long long)b * NV + k) * 3;
            float d[3], d2 = 0.f;
            for (int q = 0; q < 3; ++q) { d[q] = (vo[3 * oi + q] + ct[2][q]) - (vh[q] + ct[hs][q]); d2 += d[q] * d[q]; }
            const float w = gL[T_CD] * c / cnt / sqrtf(d2);
            for (int q = 0; q < 3; ++q) {
                const float g = w * d[q];
                gh[q] = -g;
                gct[3 * hs + q] -= g;
                gct[6 + q] += g;
                sgd[it][q] = g;
            }
            sidx[it] = (int)oi;
        }
    }
    block_reduce<9>(red, gct);          // its barriers also order the smoothing stores before the scatter below
    // the first contact of each object vertex adds all contacts of that vertex, in (hand, vertex) order
    {
        float *gv = S.grad[I_OBJ_V] + (long long)b * L * 3;
        for (int it = tid; it < 2 * NV; it += kBlock) {
            const int d = sidx[it];
            if (d < 0) continue;
            bool first = true;
            for (int p = 0; p < it && first; ++p) first = sidx[p] != d;
            if (!first) continue;
            float acc[3] = {gv[3 * d], gv[3 * d + 1], gv[3 * d + 2]};
            for (int p = it; p < 2 * NV; ++p)
                if (sidx[p] == d) { acc[0] += sgd[p][0]; acc[1] += sgd[p][1]; acc[2] += sgd[p][2]; }
            gv[3 * d] = acc[0]; gv[3 * d + 1] = acc[1]; gv[3 * d + 2] = acc[2];
        }
    }
    if (tid == 0) {
        // roots: the direct vector terms, then cam_t = (tx, ty, 2 f / (img_res max(s, 0.1) + 1e-9))
        const float *rl = S.in[I_ROOT_L] + 3 * b, *rr = S.in[I_ROOT_R] + 3 * b, *ro = S.in[I_ROOT_O] + 3 * b;
        const float *tl = a.t[G_CAMT_L] + 3 * b, *tr = a.t[G_CAMT_R] + 3 * b, *to = a.t[G_CAMT_O] + 3 * b;
        float gr[3][3];
        const float gcl = v_l ? G(T_CAMT_L) : 0.f, gcr = v_r ? G(T_CAMT_R) : 0.f, gco = v_i ? G(T_OCAMT) : 0.f;
        const float gtl = v_rl ? G(T_TRANSL_L) : 0.f, gto = v_ri ? G(T_OTRANSL) : 0.f;
        for (int c = 0; c < 3; ++c) {
            const float el = gcl != 0.f ? gcl * 2.f * (rl[c] - tl[c]) : 0.f;
            const float er = gcr != 0.f ? gcr * 2.f * (rr[c] - tr[c]) : 0.f;
            const float eo = gco != 0.f ? gco * 2.f * (ro[c] - to[c]) : 0.f;
            const float et = gtl != 0.f ? gtl * 2.f * ((rl[c] - rr[c]) - (tl[c] - tr[c])) : 0.f;
            const float eq = gto != 0.f ? gto * 2.f * ((ro[c] - rr[c]) - (to[c] - tr[c])) : 0.f;
            gr[0][c] = el + et;
            gr[1][c] = er - et - eq;
            gr[2][c] = eo + eq;
        }
        const float f = (K[0] + K[4]) / 2.0f;
        for (int h = 0; h < 3; ++h) {
            const float *r = S.in[I_ROOT_L + h] + 3 * b;
            const float sc = fmaxf(r[0], kMinS), den = a.img_res * sc + 1e-9f;
            const float dtz = r[0] >= kMinS ? -2.f * f * a.img_res / (den * den) : 0.f;
            float *g = S.grad[I_ROOT_L + h] + 3 * b;
            g[0] = gr[h][0] + red[3 * h + 2][0] * dtz;
            g[1] = gr[h][1] + red[3 * h][0];
            g[2] = gr[h][2] + red[3 * h + 1][0];
        }
    }
}

// ---- host side ----------------------------------------------------------------------------------------------------------------
void begin_entry()
{
    set_error(MSDA_OK, "");
    (void)hipGetLastError();
}

int serr(const char *msg) { return set_error(MSDA_ERR_ARGUMENT, msg); }

bool obj_dims_ok(int n_obj, int Lm, int NS, int NBt, int NBb, int NKt, int NKb)
{
    return n_obj >= 1 && n_obj <= kObjMaxObjects && Lm >= 1 && Lm <= kObjMaxLen && NS >= 0 && NS <= kObjMaxSub && NBt >= 0
           && NBb >= 0 && NBt + NBb <= kObjMaxBox && NKt >= 0 && NKb >= 0 && NKt + NKb <= kObjMaxKp;
}

int obj_setup(ObjArgs &a, const int *dims, const void *const *model, int n_groups, const int *group_B, const int *group_len,
              const void *const *inputs, int &frames, int &rows_max)
{
    memset(&a, 0, sizeof(a));
    if (dims == nullptr || model == nullptr || group_B == nullptr || group_len == nullptr || inputs == nullptr)
        return serr("msda_object: null pointer");
    if (!obj_dims_ok(dims[0], dims[1], dims[2], dims[3], dims[4], dims[5], dims[6]))
        return serr("msda_object: unsupported object model size");
    if (n_groups < 1 || n_groups > kObjMaxGroups) return serr("msda_object: 1 .. 16 groups");
    ObjModel &m = a.m;
    m.n_obj = dims[0]; m.Lm = dims[1]; m.NS = dims[2]; m.NBt = dims[3]; m.NBb = dims[4]; m.NKt = dims[5]; m.NKb = dims[6];
    m.v = (const float *)model[0]; m.parts = (const long long *)model[1]; m.v_sub = (const float *)model[2];
    m.parts_sub = (const long long *)model[3]; m.bb_top = (const float *)model[4]; m.bb_bot = (const float *)model[5];
    m.kp_top = (const float *)model[6]; m.kp_bot = (const float *)model[7];
    if (!m.v || !m.parts || (m.NS && (!m.v_sub || !m.parts_sub)) || (m.NBt && !m.bb_top) || (m.NBb && !m.bb_bot)
        || (m.NKt && !m.kp_top) || (m.NKb && !m.kp_bot))
        return serr("msda_object: null model tensor");
    a.ngroups = n_groups;
    long long f = 0;
    rows_max = 0;
    for (int i = 0; i < n_groups; ++i) {
        ObjGroup &g = a.g[i];
        if (group_B[i] < 0) return serr("msda_object: negative batch");
        if (group_len[i] < 1 || group_len[i] > m.Lm) return serr("msda_object: row count outside 1 .. padded length");
        g.B = group_B[i]; g.len = group_len[i]; g.f0 = (int)f;
        g.idx = (const long long *)inputs[4 * i]; g.angles = (const float *)inputs[4 * i + 1];
        g.go = (const float *)inputs[4 * i + 2]; g.transl = (const float *)inputs[4 * i + 3];
        if (g.B > 0 && (!g.idx || !g.angles || !g.go)) return serr("msda_object: null pointer");
        if ((long long)g.B * g.len * 3 >= (1LL << 31)) return serr("msda_object: tensors beyond 2^31 elements");
        const int R = g.len + m.NS + m.NBt + m.NBb + m.NKt + m.NKb;
        if (R > rows_max) rows_max = R;
        f += g.B;
    }
    if (f >= (1LL << 31)) return serr("msda_object: too many frames");
    a.g[n_groups].f0 = (int)f;
    frames = (int)f;
    return MSDA_OK;
}

bool sl_dims_ok(int S, int B, int J, int NV, int KO, int NB, int L)
{
    return S >= 1 && S <= kSLMaxSets && B >= 0 && J >= 1 && J <= kSLMaxJ && NV >= 1 && NV <= kSLMaxNV && KO >= 2
           && KO <= kSLMaxKO && KO % 2 == 0 && NB >= 1 && NB <= kSLMaxNB && L >= 1 && L <= kSLMaxLen;
}

int sl_setup(SLArgs &a, const int *dims, float img_res, const void *const *targets, const float *const *inputs, float *losses)
{
    memset(&a, 0, sizeof(a));
    if (dims == nullptr || targets == nullptr || inputs == nullptr || losses == nullptr) return serr("msda_small_loss: null pointer");
    if (!sl_dims_ok(dims[0], dims[1], dims[2], dims[3], dims[4], dims[5], dims[6]))
        return serr("msda_small_loss: unsupported geometry");
    if (!(img_res > 0.f)) return serr("msda_small_loss: img_res must be positive");
    a.S = dims[0]; a.B = dims[1]; a.J = dims[2]; a.NV = dims[3]; a.KO = dims[4]; a.NB = dims[5]; a.L = dims[6];
    if ((long long)a.B * a.L * 3 >= (1LL << 31) || (long long)a.S * a.B >= (1LL << 31)) return serr("msda_small_loss: too large");
    a.img_res = img_res;
    for (int k = 0; k < kTargets; ++k) {
        a.t[k] = (const float *)targets[k];
        if (a.B > 0 && a.t[k] == nullptr) return serr("msda_small_loss: null target");
    }
    a.idx_ro = (const long long *)targets[kTargets];
    a.idx_lo = (const long long *)targets[kTargets + 1];
    if (a.B > 0 && (!a.idx_ro || !a.idx_lo)) return serr("msda_small_loss: null target");
    for (int s = 0; s < a.S; ++s)
        for (int k = 0; k < kInputs; ++k) {
            a.s[s].in[k] = inputs[s * kInputs + k];
            if (a.B > 0 && a.s[s].in[k] == nullptr) return serr("msda_small_loss: null input");
        }
    a.losses = losses;
    return MSDA_OK;
}

}  // namespace

}  // namespace msda

using namespace msda;

int msda_object_supported(int n_objects, int max_len, int n_sub, int n_bbox_top, int n_bbox_bottom, int n_kp_top, int n_kp_bottom)
{
    return obj_dims_ok(n_objects, max_len, n_sub, n_bbox_top, n_bbox_bottom, n_kp_top, n_kp_bottom) ? 1 : 0;
}

int msda_object_forward_f32(const int *dims, const void *const *model, int n_groups, const int *group_B, const int *group_len,
                            const void *const *inputs, float *const *outputs, msda_stream_t stream)
{
    ObjArgs a;
    int frames = 0, rows_max = 0;
    int rc = obj_setup(a, dims, model, n_groups, group_B, group_len, inputs, frames, rows_max);
    if (rc != MSDA_OK) return rc;
    if (outputs == nullptr) return serr("msda_object: null pointer");
    for (int i = 0; i < n_groups; ++i) {
        ObjGroup &g = a.g[i];
        g.v = outputs[4 * i]; g.v_sub = outputs[4 * i + 1]; g.bbox = outputs[4 * i + 2]; g.kp = outputs[4 * i + 3];
        if (g.B > 0 && (!g.v || (a.m.NS && !g.v_sub) || (a.m.NBt + a.m.NBb && !g.bbox) || (a.m.NKt + a.m.NKb && !g.kp)))
            return serr("msda_object: null output");
    }
    begin_entry();
    if (frames == 0) return MSDA_OK;
    const int ys = (rows_max + kBlock - 1) / kBlock;
    hipLaunchKernelGGL(obj_fwd_kernel, dim3((unsigned)frames, (unsigned)(ys < 64 ? ys : 64)), dim3(kBlock), 0, (hipStream_t)stream, a);
    return check_launch("obj_fwd_kernel");
}

int msda_object_backward_f32(const int *dims, const void *const *model, int n_groups, const int *group_B, const int *group_len,
                             const void *const *inputs, const float *const *grad_outputs, float *const *grads,
                             msda_stream_t stream)
{
    ObjArgs a;
    int frames = 0, rows_max = 0;
    int rc = obj_setup(a, dims, model, n_groups, group_B, group_len, inputs, frames, rows_max);
    if (rc != MSDA_OK) return rc;
    if (grad_outputs == nullptr || grads == nullptr) return serr("msda_object: null pointer");
    for (int i = 0; i < n_groups; ++i) {
        ObjGroup &g = a.g[i];
        g.gv = grad_outputs[4 * i]; g.gv_sub = grad_outputs[4 * i + 1]; g.gbbox = grad_outputs[4 * i + 2]; g.gkp = grad_outputs[4 * i + 3];
        g.gang = grads[3 * i]; g.ggo = grads[3 * i + 1]; g.gtransl = grads[3 * i + 2];
    }
    begin_entry();
    if (frames == 0) return MSDA_OK;
    hipLaunchKernelGGL(obj_bwd_kernel, dim3((unsigned)frames), dim3(kBlock), 0, (hipStream_t)stream, a);
    return check_launch("obj_bwd_kernel");
}

int msda_small_loss_supported(int S, int B, int J, int NV, int KO, int NB, int L)
{
    return sl_dims_ok(S, B, J, NV, KO, NB, L) ? 1 : 0;
}

unsigned long long msda_small_loss_workspace_bytes(int S, int B, int J, int NV, int KO, int NB, int L)
{
    if (!sl_dims_ok(S, B, J, NV, KO, NB, L)) return 0;
    return ((unsigned long long)S * B * kParts + (unsigned long long)S * kCoef) * sizeof(float);
}

int msda_small_loss_forward_f32(const int *dims, float img_res, const void *const *targets, const float *const *inputs,
                                float *losses, void *workspace, unsigned long long workspace_bytes, msda_stream_t stream)
{
    SLArgs a;
    int rc = sl_setup(a, dims, img_res, targets, inputs, losses);
    if (rc != MSDA_OK) return rc;
    const unsigned long long need = msda_small_loss_workspace_bytes(a.S, a.B, a.J, a.NV, a.KO, a.NB, a.L);
    if (workspace == nullptr || workspace_bytes < need) return serr("msda_small_loss: workspace smaller than msda_small_loss_workspace_bytes");
    a.part = static_cast<float *>(workspace);
    a.coef = a.part + (long long)a.S * a.B * kParts;
    begin_entry();
    if (a.B == 0) return MSDA_OK;               // no frame: nothing is launched and the losses are left unwritten
    hipLaunchKernelGGL(sl_part_kernel, dim3((unsigned)(a.S * a.B)), dim3(kBlock), 0, (hipStream_t)stream, a);
    rc = check_launch("sl_part_kernel");
    if (rc != MSDA_OK) return rc;
    hipLaunchKernelGGL(sl_final_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, a);
    return check_launch("sl_final_kernel");
}

int msda_small_loss_backward_f32(const int *dims, float img_res, const void *const *targets, const float *const *inputs,
                                 const float *grad_losses, float *const *grads, const void *workspace,
                                 unsigned long long workspace_bytes, msda_stream_t stream)
{
    SLArgs a;
    float dummy = 0.f;
    int rc = sl_setup(a, dims, img_res, targets, inputs, &dummy);
    if (rc != MSDA_OK) return rc;
    if (grad_losses == nullptr || grads == nullptr) return serr("msda_small_loss: null pointer");
    const unsigned long long need = msda_small_loss_workspace_bytes(a.S, a.B, a.J, a.NV, a.KO, a.NB, a.L);
    if (workspace == nullptr || workspace_bytes < need) return serr("msda_small_loss: workspace smaller than msda_small_loss_workspace_bytes");
    a.part = static_cast<float *>(const_cast<void *>(workspace));
    a.coef = a.part + (long long)a.S * a.B * kParts;
    a.glosses = grad_losses;
    for (int s = 0; s < a.S; ++s)
        for (int k = 0; k < kInputs; ++k) {
            a.s[s].grad[k] = grads[s * kInputs + k];
            if (a.B > 0 && a.s[s].grad[k] == nullptr) return serr("msda_small_loss: null gradient");
        }
    begin_entry();
    if (a.B == 0) return MSDA_OK;
    hipLaunchKernelGGL(sl_bwd_kernel, dim3((unsigned)(a.S * a.B)), dim3(kBlock), 0, (hipStream_t)stream, a);
    return check_launch("sl_bwd_kernel");
}
