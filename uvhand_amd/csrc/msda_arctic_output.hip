// The pose, camera and projection glue of make_output / prepare_data (arctic_tools/process.py:107-149, :249-299) between the
// MANO, object and nearest-neighbour kernels: three operations, each one launch forward and one launch backward.
//
// Pose heads.  Per (hand, frame, joint): axis-angle -> quaternion -> matrix (pytorch3d's axis_angle_to_matrix, 1/2 -
// theta^2/48 below 1e-6) and back matrix -> quaternion -> axis-angle (common/rot.py: x > 0 before the root, the denominator
// 2 max(|q|, 0.1), the largest |q| chosen with the lowest index on a tie, atan2, the same polynomial below 1e-6).  Per (root,
// frame): cam_t = (tx, ty, 2 f / (img_res max(s, 0.1) + 1e-9)), f = (K00 + K11) / 2.  One thread per item.
// Matrix to axis-angle.  The second half alone, from given matrices.
// Place and project.  Up to 8 segments of points [B, n, 3], each with a camera (0 .. 2): points + cam_t, and for the
// projected ones K x, x / z, 2 u / img_res - 1 and the pixel form 0.5 img_res (u + 1).  The backward's row blocks write
// grad_points; one more block per (camera, frame) walks that camera's rows of all its segments (per-thread strided partials
// in segment order, then an LDS tree) and writes grad_cam_t.
// The backward kernels recompute the forward from the inputs; the chosen candidate and the branches are constants, as for
// autograd.  fp32, fixed summation order, no atomics: bitwise reproducible.
//
// These kernels move a few MB per step and exist to remove launches; nothing here is tuned for bandwidth.
// aa2q, aa2q_bwd, q2m, q2m_bwd, project and project_bwd come from msda_pose.h, shared with msda_small_loss.hip.
#include <cmath>
#include <cstdio>
#include <cstring>

#include "msda_common.h"
#include "msda_launch.h"
#include "msda_pose.h"

namespace msda {

namespace {

constexpr int kBlock = 256;
constexpr int kJoints = 16, kMaxHands = 2, kMaxRoots = 3, kMaxSeg = 8, kMaxRows = 8192, kCams = 3, kMaxB = 65535;
constexpr float kMinS = 0.1f;


// ---- matrix -> quaternion -> axis-angle (common/rot.py) -------------------------------------------------------------------
// Row `pick` of the candidate table is r[k] = M[ia[k]] + sb[k] M[ib[k]] for k != pick and |q_pick|^2 for k = pick.
struct M2A {
    int pick;
    bool pos, small;
    float qa, den, r[4];
    Q q;
    float n, half, ang, s;
};

__device__ __forceinline__ void m2a_terms(int pick, int k, int &ia, int &ib, float &sb)
{
    // the pair of matrix entries behind candidate row `pick`, column k (k != pick); M is row-major m00 .. m22
    const int lo = pick < k ? pick : k, hi = pick < k ? k : pick;
    if (lo == 0) {                              // the antisymmetric parts: m21 - m12, m02 - m20, m10 - m01
        ia = hi == 1 ? 7 : (hi == 2 ? 2 : 3);
        ib = hi == 1 ? 5 : (hi == 2 ? 6 : 1);
        sb = -1.f;
    } else {                                    // the symmetric parts: m10 + m01, m02 + m20, m12 + m21
        const int key = lo * 4 + hi;            // (1, 2), (1, 3), (2, 3)
        ia = key == 6 ? 3 : (key == 7 ? 2 : 5);
        ib = key == 6 ? 1 : (key == 7 ? 6 : 7);
        sb = 1.f;
    }
}

__device__ __forceinline__ void m2aa_fwd(const float M[9], float out[3], M2A &t)
{
    const float x[4] = {1.0f + M[0] + M[4] + M[8], 1.0f + M[0] - M[4] - M[8], 1.0f - M[0] + M[4] - M[8], 1.0f - M[0] - M[4] + M[8]};
    float qa[4];
    for (int i = 0; i < 4; ++i) qa[i] = x[i] > 0.f ? sqrtf(x[i]) : 0.f;
    int pick = 0;
    for (int i = 1; i < 4; ++i)
        if (qa[i] > qa[pick]) pick = i;         // argmax: the lowest index wins a tie
    t.pick = pick;
    t.pos = x[pick] > 0.f;
    t.qa = qa[pick];
    t.den = 2.0f * fmaxf(t.qa, 0.1f);
    for (int k = 0; k < 4; ++k) {
        if (k == pick) { t.r[k] = __fmul_rn(t.qa, t.qa); continue; }
        int ia, ib;
        float sb;
        m2a_terms(pick, k, ia, ib, sb);
        t.r[k] = sb > 0.f ? M[ia] + M[ib] : M[ia] - M[ib];
    }
    t.q = {t.r[0] / t.den, t.r[1] / t.den, t.r[2] / t.den, t.r[3] / t.den};
    t.n = sqrtf(t.q.x * t.q.x + t.q.y * t.q.y + t.q.z * t.q.z);
    t.half = atan2f(t.n, t.q.w);
    t.ang = 2.f * t.half;
    t.small = fabsf(t.ang) < 1e-6f;
    t.s = t.small ? 0.5f - (t.ang * t.ang) / 48.f : sinf(t.half) / t.ang;
    out[0] = t.q.x / t.s; out[1] = t.q.y / t.s; out[2] = t.q.z / t.s;
}

// adds d loss / d M to G (g = d loss / d out)
__device__ __forceinline__ void m2aa_bwd(const M2A &t, const float g[3], float G[9])
{
    const float v[3] = {t.q.x, t.q.y, t.q.z};
    float gv[3] = {g[0] / t.s, g[1] / t.s, g[2] / t.s};
    const float gs = -(g[0] * v[0] + g[1] * v[1] + g[2] * v[2]) / (t.s * t.s);
    const float ghalf = t.small ? 2.f * gs * (-t.ang / 24.f)
                                : gs * cosf(t.half) / t.ang - 2.f * gs * sinf(t.half) / (t.ang * t.ang);
    const float d2 = t.n * t.n + t.q.w * t.q.w;
    const float gn = ghalf * t.q.w / d2, gw = -ghalf * t.n / d2;
    const float kn = t.n > 0.f ? gn / t.n : 0.f;                // torch.norm's gradient is 0 at 0
    for (int c = 0; c < 3; ++c) gv[c] += kn * v[c];
    const float gq[4] = {gw, gv[0], gv[1], gv[2]};
    float gr[4], dot = 0.f;
    for (int k = 0; k < 4; ++k) { gr[k] = gq[k] / t.den; dot += gq[k] * t.r[k]; }
    const float gden = -dot / (t.den * t.den);
    const float gqa = (t.qa >= 0.1f ? 2.f * gden : 0.f) + gr[t.pick] * 2.f * t.qa;      // clamp(min=0.1) passes at equality
    const float gx = t.pos ? gqa * 0.5f / t.qa : 0.f;
    const float s1 = (t.pick == 0 || t.pick == 1) ? 1.f : -1.f, s2 = (t.pick == 0 || t.pick == 2) ? 1.f : -1.f,
                s3 = (t.pick == 0 || t.pick == 3) ? 1.f : -1.f;
    G[0] += s1 * gx; G[4] += s2 * gx; G[8] += s3 * gx;
    for (int k = 0; k < 4; ++k) {
        if (k == t.pick) continue;
        int ia, ib;
        float sb;
        m2a_terms(t.pick, k, ia, ib, sb);
        G[ia] += gr[k];
        G[ib] += sb * gr[k];
    }
}

// ---- pose heads -----------------------------------------------------------------------------------------------------------
struct PoseArgs {
    const float *pose[kMaxHands], *root[kMaxRoots], *K;
    float *mats[kMaxHands], *aa[kMaxHands], *ct[kMaxRoots];
    const float *gmats[kMaxHands], *gaa[kMaxHands], *gct[kMaxRoots];
    float *gpose[kMaxHands], *groot[kMaxRoots];
    int nh, nr, B;
    float img_res;
};

__global__ void __launch_bounds__(kBlock) arctic_pose_fwd_kernel(PoseArgs a)
{
    const int it = blockIdx.x * kBlock + threadIdx.x;
    const int per_hand = a.B * kJoints;
    if (it < a.nh * per_hand) {
        const int h = it / per_hand, e = it % per_hand;          // e = b * 16 + j
        const float *p = a.pose[h] + 3 * (long long)e;
        float M[9], out[3];
        M2A t;
        q2m(aa2q(p[0], p[1], p[2]), M);
        m2aa_fwd(M, out, t);
        float *mo = a.mats[h] + 9 * (long long)e, *ao = a.aa[h] + 3 * (long long)e;
        for (int m = 0; m < 9; ++m) mo[m] = M[m];
        ao[0] = out[0]; ao[1] = out[1]; ao[2] = out[2];
        return;
    }
    const int rt = it - a.nh * per_hand;
    if (rt >= a.nr * a.B) return;
    const int h = rt / a.B, b = rt % a.B;
    const float *r = a.root[h] + 3 * b, *K = a.K + 9 * b;
    const float f = (K[0] + K[4]) / 2.0f;
    const float s = fmaxf(r[0], kMinS);
    float *o = a.ct[h] + 3 * b;
    o[0] = r[1]; o[1] = r[2]; o[2] = (2.f * f) / __fadd_rn(__fmul_rn(a.img_res, s), 1e-9f);
}

__global__ void __launch_bounds__(kBlock) arctic_pose_bwd_kernel(PoseArgs a)
{
    const int it = blockIdx.x * kBlock + threadIdx.x;
    const int per_hand = a.B * kJoints;
    if (it < a.nh * per_hand) {
        const int h = it / per_hand, e = it % per_hand;
        if (a.gpose[h] == nullptr) return;
        const float *p = a.pose[h] + 3 * (long long)e;
        float M[9], out[3], G[9], ga[3];
        M2A t;
        const Q q = aa2q(p[0], p[1], p[2]);
        q2m(q, M);
        for (int m = 0; m < 9; ++m) G[m] = a.gmats[h] ? a.gmats[h][9 * (long long)e + m] : 0.f;
        if (a.gaa[h]) {
            const float *g = a.gaa[h] + 3 * (long long)e;
            const float g3[3] = {g[0], g[1], g[2]};
            m2aa_fwd(M, out, t);
            m2aa_bwd(t, g3, G);
        }
        aa2q_bwd(p[0], p[1], p[2], q2m_bwd(q, G), ga);
        float *go = a.gpose[h] + 3 * (long long)e;
        go[0] = ga[0]; go[1] = ga[1]; go[2] = ga[2];
        return;
    }
    const int rt = it - a.nh * per_hand;
    if (rt >= a.nr * a.B) return;
    const int h = rt / a.B, b = rt % a.B;
    if (a.groot[h] == nullptr) return;
    float *go = a.groot[h] + 3 * b;
    if (a.gct[h] == nullptr) { go[0] = go[1] = go[2] = 0.f; return; }
    const float *r = a.root[h] + 3 * b, *K = a.K + 9 * b, *g = a.gct[h] + 3 * b;
    const float f = (K[0] + K[4]) / 2.0f;
    const float s = fmaxf(r[0], kMinS), den = __fadd_rn(__fmul_rn(a.img_res, s), 1e-9f);
    const float dtz = r[0] >= kMinS ? -2.f * f * a.img_res / (den * den) : 0.f;        // torch.clamp passes at equality
    go[0] = g[2] * dtz; go[1] = g[0]; go[2] = g[1];
}

// ---- matrix to axis-angle -------------------------------------------------------------------------------------------------
struct M2AArgs {
    const float *mats[kMaxHands], *gaa[kMaxHands];
    float *aa[kMaxHands], *gmats[kMaxHands];
    int nh, B;
};

__global__ void __launch_bounds__(kBlock) arctic_m2aa_fwd_kernel(M2AArgs a)
{
    const int it = blockIdx.x * kBlock + threadIdx.x;
    const int per_hand = a.B * kJoints;
    if (it >= a.nh * per_hand) return;
    const int h = it / per_hand, e = it % per_hand;
    const float *mi = a.mats[h] + 9 * (long long)e;
    float M[9], out[3];
    M2A t;
    for (int m = 0; m < 9; ++m) M[m] = mi[m];
    m2aa_fwd(M, out, t);
    float *ao = a.aa[h] + 3 * (long long)e;
    ao[0] = out[0]; ao[1] = out[1]; ao[2] = out[2];
}

__global__ void __launch_bounds__(kBlock) arctic_m2aa_bwd_kernel(M2AArgs a)
{
    const int it = blockIdx.x * kBlock + threadIdx.x;
    const int per_hand = a.B * kJoints;
    if (it >= a.nh * per_hand) return;
    const int h = it / per_hand, e = it % per_hand;
    if (a.gmats[h] == nullptr) return;
    float *go = a.gmats[h] + 9 * (long long)e;
    float M[9], out[3], G[9];
    for (int m = 0; m < 9; ++m) G[m] = 0.f;
    if (a.gaa[h]) {
        const float *mi = a.mats[h] + 9 * (long long)e, *g = a.gaa[h] + 3 * (long long)e;
        const float g3[3] = {g[0], g[1], g[2]};
        M2A t;
        for (int m = 0; m < 9; ++m) M[m] = mi[m];
        m2aa_fwd(M, out, t);
        m2aa_bwd(t, g3, G);
    }
    for (int m = 0; m < 9; ++m) go[m] = G[m];
}

// ---- place and project ----------------------------------------------------------------------------------------------------
struct PlaceSeg {
    const float *p, *gy, *gn, *gpx;
    float *y, *n2, *px, *gp;
    int n, cam, proj, blk0;
};
struct PlaceArgs {
    PlaceSeg s[kMaxSeg];
    const float *ct[kCams], *K;
    float *gct[kCams];
    int nseg, B, nblk;
    float img_res;
};
static_assert(sizeof(PlaceArgs) <= 4000, "kernel argument table");


__device__ __forceinline__ int place_seg_of(const PlaceArgs &a, int blk)
{
    int si = 0;
    while (si + 1 < a.nseg && blk >= a.s[si + 1].blk0) ++si;
    return si;
}

__global__ void __launch_bounds__(kBlock) arctic_place_fwd_kernel(PlaceArgs a)
{
    const int b = blockIdx.y;
    const PlaceSeg &s = a.s[place_seg_of(a, blockIdx.x)];
    const int row = (blockIdx.x - s.blk0) * kBlock + threadIdx.x;
    if (row >= s.n) return;
    const long long at = (long long)b * s.n + row;
    const float *c = a.ct[s.cam] + 3 * b, *p = s.p + 3 * at;
    const float y[3] = {p[0] + c[0], p[1] + c[1], p[2] + c[2]};
    float *yo = s.y + 3 * at;
    yo[0] = y[0]; yo[1] = y[1]; yo[2] = y[2];
    if (!s.proj) return;
    float n[2], ph[3];
    project(a.K + 9 * b, y, a.img_res, n, ph);
    const float half = 0.5f * a.img_res;
    s.n2[2 * at] = n[0]; s.n2[2 * at + 1] = n[1];
    s.px[2 * at] = half * (n[0] + 1.0f); s.px[2 * at + 1] = half * (n[1] + 1.0f);
}

// d loss / d (points + cam_t) of one row
__device__ __forceinline__ void place_row_grad(const PlaceArgs &a, const PlaceSeg &s, int b, long long at, float gy[3])
{
    gy[0] = gy[1] = gy[2] = 0.f;
    if (s.gy) { gy[0] = s.gy[3 * at]; gy[1] = s.gy[3 * at + 1]; gy[2] = s.gy[3 * at + 2]; }
    if (!s.proj || (s.gn == nullptr && s.gpx == nullptr)) return;
    const float *c = a.ct[s.cam] + 3 * b, *p = s.p + 3 * at;
    const float y[3] = {p[0] + c[0], p[1] + c[1], p[2] + c[2]};
    float n[2], ph[3], gn[2] = {0.f, 0.f}, gx[3];
    project(a.K + 9 * b, y, a.img_res, n, ph);
    if (s.gn) { gn[0] = s.gn[2 * at]; gn[1] = s.gn[2 * at + 1]; }
    if (s.gpx) { gn[0] += 0.5f * a.img_res * s.gpx[2 * at]; gn[1] += 0.5f * a.img_res * s.gpx[2 * at + 1]; }
    project_bwd(a.K + 9 * b, ph, a.img_res, gn, gx);
    gy[0] += gx[0]; gy[1] += gx[1]; gy[2] += gx[2];
}

__global__ void __launch_bounds__(kBlock) arctic_place_bwd_kernel(PlaceArgs a)
{
    __shared__ float red[3][kBlock];
    const int b = blockIdx.y, tid = threadIdx.x;
    if ((int)blockIdx.x < a.nblk) {                             // the blocks that own rows
        const PlaceSeg &s = a.s[place_seg_of(a, blockIdx.x)];
        const int row = (blockIdx.x - s.blk0) * kBlock + tid;
        if (row >= s.n || s.gp == nullptr) return;
        const long long at = (long long)b * s.n + row;
        float gy[3];
        place_row_grad(a, s, b, at, gy);
        s.gp[3 * at] = gy[0]; s.gp[3 * at + 1] = gy[1]; s.gp[3 * at + 2] = gy[2];
        return;
    }
    const int cam = blockIdx.x - a.nblk;                         // one block per (camera, frame)
    if (a.gct[cam] == nullptr) return;
    float acc[3] = {0.f, 0.f, 0.f};
    for (int si = 0; si < a.nseg; ++si) {
        const PlaceSeg &s = a.s[si];
        if (s.cam != cam) continue;
        for (int row = tid; row < s.n; row += kBlock) {
            float gy[3];
            place_row_grad(a, s, b, (long long)b * s.n + row, gy);
            acc[0] += gy[0]; acc[1] += gy[1]; acc[2] += gy[2];
        }
    }
    for (int k = 0; k < 3; ++k) red[k][tid] = acc[k];
    __syncthreads();
    for (int w = kBlock / 2; w > 0; w >>= 1) {
        if (tid < w)
            for (int k = 0; k < 3; ++k) red[k][tid] += red[k][tid + w];
        __syncthreads();
    }
    if (tid < 3) a.gct[cam][3 * b + tid] = red[tid][0];
}

// ---- host side ------------------------------------------------------------------------------------------------------------
void begin_entry()
{
    set_error(MSDA_OK, "");
    (void)hipGetLastError();
}

int oerr(const char *msg) { return set_error(MSDA_ERR_ARGUMENT, msg); }

bool pose_dims_ok(int nh, int nr, int B)
{
    return nh >= 0 && nh <= kMaxHands && nr >= 0 && nr <= kMaxRoots && nh + nr >= 1 && B >= 0 && B <= kMaxB;
}

bool place_dims_ok(int nseg, int B, int max_rows)
{
    return nseg >= 1 && nseg <= kMaxSeg && B >= 0 && B <= kMaxB && max_rows >= 1 && max_rows <= kMaxRows;
}

int pose_setup(PoseArgs &a, int nh, int nr, int B, float img_res, const float *const *poses, const float *const *roots,
               const float *K)
{
    memset(&a, 0, sizeof(a));
    if (!pose_dims_ok(nh, nr, B)) return oerr("msda_arctic_pose: unsupported geometry (msda_arctic_pose_supported)");
    if (nr > 0 && !(img_res > 0.f)) return oerr("msda_arctic_pose: img_res must be positive");
    if ((nh > 0 && poses == nullptr) || (nr > 0 && roots == nullptr)) return oerr("msda_arctic_pose: null pointer");
    a.nh = nh; a.nr = nr; a.B = B; a.img_res = img_res; a.K = K;
    for (int h = 0; h < nh; ++h) {
        a.pose[h] = poses[h];
        if (B > 0 && !poses[h]) return oerr("msda_arctic_pose: null pointer");
    }
    for (int h = 0; h < nr; ++h) {
        a.root[h] = roots[h];
        if (B > 0 && !roots[h]) return oerr("msda_arctic_pose: null pointer");
    }
    if (B > 0 && nr > 0 && K == nullptr) return oerr("msda_arctic_pose: null pointer");
    return MSDA_OK;
}

unsigned pose_blocks(int nh, int nr, int B) { return (unsigned)((nh * B * kJoints + nr * B + kBlock - 1) / kBlock); }

int m2aa_setup(M2AArgs &a, int nh, int B, const float *const *mats)
{
    memset(&a, 0, sizeof(a));
    if (nh < 1 || !pose_dims_ok(nh, 0, B)) return oerr("msda_arctic_m2aa: unsupported geometry (msda_arctic_pose_supported)");
    if (mats == nullptr) return oerr("msda_arctic_m2aa: null pointer");
    a.nh = nh; a.B = B;
    for (int h = 0; h < nh; ++h) {
        a.mats[h] = mats[h];
        if (B > 0 && !mats[h]) return oerr("msda_arctic_m2aa: null pointer");
    }
    return MSDA_OK;
}

int place_setup(PlaceArgs &a, int nseg, int B, float img_res, const int *rows, const int *camera, const int *proj,
                const float *const *points, const float *const *cam_t, const float *K)
{
    memset(&a, 0, sizeof(a));
    if (nseg < 1 || nseg > kMaxSeg) return oerr("msda_arctic_place: 1 .. 8 segments");
    if (rows == nullptr || camera == nullptr || proj == nullptr || points == nullptr || cam_t == nullptr)
        return oerr("msda_arctic_place: null pointer");
    int max_rows = 1, blk = 0;
    bool any_proj = false;
    for (int i = 0; i < nseg; ++i) {
        if (rows[i] < 1 || rows[i] > kMaxRows) return oerr("msda_arctic_place: 1 .. 8192 rows per segment");
        if (camera[i] < 0 || camera[i] >= kCams) return oerr("msda_arctic_place: camera index outside 0 .. 2");
        if (proj[i] != 0 && proj[i] != 1) return oerr("msda_arctic_place: project must be 0 or 1");
        if (rows[i] > max_rows) max_rows = rows[i];
        any_proj = any_proj || proj[i];
    }
    if (!place_dims_ok(nseg, B, max_rows)) return oerr("msda_arctic_place: unsupported geometry (msda_arctic_place_supported)");
    if (any_proj && !(img_res > 0.f)) return oerr("msda_arctic_place: img_res must be positive");
    a.nseg = nseg; a.B = B; a.img_res = img_res; a.K = K;
    for (int c = 0; c < kCams; ++c) a.ct[c] = cam_t[c];
    for (int i = 0; i < nseg; ++i) {
        PlaceSeg &s = a.s[i];
        s.p = points[i]; s.n = rows[i]; s.cam = camera[i]; s.proj = proj[i]; s.blk0 = blk;
        blk += (rows[i] + kBlock - 1) / kBlock;
        if (B > 0 && (!s.p || !a.ct[s.cam])) return oerr("msda_arctic_place: null pointer");
    }
    if (B > 0 && any_proj && K == nullptr) return oerr("msda_arctic_place: null pointer");
    a.nblk = blk;
    return MSDA_OK;
}

}  // namespace

}  // namespace msda

using namespace msda;

int msda_arctic_pose_supported(int n_hands, int n_roots, int B) { return pose_dims_ok(n_hands, n_roots, B) ? 1 : 0; }

int msda_arctic_pose_forward_f32(int n_hands, int n_roots, int B, float img_res, const float *const *poses,
                                 const float *const *roots, const float *K, float *const *mats, float *const *aa,
                                 float *const *cam_t, msda_stream_t stream)
{
    PoseArgs a;
    int rc = pose_setup(a, n_hands, n_roots, B, img_res, poses, roots, K);
    if (rc != MSDA_OK) return rc;
    if ((n_hands > 0 && (mats == nullptr || aa == nullptr)) || (n_roots > 0 && cam_t == nullptr))
        return oerr("msda_arctic_pose: null pointer");
    for (int h = 0; h < n_hands; ++h) {
        a.mats[h] = mats[h]; a.aa[h] = aa[h];
        if (B > 0 && (!mats[h] || !aa[h])) return oerr("msda_arctic_pose: null output");
    }
    for (int h = 0; h < n_roots; ++h) {
        a.ct[h] = cam_t[h];
        if (B > 0 && !cam_t[h]) return oerr("msda_arctic_pose: null output");
    }
    begin_entry();
    if (B == 0) return MSDA_OK;
    hipLaunchKernelGGL(arctic_pose_fwd_kernel, dim3(pose_blocks(n_hands, n_roots, B)), dim3(kBlock), 0, (hipStream_t)stream, a);
    return check_launch("arctic_pose_fwd_kernel");
}

int msda_arctic_pose_backward_f32(int n_hands, int n_roots, int B, float img_res, const float *const *poses,
                                  const float *const *roots, const float *K, const float *const *grad_mats,
                                  const float *const *grad_aa, const float *const *grad_cam_t, float *const *grad_poses,
                                  float *const *grad_roots, msda_stream_t stream)
{
    PoseArgs a;
    int rc = pose_setup(a, n_hands, n_roots, B, img_res, poses, roots, K);
    if (rc != MSDA_OK) return rc;
    if ((n_hands > 0 && (grad_mats == nullptr || grad_aa == nullptr || grad_poses == nullptr))
        || (n_roots > 0 && (grad_cam_t == nullptr || grad_roots == nullptr)))
        return oerr("msda_arctic_pose: null pointer");
    for (int h = 0; h < n_hands; ++h) { a.gmats[h] = grad_mats[h]; a.gaa[h] = grad_aa[h]; a.gpose[h] = grad_poses[h]; }
    for (int h = 0; h < n_roots; ++h) { a.gct[h] = grad_cam_t[h]; a.groot[h] = grad_roots[h]; }
    begin_entry();
    if (B == 0) return MSDA_OK;
    hipLaunchKernelGGL(arctic_pose_bwd_kernel, dim3(pose_blocks(n_hands, n_roots, B)), dim3(kBlock), 0, (hipStream_t)stream, a);
    return check_launch("arctic_pose_bwd_kernel");
}

int msda_arctic_m2aa_forward_f32(int n_hands, int B, const float *const *mats, float *const *aa, msda_stream_t stream)
{
    M2AArgs a;
    int rc = m2aa_setup(a, n_hands, B, mats);
    if (rc != MSDA_OK) return rc;
    if (aa == nullptr) return oerr("msda_arctic_m2aa: null pointer");
    for (int h = 0; h < n_hands; ++h) {
        a.aa[h] = aa[h];
        if (B > 0 && !aa[h]) return oerr("msda_arctic_m2aa: null output");
    }
    begin_entry();
    if (B == 0) return MSDA_OK;
    hipLaunchKernelGGL(arctic_m2aa_fwd_kernel, dim3(pose_blocks(n_hands, 0, B)), dim3(kBlock), 0, (hipStream_t)stream, a);
    return check_launch("arctic_m2aa_fwd_kernel");
}

int msda_arctic_m2aa_backward_f32(int n_hands, int B, const float *const *mats, const float *const *grad_aa,
                                  float *const *grad_mats, msda_stream_t stream)
{
    M2AArgs a;
    int rc = m2aa_setup(a, n_hands, B, mats);
    if (rc != MSDA_OK) return rc;
    if (grad_aa == nullptr || grad_mats == nullptr) return oerr("msda_arctic_m2aa: null pointer");
    for (int h = 0; h < n_hands; ++h) { a.gaa[h] = grad_aa[h]; a.gmats[h] = grad_mats[h]; }
    begin_entry();
    if (B == 0) return MSDA_OK;
    hipLaunchKernelGGL(arctic_m2aa_bwd_kernel, dim3(pose_blocks(n_hands, 0, B)), dim3(kBlock), 0, (hipStream_t)stream, a);
    return check_launch("arctic_m2aa_bwd_kernel");
}

int msda_arctic_place_supported(int n_segments, int B, int max_rows) { return place_dims_ok(n_segments, B, max_rows) ? 1 : 0; }

int msda_arctic_place_forward_f32(int n_segments, int B, float img_res, const int *rows, const int *camera, const int *project,
                                  const float *const *points, const float *const *cam_t, const float *K, float *const *placed,
                                  float *const *norm2d, float *const *pix2d, msda_stream_t stream)
{
    PlaceArgs a;
    int rc = place_setup(a, n_segments, B, img_res, rows, camera, project, points, cam_t, K);
    if (rc != MSDA_OK) return rc;
    if (placed == nullptr || norm2d == nullptr || pix2d == nullptr) return oerr("msda_arctic_place: null pointer");
    for (int i = 0; i < n_segments; ++i) {
        PlaceSeg &s = a.s[i];
        s.y = placed[i]; s.n2 = norm2d[i]; s.px = pix2d[i];
        if (B > 0 && (!s.y || (s.proj && (!s.n2 || !s.px)))) return oerr("msda_arctic_place: null output");
    }
    begin_entry();
    if (B == 0) return MSDA_OK;
    hipLaunchKernelGGL(arctic_place_fwd_kernel, dim3((unsigned)a.nblk, (unsigned)B), dim3(kBlock), 0, (hipStream_t)stream, a);
    return check_launch("arctic_place_fwd_kernel");
}

int msda_arctic_place_backward_f32(int n_segments, int B, float img_res, const int *rows, const int *camera, const int *project,
                                   const float *const *points, const float *const *cam_t, const float *K,
                                   const float *const *grad_placed, const float *const *grad_norm2d,
                                   const float *const *grad_pix2d, float *const *grad_points, float *const *grad_cam_t,
                                   msda_stream_t stream)
{
    PlaceArgs a;
    int rc = place_setup(a, n_segments, B, img_res, rows, camera, project, points, cam_t, K);
    if (rc != MSDA_OK) return rc;
    if (grad_placed == nullptr || grad_norm2d == nullptr || grad_pix2d == nullptr || grad_points == nullptr || grad_cam_t == nullptr)
        return oerr("msda_arctic_place: null pointer");
    for (int i = 0; i < n_segments; ++i) {
        PlaceSeg &s = a.s[i];
        s.gy = grad_placed[i]; s.gn = grad_norm2d[i]; s.gpx = grad_pix2d[i]; s.gp = grad_points[i];
    }
    for (int c = 0; c < kCams; ++c) a.gct[c] = grad_cam_t[c];
    begin_entry();
    if (B == 0) return MSDA_OK;
    hipLaunchKernelGGL(arctic_place_bwd_kernel, dim3((unsigned)(a.nblk + kCams), (unsigned)B), dim3(kBlock), 0, (hipStream_t)stream, a);
    return check_launch("arctic_place_bwd_kernel");
}
