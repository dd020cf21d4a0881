// MANO hand layer (smplx lbs: Rodrigues, shape and pose blend shapes, the kinematic chain, linear blend skinning) for every
// hand of every group of a call, in one launch forward and two backward.
//
// A layer is one MANO model: v_template [V, 3], shapedirs [V, 3, nb], posedirs [135, 3 V] (smplx's layout: row p = pose
// feature p, column 3 v + c), J_template [16, 3] and J_shapedirs [16, 3, nb] (J_regressor folded into the template and the
// shape directions when the layer is built, so J = J_template + J_shapedirs . beta), lbs_weights [V, 16], pose_mean [48],
// parents (parents[0] = -1, 0 <= parents[j] < j) and E extra-joint vertex ids (the fingertips).  A group is one layer and
// B_g hands: betas [B_g or 1, nb], global_orient [B_g, 3], hand_pose [B_g, 45], transl [B_g, 3] or none; vertices
// [B_g, V, 3], joints [B_g, 16 + E, 3].
//
//   forward   one workgroup per (group, tile of kHT hands, slice of kVS vertices).  Each recomputes, in LDS, its hands'
//             16 Rodrigues matrices, pose features, rest joints and the chain by depth level (cheap), then streams its
//             vertices' posedirs / shapedirs / lbs_weights columns once for the whole hand tile.  Slice 0 writes the 16 posed
//             joints; the workgroup that owns a fingertip vertex writes that joint.
//   backward  launch 1, same grid: recomputes the forward's LDS state and v_posed of its slice, takes g_vertices plus the
//             fingertip rows of g_joints, and writes per (hand, slice) partials: dA (16 x 12), g_pose_feature (135), the
//             shapedirs part of g_beta and g_transl.  Launch 2, one workgroup per hand tile: sums the slices' partials in
//             slice order, then the chain backward (children pulled in a fixed order, deepest level first), the J path into
//             beta and the Rodrigues backward (the autograd gradient of smplx's formula, 1e-8 added inside the norm).
// Fixed summation order everywhere, no atomics: bitwise reproducible.
#include <cstdio>
#include <cstring>

#include "msda_common.h"
#include "msda_launch.h"

namespace msda {

namespace {

constexpr int kJ = 16, kPF = 135, kPose = 48, kMaxBetas = 16, kMaxExtra = 8, kMaxLayers = 4, kMaxGroups = 16, kMaxV = 8192;
constexpr int kHT = 8;                         // hands per tile
constexpr int kVS = 64;                        // vertices per slice
constexpr int kNC = 3 * kVS;                   // posedirs columns per slice
constexpr int kBlock = 192;                    // one thread per column in the blend-shape loops
constexpr int kPart = kJ * 12 + kPF + kMaxBetas + 3;   // per (hand, slice) partials: dA, g_pose_feature, g_beta, g_transl
constexpr int kOffPF = kJ * 12, kOffBeta = kOffPF + kPF, kOffTransl = kOffBeta + kMaxBetas;

struct ManoLayer {
    const float *v_template, *shapedirs, *posedirs, *j_template, *j_shapedirs, *weights, *pose_mean;
    signed char parent[kJ], depth[kJ];
    short extra[kMaxExtra];
    int max_depth;
};
struct ManoGroup {
    const float *betas, *go, *hp, *transl;
    float *verts, *joints;
    const float *gverts, *gjoints;
    float *gbetas, *ggo, *ghp, *gtransl;
    long long ws;                               // float offset of this group's partials [B][nslices][kPart]
    int layer, B, bcast, tile0;
};
struct ManoArgs {
    ManoLayer L[kMaxLayers];
    ManoGroup g[kMaxGroups + 1];                // g[ngroups].tile0 = total tiles
    float *ws;
    int V, nb, E, nslices, ngroups;
};
static_assert(sizeof(ManoArgs) <= 4000, "kernel argument table");

struct ManoSmem {                               // per hand of the tile
    float pose[kHT][kPose];
    float beta[kHT][kMaxBetas];
    float R[kHT][kJ][9];
    float J[kHT][kJ][3];
    float G[kHT][kJ][12];                       // global transform [R^G | t], 3 x 4 row-major
    float A[kHT][kJ][12];                       // [R^G | t - R^G J]
    float pf[kHT][kPF];
};
struct ManoSlice {                              // per slice (forward and backward launch 1)
    float W[kVS][kJ];
    float VP[kHT][kNC];                         // v_posed
    float GV[kHT][kNC];                         // incoming vertex gradient (backward)
    float DVP[kHT][kNC];                        // gradient of v_posed (backward)
};
struct ManoChain {                              // backward launch 2
    float par[kHT][kPart];
    float dRG[kHT][kJ][9];
    float dt[kHT][kJ][3];
    float dJ[kHT][kJ][3];
    float dR[kHT][kJ][9];
    float drel[kHT][kJ][3];
};

__device__ int find_group(const ManoArgs &P, int tile)
{
    int g = 0;
    while (g + 1 < P.ngroups && P.g[g + 1].tile0 <= tile) ++g;
    return g;
}

// the hands' pose, betas, Rodrigues matrices, pose features, rest joints, chain and skinning transforms
__device__ void mano_prelude(const ManoArgs &P, const ManoLayer &L, const ManoGroup &g, int h0, int nh, ManoSmem &S)
{
    const int tid = threadIdx.x, nb = P.nb;
    for (int i = tid; i < nh * kPose; i += kBlock) {
        const int h = i / kPose, k = i % kPose, b = h0 + h;
        const float v = k < 3 ? g.go[(long long)b * 3 + k] : g.hp[(long long)b * 45 + (k - 3)];
        S.pose[h][k] = v + L.pose_mean[k];
    }
    for (int i = tid; i < nh * nb; i += kBlock) {
        const int h = i / nb, k = i % nb;
        S.beta[h][k] = g.betas[(long long)(g.bcast ? 0 : h0 + h) * nb + k];
    }
    __syncthreads();
    for (int i = tid; i < nh * kJ; i += kBlock) {
        const int h = i / kJ, j = i % kJ;
        const float rx = S.pose[h][3 * j], ry = S.pose[h][3 * j + 1], rz = S.pose[h][3 * j + 2];
        const float ex = rx + 1e-8f, ey = ry + 1e-8f, ez = rz + 1e-8f;
        const float th = sqrtf(ex * ex + ey * ey + ez * ez);
        const float nx = rx / th, ny = ry / th, nz = rz / th;
        const float s = sinf(th), t = 1.f - cosf(th);
        const float K[9] = {0.f, -nz, ny, nz, 0.f, -nx, -ny, nx, 0.f};
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) {
                const float kk = K[r * 3] * K[c] + K[r * 3 + 1] * K[3 + c] + K[r * 3 + 2] * K[6 + c];
                const float v = (r == c ? 1.f : 0.f) + s * K[r * 3 + c] + t * kk;
                S.R[h][j][r * 3 + c] = v;
                if (j > 0) S.pf[h][(j - 1) * 9 + r * 3 + c] = v - (r == c ? 1.f : 0.f);
            }
    }
    for (int i = tid; i < nh * kJ * 3; i += kBlock) {
        const int h = i / (kJ * 3), jc = i % (kJ * 3);
        float v = 0.f;                              // the shape blend from zero, as mano_vposed sums it
        for (int k = 0; k < nb; ++k) v += L.j_shapedirs[jc * nb + k] * S.beta[h][k];
        S.J[h][jc / 3][jc % 3] = L.j_template[jc] + v;
    }
    __syncthreads();
    for (int lvl = 0; lvl <= L.max_depth; ++lvl) {
        for (int i = tid; i < nh * kJ * 12; i += kBlock) {
            const int h = i / (kJ * 12), j = (i / 12) % kJ, e = i % 12, r = e / 4, c = e % 4;
            if (L.depth[j] != lvl) continue;
            const int p = L.parent[j];
            float v;
            if (p < 0) {
                v = c < 3 ? S.R[h][j][r * 3 + c] : S.J[h][j][r];
            } else {
                const float *Gp = S.G[h][p];
                if (c < 3) {
                    v = Gp[r * 4] * S.R[h][j][c] + Gp[r * 4 + 1] * S.R[h][j][3 + c] + Gp[r * 4 + 2] * S.R[h][j][6 + c];
                } else {
                    v = Gp[r * 4 + 3];
                    for (int m = 0; m < 3; ++m) v += Gp[r * 4 + m] * (S.J[h][j][m] - S.J[h][p][m]);
                }
            }
            S.G[h][j][e] = v;
        }
        __syncthreads();
    }
    for (int i = tid; i < nh * kJ * 3; i += kBlock) {
        const int h = i / (kJ * 3), j = (i / 3) % kJ, r = i % 3;
        const float *Gj = S.G[h][j];
        float t = Gj[r * 4 + 3];
        for (int m = 0; m < 3; ++m) {
            S.A[h][j][r * 4 + m] = Gj[r * 4 + m];
            t -= Gj[r * 4 + m] * S.J[h][j][m];
        }
        S.A[h][j][r * 4 + 3] = t;
    }
    __syncthreads();
}

// lbs_weights of the slice into LDS, then v_posed [h][3 v + c] of the slice's vertices (one thread per column)
__device__ void mano_vposed(const ManoArgs &P, const ManoLayer &L, int v0, int nv, int nh, const ManoSmem &S, ManoSlice &Q)
{
    const int tid = threadIdx.x, nb = P.nb, V = P.V;
    for (int i = tid; i < nv * kJ; i += kBlock) Q.W[i / kJ][i % kJ] = L.weights[(long long)(v0 + i / kJ) * kJ + i % kJ];
    const int col = tid;
    if (col < 3 * nv) {
        const long long gc = (long long)v0 * 3 + col;
        // each blend is summed from zero and added to the template once: summed onto the template, its 135 (or nb) small
        // terms would each round at the template's magnitude, which is as large as a whole pose offset at small angles
        float acc[kHT], off[kHT];
        const float tmpl = L.v_template[gc];
        for (int h = 0; h < kHT; ++h) acc[h] = off[h] = 0.f;
        for (int k = 0; k < nb; ++k) {
            const float sd = L.shapedirs[gc * nb + k];
            for (int h = 0; h < kHT; ++h)
                if (h < nh) acc[h] += sd * S.beta[h][k];
        }
        const float *pd = L.posedirs + gc;
        for (int p = 0; p < kPF; ++p) {
            const float d = pd[(long long)p * 3 * V];
            for (int h = 0; h < kHT; ++h)
                if (h < nh) off[h] += S.pf[h][p] * d;
        }
        for (int h = 0; h < kHT; ++h)
            if (h < nh) Q.VP[h][col] = (tmpl + acc[h]) + off[h];
    }
    __syncthreads();
}

__device__ __forceinline__ void skin_transform(const ManoSmem &S, const ManoSlice &Q, int h, int v, float T[12])
{
    for (int e = 0; e < 12; ++e) T[e] = 0.f;
    for (int j = 0; j < kJ; ++j) {
        const float w = Q.W[v][j];
        for (int e = 0; e < 12; ++e) T[e] += w * S.A[h][j][e];
    }
}

__global__ __launch_bounds__(kBlock) void mano_fwd_kernel(ManoArgs P)
{
    __shared__ ManoSmem S;
    __shared__ ManoSlice Q;
    const int tile = blockIdx.x / P.nslices, slice = blockIdx.x % P.nslices;
    const ManoGroup &g = P.g[find_group(P, tile)];
    const ManoLayer &L = P.L[g.layer];
    const int h0 = (tile - g.tile0) * kHT, nh = min(kHT, g.B - h0);
    const int v0 = slice * kVS, nv = min(kVS, P.V - v0);
    const int tid = threadIdx.x, E = P.E, NJ = kJ + E;
    mano_prelude(P, L, g, h0, nh, S);
    if (slice == 0)
        for (int i = tid; i < nh * kJ * 3; i += kBlock) {
            const int h = i / (kJ * 3), j = (i / 3) % kJ, c = i % 3, b = h0 + h;
            float v = S.G[h][j][c * 4 + 3];
            if (g.transl) v += g.transl[(long long)b * 3 + c];
            g.joints[((long long)b * NJ + j) * 3 + c] = v;
        }
    mano_vposed(P, L, v0, nv, nh, S, Q);
    for (int i = tid; i < nh * nv; i += kBlock) {
        const int h = i / nv, v = i % nv, b = h0 + h;
        float T[12];
        skin_transform(S, Q, h, v, T);
        const float x = Q.VP[h][3 * v], y = Q.VP[h][3 * v + 1], z = Q.VP[h][3 * v + 2];
        float o[3];
        for (int r = 0; r < 3; ++r) {
            o[r] = T[r * 4] * x + T[r * 4 + 1] * y + T[r * 4 + 2] * z + T[r * 4 + 3];
            if (g.transl) o[r] += g.transl[(long long)b * 3 + r];
        }
        float *out = g.verts + ((long long)b * P.V + v0 + v) * 3;
        out[0] = o[0]; out[1] = o[1]; out[2] = o[2];
        for (int e = 0; e < E; ++e)
            if (L.extra[e] == v0 + v) {
                float *jo = g.joints + ((long long)b * NJ + kJ + e) * 3;
                jo[0] = o[0]; jo[1] = o[1]; jo[2] = o[2];
            }
    }
}

__global__ __launch_bounds__(kBlock) void mano_bwd_slice_kernel(ManoArgs P)
{
    __shared__ ManoSmem S;
    __shared__ ManoSlice Q;
    const int tile = blockIdx.x / P.nslices, slice = blockIdx.x % P.nslices;
    const ManoGroup &g = P.g[find_group(P, tile)];
    const ManoLayer &L = P.L[g.layer];
    const int h0 = (tile - g.tile0) * kHT, nh = min(kHT, g.B - h0);
    const int v0 = slice * kVS, nv = min(kVS, P.V - v0);
    const int tid = threadIdx.x, E = P.E, NJ = kJ + E, nb = P.nb, V = P.V;
    mano_prelude(P, L, g, h0, nh, S);
    mano_vposed(P, L, v0, nv, nh, S, Q);
    // incoming gradient of the slice's vertices (fingertip joints included), and of v_posed
    for (int i = tid; i < nh * nv; i += kBlock) {
        const int h = i / nv, v = i % nv, b = h0 + h;
        float gv[3] = {0.f, 0.f, 0.f};
        if (g.gverts) {
            const float *src = g.gverts + ((long long)b * V + v0 + v) * 3;
            gv[0] = src[0]; gv[1] = src[1]; gv[2] = src[2];
        }
        if (g.gjoints)
            for (int e = 0; e < E; ++e)
                if (L.extra[e] == v0 + v) {
                    const float *src = g.gjoints + ((long long)b * NJ + kJ + e) * 3;
                    gv[0] += src[0]; gv[1] += src[1]; gv[2] += src[2];
                }
        float T[12];
        skin_transform(S, Q, h, v, T);
        for (int c = 0; c < 3; ++c) {
            Q.GV[h][3 * v + c] = gv[c];
            Q.DVP[h][3 * v + c] = T[c] * gv[0] + T[4 + c] * gv[1] + T[8 + c] * gv[2];
        }
    }
    __syncthreads();
    float *part = P.ws + g.ws + ((long long)h0 * P.nslices + slice) * kPart;
    const long long hstride = (long long)P.nslices * kPart;
    // dA[j][r][c] = sum_v W[v][j] gv[v][r] [v_posed - J_j, 1][v][c]: the rotation part is taken about the rest joint, which
    // is what the gradient of R^G_j comes to (dA[c] - dA[3] J_j[c]); formed per vertex, the two products do not have to cancel
    for (int i = tid; i < nh * kJ * 3; i += kBlock) {
        const int h = i / (kJ * 3), j = (i / 3) % kJ, r = i % 3;
        const float jx = S.J[h][j][0], jy = S.J[h][j][1], jz = S.J[h][j][2];
        float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
        for (int v = 0; v < nv; ++v) {
            const float wg = Q.W[v][j] * Q.GV[h][3 * v + r];
            a0 += wg * (Q.VP[h][3 * v] - jx);
            a1 += wg * (Q.VP[h][3 * v + 1] - jy);
            a2 += wg * (Q.VP[h][3 * v + 2] - jz);
            a3 += wg;
        }
        float *d = part + h * hstride + j * 12 + r * 4;
        d[0] = a0; d[1] = a1; d[2] = a2; d[3] = a3;
    }
    // g_pose_feature[p] = sum over the slice's columns of posedirs[p][col] dvp[col]
    if (tid < kPF) {
        const int p = tid;
        const float *pd = L.posedirs + (long long)p * 3 * V + (long long)v0 * 3;
        float acc[kHT];
        for (int h = 0; h < kHT; ++h) acc[h] = 0.f;
        for (int col = 0; col < 3 * nv; ++col) {
            const float d = pd[col];
            for (int h = 0; h < kHT; ++h)
                if (h < nh) acc[h] += d * Q.DVP[h][col];
        }
        for (int h = 0; h < nh; ++h) part[h * hstride + kOffPF + p] = acc[h];
    }
    // shapedirs part of g_beta, and g_transl
    for (int i = tid; i < nh * kMaxBetas; i += kBlock) {
        const int h = i / kMaxBetas, k = i % kMaxBetas;
        float acc = 0.f;
        if (k < nb)
            for (int col = 0; col < 3 * nv; ++col) acc += L.shapedirs[((long long)v0 * 3 + col) * nb + k] * Q.DVP[h][col];
        part[h * hstride + kOffBeta + k] = acc;
    }
    for (int i = tid; i < nh * 3; i += kBlock) {
        const int h = i / 3, c = i % 3;
        float acc = 0.f;
        for (int v = 0; v < nv; ++v) acc += Q.GV[h][3 * v + c];
        part[h * hstride + kOffTransl + c] = acc;
    }
}

__global__ __launch_bounds__(kBlock) void mano_bwd_chain_kernel(ManoArgs P)
{
    __shared__ ManoSmem S;
    __shared__ ManoChain C;
    const int tile = blockIdx.x;
    const ManoGroup &g = P.g[find_group(P, tile)];
    const ManoLayer &L = P.L[g.layer];
    const int h0 = (tile - g.tile0) * kHT, nh = min(kHT, g.B - h0);
    const int tid = threadIdx.x, E = P.E, NJ = kJ + E, nb = P.nb, ns = P.nslices;
    mano_prelude(P, L, g, h0, nh, S);
    for (int i = tid; i < nh * kPart; i += kBlock) {
        const int h = i / kPart, q = i % kPart;
        const float *src = P.ws + g.ws + (long long)(h0 + h) * ns * kPart + q;
        float acc = 0.f;
        for (int s = 0; s < ns; ++s) acc += src[(long long)s * kPart];
        C.par[h][q] = acc;
    }
    __syncthreads();
    // A_j = [R^G | t - R^G J]: gradients of R^G_j (the partials' rotation part, already about J_j), t_j (posed joints
    // included) and the direct part of J_j
    for (int i = tid; i < nh * kJ; i += kBlock) {
        const int h = i / kJ, j = i % kJ, b = h0 + h;
        const float *dA = C.par[h] + j * 12;
        const float *RG = S.G[h][j];
        for (int r = 0; r < 3; ++r) {
            for (int m = 0; m < 3; ++m) C.dRG[h][j][r * 3 + m] = dA[r * 4 + m];
            C.dt[h][j][r] = dA[r * 4 + 3] + (g.gjoints ? g.gjoints[((long long)b * NJ + j) * 3 + r] : 0.f);
        }
        for (int m = 0; m < 3; ++m)
            C.dJ[h][j][m] = -(RG[m] * dA[3] + RG[4 + m] * dA[7] + RG[8 + m] * dA[11]);
    }
    __syncthreads();
    // the chain, deepest level first: G_j = G_p [R_j | J_j - J_p]
    for (int lvl = L.max_depth; lvl >= 0; --lvl) {
        for (int i = tid; i < nh * kJ; i += kBlock) {
            const int h = i / kJ, j = i % kJ;
            if (L.depth[j] != lvl) continue;
            float dRG[9], dt[3];
            for (int e = 0; e < 9; ++e) dRG[e] = C.dRG[h][j][e];
            for (int r = 0; r < 3; ++r) dt[r] = C.dt[h][j][r];
            for (int c = j + 1; c < kJ; ++c) {
                if (L.parent[c] != j) continue;
                const float *Rc = S.R[h][c], *dRc = C.dRG[h][c], *dtc = C.dt[h][c];
                float rel[3];
                for (int m = 0; m < 3; ++m) rel[m] = S.J[h][c][m] - S.J[h][j][m];
                for (int r = 0; r < 3; ++r) {
                    for (int m = 0; m < 3; ++m)
                        dRG[r * 3 + m] += dRc[r * 3] * Rc[m * 3] + dRc[r * 3 + 1] * Rc[m * 3 + 1] + dRc[r * 3 + 2] * Rc[m * 3 + 2]
                                          + dtc[r] * rel[m];
                    dt[r] += dtc[r];
                }
            }
            for (int e = 0; e < 9; ++e) C.dRG[h][j][e] = dRG[e];
            for (int r = 0; r < 3; ++r) C.dt[h][j][r] = dt[r];
            const int p = L.parent[j];
            if (p < 0) {
                for (int e = 0; e < 9; ++e) C.dR[h][j][e] = dRG[e];
                for (int r = 0; r < 3; ++r) C.drel[h][j][r] = dt[r];
            } else {
                const float *Gp = S.G[h][p];
                for (int r = 0; r < 3; ++r) {
                    for (int m = 0; m < 3; ++m)
                        C.dR[h][j][r * 3 + m] = Gp[r] * dRG[m] + Gp[4 + r] * dRG[3 + m] + Gp[8 + r] * dRG[6 + m];
                    C.drel[h][j][r] = Gp[r] * dt[0] + Gp[4 + r] * dt[1] + Gp[8 + r] * dt[2];
                }
            }
        }
        __syncthreads();
    }
    for (int i = tid; i < nh * kJ; i += kBlock) {
        const int h = i / kJ, j = i % kJ;
        for (int m = 0; m < 3; ++m) {
            float v = C.dJ[h][j][m] + C.drel[h][j][m];
            for (int c = j + 1; c < kJ; ++c)
                if (L.parent[c] == j) v -= C.drel[h][c][m];
            C.dJ[h][j][m] = v;
        }
    }
    __syncthreads();
    for (int i = tid; i < nh * nb; i += kBlock) {
        const int h = i / nb, k = i % nb;
        float v = C.par[h][kOffBeta + k];
        for (int jc = 0; jc < kJ * 3; ++jc) v += L.j_shapedirs[jc * nb + k] * C.dJ[h][jc / 3][jc % 3];
        g.gbetas[(long long)(h0 + h) * nb + k] = v;
    }
    // Rodrigues backward: R = I + sin(th) K + (1 - cos(th)) K^2, th = |r + 1e-8|, K = [r / th]_x
    for (int i = tid; i < nh * kJ; i += kBlock) {
        const int h = i / kJ, j = i % kJ, b = h0 + h;
        float Gm[9];
        for (int e = 0; e < 9; ++e) Gm[e] = C.dR[h][j][e] + (j > 0 ? C.par[h][kOffPF + (j - 1) * 9 + e] : 0.f);
        const float rx = S.pose[h][3 * j], ry = S.pose[h][3 * j + 1], rz = S.pose[h][3 * j + 2];
        const float ex = rx + 1e-8f, ey = ry + 1e-8f, ez = rz + 1e-8f;
        const float th = sqrtf(ex * ex + ey * ey + ez * ez);
        const float nx = rx / th, ny = ry / th, nz = rz / th;
        const float s = sinf(th), co = cosf(th), t = 1.f - co;
        const float K[9] = {0.f, -nz, ny, nz, 0.f, -nx, -ny, nx, 0.f};
        float K2[9];
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) K2[r * 3 + c] = K[r * 3] * K[c] + K[r * 3 + 1] * K[3 + c] + K[r * 3 + 2] * K[6 + c];
        float gK_dot = 0.f, gK2_dot = 0.f;
        for (int e = 0; e < 9; ++e) { gK_dot += Gm[e] * K[e]; gK2_dot += Gm[e] * K2[e]; }
        const float gth = co * gK_dot + s * gK2_dot;
        float gK[9];                                  // s G + t (G K^T + K^T G)
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) {
                float a = 0.f;
                for (int m = 0; m < 3; ++m) a += Gm[r * 3 + m] * K[c * 3 + m] + K[m * 3 + r] * Gm[m * 3 + c];
                gK[r * 3 + c] = s * Gm[r * 3 + c] + t * a;
            }
        const float gnx = gK[7] - gK[5], gny = gK[2] - gK[6], gnz = gK[3] - gK[1];
        const float gnr = gnx * rx + gny * ry + gnz * rz;
        const float th3 = th * th * th;
        const float dr[3] = {gnx / th - gnr * ex / th3 + gth * ex / th, gny / th - gnr * ey / th3 + gth * ey / th,
                             gnz / th - gnr * ez / th3 + gth * ez / th};
        float *dst = j == 0 ? g.ggo + (long long)b * 3 : g.ghp + (long long)b * 45 + (j - 1) * 3;
        dst[0] = dr[0]; dst[1] = dr[1]; dst[2] = dr[2];
    }
    if (g.gtransl)
        for (int i = tid; i < nh * 3; i += kBlock) {
            const int h = i / 3, c = i % 3, b = h0 + h;
            float v = C.par[h][kOffTransl + c];
            if (g.gjoints)                            // the fingertip rows are already in the vertex partials
                for (int j = 0; j < kJ; ++j) v += g.gjoints[((long long)b * NJ + j) * 3 + c];
            g.gtransl[(long long)b * 3 + c] = v;
        }
}

// ---- host side ---------------------------------------------------------------------------------------------------------------
void begin_entry()
{
    set_error(MSDA_OK, "");
    (void)hipGetLastError();
}

int serr(const char *msg) { return set_error(MSDA_ERR_ARGUMENT, msg); }

bool mano_dims_ok(int V, int nb, int E) { return V >= 1 && V <= kMaxV && nb >= 1 && nb <= kMaxBetas && E >= 0 && E <= kMaxExtra; }

int nslices_of(int V) { return (V + kVS - 1) / kVS; }

// everything but the per-group tensors; `need_ws`: the backward workspace (bytes)
int mano_setup(ManoArgs &a, int V, int nb, int E, int n_layers, const float *const *layer_tensors, const int *layer_index,
               int n_groups, const int *group_layer, const int *group_B, const int *group_bcast, unsigned long long &need_ws)
{
    if (!mano_dims_ok(V, nb, E)) return serr("msda_mano: need 1 <= V <= 8192, 1 <= n_betas <= 16, 0 <= n_extra <= 8");
    if (n_layers < 1 || n_layers > kMaxLayers || n_groups < 1 || n_groups > kMaxGroups)
        return serr("msda_mano: need 1 <= layers <= 4 and 1 <= groups <= 16");
    if (layer_tensors == nullptr || layer_index == nullptr || group_layer == nullptr || group_B == nullptr)
        return serr("msda_mano: null pointer");
    std::memset(&a, 0, sizeof(a));
    a.V = V; a.nb = nb; a.E = E; a.nslices = nslices_of(V); a.ngroups = n_groups;
    for (int l = 0; l < n_layers; ++l) {
        const float *const *t = layer_tensors + 7 * l;
        for (int k = 0; k < 7; ++k)
            if (t[k] == nullptr) return serr("msda_mano: null layer tensor");
        ManoLayer &L = a.L[l];
        L.v_template = t[0]; L.shapedirs = t[1]; L.posedirs = t[2]; L.j_template = t[3]; L.j_shapedirs = t[4];
        L.weights = t[5]; L.pose_mean = t[6];
        const int *idx = layer_index + (kJ + E) * l;
        if (idx[0] != -1) return serr("msda_mano: parents[0] must be -1");
        L.parent[0] = -1; L.depth[0] = 0;
        for (int j = 1; j < kJ; ++j) {
            if (idx[j] < 0 || idx[j] >= j) return serr("msda_mano: need 0 <= parents[j] < j for j >= 1");
            L.parent[j] = (signed char)idx[j];
            L.depth[j] = (signed char)(L.depth[idx[j]] + 1);
            if (L.depth[j] > L.max_depth) L.max_depth = L.depth[j];
        }
        for (int e = 0; e < E; ++e) {
            if (idx[kJ + e] < 0 || idx[kJ + e] >= V) return serr("msda_mano: extra joint vertex id out of range");
            L.extra[e] = (short)idx[kJ + e];
        }
    }
    long long tiles = 0, ws = 0;
    for (int i = 0; i < n_groups; ++i) {
        ManoGroup &g = a.g[i];
        if (group_layer[i] < 0 || group_layer[i] >= n_layers) return serr("msda_mano: group layer out of range");
        if (group_B[i] < 0) return serr("msda_mano: negative batch");
        if ((long long)group_B[i] * V * 3 >= (1LL << 31)) return serr("msda_mano: tensors beyond 2^31 elements");
        g.layer = group_layer[i]; g.B = group_B[i]; g.bcast = group_bcast != nullptr && group_bcast[i] != 0;
        g.tile0 = (int)tiles; g.ws = ws;
        tiles += (group_B[i] + kHT - 1) / kHT;
        ws += (long long)group_B[i] * a.nslices * kPart;
    }
    if (tiles * a.nslices >= (1LL << 31)) return serr("msda_mano: too many hands");
    a.g[n_groups].tile0 = (int)tiles;
    need_ws = (unsigned long long)ws * sizeof(float);
    return MSDA_OK;
}

int total_tiles(const ManoArgs &a) { return a.g[a.ngroups].tile0; }

}  // namespace

}  // namespace msda

using namespace msda;

int msda_mano_supported(int V, int n_betas, int n_extra) { return mano_dims_ok(V, n_betas, n_extra) ? 1 : 0; }

unsigned long long msda_mano_workspace_bytes(int V, int n_betas, int n_extra, int n_groups, const int *group_B)
{
    if (!mano_dims_ok(V, n_betas, n_extra) || n_groups < 1 || n_groups > kMaxGroups || group_B == nullptr) return 0;
    unsigned long long n = 0;
    for (int i = 0; i < n_groups; ++i) {
        if (group_B[i] < 0) return 0;
        n += (unsigned long long)group_B[i] * nslices_of(V) * kPart;
    }
    return n * sizeof(float);
}

int msda_mano_forward_f32(int V, int n_betas, int n_extra, int n_layers, const float *const *layer_tensors, const int *layer_index,
                          int n_groups, const int *group_layer, const int *group_B, const int *group_bcast,
                          const float *const *inputs, float *const *outputs, msda_stream_t stream)
{
    ManoArgs a;
    unsigned long long need_ws = 0;
    int rc = mano_setup(a, V, n_betas, n_extra, n_layers, layer_tensors, layer_index, n_groups, group_layer, group_B, group_bcast,
                        need_ws);
    if (rc != MSDA_OK) return rc;
    if (inputs == nullptr || outputs == nullptr) return serr("msda_mano: null pointer");
    for (int i = 0; i < n_groups; ++i) {
        ManoGroup &g = a.g[i];
        g.betas = inputs[4 * i]; g.go = inputs[4 * i + 1]; g.hp = inputs[4 * i + 2]; g.transl = inputs[4 * i + 3];
        g.verts = outputs[2 * i]; g.joints = outputs[2 * i + 1];
        if (g.B > 0 && (g.betas == nullptr || g.go == nullptr || g.hp == nullptr || g.verts == nullptr || g.joints == nullptr))
            return serr("msda_mano: null pointer");
    }
    begin_entry();
    const int tiles = total_tiles(a);
    if (tiles == 0) return MSDA_OK;
    hipLaunchKernelGGL(mano_fwd_kernel, dim3((unsigned)(tiles * a.nslices)), dim3(kBlock), 0, (hipStream_t)stream, a);
    return check_launch("mano_fwd_kernel");
}

int msda_mano_backward_f32(int V, int n_betas, int n_extra, int n_layers, const float *const *layer_tensors, const int *layer_index,
                           int n_groups, const int *group_layer, const int *group_B, const int *group_bcast,
                           const float *const *inputs, const float *const *grad_outputs, float *const *grads, void *workspace,
                           unsigned long long workspace_bytes, msda_stream_t stream)
{
    ManoArgs a;
    unsigned long long need_ws = 0;
    int rc = mano_setup(a, V, n_betas, n_extra, n_layers, layer_tensors, layer_index, n_groups, group_layer, group_B, group_bcast,
                        need_ws);
    if (rc != MSDA_OK) return rc;
    if (inputs == nullptr || grad_outputs == nullptr || grads == nullptr) return serr("msda_mano: null pointer");
    if (workspace == nullptr || workspace_bytes < need_ws)
        return serr("msda_mano: workspace smaller than msda_mano_workspace_bytes");
    a.ws = static_cast<float *>(workspace);
    for (int i = 0; i < n_groups; ++i) {
        ManoGroup &g = a.g[i];
        g.betas = inputs[4 * i]; g.go = inputs[4 * i + 1]; g.hp = inputs[4 * i + 2]; g.transl = inputs[4 * i + 3];
        g.gverts = grad_outputs[2 * i]; g.gjoints = grad_outputs[2 * i + 1];
        g.gbetas = grads[4 * i]; g.ggo = grads[4 * i + 1]; g.ghp = grads[4 * i + 2]; g.gtransl = grads[4 * i + 3];
        if (g.B > 0 && (g.betas == nullptr || g.go == nullptr || g.hp == nullptr || g.gbetas == nullptr || g.ggo == nullptr
                        || g.ghp == nullptr))
            return serr("msda_mano: null pointer");
    }
    begin_entry();
    const int tiles = total_tiles(a);
    if (tiles == 0) return MSDA_OK;
    hipLaunchKernelGGL(mano_bwd_slice_kernel, dim3((unsigned)(tiles * a.nslices)), dim3(kBlock), 0, (hipStream_t)stream, a);
    rc = check_launch("mano_bwd_slice_kernel");
    if (rc != MSDA_OK) return rc;
    hipLaunchKernelGGL(mano_bwd_chain_kernel, dim3((unsigned)tiles), dim3(kBlock), 0, (hipStream_t)stream, a);
    return check_launch("mano_bwd_chain_kernel");
}
