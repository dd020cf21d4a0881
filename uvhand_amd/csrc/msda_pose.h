// Pose arithmetic shared by the ARCTIC kernels (msda_small_loss.hip, msda_arctic_output.hip): quaternions as pytorch3d defines
// them (real part first, never renormalised), axis-angle -> quaternion -> matrix, the pinhole projection, and the backward of
// each.  fp32, one fixed expression per result: the files' bitwise tests hold through every caller.
#pragma once
#include "msda_common.h"

namespace msda {

struct Q { float w, x, y, z; };

__device__ __forceinline__ Q qmul(Q a, Q b)
{
    return {a.w * b.w - a.x * b.x - a.y * b.y - a.z * b.z, a.w * b.x + a.x * b.w + a.y * b.z - a.z * b.y,
            a.w * b.y - a.x * b.z + a.y * b.w + a.z * b.x, a.w * b.z + a.x * b.y - a.y * b.x + a.z * b.w};
}
__device__ __forceinline__ Q qconj(Q a) { return {a.w, -a.x, -a.y, -a.z}; }
__device__ __forceinline__ Q qadd(Q a, Q b) { return {a.w + b.w, a.x + b.x, a.y + b.y, a.z + b.z}; }

__device__ __forceinline__ void qapply(Q q, const float p[3], float o[3])
{
    const Q u = qmul(qmul(q, {0.f, p[0], p[1], p[2]}), qconj(q));
    o[0] = u.x; o[1] = u.y; o[2] = u.z;
}

// out = Im(q P q*), P = (0, p): adds d out / d q to gq and returns d out / d p in gp (g = d loss / d out)
__device__ __forceinline__ void qapply_bwd(Q q, const float p[3], const float g[3], Q &gq, float gp[3])
{
    const Q P = {0.f, p[0], p[1], p[2]};
    const Q T = qmul(q, P);
    const Q gU = {0.f, g[0], g[1], g[2]};
    const Q gT = qmul(gU, q);
    gq = qadd(gq, qadd(qconj(qmul(qconj(T), gU)), qmul(gT, qconj(P))));
    const Q gP = qmul(qconj(q), gT);
    gp[0] = gP.x; gp[1] = gP.y; gp[2] = gP.z;
}

// pytorch3d axis_angle_to_quaternion: sin(theta / 2) / theta, or 1/2 - theta^2 / 48 below 1e-6
__device__ __forceinline__ Q aa2q(float x, float y, float z)
{
    const float th = sqrtf(x * x + y * y + z * z);
    const float half = th * 0.5f;
    const float s = th < 1e-6f ? 0.5f - th * th / 48.f : sinf(half) / th;
    return {cosf(half), x * s, y * s, z * s};
}

__device__ __forceinline__ void aa2q_bwd(float x, float y, float z, Q g, float ga[3])
{
    const float th = sqrtf(x * x + y * y + z * z);
    const float half = th * 0.5f;
    const bool small = th < 1e-6f;
    const float s = small ? 0.5f - th * th / 48.f : sinf(half) / th;
    const float ds = small ? -th / 24.f : (0.5f * cosf(half) * th - sinf(half)) / (th * th);
    const float gth = -0.5f * sinf(half) * g.w + ds * (g.x * x + g.y * y + g.z * z);
    const float k = th > 0.f ? gth / th : 0.f;                 // torch.norm's gradient is 0 at 0
    ga[0] = g.x * s + k * x; ga[1] = g.y * s + k * y; ga[2] = g.z * s + k * z;
}

// pytorch3d quaternion_to_matrix (not assuming a unit quaternion)
__device__ __forceinline__ void q2m(Q q, float M[9])
{
    const float r = q.w, i = q.x, j = q.y, k = q.z;
    const float ts = 2.f / (r * r + i * i + j * j + k * k);
    M[0] = 1 - ts * (j * j + k * k); M[1] = ts * (i * j - k * r); M[2] = ts * (i * k + j * r);
    M[3] = ts * (i * j + k * r); M[4] = 1 - ts * (i * i + k * k); M[5] = ts * (j * k - i * r);
    M[6] = ts * (i * k - j * r); M[7] = ts * (j * k + i * r); M[8] = 1 - ts * (i * i + j * j);
}

__device__ __forceinline__ Q q2m_bwd(Q q, const float G[9])
{
    const float r = q.w, i = q.x, j = q.y, k = q.z;
    const float n = r * r + i * i + j * j + k * k, ts = 2.f / n;
    const float gts = -G[0] * (j * j + k * k) + G[1] * (i * j - k * r) + G[2] * (i * k + j * r) + G[3] * (i * j + k * r)
                      - G[4] * (i * i + k * k) + G[5] * (j * k - i * r) + G[6] * (i * k - j * r) + G[7] * (j * k + i * r)
                      - G[8] * (i * i + j * j);
    const float dn = -2.f * ts / n;             // d ts / d q_m = dn * q_m
    Q g;
    g.w = ts * (-G[1] * k + G[2] * j + G[3] * k - G[5] * i - G[6] * j + G[7] * i) + gts * dn * r;
    g.x = ts * (G[1] * j + G[2] * k + G[3] * j - 2.f * G[4] * i - G[5] * r + G[6] * k + G[7] * r - 2.f * G[8] * i) + gts * dn * i;
    g.y = ts * (-2.f * G[0] * j + G[1] * i + G[2] * r + G[3] * i + G[5] * k - G[6] * r + G[7] * k - 2.f * G[8] * j) + gts * dn * j;
    g.z = ts * (-2.f * G[0] * k - G[1] * r + G[2] * i + G[3] * r - 2.f * G[4] * k + G[5] * j + G[6] * i + G[7] * j) + gts * dn * k;
    return g;
}

// K x, then x / z, y / z, normalised to 2 u / img_res - 1
__device__ __forceinline__ void project(const float *K, const float x[3], float img_res, float n[2], float ph[3])
{
    for (int i = 0; i < 3; ++i) ph[i] = K[3 * i] * x[0] + K[3 * i + 1] * x[1] + K[3 * i + 2] * x[2];
    n[0] = 2.f * (ph[0] / ph[2]) / img_res - 1.f;
    n[1] = 2.f * (ph[1] / ph[2]) / img_res - 1.f;
}

__device__ __forceinline__ void project_bwd(const float *K, const float ph[3], float img_res, const float gn[2], float gx[3])
{
    const float a0 = 2.f * gn[0] / img_res, a1 = 2.f * gn[1] / img_res;
    const float gp[3] = {a0 / ph[2], a1 / ph[2], -(a0 * ph[0] + a1 * ph[1]) / (ph[2] * ph[2])};
    for (int c = 0; c < 3; ++c) gx[c] = K[c] * gp[0] + K[3 + c] * gp[1] + K[6 + c] * gp[2];
}

}  // namespace msda
