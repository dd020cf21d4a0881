// The per-frame algebra of msda_pre_fit_f32 (msda_pre_process.hip), in fp64 and callable on the host as well: the rigid fit of
// arctic_tools/common/transforms.py batch_solve_rigid_tf (Arun's method) and the camera translation of
// common/camera.py estimate_translation_k_np with unit weights.  Every loop has a bounded trip count and a fixed order.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

namespace msda {

constexpr int kFitDetNegative = 1, kFitNotUnique = 2, kFitNonFinite = 4, kFitSingular = 8;
constexpr int kFitSweeps = 12;               // at most; one-sided Jacobi on a 3 x 3 matrix converges in 4 to 6 sweeps in fp64
constexpr double kFitOrthogonal = 4e-16;     // |a_p . a_q| below this share of |a_p| |a_q|: no rotation (a sweep without one ends the loop)
constexpr double kFitRankTol = 1e-12;        // s2 / s0 below this: H has no orientation, so no reflection is reported
constexpr double kFitUniqueTol = 1e-6;       // s1 / s0 below this: the rotation is not unique
constexpr double kFitSingularTol = 1e-12;    // |det A| against the product of A's diagonal

__host__ __device__ inline void fit_cross(const double *a, const double *b, double *o)
{
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
}

__host__ __device__ inline double fit_dot(const double *a, const double *b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

// R (row-major 3 x 3) = V diag(1, 1, det(V U^T)) U^T of H = U S V^T, i.e. the proper rotation that maximises tr(R H).  H's
// columns are orthogonalised by right rotations (H V = U S, Hestenes); the third left vector is u0 x u1 and the third right
// vector v0 x v1, which is Arun's negated column whenever U S V^T has a negative determinant.  Returns the status bits.
__host__ __device__ inline int fit_rotation(const double (&H)[3][3], double *R)
{
    double A[3][3], V[3][3];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) { A[i][j] = H[i][j]; V[i][j] = i == j ? 1.0 : 0.0; }
    for (int sweep = 0; sweep < kFitSweeps; ++sweep) {
        bool rotated = false;
        for (int pq = 0; pq < 3; ++pq) {
            const int p = pq == 2 ? 1 : 0, q = pq == 0 ? 1 : 2;
            double alpha = 0.0, beta = 0.0, gamma = 0.0;
            for (int i = 0; i < 3; ++i) { alpha += A[i][p] * A[i][p]; beta += A[i][q] * A[i][q]; gamma += A[i][p] * A[i][q]; }
            if (!(fabs(gamma) > kFitOrthogonal * sqrt(alpha * beta))) continue;      // the pair is orthogonal to fp64's last bit
            rotated = true;
            const double zeta = (beta - alpha) / (2.0 * gamma);
            const double t = copysign(1.0, zeta) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
            const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
            for (int i = 0; i < 3; ++i) {
                const double x = A[i][p], y = A[i][q];
                A[i][p] = c * x - s * y; A[i][q] = s * x + c * y;
                const double vx = V[i][p], vy = V[i][q];
                V[i][p] = c * vx - s * vy; V[i][q] = s * vx + c * vy;
            }
        }
        if (!rotated) break;
    }
    double n[3];
    int ord[3] = {0, 1, 2};
    for (int j = 0; j < 3; ++j) n[j] = sqrt(A[0][j] * A[0][j] + A[1][j] * A[1][j] + A[2][j] * A[2][j]);
    for (int pass = 0; pass < 2; ++pass)                       // descending, stable
        for (int j = 0; j + 1 < 3 - pass; ++j)
            if (n[ord[j + 1]] > n[ord[j]]) { const int tmp = ord[j]; ord[j] = ord[j + 1]; ord[j + 1] = tmp; }
    double v[3][3], a0[3], a1[3], a2[3], u[3][3];
    for (int i = 0; i < 3; ++i) { v[0][i] = V[i][ord[0]]; v[1][i] = V[i][ord[1]]; a0[i] = A[i][ord[0]]; a1[i] = A[i][ord[1]]; }
    fit_cross(v[0], v[1], v[2]);
    for (int i = 0; i < 3; ++i) a2[i] = H[i][0] * v[2][0] + H[i][1] * v[2][1] + H[i][2] * v[2][2];
    const double s0 = n[ord[0]], s1 = n[ord[1]], s2 = sqrt(fit_dot(a2, a2));
    for (int i = 0; i < 3; ++i) u[0][i] = s0 > 0.0 ? a0[i] / s0 : (i == 0 ? 1.0 : 0.0);
    {
        const double along = fit_dot(u[0], a1);
        double w[3] = {a1[0] - along * u[0][0], a1[1] - along * u[0][1], a1[2] - along * u[0][2]};
        double nw = sqrt(fit_dot(w, w));
        if (!(nw > 0.0)) {                                      // no second direction at all: any unit vector orthogonal to u0
            const int e = fabs(u[0][0]) <= fabs(u[0][1]) ? (fabs(u[0][0]) <= fabs(u[0][2]) ? 0 : 2)
                                                          : (fabs(u[0][1]) <= fabs(u[0][2]) ? 1 : 2);
            for (int i = 0; i < 3; ++i) w[i] = (i == e ? 1.0 : 0.0) - u[0][e] * u[0][i];
            nw = sqrt(fit_dot(w, w));
        }
        for (int i = 0; i < 3; ++i) u[1][i] = w[i] / nw;
    }
    fit_cross(u[0], u[1], u[2]);
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) R[3 * i + j] = v[0][i] * u[0][j] + v[1][i] * u[1][j] + v[2][i] * u[2][j];
    int status = 0;
    if (fit_dot(u[2], a2) < 0.0 && s2 > kFitRankTol * s0) status |= kFitDetNegative;
    if (!(s1 >= kFitUniqueTol * s0) || !(s0 > 0.0)) status |= kFitNotUnique;
    return status;
}

// kp_full, kp_cano [NK, 3], kp2d_norm [NK, 2], K [3, 3] of one frame (finite values).  R [9], T0 [3], t [3]; t is NaN with
// kFitSingular.  Returns the status bits.
__host__ __device__ inline int fit_frame(const float *kp_full, const float *kp_cano, const float *kp2d_norm, const float *K, int NK,
                                         double img_res, double *R, double *T0, double *t)
{
    double cA[3] = {0.0, 0.0, 0.0}, cB[3] = {0.0, 0.0, 0.0};
    for (int k = 0; k < NK; ++k)
        for (int c = 0; c < 3; ++c) { cA[c] += (double)kp_full[3 * k + c]; cB[c] += (double)kp_cano[3 * k + c]; }
    for (int c = 0; c < 3; ++c) { cA[c] /= (double)NK; cB[c] /= (double)NK; }
    double H[3][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
    for (int k = 0; k < NK; ++k) {
        double a[3], b[3];
        for (int c = 0; c < 3; ++c) { a[c] = (double)kp_full[3 * k + c] - cA[c]; b[c] = (double)kp_cano[3 * k + c] - cB[c]; }
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) H[i][j] += a[i] * b[j];
    }
    int status = fit_rotation(H, R);
    for (int i = 0; i < 3; ++i) T0[i] = cB[i] - (R[3 * i] * cA[0] + R[3 * i + 1] * cA[1] + R[3 * i + 2] * cA[2]);

    // normal equations of Q t = c, rows (fx, 0, cx - u) and (0, fy, cy - v) per keypoint; A01 = 0
    const double fx = (double)K[0], fy = (double)K[4], cx = (double)K[2], cy = (double)K[5];
    double A02 = 0.0, A12 = 0.0, A22 = 0.0, b0 = 0.0, b1 = 0.0, b2 = 0.0;
    for (int k = 0; k < NK; ++k) {
        const double px = 0.5 * img_res * ((double)kp2d_norm[2 * k] + 1.0), py = 0.5 * img_res * ((double)kp2d_norm[2 * k + 1] + 1.0);
        const double X = (double)kp_cano[3 * k], Y = (double)kp_cano[3 * k + 1], Z = (double)kp_cano[3 * k + 2];
        const double qx = cx - px, qy = cy - py;
        const double ex = (px - cx) * Z - fx * X, ey = (py - cy) * Z - fy * Y;
        A02 += fx * qx; A12 += fy * qy; A22 += qx * qx + qy * qy;
        b0 += fx * ex; b1 += fy * ey; b2 += qx * ex + qy * ey;
    }
    const double A00 = (double)NK * fx * fx, A11 = (double)NK * fy * fy;
    const double det = A00 * A11 * A22 - A00 * A12 * A12 - A02 * A02 * A11;
    if (!(fabs(det) > kFitSingularTol * (A00 * A11 * A22))) {
        status |= kFitSingular;
        t[0] = t[1] = t[2] = NAN;
        return status;
    }
    t[2] = (b2 - A02 * b0 / A00 - A12 * b1 / A11) / (A22 - A02 * A02 / A00 - A12 * A12 / A11);
    t[0] = (b0 - A02 * t[2]) / A00;
    t[1] = (b1 - A12 * t[2]) / A11;
    return status;
}

}  // namespace msda
