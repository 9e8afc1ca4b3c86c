// The 3-point alignment and the stereo-reprojection inlier test of the RANSAC front end (point_cloud_aligner.cpp:12-62 and
// :117-124), shared by libssba.so (ssba_frontend.hip: ssba_frontend_vo, ssba_frontend_ransac) and libssba_tracks.so (the
// streaming odometry of ssba_tracks_odometry.h): one statement of the arithmetic, checked against long double by
// tests/test_gpu_hp_frontend.py.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

namespace ssba {
namespace {

struct Cam { double fu, fv, cu, cv, b; };

__device__ __forceinline__ double dot3d(const double a[3], const double b[3]) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
__device__ __forceinline__ void cross3d(const double a[3], const double b[3], double o[3]) {
    o[0] = a[1] * b[2] - a[2] * b[1]; o[1] = a[2] * b[0] - a[0] * b[2]; o[2] = a[0] * b[1] - a[1] * b[0];
}

// one-sided (Hestenes) Jacobi on a 3x3 W (row-major): plane rotations from the right until the columns of G = W V are
// orthogonal, |g_p . g_q| <= 2^-51 |g_p||g_q| (the rounding of the dot product itself; 4 to 6 sweeps).  The singular values
// are the column norms and V holds the right singular vectors.  Nothing is squared before the rotation angles are formed,
// so the pair (s2, v2) keeps a relative accuracy of u s1 / s2 where an eigen-decomposition of W^T W leaves u (s1 / s2)^2.
__device__ void jacobi_svd3(const double W[9], double G[9], double V[9]) {
    for (int i = 0; i < 9; ++i) { G[i] = W[i]; V[i] = (i % 4 == 0) ? 1.0 : 0.0; }
    for (int sweep = 0; sweep < 12; ++sweep) {
        bool rotated = false;
        for (int p = 0; p < 2; ++p)
            for (int q = p + 1; q < 3; ++q) {
                const double al = G[p] * G[p] + G[3 + p] * G[3 + p] + G[6 + p] * G[6 + p];
                const double be = G[q] * G[q] + G[3 + q] * G[3 + q] + G[6 + q] * G[6 + q];
                const double ga = G[p] * G[q] + G[3 + p] * G[3 + q] + G[6 + p] * G[6 + q];
                if (ga == 0.0 || fabs(ga) <= 0x1p-51 * sqrt(al) * sqrt(be)) continue;
                const double zeta = (be - al) / (2.0 * ga);
                const double t = (zeta >= 0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(zeta * zeta + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                for (int k = 0; k < 3; ++k) {
                    const double gp = G[3 * k + p], gq = G[3 * k + q];
                    G[3 * k + p] = c * gp - s * gq; G[3 * k + q] = s * gp + c * gq;
                    const double vp = V[3 * k + p], vq = V[3 * k + q];
                    V[3 * k + p] = c * vp - s * vq; V[3 * k + q] = s * vp + c * vq;
                }
                rotated = true;
            }
        if (!rotated) break;
    }
}

// PointCloudAligner::compute_transformation (point_cloud_aligner.cpp:12-62) for 3 points: W has rank <= 2, so
// C_1_0 = U diag(1, 1, det U det V) V^T = u1 v1^T + u2 v2^T + (u1 x u2)(v1 x v2)^T.  The two leading singular pairs come
// from a one-sided Jacobi SVD of W itself (the reference's Eigen::JacobiSVD works on W too): u_i = (W v_i) / s_i are the
// two longest columns of W V.  T = [t | R row-major].
__device__ void align3(const double s0[9], const double s1[9], double T[12]) {
    double c0[3], c1[3];
    for (int c = 0; c < 3; ++c) { c0[c] = (s0[c] + s0[3 + c] + s0[6 + c]) / 3.0; c1[c] = (s1[c] + s1[3 + c] + s1[6 + c]) / 3.0; }
    double W[9];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) {
            double v = 0.0;
            for (int i = 0; i < 3; ++i) v += (s1[3 * i + r] - c1[r]) * (s0[3 * i + c] - c0[c]);
            W[3 * r + c] = v / 3.0;
        }
    double G[9], V[9], sv[3];
    jacobi_svd3(W, G, V);
    for (int c = 0; c < 3; ++c) sv[c] = sqrt(G[c] * G[c] + G[3 + c] * G[3 + c] + G[6 + c] * G[6 + c]);
    int i1 = 0;                                   // the two largest singular values, the first of equals
    if (sv[1] > sv[i1]) i1 = 1;
    if (sv[2] > sv[i1]) i1 = 2;
    int i2 = i1 == 0 ? 1 : 0;
    for (int c = i2 + 1; c < 3; ++c) if (c != i1 && sv[c] > sv[i2]) i2 = c;
    const double n1 = sv[i1], n2 = sv[i2];
    double v1[3] = {V[i1], V[3 + i1], V[6 + i1]}, v2[3] = {V[i2], V[3 + i2], V[6 + i2]};
    double u1[3] = {G[i1], G[3 + i1], G[6 + i1]}, u2[3] = {G[i2], G[3 + i2], G[6 + i2]};
    double v3[3], u3[3];
    // the accumulated rotations leave V orthonormal to a few u per rotation: bring v1, v2 back to one rounding
    const double nv1 = sqrt(dot3d(v1, v1));
    for (int r = 0; r < 3; ++r) v1[r] /= nv1;
    const double dv = dot3d(v1, v2);
    for (int r = 0; r < 3; ++r) v2[r] -= dv * v1[r];
    const double nv2 = sqrt(dot3d(v2, v2));
    for (int r = 0; r < 3; ++r) v2[r] /= nv2;
    // A degenerate sample (collinear or coincident points: rank W < 2) has s_i = 0; an SVD still returns orthonormal U
    // columns there -- complete the basis instead of dividing by zero (point_cloud_aligner.cpp:49-55 uses JacobiSVD,
    // which does the same up to the choice of the null-space basis).  s2 <= 2^-50 s1 is below the rounding of W's own
    // entries: such a column holds no direction.
    if (n1 > 0.0) { for (int r = 0; r < 3; ++r) u1[r] /= n1; }
    else { u1[0] = 1.0; u1[1] = 0.0; u1[2] = 0.0; }
    bool have_u2 = n2 > 0x1p-50 * n1;
    if (have_u2) {
        for (int r = 0; r < 3; ++r) u2[r] /= n2;
        const double d12 = dot3d(u1, u2);             // orthogonal to the rotations' stopping bound already
        for (int r = 0; r < 3; ++r) u2[r] -= d12 * u1[r];
        const double m2 = sqrt(dot3d(u2, u2));
        have_u2 = m2 > 0.5;
        if (have_u2) for (int r = 0; r < 3; ++r) u2[r] /= m2;
    }
    if (!have_u2) {      // any unit vector orthogonal to u1
        const int m = fabs(u1[0]) <= fabs(u1[1]) ? (fabs(u1[0]) <= fabs(u1[2]) ? 0 : 2) : (fabs(u1[1]) <= fabs(u1[2]) ? 1 : 2);
        double e[3] = {0.0, 0.0, 0.0};
        e[m] = 1.0;
        const double de = dot3d(u1, e);
        for (int r = 0; r < 3; ++r) u2[r] = e[r] - de * u1[r];
        const double ne = sqrt(dot3d(u2, u2));
        for (int r = 0; r < 3; ++r) u2[r] /= ne;
    }
    cross3d(v1, v2, v3);
    cross3d(u1, u2, u3);
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) T[3 + 3 * r + c] = u1[r] * v1[c] + u2[r] * v2[c] + u3[r] * v3[c];
    for (int r = 0; r < 3; ++r) T[r] = c1[r] - (T[3 + 3 * r] * c0[0] + T[4 + 3 * r] * c0[1] + T[5 + 3 * r] * c0[2]);
}

// (camera->project(pts_1[i]) - camera->project(T_1_0 * pts_0[i])).squaredNorm() < thresh   (:117-124)
__device__ __forceinline__ bool is_inlier(const Cam &cam, const double T[12], const double *p0, const double *p1, double thresh) {
    const double q0 = T[3] * p0[0] + T[4] * p0[1] + T[5] * p0[2] + T[0];
    const double q1 = T[6] * p0[0] + T[7] * p0[1] + T[8] * p0[2] + T[1];
    const double q2 = T[9] * p0[0] + T[10] * p0[1] + T[11] * p0[2] + T[2];
    const double du = (cam.fu * p1[0] / p1[2] + cam.cu) - (cam.fu * q0 / q2 + cam.cu);
    const double dv = (cam.fv * p1[1] / p1[2] + cam.cv) - (cam.fv * q1 / q2 + cam.cv);
    const double dd = cam.fu * cam.b / p1[2] - cam.fu * cam.b / q2;
    return du * du + dv * dv + dd * dd < thresh;
}

}  // namespace
}  // namespace ssba
