// Dense photometric alignment: the reference's ImageError blocks (include/ceres_slam/image_error.hpp, driven by
// tests/dense_stereo_test.cpp:94-136) on the device.  One SE(3) pose T_track_ref and one 1-D disparity block per reference pixel
// with a usable disparity; no stiffness; the loss is NULL (cost = 1/2 sum r^2) or Ceres' HuberLoss of width a = Dev::huber_a > 0
// (ssba_set_huber_loss), cost = 1/2 sum rho(r^2), applied by Ceres' corrector with rho'' <= 0 as on the stereo rows
// (ssba_device.h: obs_linearize_S):
//     r^2 > a^2:  sc = sqrt(max(DBL_MIN, a / |r|)),  r~ = sc r,  J~ = sc J,  1/2 rho = 1/2 (2 a |r| - a^2);   else unchanged.
// The row buffer, every sum, the Jacobi scales, the damping, V and dd are formed from the corrected row (LOSS = true below); the
// candidate cost is 1/2 rho of the raw candidate residual.  Out-of-bounds rows have r = 0 and are never corrected.  The kernels
// without a loss (LOSS = false) keep every expression they had.
//
// A block at reference pixel (u_r, v_r) with disparity d and pose [t | R] (all fp64):
//     p = triangulate(u_r, v_r, d)                      stereo_camera.hpp:112-144
//     q = R p + t,   (u, v) = project(q)[0:2]           stereo_camera.hpp:77-108
//     in bounds:  0 <= u, 0 <= v and every pixel the sample reads lies inside the image
//                 NEAREST   I[floor(v + 1/2)][floor(u + 1/2)]       u < cols - 1/2, v < rows - 1/2
//                 BILINEAR  the four neighbours of (floor u, floor v)  u < cols - 1,  v < rows - 1
//     r      = track(u, v) - ref[v_r][u_r],   g = [gradx(u, v), grady(u, v)]
//     J_pose = g P(q) [I | -q^]      (1 x 6, local coordinates of SE3Perturbation: exp(eps) T, translation first)
//     J_disp = g P(q) R dp/dd        (dp/dd: the third column of the triangulation Jacobian)
//     out of bounds: r = 0, both Jacobians 0 (image_error.hpp:102-128)
// P(q) = the first two rows of the projection Jacobian.  (The reference tests u < cols, v < rows only and so reads past the end of
// a row in the last half pixel; and it takes tri_jac.block(2, 0, 3, 1), which lies outside the 3 x 3 matrix, where the third
// column is meant: include/ssba.h.)
//
// Levenberg-Marquardt with the rules of every other layout (k_check / k_decide unchanged).  The free disparities are part of x:
// Jacobi scale 1 / (1 + |J_d|) at iteration 0, damping D_d = clamp(J_d^2 s^2, min, max) / (radius s^2), and they are eliminated
// per block:  V = J_d^2 + D_d,
//     S   = H_pp + D_p - sum (J_p^T J_d)(J_d J_p) / V  =  D_p + sum J_p^T J_p (D_d / V)
//     rhs = -(g_p - sum J_p^T J_d J_d r / V)           = -sum J_p^T r (D_d / V)
//     dd  = -(J_d r + J_d J_p dp) / V,    model cost change = -sum (J delta)(r + 1/2 J delta)  from the rows.
// Constant disparities: D_d / V -> 1, dd = 0.
//
// An iteration is five launches: k_im_lin (one lane per block: row, local elimination, partial sums per work-group; commits the
// step the last iteration accepted on the way) . k_im_solve (one work-group: sums in fixed order, scale, damp, po_solve6,
// candidate pose) . k_im_eval (dd, candidate disparity and cost, model cost change; its first work-group does k_check's work) .
// k_decide . k_best.  No atomics, every sum in fixed order.
#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>
#include <stdint.h>

#include "ssba_types.h"
#include "ssba_launch.h"
#include "ssba_device.h"
#include "ssba_check.h"
#include "ssba_solve6.h"

namespace ssba {

constexpr int IM_SOLVE_THREADS = 512, IM_SLICES = IM_SOLVE_THREADS / 64;
constexpr int IM_SYS_RHS = 36, IM_SYS_DP = 42, IM_SYS_SP = 48;

static __device__ __forceinline__ bool im_in_bounds(const ImageSys &im, double u, double v) {      // false for NaN
    const double mu = im.interp ? 1.0 : 0.5;
    return u >= 0.0 && v >= 0.0 && u < (double)im.cols - mu && v < (double)im.rows - mu;
}
// (u, v) in bounds
static __device__ __forceinline__ double im_sample(const ImageSys &im, const double *__restrict__ img, double u, double v) {
    if (im.interp == 0) {
        const int x = min((int)floor(u + 0.5), im.cols - 1), y = min((int)floor(v + 0.5), im.rows - 1);
        return img[(size_t)y * im.cols + x];
    }
    const double fx = floor(u), fy = floor(v);
    const double a = u - fx, b = v - fy;
    const double *p = img + (size_t)min((int)fy, im.rows - 2) * im.cols + min((int)fx, im.cols - 2);
    return (1.0 - b) * ((1.0 - a) * p[0] + a * p[1]) + b * ((1.0 - a) * p[im.cols] + a * p[im.cols + 1]);
}

// triangulate, transform, project: p (camera frame of the reference image), q = R p + t, (u, v)
template <bool LIN> static __device__ __forceinline__ void im_project(const Dev &d, const double *__restrict__ T, double ur, double vr, double dd, double q[3],
                                                  double &iz, double &u, double &v) {
    const double bd = d.b / dd, ff = d.fu / d.fv;
    const double px = (ur - d.cu) * bd, py = (vr - d.cv) * bd * ff, pz = d.fu * bd;
    // Which product of a sum of two the compiler fuses into an fma is its own choice, and it falls differently in different
    // kernels around the same source line; the solo and the batched kernels must agree to the bit, so the rows say it themselves
    // (the forms k_im_lin and k_im_eval had before the bodies were shared, read off their assembly: they differ in row 0).
    q[0] = (LIN ? fma(T[5], pz, fma(T[4], py, T[3] * px)) : fma(T[5], pz, fma(T[3], px, T[4] * py))) + T[0];
    q[1] = fma(T[8], pz, fma(T[6], px, T[7] * py)) + T[1];
    q[2] = fma(T[11], pz, fma(T[9], px, T[10] * py)) + T[2];
    iz = 1.0 / q[2];
    u = d.fu * q[0] * iz + d.cu;
    v = d.fv * q[1] * iz + d.cv;
}

// the residual alone (candidate evaluation)
static __device__ __forceinline__ double im_residual(const Dev &d, const ImageSys &im, const double *__restrict__ T, uint32_t pix, double dd) {
    const uint32_t vr = pix / (uint32_t)im.cols, ur = pix - vr * (uint32_t)im.cols;
    double q[3], iz, u, v;
    im_project<false>(d, T, (double)ur, (double)vr, dd, q, iz, u, v);
    if (!im_in_bounds(im, u, v)) return 0.0;
    return im_sample(im, im.track, u, v) - im.ref[pix];
}

// the row of a block: residual, J_pose (6), J_disp
static __device__ __forceinline__ void im_row(const Dev &d, const ImageSys &im, const double *__restrict__ T, uint32_t pix, double dd,
                                              double &r, double jp[6], double &jd) {
    const uint32_t vr = pix / (uint32_t)im.cols, ur = pix - vr * (uint32_t)im.cols;
    double q[3], iz, u, v;
    im_project<true>(d, T, (double)ur, (double)vr, dd, q, iz, u, v);
    r = 0.0; jd = 0.0;
#pragma unroll
    for (int c = 0; c < 6; ++c) jp[c] = 0.0;
    if (!im_in_bounds(im, u, v)) return;
    r = im_sample(im, im.track, u, v) - im.ref[pix];
    const double gx = im_sample(im, im.gradx, u, v), gy = im_sample(im, im.grady, u, v);
    const double iz2 = iz * iz;
    const double a0 = gx * (d.fu * iz), a1 = gy * (d.fv * iz);
    const double a2 = gx * (-d.fu * q[0] * iz2) + gy * (-d.fv * q[1] * iz2);
    jp[0] = a0; jp[1] = a1; jp[2] = a2;       // g P [I | -q^]  (jac_pose)
    jp[3] = -a1 * q[2] + a2 * q[1];
    jp[4] = a0 * q[2] - a2 * q[0];
    jp[5] = -a0 * q[1] + a1 * q[0];
    // dp/dd = third column of the triangulation Jacobian (stereo_camera.hpp:125-140)
    const double bd2 = d.b / dd / dd, ff = d.fu / d.fv;
    const double t0 = (d.cu - (double)ur) * bd2, t1 = (d.cv - (double)vr) * bd2 * ff, t2 = -d.fu * bd2;
    const double w0 = fma(T[5], t2, fma(T[4], t1, T[3] * t0)), w1 = fma(T[8], t2, fma(T[6], t0, T[7] * t1));      // (as im_project's rows)
    const double w2 = fma(T[11], t2, fma(T[9], t0, T[10] * t1));
    jd = a0 * w0 + a1 * w1 + a2 * w2;
}

// Huber: 1/2 rho(r^2) of a raw residual (the fma is written out: the solo and the batched kernels must round alike)
static __device__ __forceinline__ double im_half_rho(double a, double r) {
    const double sq = r * r;
    return sq > a * a ? 0.5 * fma(2.0 * a, fabs(r), -(a * a)) : 0.5 * sq;
}

// damping of a free disparity in unscaled coordinates (landmark_damping's rule for a 1 x 1 block)
static __device__ __forceinline__ double im_damping(const State &st, double jd, double s) {
    const double s2 = s * s;
    return fmin(fmax(jd * jd * s2, st.opt.min_lm_diag), st.opt.max_lm_diag) / (damp_radius(st) * s2);
}

// One lane per block.  The iterate is read from the candidate buffers when the last decision accepted its step, and committed
// on the way (as k_po_step does).  The linearisation is repeated after a rejected step: same point, same sums, another radius.
// Per work-group: IM_NSUM sums into ImageSys::part, and (cost, |d|^2 of the free disparities, max |J_d r|) into Dev::part_lin,
// which check_body reduces.
// The three bodies below take the problem's Dev and the index of the work-group inside the problem: k_im_* hand them the
// kernel argument and blockIdx.x, the batched kernels k_imb_* an entry of their device array and blockIdx.x under that problem's
// count.  Nothing is written through `d` itself (only through the pointers it holds), so a batched work-group reads it in place.
template <bool FREE, bool LOSS> static __device__ __forceinline__ void im_lin_body(const Dev &d, const uint32_t wg) {
    const State &st = *d.st;
    const ImageSys &im = *d.image;
    if (st.terminated) return;
    constexpr int NS = FREE ? IM_NSUM : 27;
    const bool commit = st.accepted != 0;
    const double *PS = commit ? d.cand_poses : d.poses;
    double T[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) T[i] = PS[i];
    const uint32_t i = wg * IM_THREADS + threadIdx.x;
    double acc[NS + 2];      // .. | cost | |d|^2
#pragma unroll
    for (int q = 0; q < NS + 2; ++q) acc[q] = 0.0;
    double gm = 0.0;
    if (i < im.n_blk) {
        const uint32_t pix = im.blk_pix[i];
        const double dd = (FREE && commit ? d.cand_pts : d.pts)[pix];
        if (FREE && commit) d.pts[pix] = dd;
        double r, jp[6], jd;
        im_row(d, im, T, pix, dd, r, jp, jd);
        double half_rho = 0.0;
        if (LOSS) {      // the corrector: everything below reads the corrected row
            const double a = d.huber_a;
            half_rho = im_half_rho(a, r);
            if (r * r > a * a) {
                const double sc = sqrt(fmax(DBL_MIN, a / fabs(r)));
                r *= sc; jd *= sc;
#pragma unroll
                for (int c = 0; c < 6; ++c) jp[c] *= sc;
            }
        }
#pragma unroll
        for (int c = 0; c < 6; ++c) im.row[(size_t)c * im.n_blk + i] = jp[c];
        im.row[(size_t)6 * im.n_blk + i] = jd;
        im.row[(size_t)7 * im.n_blk + i] = r;
        double w = 1.0;      // D_d / V: what the elimination of the disparity leaves of this row
        if (FREE) {
            double s;
            if (st.iteration == 0) { s = st.opt.jacobi_scaling ? 1.0 / (1.0 + fabs(jd)) : 1.0; im.sd[i] = s; }
            else s = im.sd[i];
            const double dmp = im_damping(st, jd, s), V = jd * jd + dmp;
            if (V > 0.0) w = dmp / V;
            else d.st->step_failed = 1;      // LINEAR_SOLVER_FAILURE (min_lm_diagonal = 0 on a row without gradient)
            acc[NS + 1] = dd * dd;
            gm = fabs(jd * r);
        }
        int n = 0;
#pragma unroll
        for (int a = 0; a < 6; ++a)
#pragma unroll
            for (int c = a; c < 6; ++c) acc[n++] = jp[a] * jp[c] * w;
#pragma unroll
        for (int a = 0; a < 6; ++a) acc[21 + a] = jp[a] * r * w;
        if (FREE) {
#pragma unroll
            for (int a = 0; a < 6; ++a) { acc[27 + a] = jp[a] * jp[a]; acc[33 + a] = jp[a] * r; }
        }
        acc[NS] = LOSS ? half_rho : 0.5 * r * r;
    }
    if (commit && wg == 0 && threadIdx.x < 12) d.poses[threadIdx.x] = T[threadIdx.x];
    __shared__ double sm[IM_THREADS / 64][NS + 3];
    const int w = threadIdx.x >> 6;
#pragma unroll
    for (int q = 0; q < NS + 2; ++q) {
        const double v = wave_sum(acc[q]);
        if ((threadIdx.x & 63) == 0) sm[w][q] = v;
    }
    gm = wave_max(gm);
    if ((threadIdx.x & 63) == 0) sm[w][NS + 2] = gm;
    __syncthreads();
    if (threadIdx.x >= NS + 3) return;
    double v = 0.0;
    if (threadIdx.x == NS + 2) {
#pragma unroll
        for (int q = 0; q < IM_THREADS / 64; ++q) v = fmax(v, sm[q][threadIdx.x]);
    } else {
#pragma unroll
        for (int q = 0; q < IM_THREADS / 64; ++q) v += sm[q][threadIdx.x];
    }
    if (threadIdx.x < NS) im.part[(size_t)wg * IM_REC + threadIdx.x] = v;
    else d.part_lin[(size_t)wg * 4 + (threadIdx.x - NS)] = v;
}
template <bool FREE, bool LOSS> __global__ __launch_bounds__(IM_THREADS) void k_im_lin(Dev d) { im_lin_body<FREE, LOSS>(d, blockIdx.x); }

// One work-group: the sums of k_im_lin's partials in fixed order (lane = column of the record, 8 slices of work-groups, the
// slices added in order), then lane 0 scales, damps, solves and forms the candidate pose, and leaves the pose shares that
// check_body (gradient max norm, |x|^2) and k_decide (|dx|^2, non-finite) read.
// k_im_solve's body as text and not as a function, so that k_im_solve keeps the very code it had: as a __forceinline__ function
// called from a wrapper kernel its sums of two products (se3_plus, po_solve6: shared headers that cannot say fma themselves
// without changing the stereo kernels) were contracted differently in a rarely taken path, and a solo solve lost its recorded
// bits at iteration 32 of one case.  `d` is the problem's Dev in scope.
#define IM_SOLVE_BODY \
    State &st = *d.st; \
    const ImageSys &im = *d.image; \
    if (st.terminated) return; \
    __shared__ double sm[IM_SLICES][64]; \
    __shared__ double tot[IM_NSUM]; \
    const int col = threadIdx.x & 63, slice = threadIdx.x >> 6; \
    const int ns = im.disp_const ? 27 : IM_NSUM; \
    double v = 0.0; \
    if (col < ns) { \
        const double *__restrict__ P = im.part + col; \
        int wg = slice; \
        for (; wg + 3 * IM_SLICES < im.n_wg; wg += 4 * IM_SLICES) { \
            const double x0 = P[(size_t)wg * IM_REC], x1 = P[(size_t)(wg + IM_SLICES) * IM_REC]; \
            const double x2 = P[(size_t)(wg + 2 * IM_SLICES) * IM_REC], x3 = P[(size_t)(wg + 3 * IM_SLICES) * IM_REC]; \
            v += x0; v += x1; v += x2; v += x3; \
        } \
        for (; wg < im.n_wg; wg += IM_SLICES) v += P[(size_t)wg * IM_REC]; \
    } \
    sm[slice][col] = v; \
    __syncthreads(); \
    if (threadIdx.x < IM_NSUM) { \
        double t = 0.0; \
        if ((int)threadIdx.x < ns) { \
_Pragma("unroll") \
            for (int q = 0; q < IM_SLICES; ++q) t += sm[q][threadIdx.x]; \
        } \
        tot[threadIdx.x] = t; \
    } \
    __syncthreads(); \
    if (threadIdx.x != 0) return; \
    double T[12], H[21], A[21], g[6], gf[6], hd[6]; \
_Pragma("unroll") \
    for (int i = 0; i < 12; ++i) T[i] = d.poses[i]; \
_Pragma("unroll") \
    for (int i = 0; i < 21; ++i) { H[i] = tot[i]; A[i] = tot[i]; d.hpp[i] = tot[i]; } \
_Pragma("unroll") \
    for (int c = 0; c < 6; ++c) { \
        g[c] = tot[21 + c]; \
        hd[c] = im.disp_const ? H[tri21(c, c)] : tot[27 + c]; \
        gf[c] = im.disp_const ? g[c] : tot[33 + c]; \
        d.gp[c] = gf[c]; \
    } \
_Pragma("unroll") \
    for (int c = 0; c < 6; ++c) { \
        double sc; \
        if (st.iteration == 0) { sc = st.opt.jacobi_scaling ? 1.0 / (1.0 + sqrt(hd[c])) : 1.0; d.sp[c] = sc; } \
        else sc = d.sp[c]; \
        const double s2 = sc * sc; \
        A[tri21(c, c)] += fmin(fmax(hd[c] * s2, st.opt.min_lm_diag), st.opt.max_lm_diag) / (damp_radius(st) * s2); \
        im.sys[IM_SYS_SP + c] = sc; \
    } \
    double dx[6] = {0, 0, 0, 0, 0, 0}, Tn[12], dn = 0.0, nonfinite = 0.0; \
    if (po_solve6(A, g, dx)) { \
_Pragma("unroll") \
        for (int c = 0; c < 6; ++c) if (!isfinite(dx[c])) nonfinite = 1.0; \
        se3_plus(T, dx, Tn); \
_Pragma("unroll") \
        for (int c = 0; c < 12; ++c) { const double df = Tn[c] - T[c]; dn += df * df; } \
    } else { \
        st.step_failed = 1; \
_Pragma("unroll") \
        for (int c = 0; c < 6; ++c) dx[c] = 0.0; \
_Pragma("unroll") \
        for (int c = 0; c < 12; ++c) Tn[c] = T[c]; \
    } \
_Pragma("unroll") \
    for (int c = 0; c < 12; ++c) d.cand_poses[c] = Tn[c]; \
_Pragma("unroll") \
    for (int r = 0; r < 6; ++r) { \
_Pragma("unroll") \
        for (int c = 0; c < 6; ++c) im.sys[6 * r + c] = A[tri21(r < c ? r : c, r < c ? c : r)]; \
        im.sys[IM_SYS_RHS + r] = -g[r]; \
        im.sys[IM_SYS_DP + r] = dx[r]; \
    } \
    d.part_pose[0] = dn; d.part_pose[1] = nonfinite; d.part_pose[2] = 0.0; d.part_pose[3] = 0.0; \
    double ng[6], Tg[12], gm = 0.0, xn = 0.0; \
_Pragma("unroll") \
    for (int c = 0; c < 6; ++c) ng[c] = -gf[c]; \
    se3_plus(T, ng, Tg); \
_Pragma("unroll") \
    for (int c = 0; c < 12; ++c) { gm = fmax(gm, fabs(T[c] - Tg[c])); xn += T[c] * T[c]; } \
    d.part_chk[0] = gm; \
    d.part_chk[1] = xn;
__global__ __launch_bounds__(IM_SOLVE_THREADS) void k_im_solve(Dev d) {
    IM_SOLVE_BODY
}

// Work-group 0 does k_check's work (check_body reads what k_im_lin and k_im_solve left; nothing it writes is read here beyond
// the termination flag, where a stale 0 costs one wasted pass).  The other work-groups rely on the words of the state that
// check_body leaves alone: st.radius, st.mu and st.opt (im_damping), which only k_decide and k_reset_state write.  They must
// not read st.iteration, st.accepted or st.last_successful, which check_body changes in this launch.  The others, one lane per block: the disparity step, the
// candidate disparity, the candidate cost, the row's share of the model cost change; part_eval[w] = (cost, model cost change,
// |dd|^2, non-finite) of work-group w: the shape k_decide reduces.
template <bool FREE, bool LOSS> static __device__ __forceinline__ void im_eval_body(const Dev &d, const uint32_t wg, double *__restrict__ delta_disp) {
    const ImageSys &im = *d.image;
    const State &st = *d.st;
    if (st.terminated) return;
    const uint32_t i = wg * IM_THREADS + threadIdx.x;
    double Tc[12], dp[6];
#pragma unroll
    for (int c = 0; c < 12; ++c) Tc[c] = d.cand_poses[c];
#pragma unroll
    for (int c = 0; c < 6; ++c) dp[c] = im.sys[IM_SYS_DP + c];
    double red[4] = {0.0, 0.0, 0.0, 0.0};      // cost, model cost change, |dd|^2, non-finite
    if (i < im.n_blk) {
        const uint32_t pix = im.blk_pix[i];
        double jdp = 0.0;
#pragma unroll
        for (int c = 0; c < 6; ++c) jdp += im.row[(size_t)c * im.n_blk + i] * dp[c];
        const double jd = im.row[(size_t)6 * im.n_blk + i], r = im.row[(size_t)7 * im.n_blk + i];
        const double dd = d.pts[pix];
        double ddl = 0.0, dc = dd, jdelta = jdp;
        if (FREE) {
            const double V = jd * jd + im_damping(st, jd, im.sd[i]);
            if (V > 0.0) ddl = -(jd * r + jd * jdp) / V;
            dc = dd + ddl;
            d.cand_pts[pix] = dc;
            jdelta += jd * ddl;
            red[2] = ddl * ddl;
            if (!isfinite(dc)) red[3] = 1.0;
        }
        red[1] = -jdelta * (r + 0.5 * jdelta);
        const double rc = im_residual(d, im, Tc, pix, dc);
        red[0] = LOSS ? im_half_rho(d.huber_a, rc) : 0.5 * rc * rc;
        if (delta_disp) delta_disp[i] = ddl;
    }
    __shared__ double sm[4 * IM_THREADS / 64];
    block_sums(red, sm);
    if (threadIdx.x == 0) reinterpret_cast<double4 *>(d.part_eval)[wg] = make_double4(red[0], red[1], red[2], red[3]);
}
template <bool FREE, bool LOSS> __global__ __launch_bounds__(IM_THREADS) void k_im_eval(Dev d, double *__restrict__ delta_disp) {
    if (blockIdx.x == 0) { check_body(d, d.image->n_wg, false); return; }
    im_eval_body<FREE, LOSS>(d, blockIdx.x - 1, delta_disp);
}

// ------------------------------------------------------------------- batch ---
// n image handles in shared launches (ssba_image_solve_batch): blockIdx.y is the problem, gridDim.x the largest work-group
// count of the batch, and a work-group past its own problem's count returns at once.  The Dev of a work-group is an entry of a
// device array; its index is uniform over the work-group, so its fields arrive by scalar loads and no lane holds a copy.  Free or
// constant disparities and the loss (the template arguments of the solo kernels) are branches on ImageSys::disp_const and on the
// member's own Dev::huber_a > 0, uniform per work-group: the members of a batch may differ in both.
// No atomics, every sum in the solo kernels' order.  k_imb_lin and k_imb_eval call the bodies k_im_lin and k_im_eval are wrappers
// over; k_imb_solve compiles k_im_solve's statements (IM_SOLVE_BODY).  A member's result is bit-equal to solving it alone as far
// as the compiler contracts the same sums the same way in both kernels, which tests/test_gpu_image_batch.py checks on the device.
__global__ __launch_bounds__(IM_THREADS) void k_imb_lin(const Dev *__restrict__ devs) {
    const Dev &d = devs[blockIdx.y];
    if (blockIdx.x >= (unsigned)d.image->n_wg) return;
    if (d.huber_a > 0.0) {
        if (d.image->disp_const) im_lin_body<false, true>(d, blockIdx.x);
        else im_lin_body<true, true>(d, blockIdx.x);
        return;
    }
    if (d.image->disp_const) im_lin_body<false, false>(d, blockIdx.x);
    else im_lin_body<true, false>(d, blockIdx.x);
}
__global__ __launch_bounds__(IM_SOLVE_THREADS) void k_imb_solve(const Dev *__restrict__ devs) {
    const Dev &d = devs[blockIdx.y];
    IM_SOLVE_BODY
}
// work-group 0 of every problem does check_body, as in k_im_eval
__global__ __launch_bounds__(IM_THREADS) void k_imb_eval(const Dev *__restrict__ devs) {
    Dev &d = const_cast<Dev &>(devs[blockIdx.y]);      // (check_body's signature; it writes through the pointers d holds only)
    const int n_wg = d.image->n_wg;
    if (blockIdx.x > (unsigned)n_wg) return;
    if (blockIdx.x == 0) { check_body(d, n_wg, false); return; }
    if (d.huber_a > 0.0) {
        if (d.image->disp_const) im_eval_body<false, true>(d, blockIdx.x - 1, nullptr);
        else im_eval_body<true, true>(d, blockIdx.x - 1, nullptr);
        return;
    }
    if (d.image->disp_const) im_eval_body<false, false>(d, blockIdx.x - 1, nullptr);
    else im_eval_body<true, false>(d, blockIdx.x - 1, nullptr);
}

// ----------------------------------------------------------------- launchers ---
void launch_image_lin_solve(Launcher &L, const Dev &d) {
    const ImageSys &im = L.image;
    const bool loss = d.huber_a > 0.0;
    if (im.disp_const) {
        if (loss) LAUNCH(KC_LIN_LM, (k_im_lin<false, true>), dim3(im.n_wg), dim3(IM_THREADS), 0, d);
        else LAUNCH(KC_LIN_LM, (k_im_lin<false, false>), dim3(im.n_wg), dim3(IM_THREADS), 0, d);
    } else {
        if (loss) LAUNCH(KC_LIN_LM, (k_im_lin<true, true>), dim3(im.n_wg), dim3(IM_THREADS), 0, d);
        else LAUNCH(KC_LIN_LM, (k_im_lin<true, false>), dim3(im.n_wg), dim3(IM_THREADS), 0, d);
    }
    LAUNCH(KC_SMALL, k_im_solve, dim3(1), dim3(IM_SOLVE_THREADS), 0, d);
}

void launch_image(Launcher &L, const Dev &d, double *delta_disp) {
    const ImageSys &im = L.image;
    launch_image_lin_solve(L, d);
    const bool loss = d.huber_a > 0.0;
    if (im.disp_const) {
        if (loss) LAUNCH(KC_BACKSUB_EVAL, (k_im_eval<false, true>), dim3(im.n_wg + 1), dim3(IM_THREADS), 0, d, delta_disp);
        else LAUNCH(KC_BACKSUB_EVAL, (k_im_eval<false, false>), dim3(im.n_wg + 1), dim3(IM_THREADS), 0, d, delta_disp);
    } else {
        if (loss) LAUNCH(KC_BACKSUB_EVAL, (k_im_eval<true, true>), dim3(im.n_wg + 1), dim3(IM_THREADS), 0, d, delta_disp);
        else LAUNCH(KC_BACKSUB_EVAL, (k_im_eval<true, false>), dim3(im.n_wg + 1), dim3(IM_THREADS), 0, d, delta_disp);
    }
    launch_decide_commit(L, d, true, true, 1);      // k_decide alone: Dev::n_groups = n_wg evaluation partials, one pose partial
    launch_best(L, d);
}

// One iteration of n problems: five launches whatever n is.  max_wg: the largest ImageSys::n_wg, best_groups: the largest grid
// launch_best would take, terminated: n words (State::terminated of every problem after its decision).
void launch_image_batch(hipStream_t stream, const Dev *devs, int n, int max_wg, int best_groups, int *terminated) {
    hipLaunchKernelGGL(k_imb_lin, dim3(max_wg, n), dim3(IM_THREADS), 0, stream, devs);
    hipLaunchKernelGGL(k_imb_solve, dim3(1, n), dim3(IM_SOLVE_THREADS), 0, stream, devs);
    hipLaunchKernelGGL(k_imb_eval, dim3(max_wg + 1, n), dim3(IM_THREADS), 0, stream, devs);
    launch_batch_decide_best(stream, devs, n, best_groups, terminated);
}

}  // namespace ssba
