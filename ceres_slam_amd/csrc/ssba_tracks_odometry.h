// Streaming stereo odometry of libssba_tracks.so (include/ssba_tracks.h, "Odometry"; the statement is
// tests/tracks_odometry_reference.py): the second half of sparse_stereo_odometry_node.cpp's callback, lines 176-301, for the
// matches of one pushed frame to the frame before, without leaving the device.  Included by ssba_tracks.hip after its stream
// kernels, whose scan and constants it uses.
//
//   k_od_match     stream: the kept survivors that inherited from a kept one, compacted     grid (1)
//                  in keypoint order, both sides triangulated; the frame's observations
//                  retained for the next push
//   k_od_pairs     ssba_track_relative_pose: the caller's list triangulated                 grid (n / 256)
//   k_od_align     one LANE per hypothesis: its draw and the 3-point alignment              grid (H / 256)
//   k_od_score     one WAVE per hypothesis: the inlier count, ballot + popcount             grid (H / 4)
//   k_od_solve     one work-group: the first maximum, the flags, the whole Levenberg-       grid (1)
//                  Marquardt loop of the two-view problem, the chain, the pose block
// Everything is fp64.  Every sum runs over the inliers in a fixed order (a lane adds its own inliers in ascending order, the 64
// lanes of a wave are folded by shuffles, the 4 waves in wave order): no floating-point atomic, two runs give the same bytes.
#pragma once
#include <float.h>
#include <math.h>

#include "ssba_align3.h"
#include "ssba_solve6.h"

namespace ssba {
namespace {

constexpr int OD_BLOCK = 256;                       // k_od_solve: one wave per SIMD, so that a lane may hold the whole linearisation
constexpr int OD_WAVES = OD_BLOCK / 64;
constexpr int OD_MAX = SSBA_TRACK_ODOMETRY_MAX;     // matches and hypotheses
constexpr int OD_ITEMS = OD_MAX / OD_BLOCK;
constexpr int OD_SUMS = 62;                         // what a linearisation reduces, see od_linearise

static_assert(OD_MAX == SSBA_TRACK_MAX_FEATURES, "a frame's survivors fit the match list");

// the pose block: what a push with odometry brings down behind its other outputs, and what ssba_track_relative_pose returns
struct OdPose {
    double T_rel[12], T_abs[12], T_ransac[12], initial_cost, final_cost;
    int32_t status;
    uint32_t num_matches, num_inliers, num_iterations;
};
static_assert(sizeof(OdPose) % sizeof(double) == 0, "pose blocks are copied as doubles");

struct OdRule {
    Cam cam;
    uint32_t hypotheses, iterations;
    double threshold, stiffness;        // stiffness = 1 / sqrt(observation_variance): the blocks' S is stiffness * I
};

struct OdWork {
    uint32_t *n;                        // the number of matches
    double *obs0, *obs1, *pts0, *pts1;  // OD_MAX x 3 each: (u, v, d) and the triangulated points of frame k - 1 and frame k
    double *hyp;                        // hypotheses x 12
    uint32_t *count;                    // hypotheses
    uint8_t *inlier;                    // OD_MAX
    uint32_t *index;                    // OD_MAX: the inliers' match indices, ascending
    double *x, *c, *scale;              // OD_MAX x 3 each: the points, the candidate's, their Jacobi scales
    double *cost_log;                   // iterations + 1
    int32_t *step_ok;                   // iterations + 1
    double *chain;                      // 12: T_km1_0 (streams only)
};

// StereoCamera::triangulate (stereo_camera.hpp:112-120)
__device__ __forceinline__ void od_triangulate(const Cam &cam, const double *z, double *p) {
    const double b_over_d = cam.b / z[2];
    p[0] = (z[0] - cam.cu) * b_over_d;
    p[1] = (z[1] - cam.cv) * b_over_d * (cam.fu / cam.fv);
    p[2] = cam.fu * b_over_d;
}

__device__ __forceinline__ void od_pair(const Cam &cam, const double *z0, const double *z1, uint32_t at, const OdWork &w) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        w.obs0[3 * (size_t)at + c] = z0[c];
        w.obs1[3 * (size_t)at + c] = z1[c];
    }
    od_triangulate(cam, z0, w.pts0 + 3 * (size_t)at);
    od_triangulate(cam, z1, w.pts1 + 3 * (size_t)at);
}

// The matches of a pushed frame: its kept survivors whose id was inherited from a kept survivor of the frame before, in
// keypoint order.  Those are the ids present in both pushes' outputs, with the (u, v, d) those pushes returned.  The frame's own
// kept flags and observations go to now_kept / now_uvd for the next push (refined / status are single-buffered).
__global__ __launch_bounds__(TR_BLOCK) void k_od_match(Cam cam, const uint32_t *__restrict__ cur_count, const uint16_t *__restrict__ xy,
                                                       const int32_t *__restrict__ d16s, const uint32_t *__restrict__ from,
                                                       const int32_t *__restrict__ refined, const int32_t *__restrict__ status, uint32_t stride,
                                                       int has_prev, const uint8_t *__restrict__ before_kept, const double *__restrict__ before_uvd,
                                                       uint8_t *__restrict__ now_kept, double *__restrict__ now_uvd, OdWork w) {
    __shared__ uint32_t part[TR_BLOCK / 64];
    const uint32_t n = min(*cur_count, stride);
    uint32_t src[TR_ITEMS], mine = 0;
    double z[TR_ITEMS][3];
#pragma unroll
    for (int i = 0; i < TR_ITEMS; ++i) {
        const uint32_t j = threadIdx.x * TR_ITEMS + i;
        src[i] = TR_NONE;
        if (j >= stride) continue;
        bool kept = false;
        if (j < n) {
            kept = status ? status[j] == SSBA_TRACK_REFINE_OK : true;
            int32_t v[3];
            if (refined) {
#pragma unroll
                for (int c = 0; c < 3; ++c) v[c] = refined[3 * j + c];
            } else {
                v[0] = xy[2 * j];
                v[1] = xy[2 * j + 1];
                v[2] = d16s[j];
            }
            ts_uvd(v, refined != nullptr, z[i]);
#pragma unroll
            for (int c = 0; c < 3; ++c) now_uvd[3 * (size_t)j + c] = z[i][c];
            const uint32_t a = from[j];
            if (kept && has_prev && a < stride && before_kept[a]) src[i] = a;
        }
        now_kept[j] = kept ? 1 : 0;
        mine += src[i] != TR_NONE;
    }
    uint32_t total;
    uint32_t pos = tr_block_exscan(mine, part, &total);
#pragma unroll
    for (int i = 0; i < TR_ITEMS; ++i) {
        if (src[i] == TR_NONE) continue;
        if (pos < (uint32_t)OD_MAX) od_pair(cam, before_uvd + 3 * (size_t)src[i], z[i], pos, w);      // holds: one match per survivor slot
        ++pos;
    }
    if (threadIdx.x == 0) *w.n = min(total, (uint32_t)OD_MAX);
}

// a list the caller supplies, paired by position
__global__ __launch_bounds__(256) void k_od_pairs(Cam cam, const double *__restrict__ uvd_prev, const double *__restrict__ uvd_cur, uint32_t n, OdWork w) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i == 0) *w.n = n;
    if (i < n && i < (uint32_t)OD_MAX) od_pair(cam, uvd_prev + 3 * (size_t)i, uvd_cur + 3 * (size_t)i, i, w);
}

// The draws: a counter-based 32-bit mixer, so that hypothesis h of frame f needs neither a stream of earlier draws nor the host
// (n is known on the device only).  Three distinct indices below n >= 3 by construction, no rejection loop.
__device__ __forceinline__ uint32_t od_mix(uint32_t x) {
    x ^= x >> 16;
    x *= 0x7feb352du;
    x ^= x >> 15;
    x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}
__device__ __forceinline__ void od_draw(uint32_t frame, uint32_t hypotheses, uint32_t h, uint32_t n, uint32_t s[3]) {
    const uint32_t c = 3u * (frame * hypotheses + h);      // mod 2^32
    const uint32_t i0 = od_mix(c) % n;
    uint32_t i1 = od_mix(c + 1u) % (n - 1u);
    i1 += i1 >= i0;
    uint32_t i2 = od_mix(c + 2u) % (n - 2u);
    i2 += i2 >= min(i0, i1);
    i2 += i2 >= max(i0, i1);
    s[0] = i0;
    s[1] = i1;
    s[2] = i2;
}

__global__ __launch_bounds__(256) void k_od_align(OdRule rule, uint32_t frame, OdWork w) {
    const uint32_t h = blockIdx.x * 256 + threadIdx.x, n = min(*w.n, (uint32_t)OD_MAX);
    if (h >= rule.hypotheses) return;
    double T[12] = {0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1};
    if (n >= 3) {
        uint32_t s[3];
        od_draw(frame, rule.hypotheses, h, n, s);
        double s0[9], s1[9];
        for (int k = 0; k < 3; ++k)
            for (int c = 0; c < 3; ++c) {
                s0[3 * k + c] = w.pts0[3 * (size_t)s[k] + c];
                s1[3 * k + c] = w.pts1[3 * (size_t)s[k] + c];
            }
        align3(s0, s1, T);
    }
    for (int i = 0; i < 12; ++i) w.hyp[12 * (size_t)h + i] = T[i];
}

// One wave per hypothesis.  The count is an integer and wave-uniform from the start: the ballot of the 64 decisions is a scalar
// pair, its population count one scalar instruction, so there is no cross-lane reduction at all (shorter than the DPP adds).
__global__ __launch_bounds__(256) void k_od_score(OdRule rule, OdWork w) {
    const uint32_t h = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63, n = min(*w.n, (uint32_t)OD_MAX);
    if (h >= rule.hypotheses) return;
    uint32_t count = 0;
    if (n >= 3) {
        double T[12];
        for (int i = 0; i < 12; ++i) T[i] = w.hyp[12 * (size_t)h + i];
        for (uint32_t base = 0; base < n; base += 64) {
            const uint32_t i = base + lane;
            const bool in = i < n && is_inlier(rule.cam, T, w.pts0 + 3 * (size_t)i, w.pts1 + 3 * (size_t)i, rule.threshold);
            count += (uint32_t)__popcll(__ballot(in));
        }
    }
    if (lane == 0) w.count[h] = count;
}

// ---- the two-view problem ----------------------------------------------------------------------------------------------------
// Pose k - 1 is the identity and constant, pose k is T (free, updated by exp(eps) T), one free point per inlier; two
// StereoReprojectionError blocks per point, r = s (project(T p) - z) (stereo_reprojection_error.hpp:27-55), with the local
// Jacobians of oracle/ssba_oracle.c orc_stereo_residual: Jp = s Jpi [I | -q^], Jl = s Jpi R.
__device__ __forceinline__ void od_project(const Cam &cam, const double q[3], double pred[3]) {
    const double one_over_z = 1.0 / q[2];
    pred[0] = cam.fu * q[0] * one_over_z + cam.cu;
    pred[1] = cam.fv * q[1] * one_over_z + cam.cv;
    pred[2] = cam.fu * cam.b * one_over_z;
}
__device__ __forceinline__ void od_transform(const double T[12], const double p[3], double q[3]) {
    q[0] = T[3] * p[0] + T[4] * p[1] + T[5] * p[2] + T[0];
    q[1] = T[6] * p[0] + T[7] * p[1] + T[8] * p[2] + T[1];
    q[2] = T[9] * p[0] + T[10] * p[1] + T[11] * p[2] + T[2];
}
// s Jpi(q) as its five entries (0,0) (0,2) (1,1) (1,2) (2,2)
__device__ __forceinline__ void od_projection_jacobian(const Cam &cam, double s, const double q[3], double A[5]) {
    const double one_over_z = 1.0 / q[2], one_over_z2 = one_over_z * one_over_z;
    A[0] = s * (cam.fu * one_over_z);
    A[1] = s * (-cam.fu * q[0] * one_over_z2);
    A[2] = s * (cam.fv * one_over_z);
    A[3] = s * (-cam.fv * q[1] * one_over_z2);
    A[4] = s * (-cam.fu * cam.b * one_over_z2);
}

__device__ __forceinline__ double od_point_cost(const Cam &cam, double s, const double T[12], const double p[3], const double z0[3], const double z1[3]) {
    double q[3], a[3], b[3], sq0 = 0.0, sq1 = 0.0;
    od_project(cam, p, a);
    od_transform(T, p, q);
    od_project(cam, q, b);
#pragma unroll
    for (int m = 0; m < 3; ++m) {
        const double r0 = s * (a[m] - z0[m]), r1 = s * (b[m] - z1[m]);
        sq0 += r0 * r0;
        sq1 += r1 * r1;
    }
    return 0.5 * sq0 + 0.5 * sq1;
}

// (so3group.hpp:273-291, perturbations.hpp:45-65) T_new = exp(eps) T with exp(xi) = (xi[0:3], Exp_SO3(xi[3:6]))
__device__ void od_se3_plus(const double T[12], const double eps[6], double out[12]) {
    const double *phi = eps + 3;
    const double angle = sqrt(phi[0] * phi[0] + phi[1] * phi[1] + phi[2] * phi[2]);
    double E[9];
    if (angle <= DBL_EPSILON) {
        E[0] = 1.0;     E[1] = -phi[2]; E[2] = phi[1];
        E[3] = phi[2];  E[4] = 1.0;     E[5] = -phi[0];
        E[6] = -phi[1]; E[7] = phi[0];  E[8] = 1.0;
    } else {
        const double a[3] = {phi[0] / angle, phi[1] / angle, phi[2] / angle};
        const double cp = cos(angle), sp = sin(angle), omc = 1.0 - cp;
        E[0] = cp + omc * a[0] * a[0];
        E[1] = omc * a[0] * a[1] - sp * a[2];
        E[2] = omc * a[0] * a[2] + sp * a[1];
        E[3] = omc * a[1] * a[0] + sp * a[2];
        E[4] = cp + omc * a[1] * a[1];
        E[5] = omc * a[1] * a[2] - sp * a[0];
        E[6] = omc * a[2] * a[0] - sp * a[1];
        E[7] = omc * a[2] * a[1] + sp * a[0];
        E[8] = cp + omc * a[2] * a[2];
    }
    for (int i = 0; i < 3; ++i) {
        out[i] = E[3 * i] * T[0] + E[3 * i + 1] * T[1] + E[3 * i + 2] * T[2] + eps[i];
        for (int j = 0; j < 3; ++j) out[3 + 3 * i + j] = E[3 * i] * T[3 + j] + E[3 * i + 1] * T[6 + j] + E[3 * i + 2] * T[9 + j];
    }
}

// inverse of a 3 x 3 SPD matrix through its Cholesky factor, packed 00 01 02 11 12 22 (the oracle's inv_spd)
__device__ __forceinline__ bool od_inverse3(const double C[6], double Ci[6]) {
    bool ok = C[0] > 0.0 && isfinite(C[0]);
    const double l00 = sqrt(C[0]), l10 = C[1] / l00, l20 = C[2] / l00;
    const double d1 = C[3] - l10 * l10;
    ok = ok && d1 > 0.0 && isfinite(d1);
    const double l11 = sqrt(d1), l21 = (C[4] - l20 * l10) / l11;
    const double d2 = C[5] - l20 * l20 - l21 * l21;
    ok = ok && d2 > 0.0 && isfinite(d2);
    const double l22 = sqrt(d2);
    const double m00 = 1.0 / l00, m11 = 1.0 / l11, m22 = 1.0 / l22;
    const double m10 = -(l10 * m00) / l11, m21 = -(l21 * m11) / l22, m20 = -(l20 * m00 + l21 * m10) / l22;
    Ci[0] = m00 * m00 + m10 * m10 + m20 * m20;
    Ci[1] = m10 * m11 + m20 * m21;
    Ci[2] = m20 * m22;
    Ci[3] = m11 * m11 + m21 * m21;
    Ci[4] = m21 * m22;
    Ci[5] = m22 * m22;
    return ok;
}

// Everything the linearisation and the back-substitution need from one point at (T, p) under the trust-region radius: the
// residuals and Jacobians of its two blocks, its gradient, its damped and scaled 3 x 3 block inverted, and W = Jp^T Jl in the
// point's scale (the pose's scale sp multiplies rows afterwards: it is not known while iteration zero is being summed).
struct OdPoint {
    double r0[3], r1[3];
    double A0[5], Jl[9], Jp[18];
    double gl[3], sq[3], scale[3], gls[3];
    double Ci[6], W[18];
    bool ok;
};
__device__ __forceinline__ double od_sym3(const double M[6], int a, int b) {
    return M[a <= b ? (a == 0 ? b : a + b + 1) : (b == 0 ? a : a + b + 1)];      // 00 01 02 11 12 22
}
__device__ __forceinline__ void od_point(const Cam &cam, double s, const double T[12], const double p[3], const double z0[3], const double z1[3], double radius,
                                         bool first, double *__restrict__ scale, OdPoint *o) {
    double q[3], pred[3], A[5];
    od_project(cam, p, pred);
#pragma unroll
    for (int m = 0; m < 3; ++m) o->r0[m] = s * (pred[m] - z0[m]);
    od_projection_jacobian(cam, s, p, o->A0);
    od_transform(T, p, q);
    od_project(cam, q, pred);
#pragma unroll
    for (int m = 0; m < 3; ++m) o->r1[m] = s * (pred[m] - z1[m]);
    od_projection_jacobian(cam, s, q, A);
    const double rows[3][3] = {{A[0], 0.0, A[1]}, {0.0, A[2], A[3]}, {0.0, 0.0, A[4]}};
    const double rows0[3][3] = {{o->A0[0], 0.0, o->A0[1]}, {0.0, o->A0[2], o->A0[3]}, {0.0, 0.0, o->A0[4]}};
#pragma unroll
    for (int m = 0; m < 3; ++m) {
        const double *a = rows[m];
        o->Jp[6 * m + 0] = a[0];
        o->Jp[6 * m + 1] = a[1];
        o->Jp[6 * m + 2] = a[2];
        o->Jp[6 * m + 3] = -a[1] * q[2] + a[2] * q[1];
        o->Jp[6 * m + 4] = a[0] * q[2] - a[2] * q[0];
        o->Jp[6 * m + 5] = -a[0] * q[1] + a[1] * q[0];
#pragma unroll
        for (int c = 0; c < 3; ++c) o->Jl[3 * m + c] = a[0] * T[3 + c] + a[1] * T[6 + c] + a[2] * T[9 + c];
    }
    double C[6] = {0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        double g = 0.0, n2 = 0.0;
#pragma unroll
        for (int m = 0; m < 3; ++m) {
            g += rows0[m][c] * o->r0[m];
            n2 += rows0[m][c] * rows0[m][c];
        }
#pragma unroll
        for (int m = 0; m < 3; ++m) {
            g += o->Jl[3 * m + c] * o->r1[m];
            n2 += o->Jl[3 * m + c] * o->Jl[3 * m + c];
        }
        o->gl[c] = g;
        o->sq[c] = n2;
        if (first) scale[c] = 1.0 / (1.0 + sqrt(n2));        // Jacobi scaling, once (trust_region_minimizer.cc IterationZero)
        o->scale[c] = scale[c];
        o->gls[c] = g * o->scale[c];
    }
    int at = 0;
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = a; b < 3; ++b, ++at) {
            double v = 0.0;
#pragma unroll
            for (int m = 0; m < 3; ++m) v += rows0[m][a] * rows0[m][b] * o->scale[a] * o->scale[b];
#pragma unroll
            for (int m = 0; m < 3; ++m) v += o->Jl[3 * m + a] * o->Jl[3 * m + b] * o->scale[a] * o->scale[b];
            if (a == b) v += fmin(fmax(o->sq[a] * o->scale[a] * o->scale[a], 1e-6), 1e32) / radius;      // min / max_lm_diagonal
            C[at] = v;
        }
    o->ok = od_inverse3(C, o->Ci);
#pragma unroll
    for (int c = 0; c < 6; ++c)
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            double v = 0.0;
#pragma unroll
            for (int m = 0; m < 3; ++m) v += o->Jp[6 * m + c] * o->Jl[3 * m + d];
            o->W[3 * c + d] = v * o->scale[d];
        }
}

// the sum of K values per lane over the work-group, in a fixed order; every lane gets the sums
template <int K> __device__ __forceinline__ void od_reduce(double (&v)[K], double *lds) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < K; ++k) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v[k] += __shfl_down(v[k], o, 64);
        if (lane == 0) lds[wave * K + k] = v[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) {
        double s = lds[k];
#pragma unroll
        for (int wv = 1; wv < OD_WAVES; ++wv) s += lds[wv * K + k];
        v[k] = s;
    }
    __syncthreads();
}
__device__ __forceinline__ double od_reduce_max(double v, double *lds) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_down(v, o, 64));
    if (lane == 0) lds[wave] = v;
    __syncthreads();
    double s = lds[0];
#pragma unroll
    for (int wv = 1; wv < OD_WAVES; ++wv) s = fmax(s, lds[wv]);
    __syncthreads();
    return s;
}

// One strided pass over the m inliers at (T, x) under `radius`.  sums: [0] cost, [1..6] g_p, [7..12] the squared column norms
// of J_p, [13..33] J_p^T J_p, [34..54] sum (W Ci) W^T, [55..60] sum (W Ci) g_l (all in the points' scale, not yet the pose's;
// 21 = the packed upper triangle), [61] |x|^2.  Returns through *gl_max the largest |g_l| entry; false if a point block was
// not positive definite.
__device__ __forceinline__ bool od_linearise(const OdRule &rule, const OdWork &w, uint32_t m, const double T[12], const double *__restrict__ x, double radius,
                                             bool first, double (&sums)[OD_SUMS], double *gl_max, double *lds) {
    double top = 0.0;
    int bad = 0;
#pragma unroll
    for (int i = 0; i < OD_SUMS; ++i) sums[i] = 0.0;
    for (uint32_t k = threadIdx.x; k < m; k += OD_BLOCK) {
        const uint32_t i = w.index[k];
        OdPoint o;
        od_point(rule.cam, rule.stiffness, T, x + 3 * (size_t)k, w.obs0 + 3 * (size_t)i, w.obs1 + 3 * (size_t)i, radius, first, w.scale + 3 * (size_t)k, &o);
        bad |= !o.ok;
        sums[0] += 0.5 * (o.r0[0] * o.r0[0] + o.r0[1] * o.r0[1] + o.r0[2] * o.r0[2]) + 0.5 * (o.r1[0] * o.r1[0] + o.r1[1] * o.r1[1] + o.r1[2] * o.r1[2]);
        double Y[18];
#pragma unroll
        for (int c = 0; c < 6; ++c) {
            double g = 0.0, n2 = 0.0;
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                g += o.Jp[6 * r + c] * o.r1[r];
                n2 += o.Jp[6 * r + c] * o.Jp[6 * r + c];
            }
            sums[1 + c] += g;
            sums[7 + c] += n2;
#pragma unroll
            for (int d = 0; d < 3; ++d) Y[3 * c + d] = o.W[3 * c] * od_sym3(o.Ci, 0, d) + o.W[3 * c + 1] * od_sym3(o.Ci, 1, d) + o.W[3 * c + 2] * od_sym3(o.Ci, 2, d);
            sums[55 + c] += Y[3 * c] * o.gls[0] + Y[3 * c + 1] * o.gls[1] + Y[3 * c + 2] * o.gls[2];
        }
#pragma unroll
        for (int c = 0; c < 6; ++c)
#pragma unroll
            for (int d = c; d < 6; ++d) {
                sums[13 + tri21(c, d)] += o.Jp[c] * o.Jp[d] + o.Jp[6 + c] * o.Jp[6 + d] + o.Jp[12 + c] * o.Jp[12 + d];
                sums[34 + tri21(c, d)] += Y[3 * c] * o.W[3 * d] + Y[3 * c + 1] * o.W[3 * d + 1] + Y[3 * c + 2] * o.W[3 * d + 2];
            }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            top = fmax(top, fabs(o.gl[c]));
            sums[61] += x[3 * (size_t)k + c] * x[3 * (size_t)k + c];
        }
    }
    od_reduce(sums, lds);
    *gl_max = od_reduce_max(top, lds);
    return !__syncthreads_or(bad);
}

// The back-substitution for the pose step dp, the candidate points c = x + dl, and what the step is judged by.
// out: [0] the model cost change -(J d)^T (r + J d / 2), [1] the candidate's cost at (Tc, c), [2] |x - c|^2.
__device__ __forceinline__ bool od_candidate(const OdRule &rule, const OdWork &w, uint32_t m, const double T[12], const double Tc[12], const double dp[6],
                                             const double *__restrict__ x, double *__restrict__ c, double radius, double (&out)[3], double *lds) {
    int bad = 0;
    out[0] = out[1] = out[2] = 0.0;
    for (uint32_t k = threadIdx.x; k < m; k += OD_BLOCK) {
        const uint32_t i = w.index[k];
        const double *z0 = w.obs0 + 3 * (size_t)i, *z1 = w.obs1 + 3 * (size_t)i, *p = x + 3 * (size_t)k;
        OdPoint o;
        od_point(rule.cam, rule.stiffness, T, p, z0, z1, radius, false, w.scale + 3 * (size_t)k, &o);
        // y_l = C^-1 (g_l - W^T y_p) with y_p = -dp / sp, the rows of W scaled by sp: g_l + W^T dp in the point's scale
        double t[3], dl[3], pc[3];
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            double v = o.gls[d];
#pragma unroll
            for (int a = 0; a < 6; ++a) v += o.W[3 * a + d] * dp[a];
            t[d] = v;
        }
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const double y = od_sym3(o.Ci, a, 0) * t[0] + od_sym3(o.Ci, a, 1) * t[1] + od_sym3(o.Ci, a, 2) * t[2];
            dl[a] = -y * o.scale[a];
            bad |= !isfinite(dl[a]);
        }
        const double rows0[3][3] = {{o.A0[0], 0.0, o.A0[1]}, {0.0, o.A0[2], o.A0[3]}, {0.0, 0.0, o.A0[4]}};
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const double jd0 = rows0[r][0] * dl[0] + rows0[r][1] * dl[1] + rows0[r][2] * dl[2];
            double jd1 = o.Jl[3 * r] * dl[0] + o.Jl[3 * r + 1] * dl[1] + o.Jl[3 * r + 2] * dl[2];
#pragma unroll
            for (int a = 0; a < 6; ++a) jd1 += o.Jp[6 * r + a] * dp[a];
            out[0] -= jd0 * (o.r0[r] + 0.5 * jd0);
            out[0] -= jd1 * (o.r1[r] + 0.5 * jd1);
        }
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            pc[a] = p[a] + dl[a];
            c[3 * (size_t)k + a] = pc[a];
            const double d = p[a] - pc[a];
            out[2] += d * d;
        }
        out[1] += od_point_cost(rule.cam, rule.stiffness, Tc, pc, z0, z1);
    }
    od_reduce(out, lds);
    return !__syncthreads_or(bad);
}

// T_k_0 = T_k_km1 o T_km1_0 (dataset_problem.cpp:255; the arithmetic of k_fe_chain)
__device__ __forceinline__ void od_compose(const double Tk[12], const double P[12], double N[12]) {
    for (int i = 0; i < 3; ++i) {
        N[i] = Tk[3 + 3 * i] * P[0] + Tk[4 + 3 * i] * P[1] + Tk[5 + 3 * i] * P[2] + Tk[i];
        for (int j = 0; j < 3; ++j) N[3 + 3 * i + j] = Tk[3 + 3 * i] * P[3 + j] + Tk[4 + 3 * i] * P[6 + j] + Tk[5 + 3 * i] * P[9 + j];
    }
}

// The winner, its flags, the refinement and the chain in one launch of one work-group.  Every scalar of the minimiser is
// computed by every lane from the same reduced sums, so all branches are uniform and nothing is broadcast.
// mode 0: a pushed frame that has a predecessor; 1: a stream's first push (FIRST_FRAME, the chain starts at `first_pose`);
// 2: ssba_track_relative_pose (no chain).
__global__ __launch_bounds__(OD_BLOCK) void k_od_solve(OdRule rule, OdWork w, int mode, const double *__restrict__ first_pose, OdPose *__restrict__ out) {
    __shared__ double lds[OD_WAVES * OD_SUMS];
    __shared__ uint32_t s_best[OD_BLOCK], s_it[OD_BLOCK], s_part[OD_WAVES];
    const uint32_t t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const uint32_t n = mode == 1 ? 0u : min(*w.n, (uint32_t)OD_MAX);
    double T[12] = {0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1}, Tr[12] = {0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1};
    int status = mode == 1 ? SSBA_TRACK_POSE_FIRST_FRAME : (n < 3 ? SSBA_TRACK_POSE_FEW_MATCHES : SSBA_TRACK_POSE_OK);
    uint32_t m = 0, nlog = 0;
    double initial_cost = 0.0, final_cost = 0.0;
    for (uint32_t i = t; i <= rule.iterations; i += OD_BLOCK) {
        w.cost_log[i] = nan("");
        w.step_ok[i] = 0;
    }
    if (status != SSBA_TRACK_POSE_OK)
        for (uint32_t j = t; j < n; j += OD_BLOCK) w.inlier[j] = 0;
    if (status == SSBA_TRACK_POSE_OK) {
        // the first maximum: a hypothesis replaces the best only with MORE inliers (point_cloud_aligner.cpp:127-130)
        uint32_t best = 0, bit = 0;
        for (uint32_t it = t; it < rule.hypotheses; it += OD_BLOCK) {
            const uint32_t c = w.count[it];
            if (c > best) { best = c; bit = it; }
        }
        s_best[t] = best;
        s_it[t] = bit;
        __syncthreads();
        for (uint32_t o = OD_BLOCK / 2; o > 0; o >>= 1) {
            if (t < o) {
                const uint32_t b2 = s_best[t + o], i2 = s_it[t + o];
                if (b2 > s_best[t] || (b2 == s_best[t] && b2 > 0 && i2 < s_it[t])) { s_best[t] = b2; s_it[t] = i2; }
            }
            __syncthreads();
        }
        best = s_best[0];
        bit = s_it[0];
        if (best > 0)
            for (int i = 0; i < 12; ++i) Tr[i] = w.hyp[12 * (size_t)bit + i];
        // the winner's flags, and its inliers' indices in ascending order
        uint32_t flags = 0, mine = 0;
#pragma unroll
        for (int i = 0; i < OD_ITEMS; ++i) {
            const uint32_t j = t * OD_ITEMS + i;
            const bool in = j < n && best > 0 && is_inlier(rule.cam, Tr, w.pts0 + 3 * (size_t)j, w.pts1 + 3 * (size_t)j, rule.threshold);
            flags |= (in ? 1u : 0u) << i;
            mine += in;
            if (j < n) w.inlier[j] = in ? 1 : 0;
        }
        uint32_t inc = mine;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t up = __shfl_up(inc, d, 64);
            if (lane >= d) inc += up;
        }
        if (lane == 63) s_part[wave] = inc;
        __syncthreads();
        uint32_t pos = inc - mine;
        for (uint32_t wv = 0; wv < OD_WAVES; ++wv) {
            pos += wv < wave ? s_part[wv] : 0u;
            m += s_part[wv];
        }
#pragma unroll
        for (int i = 0; i < OD_ITEMS; ++i)
            if (flags >> i & 1u) w.index[pos++] = t * OD_ITEMS + i;
        __syncthreads();          // the index list is read by other lanes from here on
        for (int i = 0; i < 12; ++i) T[i] = Tr[i];
        if (m < 3) status = SSBA_TRACK_POSE_FEW_INLIERS;
    }
    if (status == SSBA_TRACK_POSE_OK) {
        // Levenberg-Marquardt as oracle/ssba_oracle.c orc_solve states it under orc_default_options (monotonic steps, Jacobi
        // scaling, radius 1e4, min_relative_decrease 1e-3, tolerances 1e-6 / 1e-10 / 1e-8, 5 invalid steps).  With monotonic
        // steps the step evaluator's reference cost is the current cost, so the step quality is cost_change / model change.
        double *x = w.x, *c = w.c;
        for (uint32_t k = t; k < m; k += OD_BLOCK)
#pragma unroll
            for (int a = 0; a < 3; ++a) x[3 * (size_t)k + a] = w.pts0[3 * (size_t)w.index[k] + a];      // a lane owns the same points in every pass
        double sp[6] = {1, 1, 1, 1, 1, 1}, radius = 1e4, decrease_factor = 2.0, x_cost = 0.0, lowest = 0.0;
        bool first = true, log_pending = true, failed = false;
        int log_ok = 0, invalid = 0;
        uint32_t iteration = 0;
        auto log_push = [&](double cost, int ok) {
            if (t == 0 && nlog <= rule.iterations) {
                w.cost_log[nlog] = cost;
                w.step_ok[nlog] = ok;
            }
            lowest = nlog == 0 ? cost : fmin(lowest, cost);
            ++nlog;
        };
        for (;;) {
            double sums[OD_SUMS], gl_max;
            const bool blocks_ok = od_linearise(rule, w, m, T, x, radius, first, sums, &gl_max, lds);
            if (first)
#pragma unroll
                for (int a = 0; a < 6; ++a) sp[a] = 1.0 / (1.0 + sqrt(sums[7 + a]));
            x_cost = sums[0];
            if (log_pending) log_push(x_cost, log_ok);
            log_pending = false;
            if (first) {
                initial_cost = x_cost;
                if (!isfinite(x_cost)) { failed = true; break; }
            }
            first = false;
            double x_norm2 = sums[61], neg_g[6], Tn[12], g_max = gl_max;
#pragma unroll
            for (int a = 0; a < 12; ++a) x_norm2 += T[a] * T[a];
#pragma unroll
            for (int a = 0; a < 6; ++a) neg_g[a] = -sums[1 + a];
            od_se3_plus(T, neg_g, Tn);            // the projected gradient |x - Plus(x, -g)|_inf
#pragma unroll
            for (int a = 0; a < 12; ++a) g_max = fmax(g_max, fabs(T[a] - Tn[a]));
            if (iteration >= rule.iterations || g_max <= 1e-10 || radius <= 1e-32) break;
            ++iteration;
            // the reduced 6 x 6 system in scaled coordinates, its LM diagonal, the pose step
            double S[21], gr[6], ys[6], dp[6], Tc[12], judged[3] = {0, 0, 0};
#pragma unroll
            for (int a = 0; a < 6; ++a) {
#pragma unroll
                for (int b = a; b < 6; ++b) S[tri21(a, b)] = (sums[13 + tri21(a, b)] - sums[34 + tri21(a, b)]) * sp[a] * sp[b];
                S[tri21(a, a)] += fmin(fmax(sums[7 + a] * sp[a] * sp[a], 1e-6), 1e32) / radius;
                gr[a] = (sums[1 + a] - sums[55 + a]) * sp[a];
            }
            bool valid = blocks_ok && po_solve6(S, gr, ys);       // ys = -S^-1 gr: the scaled step
#pragma unroll
            for (int a = 0; a < 6; ++a) {
                dp[a] = valid ? ys[a] * sp[a] : 0.0;
                valid = valid && isfinite(dp[a]);
            }
            if (valid) {
                od_se3_plus(T, dp, Tc);
                valid = od_candidate(rule, w, m, T, Tc, dp, x, c, radius, judged, lds) && judged[0] > 0.0;
            }
            if (!valid) {
                if (++invalid >= 5) {
                    failed = true;
                    log_push(x_cost, 0);
                    break;
                }
                radius /= decrease_factor;
                decrease_factor *= 2.0;
                log_push(x_cost, 0);
                continue;
            }
            invalid = 0;
            const double candidate_cost = isfinite(judged[1]) ? judged[1] : DBL_MAX;
            double step2 = judged[2];
#pragma unroll
            for (int a = 0; a < 12; ++a) step2 += (T[a] - Tc[a]) * (T[a] - Tc[a]);
            if (sqrt(step2) <= 1e-8 * (sqrt(x_norm2) + 1e-8)) break;
            const double cost_change = x_cost - candidate_cost;
            if (fabs(cost_change) <= 1e-6 * x_cost) break;
            const double quality = cost_change / judged[0];
            if (quality > 1e-3) {
                double *swap = x;
                x = c;
                c = swap;
#pragma unroll
                for (int a = 0; a < 12; ++a) T[a] = Tc[a];
                const double u = 2.0 * quality - 1.0;
                radius = fmin(1e16, radius / fmax(1.0 / 3.0, 1.0 - u * u * u));
                decrease_factor = 2.0;
                log_pending = true;           // the accepted point's cost is that of its own linearisation, next
                log_ok = 1;
            } else {
                radius /= decrease_factor;
                decrease_factor *= 2.0;
                log_push(candidate_cost, 0);
            }
        }
        final_cost = lowest;
        if (failed) {
            status = SSBA_TRACK_POSE_NUMERICAL;
            for (int i = 0; i < 12; ++i) T[i] = Tr[i];
        }
    }
    if (t == 0) {
        double chain[12] = {0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1}, Ta[12];
        if (mode == 1)
            for (int i = 0; i < 12; ++i) Ta[i] = first_pose[i];
        else {
            if (mode == 0)
                for (int i = 0; i < 12; ++i) chain[i] = w.chain[i];
            od_compose(T, chain, Ta);
        }
        for (int i = 0; i < 12; ++i) {
            out->T_rel[i] = T[i];
            out->T_abs[i] = Ta[i];
            out->T_ransac[i] = Tr[i];
            if (mode != 2) w.chain[i] = Ta[i];
        }
        out->initial_cost = initial_cost;
        out->final_cost = final_cost;
        out->status = status;
        out->num_matches = n;
        out->num_inliers = m;
        out->num_iterations = nlog;
    }
}

}  // namespace
}  // namespace ssba
