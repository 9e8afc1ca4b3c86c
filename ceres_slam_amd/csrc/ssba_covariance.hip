// Covariance blocks of (J^T J)^-1 at the current parameters (ssba_covariance_blocks, include/ssba.h).
//
// Poses.  Windowed layout: the SELECTED INVERSION of the block-tridiagonal reduced camera system S, from the factors that
// launch_bcr(L, d, false) keeps at every level (ssba_bcr.hip: for an odd block i, G with D_i = G G^T and 1/G_kk on its
// diagonal in place of D_i, YL = G^-1 L_i in place of L_i, YU = G^-1 L_{i+1}^T).  The inverse of a level's Schur complement
// onto its even blocks is the even-even part of the level's inverse, so the levels are walked from the top down:
//   top (one block):  Sigma = G^-T G^-1
//   level l, odd i:   the even neighbours' Sigma_{i-1,i-1}, Sigma_{i+1,i+1}, Sigma_{i+1,i-1} came from level l + 1, and
//                     row i of S Sigma = I gives
//                       A = YL Sigma_{i-1,i-1} + YU Sigma_{i+1,i-1}       Sigma_{i,i-1} = -G^-T A
//                       B = YL Sigma_{i-1,i+1} + YU Sigma_{i+1,i+1}       Sigma_{i,i+1} = -G^-T B
//                       Sigma_ii = G^-T (I + YL A^T + YU B^T) G^-1
// (at the end of the chain, without an i + 1, the YU terms drop out).  One launch per level, one workgroup per odd block;
// the output is the diagonal (at level-0 block positions) and the first sub-diagonal of every level, of which level 0's is
// the sub-diagonal of Sigma.  Products are 72 x 72 x 72, staged through LDS in panels of 24.
//
// Landmarks.  k_cov_jobs: one lane per requested block.  For a landmark l with free observing poses T and W_s = J_s^T J_l:
//   Sigma_ll = V^-1 + V^-1 (sum_{s,t} W_s^T Sigma_{st} W_t) V^-1,     Sigma_il = -(sum_s Sigma_{i,s} W_s) V^-1
// W is formed again from the observation (as the linearisation does).  Pose-pose blocks come from the band (windowed
// layout: every co-observing pose pair lies in the same or an adjacent super-block) or from whole columns of Sigma solved
// for the poses outside it (multi-right-hand-side sweep; general layout: every pose the request touches).
// No atomics: every output element is written by one lane, in a fixed order, so a call is bit-reproducible.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "ssba_device.h"
#include "ssba_launch.h"
#include "ssba_types.h"

namespace ssba {

constexpr int SI_THREADS = 256;
constexpr int SI_KP = 24;                                          // k panel of the products
constexpr int SI_PER = (BD * BD + SI_THREADS - 1) / SI_THREADS;   // 21 outputs per lane
constexpr size_t SI_BB = (size_t)BD * BD;

// C = Cadd + alpha op(X) op(Y), 72 x 72 row-major in global memory (C may be Cadd, never X or Y).  Ends with a barrier.
static __device__ void si_mm(double *C, const double *X, bool tX, const double *Y, bool tY, double alpha, const double *Cadd,
                             double *lds) {
    double *sX = lds, *sY = lds + BD * SI_KP;
    const int t = threadIdx.x;
    double acc[SI_PER];
#pragma unroll
    for (int q = 0; q < SI_PER; ++q) acc[q] = 0.0;
    for (int k0 = 0; k0 < BD; k0 += SI_KP) {
        for (int e = t; e < BD * SI_KP; e += SI_THREADS) {
            const int r = e / SI_KP, kk = e - r * SI_KP, k = k0 + kk;
            sX[e] = tX ? X[(size_t)k * BD + r] : X[(size_t)r * BD + k];
            const int k2 = e / BD, c = e - k2 * BD, kb = k0 + k2;
            sY[e] = tY ? Y[(size_t)c * BD + kb] : Y[(size_t)kb * BD + c];
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < SI_PER; ++q) {
            const int e = t + q * SI_THREADS;
            if (e < BD * BD) {
                const int r = e / BD, c = e - r * BD;
                double s = acc[q];
#pragma unroll 8
                for (int kk = 0; kk < SI_KP; ++kk) s = fma(sX[r * SI_KP + kk], sY[kk * BD + c], s);
                acc[q] = s;
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int q = 0; q < SI_PER; ++q) {
        const int e = t + q * SI_THREADS;
        if (e < BD * BD) C[e] = (Cadd ? Cadd[e] : 0.0) + alpha * acc[q];
    }
    __syncthreads();
}

// T = G^-1 (lower triangular; the factor kernels leave 1/G_kk on G's diagonal and leave its upper triangle undefined).
// Row by row, one lane per column: T_ij = -(1/G_ii) sum_{j <= k < i} G_ik T_kj.
static __device__ void si_tri_inv(double *T, const double *G, double *lds) {
    double *sT = lds;                                  // BD x BD
    const int t = threadIdx.x;
    for (int i = 0; i < BD; ++i) {
        if (t < BD) {
            double v = 0.0;
            if (t < i) {
                double s = 0.0;
                for (int k = t; k < i; ++k) s = fma(G[(size_t)i * BD + k], sT[k * BD + t], s);
                v = -G[(size_t)i * BD + i] * s;
            } else if (t == i) {
                v = G[(size_t)i * BD + i];
            }
            sT[i * BD + t] = v;
        }
        __syncthreads();
    }
    for (int e = t; e < BD * BD; e += SI_THREADS) T[e] = sT[e];
    __syncthreads();
}

// C = (C + C^T) / 2 in place (the diagonal blocks of Sigma are stored exactly symmetric)
static __device__ void si_symmetrize(double *C) {
    const int t = threadIdx.x;
    double v[SI_PER];
#pragma unroll
    for (int q = 0; q < SI_PER; ++q) {
        const int e = t + q * SI_THREADS;
        if (e < BD * BD) {
            const int r = e / BD, c = e - r * BD;
            v[q] = 0.5 * (C[(size_t)r * BD + c] + C[(size_t)c * BD + r]);
        }
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < SI_PER; ++q) {
        const int e = t + q * SI_THREADS;
        if (e < BD * BD) C[e] = v[q];
    }
    __syncthreads();
}

static __device__ __forceinline__ bool si_dead(const Dev &d) {
    const State &st = *d.st;
    return st.terminated || st.step_failed || st.dl_reuse;
}

__global__ __launch_bounds__(SI_THREADS) void k_selinv_top(Dev d, SelInv si) {
    __shared__ double lds[BD * BD];
    if (si_dead(d)) return;
    const BcrLevel &B = d.lev[d.n_levels - 1];
    double *T = si.ws;
    si_tri_inv(T, B.D, lds);
    double *S = si.sd + (size_t)B.pos[0] * SI_BB;
    si_mm(S, T, true, T, false, 1.0, nullptr, lds);
    si_symmetrize(S);
}

__global__ __launch_bounds__(SI_THREADS) void k_selinv_level(Dev d, SelInv si, int l) {
    __shared__ double lds[BD * BD];
    if (si_dead(d)) return;
    const BcrLevel &B = d.lev[l];
    const int i = 2 * (int)blockIdx.x + 1;
    const bool hasU = i + 1 < B.n;
    double *ws = si.ws + (size_t)blockIdx.x * 5 * SI_BB;
    double *T = ws, *A = ws + SI_BB, *Bm = ws + 2 * SI_BB, *M = ws + 3 * SI_BB, *N = ws + 4 * SI_BB;
    const double *G = B.D + (size_t)i * SI_BB, *YL = B.L + (size_t)i * SI_BB, *YU = B.YU + (size_t)blockIdx.x * SI_BB;
    const double *Sm = si.sd + (size_t)B.pos[i - 1] * SI_BB;
    const double *Sp = hasU ? si.sd + (size_t)B.pos[i + 1] * SI_BB : nullptr;
    const double *Cpm = hasU ? si.sc + (size_t)(si.sc_off[l + 1] + (i + 1) / 2) * SI_BB : nullptr;     // Sigma_{i+1,i-1}
    double *SC = si.sc + (size_t)si.sc_off[l] * SI_BB;                                                // SC[k] = Sigma_{k,k-1}
    si_tri_inv(T, G, lds);
    si_mm(A, YL, false, Sm, false, 1.0, nullptr, lds);
    if (hasU) {
        si_mm(A, YU, false, Cpm, false, 1.0, A, lds);
        si_mm(Bm, YL, false, Cpm, true, 1.0, nullptr, lds);
        si_mm(Bm, YU, false, Sp, false, 1.0, Bm, lds);
    }
    si_mm(SC + (size_t)i * SI_BB, T, true, A, false, -1.0, nullptr, lds);              // Sigma_{i,i-1} = -G^-T A
    if (hasU) si_mm(SC + (size_t)(i + 1) * SI_BB, Bm, true, T, false, -1.0, nullptr, lds);   // Sigma_{i+1,i} = -B^T G^-1
    si_mm(M, YL, false, A, true, 1.0, nullptr, lds);
    if (hasU) si_mm(M, YU, false, Bm, true, 1.0, M, lds);
    for (int k = threadIdx.x; k < BD; k += SI_THREADS) M[(size_t)k * BD + k] += 1.0;
    __syncthreads();
    si_symmetrize(M);
    si_mm(N, M, false, T, false, 1.0, nullptr, lds);
    double *S = si.sd + (size_t)B.pos[i] * SI_BB;
    si_mm(S, T, true, N, false, 1.0, nullptr, lds);                                    // Sigma_ii = G^-T M G^-1
    si_symmetrize(S);
}

void launch_selinv(Launcher &L, const Dev &d, const SelInv &si) {
    const int nl = d.n_levels;
    LAUNCH(KC_SMALL, k_selinv_top, dim3(1), dim3(SI_THREADS), 0, d, si);
    for (int l = nl - 2; l >= 0; --l) LAUNCH(KC_SMALL, k_selinv_level, dim3(d.lev[l].n / 2), dim3(SI_THREADS), 0, d, si, l);
}

// ------------------------------------------------------------------ blocks ---

// Sigma(6 fa + r, 6 fb + c) for free poses fa, fb: from a solved column when either pose has one, else from the band
static __device__ __forceinline__ double cov_sig(const CovSrc &s, int fa, int fb, int r, int c) {
    const int sb = s.slot ? s.slot[fb] : -1;
    if (sb >= 0) return s.cols[((size_t)sb * 6 + c) * s.nrow + 6 * (size_t)fa + r];
    const int sa = s.slot ? s.slot[fa] : -1;
    if (sa >= 0) return s.cols[((size_t)sa * 6 + r) * s.nrow + 6 * (size_t)fb + c];
    const int Ia = fa / SBP, Ib = fb / SBP, ra = 6 * (fa - Ia * SBP) + r, cb = 6 * (fb - Ib * SBP) + c;
    if (!s.sd || Ia - Ib > 1 || Ib - Ia > 1) return __builtin_nan("");     // outside what the host provided: never read past it
    if (Ia == Ib) return s.sd[(size_t)Ia * SI_BB + (size_t)ra * BD + cb];
    if (Ia == Ib + 1) return s.sc0[(size_t)Ia * SI_BB + (size_t)ra * BD + cb];
    return s.sc0[(size_t)Ib * SI_BB + (size_t)cb * BD + ra];       // Ib == Ia + 1
}

// W = J_p^T J_l (6 x 3, row-major) of slot s of landmark l
template <bool DN>
static __device__ __forceinline__ void cov_obs_w(const Dev &d, const LmObs<DN> &ob, int s, double px, double py, double pz, double W[18]) {
    const uint32_t k = ob.pose(d, s);
    const double *T = d.poses + (size_t)k * 12;
    double Sk[9];
    ob.stiffness(d, s, Sk);
    ObsLin o;
    obs_linearize_S(d, Sk, T, px, py, pz, ob.u(d, s), ob.v(d, s), ob.dd(d, s), o);
    double Jp[18], Jl[9];
    jac_pose(o, Jp);
    jac_point(o, T, Jl);
#pragma unroll
    for (int a = 0; a < 6; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) W[3 * a + b] = Jp[a] * Jl[b] + Jp[6 + a] * Jl[3 + b] + Jp[12 + a] * Jl[6 + b];
}

// V^-1 of the landmark's undamped 3 x 3 block (packed upper triangle of H_ll), false when V is not positive definite
static __device__ __forceinline__ bool cov_vinv(const Dev &d, int l, double Vi[9]) {
    double h[6];
#pragma unroll
    for (int c = 0; c < 6; ++c) h[c] = d.hll[(size_t)c * d.Lpad + l];
    // V = R^T R, R upper triangular
    if (!(h[0] > 0.0)) return false;
    const double r00 = sqrt(h[0]), r01 = h[1] / r00, r02 = h[2] / r00;
    const double a11 = h[3] - r01 * r01;
    if (!(a11 > 0.0)) return false;
    const double r11 = sqrt(a11), r12 = (h[4] - r01 * r02) / r11;
    const double a22 = h[5] - r02 * r02 - r12 * r12;
    if (!(a22 > 0.0)) return false;
    const double r22 = sqrt(a22);
    // R^-1 (upper), V^-1 = R^-1 R^-T
    const double i00 = 1.0 / r00, i11 = 1.0 / r11, i22 = 1.0 / r22;
    const double i01 = -r01 * i00 * i11, i12 = -r12 * i11 * i22, i02 = -(r02 * i00 + r12 * i01) * i22;
    Vi[0] = i00 * i00 + i01 * i01 + i02 * i02;
    Vi[1] = i01 * i11 + i02 * i12;
    Vi[2] = i02 * i22;
    Vi[4] = i11 * i11 + i12 * i12;
    Vi[5] = i12 * i22;
    Vi[8] = i22 * i22;
    Vi[3] = Vi[1]; Vi[6] = Vi[2]; Vi[7] = Vi[5];
    return true;
}

template <bool DN> __global__ __launch_bounds__(256) void k_cov_jobs(Dev d, CovSrc src, const CovJob *__restrict__ jobs, int n, double *out, int *fail) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    const CovJob J = jobs[j];
    double *o = out + J.off;
    if (J.kind == COV_JOB_POSE_POSE) {
        for (int r = 0; r < 6; ++r)
            for (int c = 0; c < 6; ++c) {
                const double v = cov_sig(src, J.a, J.b, r, c);
                if (J.tr) o[6 * c + r] = v; else o[6 * r + c] = v;
            }
        return;
    }
    const int l = J.b;
    double Vi[9];
    if (!cov_vinv(d, l, Vi)) { *fail = 1; return; }
    const double px = d.pts[l], py = d.pts[(size_t)d.Lpad + l], pz = d.pts[2 * (size_t)d.Lpad + l];
    const LmObs<DN> ob(d, l, DN ? 0u : d.lm_mask[l]);
    if (J.kind == COV_JOB_POINT) {
        double X[9];
#pragma unroll
        for (int e = 0; e < 9; ++e) X[e] = 0.0;
        for (int s = 0; s < ob.count(); ++s) {
            if (!ob.has(s)) continue;
            const int fs = d.pose_free[ob.pose(d, s)];
            if (fs < 0) continue;
            double Z[18];                               // sum_t Sigma_{st} W_t
#pragma unroll
            for (int e = 0; e < 18; ++e) Z[e] = 0.0;
            for (int t = 0; t < ob.count(); ++t) {
                if (!ob.has(t)) continue;
                const int ft = d.pose_free[ob.pose(d, t)];
                if (ft < 0) continue;
                double W[18];
                cov_obs_w(d, ob, t, px, py, pz, W);
                for (int r = 0; r < 6; ++r)
#pragma unroll
                    for (int c = 0; c < 6; ++c) {
                        const double sg = cov_sig(src, fs, ft, r, c);
                        Z[3 * r] = fma(sg, W[3 * c], Z[3 * r]);
                        Z[3 * r + 1] = fma(sg, W[3 * c + 1], Z[3 * r + 1]);
                        Z[3 * r + 2] = fma(sg, W[3 * c + 2], Z[3 * r + 2]);
                    }
            }
            double W[18];
            cov_obs_w(d, ob, s, px, py, pz, W);
#pragma unroll
            for (int a = 0; a < 3; ++a)
#pragma unroll
                for (int b = 0; b < 3; ++b) {
                    double v = X[3 * a + b];
#pragma unroll
                    for (int r = 0; r < 6; ++r) v = fma(W[3 * r + a], Z[3 * r + b], v);
                    X[3 * a + b] = v;
                }
        }
        // Sigma_ll = V^-1 + V^-1 X V^-1, symmetrised
        double Y[9], S[9];
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int b = 0; b < 3; ++b) Y[3 * a + b] = X[3 * a] * Vi[b] + X[3 * a + 1] * Vi[3 + b] + X[3 * a + 2] * Vi[6 + b];
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int b = 0; b < 3; ++b) S[3 * a + b] = Vi[3 * a + b] + (Vi[3 * a] * Y[b] + Vi[3 * a + 1] * Y[3 + b] + Vi[3 * a + 2] * Y[6 + b]);
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int b = 0; b < 3; ++b) o[3 * a + b] = 0.5 * (S[3 * a + b] + S[3 * b + a]);
        return;
    }
    // COV_JOB_POSE_POINT: Sigma_il = -(sum_s Sigma_{i,s} W_s) V^-1 (6 x 3), or its transpose
    double Z[18];
#pragma unroll
    for (int e = 0; e < 18; ++e) Z[e] = 0.0;
    for (int s = 0; s < ob.count(); ++s) {
        if (!ob.has(s)) continue;
        const int fs = d.pose_free[ob.pose(d, s)];
        if (fs < 0) continue;
        double W[18];
        cov_obs_w(d, ob, s, px, py, pz, W);
        for (int r = 0; r < 6; ++r)
#pragma unroll
            for (int c = 0; c < 6; ++c) {
                const double sg = cov_sig(src, J.a, fs, r, c);
                Z[3 * r] = fma(sg, W[3 * c], Z[3 * r]);
                Z[3 * r + 1] = fma(sg, W[3 * c + 1], Z[3 * r + 1]);
                Z[3 * r + 2] = fma(sg, W[3 * c + 2], Z[3 * r + 2]);
            }
    }
    for (int r = 0; r < 6; ++r)
#pragma unroll
        for (int b = 0; b < 3; ++b) {
            const double v = -(Z[3 * r] * Vi[b] + Z[3 * r + 1] * Vi[3 + b] + Z[3 * r + 2] * Vi[6 + b]);
            if (J.tr) o[6 * b + r] = v; else o[3 * r + b] = v;
        }
}

void launch_cov_jobs(Launcher &L, const Dev &d, const CovSrc &src, const CovJob *jobs, int n, double *out, int *fail) {
    if (d.dense) LAUNCH(KC_SMALL, k_cov_jobs<true>, dim3((n + 255) / 256), dim3(256), 0, d, src, jobs, n, out, fail);
    else LAUNCH(KC_SMALL, k_cov_jobs<false>, dim3((n + 255) / 256), dim3(256), 0, d, src, jobs, n, out, fail);
}

// columns 6q + c (q < nq) of the multi-right-hand-side solution Zb (rows x NBP) -> column slots slot0 + q of cols
__global__ __launch_bounds__(256) void k_cov_gather(const double *__restrict__ Zb, double *__restrict__ cols, int slot0, int nq, long nrow) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long)nq * 6 * nrow) return;
    const long row = e % nrow, qc = e / nrow;      // qc = 6 q + c
    cols[((long)slot0 * 6 + qc) * nrow + row] = Zb[row * NBP + qc];
}

void launch_cov_gather(Launcher &L, const double *Zb, double *cols, int slot0, int nq, long nrow) {
    const long n = (long)nq * 6 * nrow;
    LAUNCH(KC_SMALL, k_cov_gather, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, Zb, cols, slot0, nq, nrow);
}

}  // namespace ssba
