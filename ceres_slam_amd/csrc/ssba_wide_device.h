// Tile helpers of the 144-row super-block kernels (ssba_wide.hip, ssba_wide_covariance.hip): 16 x 16 tiles on
// v_mfma_f64_16x16x4_f64 in accumulator layout (register q of lane (g, j) = row 4 q + g, column j), the factorisation of a
// diagonal tile with its sub-step operands, and the 144-row product of the reduction.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include "ssba_types.h"

namespace ssba {

typedef double wd4 __attribute__((ext_vector_type(4)));
static __device__ __forceinline__ wd4 wmf(double a, double b, wd4 c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }
static __device__ __forceinline__ double wd_readlane(double v, int lane) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), lane);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
    return __hiloint2double(hi, lo);
}
// slab tiles: row tile i <= column tile j <= WNT (column tile WNT = the gradient column); upper tiles of a 9 x 9 block
static __host__ __device__ __forceinline__ int wd_slab_tile(int i, int j) { return i * (WNT + 1) - (i * (i - 1)) / 2 + (j - i); }
static __host__ __device__ __forceinline__ int wd_utile(int i, int j) { return i * WNT - (i * (i - 1)) / 2 + (j - i); }

// Lanes of ONE wave hand values to each other through LDS below (the LDS unit serves a wave's requests in issue order, so no
// hardware wait is needed) -- but to the compiler a lane that skips a predicated store has not changed memory, and it reuses
// what it loaded before the store (measured: the loads were sunk into the `if (lane < 16)` block, the other 48 lanes read
// stale registers).  A compiler-level memory barrier makes it store what is pending and load again.
#define WD_WAVE_LDS_SYNC() do { asm volatile("" ::: "memory"); } while (0)

constexpr int WF_THREADS = 512;
constexpr int WF_NU = WNT * (WNT + 1) / 2;      // 45 upper tiles of U
// U tiles | U_kk^-T tiles (decoupled step) | sub-step operands P, Q of two diagonal tiles | 1 / sqrt(pivot) of two | y | x | t
constexpr int WF_OFF_W = WF_NU * 256, WF_OFF_P = WF_OFF_W + WNT * 256, WF_OFF_Q = WF_OFF_P + 2 * 256, WF_OFF_RS = WF_OFF_Q + 2 * 256,
              WF_OFF_Y = WF_OFF_RS + 32, WF_OFF_X = WF_OFF_Y + WBD, WF_OFF_T = WF_OFF_X + WBD;
constexpr int WF_LDS_DOUBLES = WF_OFF_T + 16;

// Diagonal tile T (16 x 16, accumulator layout: register q of lane (g, j) = row 4 q + g, column j), four sub-steps of four
// pivots -- the scheme of ssba_bcr_mfma.hip's factor_tile: the 4 x 4 pivot block is factored LDL^T "uniformly" (every lane
// computes the same scalars from v_readlane copies; the serial chain is four reciprocals), the inverse M of its unit-lower
// factor becomes the A operand P of ONE instruction  c = M T[rows]  and the scaled pivot rows Q = -c / d the A operand of ONE
// instruction that updates the rows below.  Every other tile of the block row (panel tiles, right-hand sides) follows with the
// same two operands per sub-step (wd_apply).  Rows stay in the LDL^T scaling; rs = 1 / sqrt(d) normalises them afterwards.
// sP / sQ: [sub-step][lane]; srs: 16 reciprocal square roots.  Returns false on a non-positive / non-finite pivot.
static __device__ __forceinline__ bool wd_factor_tile(wd4 &T, double *__restrict__ sP, double *__restrict__ sQ, double *__restrict__ srs, int lane) {
    const int g = lane >> 4, j = lane & 15;
    const double kDiag = (j < 4 && g == j) ? 1.0 : 0.0, k10 = (j == 1 && g == 0) ? 1.0 : 0.0, k20 = (j == 2 && g == 0) ? 1.0 : 0.0,
                 k21 = (j == 2 && g == 1) ? 1.0 : 0.0, k30 = (j == 3 && g == 0) ? 1.0 : 0.0, k31 = (j == 3 && g == 1) ? 1.0 : 0.0,
                 k32 = (j == 3 && g == 2) ? 1.0 : 0.0;
    const double kG0 = g == 0 ? 1.0 : 0.0, kG1 = g == 1 ? 1.0 : 0.0, kG2 = g == 2 ? 1.0 : 0.0, kG3 = g == 3 ? 1.0 : 0.0;
    bool ok = true;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int b = 4 * r;      // S[a][c] = T[4r + a][4r + c] sits in register r of lane 16 a + 4r + c
        const double tr = T[r];
        const double s00 = wd_readlane(tr, b), s10 = wd_readlane(tr, 16 + b), s20 = wd_readlane(tr, 32 + b), s30 = wd_readlane(tr, 48 + b);
        const double s11 = wd_readlane(tr, 16 + b + 1);
        double s21 = wd_readlane(tr, 32 + b + 1), s31 = wd_readlane(tr, 48 + b + 1);
        const double s22 = wd_readlane(tr, 32 + b + 2);
        double s32 = wd_readlane(tr, 48 + b + 2);
        const double s33 = wd_readlane(tr, 48 + b + 3);
        const double x0 = __builtin_amdgcn_rcp(s00), e0 = fma(-s00, x0, 1.0);
        const double t10 = s10 * x0, t20 = s20 * x0, t30 = s30 * x0;
        const double l10 = fma(t10, e0, t10), l20 = fma(t20, e0, t20), l30 = fma(t30, e0, t30);
        const double d1 = fma(-s10, l10, s11);
        s21 = fma(-s20, l10, s21); s31 = fma(-s30, l10, s31);
        const double x1 = __builtin_amdgcn_rcp(d1), e1 = fma(-d1, x1, 1.0);
        const double t21 = s21 * x1, t31 = s31 * x1;
        const double l21 = fma(t21, e1, t21), l31 = fma(t31, e1, t31);
        const double d2 = fma(-s21, l21, fma(-s20, l20, s22));
        s32 = fma(-s31, l21, fma(-s30, l20, s32));
        const double x2 = __builtin_amdgcn_rcp(d2), e2 = fma(-d2, x2, 1.0);
        const double t32 = s32 * x2;
        const double l32 = fma(t32, e2, t32);
        const double d3 = fma(-s32, l32, fma(-s31, l31, fma(-s30, l30, s33)));
        const double x3 = __builtin_amdgcn_rcp(d3), e3 = fma(-d3, x3, 1.0);
        const double rc0 = fma(x0, e0, x0), rc1 = fma(x1, e1, x1), rc2 = fma(x2, e2, x2), rc3 = fma(x3, e3, x3);
        ok = ok && rc0 > 0.0 && rc1 > 0.0 && rc2 > 0.0 && rc3 > 0.0 && rc0 < INFINITY && rc1 < INFINITY && rc2 < INFINITY && rc3 < INFINITY;
        // M = l^-1 (unit lower); P: lane (g, i = j) holds M[i][g] for i < 4
        const double n20 = fma(l21, l10, -l20);
        const double n31 = fma(l32, l21, -l31);
        const double n30 = -fma(l32, n20, fma(l31, -l10, l30));
        double Pv = fma(-l10, k10, kDiag);
        Pv = fma(n20, k20, Pv);
        Pv = fma(-l21, k21, Pv);
        Pv = fma(n31, k31, Pv);
        Pv = fma(-l32, k32, Pv);
        Pv = fma(n30, k30, Pv);
        const wd4 y4 = wmf(Pv, tr, wd4{0.0, 0.0, 0.0, 0.0});
        const double rcg = fma(rc3, kG3, fma(rc2, kG2, fma(rc1, kG1, rc0 * kG0)));
        const double qs = (j > b + 3) ? -rcg : 0.0;
        const double y = y4[0];             // lane (g, j): unnormalised pivot row c_g[j]
        T[r] = y;
        const double Qv = y * qs;
        if (r < 3) T = wmf(Qv, y, T);
        sP[r * 64 + lane] = Pv;
        sQ[r * 64 + lane] = Qv;
        if (j == 0) srs[b + g] = sqrt(rcg);
    }
    return ok;
}
// the four sub-steps on another tile of the block row (accumulator layout), then the rows normalised by 1 / sqrt(pivot)
static __device__ __forceinline__ void wd_apply(wd4 &X, const double *__restrict__ sP, const double *__restrict__ sQ, const double *__restrict__ srs, int lane) {
    double P[4], Q[4], rs[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) { P[r] = sP[r * 64 + lane]; Q[r] = sQ[r * 64 + lane]; rs[r] = srs[4 * r + (lane >> 4)]; }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const wd4 y4 = wmf(P[r], X[r], wd4{0.0, 0.0, 0.0, 0.0});
        X[r] = y4[0];
        if (r < 3) X = wmf(Q[r], y4[0], X);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) X[r] *= rs[r];
}
static __device__ __forceinline__ wd4 wd_tile_load(const double *__restrict__ T, int lane) {
    wd4 v;
#pragma unroll
    for (int q = 0; q < 4; ++q) v[q] = T[(4 * q + (lane >> 4)) * 16 + (lane & 15)];
    return v;
}
static __device__ __forceinline__ void wd_tile_store(double *__restrict__ T, const wd4 &v, int lane) {
#pragma unroll
    for (int q = 0; q < 4; ++q) T[(4 * q + (lane >> 4)) * 16 + (lane & 15)] = v[q];
}
// T_ij -= U_ki^T U_kj  (normalised row tiles, row-major in LDS); returns the updated tile
static __device__ __forceinline__ wd4 wd_tile_update(const double *__restrict__ Uki, const double *__restrict__ Ukj, const double *__restrict__ Tij, int lane) {
    const int kq = lane >> 4, i = lane & 15;
    double a[4], b[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) { a[s] = -Uki[(4 * s + kq) * 16 + i]; b[s] = Ukj[(4 * s + kq) * 16 + i]; }
    wd4 acc = wd_tile_load(Tij, lane);
#pragma unroll
    for (int s = 0; s < 4; ++s) acc = wmf(a[s], b[s], acc);
    return acc;
}

// acc -= A[:, 16 ti ..]^T B[:, 16 tj ..]  over the 144 rows (B = a vector in column 0 when bvec)
static __device__ __forceinline__ wd4 wd_product(const double *__restrict__ A, const double *__restrict__ B, int ti, int tj, bool bvec, wd4 acc, int lane) {
    const int kq = lane >> 4, i = lane & 15;
    const double *pa = A + (size_t)kq * WBD + 16 * ti + i;
    double a[WBD / 4], b[WBD / 4];
    if (bvec) {
#pragma unroll
        for (int ks = 0; ks < WBD / 4; ++ks) { a[ks] = pa[(size_t)4 * ks * WBD]; b[ks] = i == 0 ? B[4 * ks + kq] : 0.0; }
    } else {
        const double *pb = B + (size_t)kq * WBD + 16 * tj + i;
#pragma unroll
        for (int ks = 0; ks < WBD / 4; ++ks) { a[ks] = pa[(size_t)4 * ks * WBD]; b[ks] = pb[(size_t)4 * ks * WBD]; }
    }
#pragma unroll
    for (int ks = 0; ks < WBD / 4; ++ks) acc = wmf(-a[ks], b[ks], acc);
    return acc;
}

}  // namespace ssba
