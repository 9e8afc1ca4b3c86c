// Columns of Sigma = S^-1 on the 144-row super-blocks of long tracks (ssba_wide.hip), for the covariance entries on a wide
// handle that has been solved: a panel R of up to WPC = 48 right-hand-side columns (the unit columns of 8 free poses) goes
// through the same parallel cyclic reduction that the solve runs for one vector.
//
//   k_wdc_rhs        the unit columns of the sweep's poses into the panel R (n x 144 x 48, row-major)
//   k_wdc_factor<0>  step s, block e:  D_e = U^T U  and  [YL | YU | Yr] = U^-T [S(e, e-s) | S(e, e+s) | R_e].  The column tiles
//                    are dealt as in k_wd_factor, c = part + 3 (wave - 1): 9 of L, 9 of U and the 3 panel tiles fill the 21
//                    slots of three workgroups; a panel tile is nine 16 x 16 accumulator tiles of its wave, as the vector was
//   k_wdc_reduce     one wave per output tile:  D', S'(e, e -+ 2s) as k_wd_reduce forms them, and
//                    R'(e) = R(e) - YU(e-s)^T Yr(e-s) - YL(e+s)^T Yr(e+s)  as full 16-column tile products
//   k_wdc_factor<1>  the decoupled blocks: factor, forward solve of the three panel tiles (waves 1..3), and the backward solve
//                    X_k = U_kk^-1 (Y_k - sum_{j > k} U_kj X_j)  on the matrix cores with the panel still in the accumulator
//                    registers of its wave (a 144 x 48 panel does not fit into LDS beside the factor); the columns go to the
//                    column store that k_cov_jobs reads (column c at cols + c * nrow)
// The system is the one k_wd_schur / k_wd_assemble / k_wd_finish leave (D, L, in place); the reduction overwrites it, as in a
// solve, and every sweep assembles it again.  No atomics: every element has one writer, a call is bit-reproducible.
#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>
#include <stdint.h>

#include "ssba_device.h"
#include "ssba_launch.h"
#include "ssba_types.h"
#include "ssba_wide_device.h"

namespace ssba {

struct WdcPoses { int f[WPC / 6]; };

__global__ __launch_bounds__(256) void k_wdc_rhs(Dev d, WdcPoses ps, int nq) {
    const WideSys &w = *d.wide;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)w.n * WBD * WPC) return;
    const size_t row = i / WPC;
    const int col = (int)(i - row * WPC), q = col / 6, c = col - 6 * q;
    w.Rp[i] = (q < nq && row == (size_t)ps.f[q] * 6 + c) ? 1.0 : 0.0;
}

// FINAL = 0: a step of the reduction (grid n x ng);  FINAL = 1: the decoupled last step (grid n).  The factorisation of the
// block is k_wd_factor's, schedule included (look-ahead of the pivot wave, its SIMD partner wave 4 takes no trailing tiles);
// ncol: columns of the panel in use (tiles beyond them are not carried).
template <int FINAL>
__global__ __launch_bounds__(WF_THREADS) void k_wdc_factor(Dev d, int step, int ng, int ncol, double *__restrict__ cols, long nrow, int col0) {
    const WideSys &w = *d.wide;
    const StateFlags sf = state_flags_vmem(d.st);
    extern __shared__ __align__(16) double wf_lds[];
    double *sU = wf_lds, *sW = wf_lds + WF_OFF_W, *sP = wf_lds + WF_OFF_P, *sQ = wf_lds + WF_OFF_Q, *sRS = wf_lds + WF_OFF_RS;
    __shared__ int s_bad;
    const int e = (int)blockIdx.x / ng, part = (int)blockIdx.x - e * ng;
    const int n = w.n, s = 1 << step;
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6, g = lane >> 4, jj = lane & 15;
    const size_t blk = (size_t)WBD * WBD, pblk = (size_t)WBD * WPC;
    const bool hasL = !FINAL && e - s >= 0, hasU = !FINAL && e + s < n;
    const double *Dg = w.xw + (size_t)e * blk;
    const double *Lg = w.xw + w.off_L + (size_t)e * blk;
    // S(e, e + s): the transpose of L[e + 1] in the first step, the reduce kernel's output afterwards
    const double *Ug = step == 0 ? w.xw + w.off_L + (size_t)(hasU ? e + 1 : e) * blk : w.U + (size_t)e * blk;
    // this wave's column tile of [L | U | R]: 0..8, 9..17, 18..20 (wave 0 factors the diagonal tiles: it carries none)
    const int c = wv == 0 ? -1 : FINAL ? (wv <= WPT ? 2 * WNT + wv - 1 : -1) : part + ng * (wv - 1);
    const int tp = c - 2 * WNT;        // panel tile, when >= 0
    const bool act = c >= 0 && c < 2 * WNT + WPT && (c < WNT ? hasL : c < 2 * WNT ? hasU : 16 * tp < ncol);
    if (t == 0) s_bad = 0;
    wd4 rt[WNT];
#pragma unroll
    for (int j = 0; j < WNT; ++j) rt[j] = wd4{0.0, 0.0, 0.0, 0.0};
    if (act) {
        if (c >= 2 * WNT) {
            const double *pp = w.Rp + (size_t)e * pblk + (size_t)g * WPC + 16 * tp + jj;
#pragma unroll
            for (int j = 0; j < WNT; ++j)
#pragma unroll
                for (int q = 0; q < 4; ++q) rt[j][q] = pp[(16 * j + 4 * q) * WPC];
        } else if (c < WNT) {
            const double *pp = Lg + (size_t)g * WBD + 16 * c + jj;
#pragma unroll
            for (int j = 0; j < WNT; ++j)
#pragma unroll
                for (int q = 0; q < 4; ++q) rt[j][q] = pp[(16 * j + 4 * q) * WBD];
        } else if (step == 0) {
            const double *pp = Ug + (size_t)(16 * (c - WNT) + jj) * WBD + g;
#pragma unroll
            for (int j = 0; j < WNT; ++j)
#pragma unroll
                for (int q = 0; q < 4; ++q) rt[j][q] = pp[16 * j + 4 * q];
        } else {
            const double *pp = Ug + (size_t)g * WBD + 16 * (c - WNT) + jj;
#pragma unroll
            for (int j = 0; j < WNT; ++j)
#pragma unroll
                for (int q = 0; q < 4; ++q) rt[j][q] = pp[(16 * j + 4 * q) * WBD];
        }
    }
    // upper tiles of D into LDS, tile by tile (row-major 16 x 16); wave 0 keeps the first diagonal tile in registers
    wd4 dg = {0.0, 0.0, 0.0, 0.0};
    {
        constexpr int WF_TPW = (WF_NU + 7) / 8;       // tiles per wave: 6
        wd4 v[WF_TPW];
#pragma unroll
        for (int m = 0; m < WF_TPW; ++m) {
            const int tl = wv + 8 * m;
            if (tl < WF_NU) {
                int ti = 0, rem = tl;                   // tile tl = (ti, tj) of the upper triangle, row by row
                while (rem >= WNT - ti) { rem -= WNT - ti; ++ti; }
                const int tj = ti + rem;
                const double *pp = Dg + (size_t)(16 * ti + g) * WBD + 16 * tj + jj;
#pragma unroll
                for (int q = 0; q < 4; ++q) v[m][q] = pp[(size_t)4 * q * WBD];
            }
        }
#pragma unroll
        for (int m = 0; m < WF_TPW; ++m) {
            const int tl = wv + 8 * m;
            if (tl >= WF_NU) continue;
            if (tl == 0) dg = v[m];
            else wd_tile_store(sU + tl * 256, v[m], lane);
        }
    }
    if (sf.dead()) return;
    if (wv == 0) {
        if (!wd_factor_tile(dg, sP, sQ, sRS, lane)) s_bad = 1;
    }
    __syncthreads();

#pragma unroll
    for (int k = 0; k < WNT; ++k) {
        const double *kP = sP + (k & 1) * 256, *kQ = sQ + (k & 1) * 256, *kRS = sRS + (k & 1) * 16;
        // (b) the panel tiles of block row k of U (one per wave)
        {
            const int j = k + 1 + wv;
            if (j < WNT) {
                wd4 x = wd_tile_load(sU + wd_utile(k, j) * 256, lane);
                wd_apply(x, kP, kQ, kRS, lane);
                wd_tile_store(sU + wd_utile(k, j) * 256, x, lane);
            }
            if (FINAL && wv == 5) {        // U_kk^-T (row-major) for the backward solve: the sub-steps applied to the identity
                wd4 x;
#pragma unroll
                for (int q = 0; q < 4; ++q) x[q] = (4 * q + g == jj) ? 1.0 : 0.0;
                wd_apply(x, kP, kQ, kRS, lane);
                wd_tile_store(sW + k * 256, x, lane);
            }
        }
        __syncthreads();
        // (c) wave 0: diagonal tile k + 1, updated and factored at once; the others: the rest of the trailing tiles
        //     (i, j), k < i <= j, and the right-hand sides from block row k down
        if (wv == 0) {
            if (k + 1 < WNT) {
                wd4 x = wd_tile_update(sU + wd_utile(k, k + 1) * 256, sU + wd_utile(k, k + 1) * 256, sU + wd_utile(k + 1, k + 1) * 256, lane);
                if (!wd_factor_tile(x, sP + ((k + 1) & 1) * 256, sQ + ((k + 1) & 1) * 256, sRS + ((k + 1) & 1) * 16, lane)) s_bad = 1;
            }
        } else {
            int cnt = -1;
#pragma unroll
            for (int i = k + 1; i < WNT; ++i)
#pragma unroll
                for (int j = i; j < WNT; ++j, ++cnt) {
                    if (cnt < 0) continue;          // (k + 1, k + 1) is wave 0's
                    if (wv != 4 && cnt % 6 == (wv < 4 ? wv - 1 : wv - 2)) {     // wave 4 shares its SIMD with the pivot wave
                        const wd4 x = wd_tile_update(sU + wd_utile(k, i) * 256, sU + wd_utile(k, j) * 256, sU + wd_utile(i, j) * 256, lane);
                        wd_tile_store(sU + wd_utile(i, j) * 256, x, lane);
                    }
                }
            if (act) {
                wd_apply(rt[k], kP, kQ, kRS, lane);
#pragma unroll
                for (int j = k + 1; j < WNT; ++j) {
                    double a[4];
#pragma unroll
                    for (int q = 0; q < 4; ++q) a[q] = -sU[wd_utile(k, j) * 256 + (4 * q + g) * 16 + jj];
#pragma unroll
                    for (int q = 0; q < 4; ++q) rt[j] = wmf(a[q], rt[k][q], rt[j]);
                }
            }
        }
        __syncthreads();
    }
    if (s_bad) {        // non-positive pivot: the system is not positive definite
        if (t == 0) d.st->step_failed = 1;
        return;
    }
    if (!act) return;
    if (!FINAL) {
        if (c >= 2 * WNT) {
            double *pp = w.Yp + (size_t)e * pblk + (size_t)g * WPC + 16 * tp + jj;
#pragma unroll
            for (int j = 0; j < WNT; ++j)
#pragma unroll
                for (int q = 0; q < 4; ++q) pp[(16 * j + 4 * q) * WPC] = rt[j][q];
        } else {
            double *pp = (c < WNT ? w.YL : w.YU) + (size_t)e * blk + (size_t)g * WBD + 16 * (c < WNT ? c : c - WNT) + jj;
#pragma unroll
            for (int j = 0; j < WNT; ++j)
#pragma unroll
                for (int q = 0; q < 4; ++q) pp[(16 * j + 4 * q) * WBD] = rt[j][q];
        }
        return;
    }
    // ---- decoupled block: U X = Y by block rows from the bottom; rt[j] holds Y_j, then X_j.  A operand of lane (g, jj) in
    //      k-step q: element (jj, 4 q + g) of U_kj, or of U_kk^-1 = (sW tile k)^T; B operand: register q of the tile
#pragma unroll
    for (int k = WNT - 1; k >= 0; --k) {
        wd4 acc = rt[k];
#pragma unroll
        for (int j = k + 1; j < WNT; ++j) {
            double a[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) a[q] = -sU[wd_utile(k, j) * 256 + jj * 16 + 4 * q + g];
#pragma unroll
            for (int q = 0; q < 4; ++q) acc = wmf(a[q], rt[j][q], acc);
        }
        double a[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) a[q] = sW[k * 256 + (4 * q + g) * 16 + jj];
        wd4 x = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int q = 0; q < 4; ++q) x = wmf(a[q], acc[q], x);
        rt[k] = x;
    }
    if (16 * tp + jj < ncol) {
        double *pc = cols + (size_t)(col0 + 16 * tp + jj) * (size_t)nrow + (size_t)e * WBD + g;
#pragma unroll
        for (int j = 0; j < WNT; ++j)
#pragma unroll
            for (int q = 0; q < 4; ++q) pc[16 * j + 4 * q] = rt[j][q];
    }
}

// one wave per 16 x 16 output tile of block e: jobs 0..44 tiles of D' (upper), 45..71 tiles of R' (block row, panel tile),
// 72..152 tiles of S'(e, e - 2s), 153..233 tiles of S'(e, e + 2s)
constexpr int WCR_JOBS = WF_NU + WNT * WPT + 2 * WNT * WNT;       // 234
constexpr int WCR_WG_PER_BLOCK = (WCR_JOBS + 3) / 4;              // 59 workgroups of four waves (two idle waves)

// acc -= A[:, 16 ti ..]^T B[:, 16 tp ..]  over the 144 rows, B a panel (row stride WPC)
static __device__ __forceinline__ wd4 wdc_product(const double *__restrict__ A, const double *__restrict__ B, int ti, int tp, wd4 acc, int lane) {
    const int kq = lane >> 4, i = lane & 15;
    const double *pa = A + (size_t)kq * WBD + 16 * ti + i;
    const double *pb = B + (size_t)kq * WPC + 16 * tp + i;
    double a[WBD / 4], b[WBD / 4];
#pragma unroll
    for (int ks = 0; ks < WBD / 4; ++ks) { a[ks] = pa[(size_t)4 * ks * WBD]; b[ks] = pb[(size_t)4 * ks * WPC]; }
#pragma unroll
    for (int ks = 0; ks < WBD / 4; ++ks) acc = wmf(-a[ks], b[ks], acc);
    return acc;
}

__global__ __launch_bounds__(256, 2) void k_wdc_reduce(Dev d, int step, int ncol) {
    const WideSys &w = *d.wide;
    const StateFlags sf = state_flags_vmem(d.st);
    const int e = (int)blockIdx.x / WCR_WG_PER_BLOCK;
    const int lane = threadIdx.x & 63, g = lane >> 4, jj = lane & 15;
    const int job = ((int)blockIdx.x - e * WCR_WG_PER_BLOCK) * 4 + (threadIdx.x >> 6);
    const int n = w.n, s = 1 << step, prev = e - s, next = e + s;
    const size_t blk = (size_t)WBD * WBD, pblk = (size_t)WBD * WPC;
    const bool hasP = prev >= 0, hasN = next < n;
    if (sf.dead() || job >= WCR_JOBS) return;
    if (job < WF_NU) {
        if (!hasP && !hasN) return;
        int ti = 0, q0 = job;
        while (q0 >= WNT - ti) { q0 -= WNT - ti; ++ti; }
        const int tj = ti + q0;
        double *out = w.xw + (size_t)e * blk + (size_t)(16 * ti + g) * WBD + 16 * tj + jj;
        wd4 acc;
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[q] = out[(size_t)4 * q * WBD];
        if (hasP) acc = wd_product(w.YU + (size_t)prev * blk, w.YU + (size_t)prev * blk, ti, tj, false, acc, lane);
        if (hasN) acc = wd_product(w.YL + (size_t)next * blk, w.YL + (size_t)next * blk, ti, tj, false, acc, lane);
#pragma unroll
        for (int q = 0; q < 4; ++q) out[(size_t)4 * q * WBD] = acc[q];
        return;
    }
    if (job < WF_NU + WNT * WPT) {
        const int q0 = job - WF_NU, ti = q0 / WPT, tp = q0 - ti * WPT;
        if ((!hasP && !hasN) || 16 * tp >= ncol) return;
        double *out = w.Rp + (size_t)e * pblk + (size_t)(16 * ti + g) * WPC + 16 * tp + jj;
        wd4 acc;
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[q] = out[(size_t)4 * q * WPC];
        if (hasP) acc = wdc_product(w.YU + (size_t)prev * blk, w.Yp + (size_t)prev * pblk, ti, tp, acc, lane);
        if (hasN) acc = wdc_product(w.YL + (size_t)next * blk, w.Yp + (size_t)next * pblk, ti, tp, acc, lane);
#pragma unroll
        for (int q = 0; q < 4; ++q) out[(size_t)4 * q * WPC] = acc[q];
        return;
    }
    const bool lower = job < WF_NU + WNT * WPT + WNT * WNT;
    const int q2 = job - (WF_NU + WNT * WPT) - (lower ? 0 : WNT * WNT);
    const int ti = q2 / WNT, tj = q2 - ti * WNT;
    wd4 acc = {0.0, 0.0, 0.0, 0.0};
    double *out;
    if (lower) {        // S'(e, e - 2s) = -YU(prev)^T YL(prev): needs prev and its own lower neighbour
        if (!hasP || prev - s < 0) return;
        acc = wd_product(w.YU + (size_t)prev * blk, w.YL + (size_t)prev * blk, ti, tj, false, acc, lane);
        out = w.xw + w.off_L + (size_t)e * blk;
    } else {            // S'(e, e + 2s) = -YL(next)^T YU(next)
        if (!hasN || next + s >= n) return;
        acc = wd_product(w.YL + (size_t)next * blk, w.YU + (size_t)next * blk, ti, tj, false, acc, lane);
        out = w.U + (size_t)e * blk;
    }
    out += (size_t)(16 * ti + g) * WBD + 16 * tj + jj;
#pragma unroll
    for (int q = 0; q < 4; ++q) out[(size_t)4 * q * WBD] = acc[q];
}

// ---- host side ---------------------------------------------------------------------------------------------------
int configure_wide_panel() {
    if (hipFuncSetAttribute((const void *)k_wdc_factor<0>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(WF_LDS_DOUBLES * sizeof(double))) != hipSuccess) return -1;
    return hipFuncSetAttribute((const void *)k_wdc_factor<1>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(WF_LDS_DOUBLES * sizeof(double))) == hipSuccess ? 0 : -1;
}
// The unit columns of nq <= WPC / 6 free poses through the reduction of the assembled system: column 6 q + c of pose q lands at
// cols + (col0 + 6 q + c) * nrow, nrow >= n * WBD rows each (row 6 f + r: free pose f).
void launch_wide_solve_panel(Launcher &L, const Dev &d, const int *free_pose, int nq, double *cols, long nrow, int col0) {
    const WideSys &w = L.wide;
    const int ng = 3, ncol = 6 * nq;
    WdcPoses ps{};
    for (int q = 0; q < nq; ++q) ps.f[q] = free_pose[q];
    LAUNCH(KC_SMALL, k_wdc_rhs, dim3((unsigned)(((size_t)w.n * WBD * WPC + 255) / 256)), dim3(256), 0, d, ps, nq);
    for (int q = 0; q < w.steps; ++q) {
        LAUNCH(KC_BCR_FACTOR, k_wdc_factor<0>, dim3(w.n * ng), dim3(WF_THREADS), WF_LDS_DOUBLES * sizeof(double), d, q, ng, ncol, cols, nrow, col0);
        LAUNCH(KC_BCR_REDUCE, k_wdc_reduce, dim3(w.n * WCR_WG_PER_BLOCK), dim3(256), 0, d, q, ncol);
    }
    LAUNCH(KC_BCR_FACTOR, k_wdc_factor<1>, dim3(w.n), dim3(WF_THREADS), WF_LDS_DOUBLES * sizeof(double), d, w.steps, 1, ncol, cols, nrow, col0);
}

}  // namespace ssba
