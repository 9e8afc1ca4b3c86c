// Block cyclic reduction (BCR) of the block-tridiagonal reduced camera system S on gfx950.
//
// S has Nsb diagonal blocks D_i (BD x BD, BD = 72 = 12 poses) and couplings L_i = S[i, i-1].
// Level l eliminates its odd blocks (all in parallel):
//   factor  (odd i):  D_i = G G^T ; YL = G^-1 L_i ; YU = G^-1 L_{i+1}^T ; yr = G^-1 r_i
//   reduce  (even e): D' = D_e - YU(e-1)^T YU(e-1) - YL(e+1)^T YL(e+1)
//                     L' = -YU(e-1)^T YL(e-1) ;  r' = r_e - YU(e-1)^T yr(e-1) - YL(e+1)^T yr(e+1)
//   k_bcr_backsub (odd i):  x_i = G^-T (yr - YL x_{i-1} - YU x_{i+1})      (top-down)
// and recurses on the even blocks; the last level (one block) is a plain Cholesky solve.  The factor and reduce kernels
// run on the matrix cores (ssba_bcr_mfma.hip, k_bcr_factor_mf / k_bcr_reduce_mf).
// From the first level with <= PCR_MAX_BLOCKS blocks on, the same kernels run PARALLEL cyclic reduction (which = 2,
// PcrPlan): at stride 2^k every block is factored and folds in both neighbours at +-2^k, so after log2(n) steps the
// blocks are decoupled and one factor + solve over all of them finishes -- no back-substitution sweep over those levels.
// G (with 1/G_kk on its diagonal), YL and yr overwrite D_i, L_i and r_i in place.
// Coupling blocks with an EVEN index are only ever consumed transposed (as L_{i+1}^T of the
// odd block before them), so they are stored transposed at every level: the factor kernel
// then stages all three operands with plain row-major copies (no LDS transpose).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <stdlib.h>

#include "ssba_launch.h"
#include "ssba_types.h"

namespace ssba {

// copy of one block, all reads of a lane in flight before its first store (nthreads is a launch constant: >= 448)
__device__ __forceinline__ void stage_block(double *dst, const double *__restrict__ src, int nthreads) {
    const double2 *s2 = reinterpret_cast<const double2 *>(src);
    double2 *d2 = reinterpret_cast<double2 *>(dst);
    constexpr int NLD = (BD * BD / 2 + 447) / 448;     // 6
    double2 v[NLD];
#pragma unroll
    for (int q = 0; q < NLD; ++q) {
        const int e = threadIdx.x + q * nthreads;
        v[q] = e < BD * BD / 2 ? s2[e] : make_double2(0.0, 0.0);
    }
#pragma unroll
    for (int q = 0; q < NLD; ++q) {
        const int e = threadIdx.x + q * nthreads;
        if (e < BD * BD / 2) d2[e] = v[q];
    }
}

__device__ __forceinline__ double lane_bcast(double v, int lane) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), lane);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
    return __hiloint2double(hi, lo);
}

// x_i = G^-T (yr - YL x_{i-1} - YU x_{i+1}); x lives in d.x0 at level-0 block positions.
// G, YL, YU are staged into LDS with one coalesced sweep.
constexpr int BS_THREADS = 512;
__global__ __launch_bounds__(BS_THREADS) void k_bcr_backsub(Dev d, int lev, int top, int which) {
    const State &st = *d.st;
    const int dead = st.terminated | st.step_failed | st.dl_reuse;      // tested once the staging reads are in flight (a cold read)
    extern __shared__ __align__(16) double lds[];
    double *sG = lds, *sL = lds + BD * BD, *sU = lds + 2 * BD * BD;
    __shared__ double sv[BD], sxm[BD], sxp[BD];
    // which = 2 / 3: last step of the parallel cyclic reduction -- every block of the plan's level is decoupled from the
    // others; in a chain with pinned ends (partitioned solve) it still has its couplings to those (x known by now)
    const bool pcr = which >= 2;
    const PcrPlan &P = which == 3 ? d.spcr : d.pcr;
    const BcrLevel &L = which == 3 ? d.slev[0] : d.lev[pcr ? d.pcr.level : lev];
    const int blk = pcr ? (int)blockIdx.x : (top ? 0 : 2 * blockIdx.x + 1);
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    if (pcr && ((P.pin0 && blk == 0) || (P.pin1 && blk == L.n - 1))) return;
    const bool hasL = pcr ? (P.pin0 != 0) : !top;
    const bool hasU = pcr ? (P.pin1 != 0) : (!top && (blk + 1 < L.n));
    const int iL = pcr ? 0 : blk - 1, iU = pcr ? L.n - 1 : blk + 1;
    double *xb = which == 3 ? d.xsep : d.x0 + (size_t)d.chain0 * BD;     // solution at level-0 block positions
    double *xi = xb + (size_t)L.pos[blk] * BD;
    stage_block(sG, L.D + (size_t)blk * BD * BD, BS_THREADS);
    if (hasL) stage_block(sL, (pcr ? P.YL : L.L) + (size_t)blk * BD * BD, BS_THREADS);
    if (hasU) stage_block(sU, pcr ? P.YU + (size_t)blk * BD * BD : L.YU + (size_t)blockIdx.x * BD * BD, BS_THREADS);
    if (t < BD) {
        sxm[t] = hasL ? xb[(size_t)L.pos[iL] * BD + t] : 0.0;
        sxp[t] = hasU ? xb[(size_t)L.pos[iU] * BD + t] : 0.0;
        sv[t] = L.r[(size_t)blk * BD + t];
    }
    if (dead) return;
    __syncthreads();
    // v = yr - YL x_{i-1} - YU x_{i+1}: 8 waves x 9 rows, lanes stride the row
    for (int r = w * 9; r < w * 9 + 9; ++r) {
        double p = 0.0;
        if (hasL) {
            p += sL[r * BD + lane] * sxm[lane];
            if (lane < BD - 64) p += sL[r * BD + 64 + lane] * sxm[64 + lane];
        }
        if (hasU) {
            p += sU[r * BD + lane] * sxp[lane];
            if (lane < BD - 64) p += sU[r * BD + 64 + lane] * sxp[64 + lane];
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) p += __shfl_down(p, o, 64);
        if (lane == 0) sv[r] -= p;
    }
    __syncthreads();
    if (w != 0) return;
    // wave 0: solve G^T x = v by a column sweep from the bottom; the diagonal of G holds 1/G_kk.
    double lo = sv[lane];
    double hi = lane < BD - 64 ? sv[64 + lane] : 0.0;
#pragma unroll
    for (int k = BD - 1; k >= 64; --k) {
        const double xk = lane_bcast(hi, k - 64) * sG[k * BD + k];
        const double gl = sG[k * BD + lane];
        const double gh = (lane < k - 64) ? sG[k * BD + 64 + lane] : 0.0;
        lo -= gl * xk;
        hi = (lane == k - 64) ? xk : hi - gh * xk;
    }
#pragma unroll
    for (int k = 63; k >= 0; --k) {
        const double xk = lane_bcast(lo, k) * sG[k * BD + k];
        const double gl = (lane < k) ? sG[k * BD + lane] : 0.0;
        lo = (lane == k) ? xk : lo - gl * xk;
    }
    xi[lane] = lo;
    if (lane < BD - 64) xi[64 + lane] = hi;
}

// blocks eliminated at a level: all odd ones, except the pinned end of a partitioned chain
static int n_odd(const BcrLevel &lv, int pinned) { return pinned ? (lv.n - 1) / 2 : lv.n / 2; }

// The border columns (free shared blocks of config 3, closure border) go through the forward part of the solve INSIDE
// the matrix-core factor / reduce launches -- two more right-hand-side tiles -- instead of a forward + update launch per
// level afterwards (ssba_border.hip).  SSBA_BORDER_SWEEPS=1 keeps the separate sweeps (A/B, tests).  A border of two
// panels (nb > NBP) never rides: each panel takes the sweeps.
bool bcr_border_rides(const Dev &d) {
    const char *e = getenv("SSBA_BORDER_SWEEPS");        // read per call: tests switch it between handles
    return d.nb > 0 && d.nb <= NBP && !d.part && !d.dense && !(e && e[0] == '1');
}

// the decoupled last step of a plan that covers the whole chain can solve its blocks AND update their poses
static bool bcr_fused_solve(const Dev &d) {
    return !d.part && d.pcr.level >= 0 && d.nb == 0;
}
// the fused plan (PcrFused buffers allocated: single GPU, no border columns); SSBA_NO_PCR_FUSED=1 keeps factor + reduce launches (A/B, tests)
static bool bcr_fused_steps(const Dev &d) {
    const char *e = getenv("SSBA_NO_PCR_FUSED");        // read per call: tests switch it between handles
    return d.pcrf.on && !d.part && !d.pcr.keep && d.nb == 0 && !(e && e[0] == '1');
}
// Border columns riding through the parallel plan: the right-hand side of the decoupled last step is solved as column NBP - 1 (a
// padding column while nb < NBP) of the border columns' backward sweep -- k_bcrm_bwd does for 32 columns what k_bcr_backsub does for
// one, lane for lane in the same order -- so k_bcr_backsub's launch (11 us) is not needed.  SSBA_NO_RHS_RIDE=1 keeps it (A/B, tests).
bool bcr_rhs_rides_in_bwd(const Dev &d) {
    const char *e = getenv("SSBA_NO_RHS_RIDE");
    return bcr_border_rides(d) && d.nb < NBP && d.pcr.level >= 0 && d.pcr.keep && !d.pcr.pin0 && !d.pcr.pin1 && !(e && e[0] == '1');
}
bool bcr_updates_poses(const Dev &d) { return bcr_fused_solve(d) && d.pcr.level == 0 && d.n_pf == 0; }

void launch_bcr(Launcher &L, const Dev &d, bool allow_pcr, bool fuse_update) {
    const size_t sh_backsub = (size_t)3 * BD * BD * sizeof(double);
    const int nl = d.n_levels;
    const bool ride = allow_pcr && bcr_border_rides(d);
    const bool spb_rides = L.spb_rides;     // k_ph_spb_assemble has written the border columns in place (launch_ph_schur of this iteration)
    L.spb_rides = false;
    if (!d.part && allow_pcr && d.pcr.level >= 0) {
        // cyclic reduction down to the plan's level, parallel cyclic reduction of what is left (no back-substitution
        // sweep over those levels: log2(n) x (factor + reduce) + one decoupled solve), back-substitution of the rest
        const int k = d.pcr.level, n = d.pcr.n;
        if (ride && !spb_rides)       // (a plan with border columns always starts at level 0: ssba_finalize)
            hipMemcpyAsync(d.pcr.Bb, d.Spb, (size_t)n * BD * NBP * sizeof(double), hipMemcpyDeviceToDevice, L.stream);
        for (int l = 0; l < k; ++l) {
            const int nn = d.lev[l].n;
            launch_bcr_factor_mf(L, d, nn / 2, l, 0, 0, true);
            launch_bcr_reduce_mf(L, d, (nn + 1) / 2, 2, l, 0);
        }
        const bool fsolve = bcr_fused_solve(d);
        const int solve = fsolve ? (fuse_update && bcr_updates_poses(d) ? 2 : 1) : 0;
        if (bcr_fused_steps(d)) {
            // one launch per step: the factorisation of a block also forms the Gram products the next step assembles its
            // operands from (ssba_bcr_mfma.hip, PcrFused) -- steps + 1 launches instead of 2 x steps + 1
            for (int q = 0; q < d.pcr.steps; ++q) launch_pcr_fused_step(L, d, n, q);
            launch_pcr_fused_top(L, d, n, d.pcr.steps, solve);
        } else {
        for (int q = 0; q < d.pcr.steps; ++q) {
            launch_bcr_factor_mf(L, d, n, q, 0, 2, true, ride);
            launch_bcr_reduce_mf(L, d, n, 2, q, 2, ride);
        }
        // the decoupled last step solves its blocks itself (matrix-core kernels, no border columns): no k_bcr_backsub launch
        launch_bcr_factor_mf(L, d, n, d.pcr.steps, 1, 2, false, ride, solve);
        }
        if (!fsolve && !(ride && bcr_rhs_rides_in_bwd(d))) LAUNCH(KC_BCR_BACKSUB, k_bcr_backsub, dim3(n), dim3(BS_THREADS), sh_backsub, d, k, 1, 2);
        for (int l = k - 1; l >= 0; --l)
            LAUNCH(KC_BCR_BACKSUB, k_bcr_backsub, dim3(d.lev[l].n / 2), dim3(BS_THREADS), sh_backsub, d, l, 0, 0);
        return;
    }
    if (!d.part) {
        if (ride && !spb_rides) hipMemcpyAsync(d.lev[0].B, d.Spb, (size_t)d.Nsb * BD * NBP * sizeof(double), hipMemcpyDeviceToDevice, L.stream);
        for (int l = 0; l + 1 < nl; ++l) {
            const int n = d.lev[l].n;
            launch_bcr_factor_mf(L, d, n / 2, l, 0, 0, true, ride);
            launch_bcr_reduce_mf(L, d, (n + 1) / 2, 2, l, 0, ride);
        }
        launch_bcr_factor_mf(L, d, 1, nl - 1, 1, 0, false, ride);
        LAUNCH(KC_BCR_BACKSUB, k_bcr_backsub, dim3(1), dim3(BS_THREADS), sh_backsub, d, nl - 1, 1, 0);
        for (int l = nl - 2; l >= 0; --l)
            LAUNCH(KC_BCR_BACKSUB, k_bcr_backsub, dim3(d.lev[l].n / 2), dim3(BS_THREADS), sh_backsub, d, l, 0, 0);
        return;
    }
    // Partitioned solve, forward part: eliminate the interior of this rank's chain.  Plain levels (the pinned end of an
    // even-length level is carried over) down to the plan's level, then parallel cyclic reduction with pinned ends: the
    // pinned rows end up holding this rank's share of the separator system, every other block its factor and its
    // couplings to the pinned ones.  launch_bcr_separators() continues after the separator exchange.
    const int k = d.pcr.level, n = d.pcr.n;
    for (int l = 0; l < k; ++l) {
        launch_bcr_factor_mf(L, d, n_odd(d.lev[l], d.lev[l].pin), l, 0, 0, true);
        launch_bcr_reduce_mf(L, d, d.lev[l + 1].n, 2, l, 0);
    }
    const char *fe = getenv("SSBA_NO_PCR_FUSED");
    if (d.pcrf.on && !(fe && fe[0] == '1')) {
        // one launch per step, with the couplings to the pinned ends kept (PcrFused::Lkeep / Ukeep); the last launch
        // factors the interior blocks with those couplings as right-hand sides and leaves the pinned rows in place
        for (int q = 0; q < d.pcr.steps; ++q) launch_pcr_fused_step(L, d, n, q, 2);
        launch_pcr_fused_top(L, d, n, d.pcr.steps, 0, 2);
        return;
    }
    for (int q = 0; q < d.pcr.steps; ++q) {
        launch_bcr_factor_mf(L, d, n, q, 0, 2, true);
        launch_bcr_reduce_mf(L, d, n, d.pcr.pin1 ? 3 : 2, q, 2);
    }
    launch_bcr_factor_mf(L, d, n, d.pcr.steps, 1, 2, d.pcr.pin0 || d.pcr.pin1);
}

// separator system (the blocks shared by neighbouring ranks, summed over the ranks): parallel cyclic reduction,
// replicated on every rank; then the back-substitution of this rank's chain interior
void launch_bcr_separators(Launcher &L, const Dev &d) {
    const size_t sh_backsub = (size_t)3 * BD * BD * sizeof(double);
    const int ns = d.n_sep;
    const char *fe = getenv("SSBA_NO_PCR_FUSED");
    if (d.spcrf.on && !(fe && fe[0] == '1')) {
        // one launch per step, the decoupled last step solves its blocks itself: steps + 1 launches instead of 2 steps + 2
        for (int q = 0; q < d.spcr.steps; ++q) launch_pcr_fused_step(L, d, ns, q, 3);
        launch_pcr_fused_top(L, d, ns, d.spcr.steps, 1, 3);
    } else {
    for (int q = 0; q < d.spcr.steps; ++q) {
        launch_bcr_factor_mf(L, d, ns, q, 0, 3, true);
        launch_bcr_reduce_mf(L, d, ns, 2, q, 3);
    }
    launch_bcr_factor_mf(L, d, ns, d.spcr.steps, 1, 3, false);
    LAUNCH(KC_BCR_BACKSUB, k_bcr_backsub, dim3(ns), dim3(BS_THREADS), sh_backsub, d, 0, 1, 3);
    }
    launch_sep_scatter(L, d);       // x0 at the separator poses <- separator solution
    LAUNCH(KC_BCR_BACKSUB, k_bcr_backsub, dim3(d.pcr.n), dim3(BS_THREADS), sh_backsub, d, d.pcr.level, 1, 2);
    for (int l = d.pcr.level - 1; l >= 0; --l)
        LAUNCH(KC_BCR_BACKSUB, k_bcr_backsub, dim3(n_odd(d.lev[l], d.lev[l].pin)), dim3(BS_THREADS), sh_backsub, d, l, 0, 0);
}

int configure_kernels() {
    if (hipFuncSetAttribute((const void *)k_bcr_backsub, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(3 * BD * BD * sizeof(double))) != hipSuccess) return -1;
    return configure_bcr_mf();
}

}  // namespace ssba
