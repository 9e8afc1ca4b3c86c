// Semi-global stereo matching (Hirschmueller 2008) in the single-pass, five-direction mode of the reference's dense driver
// (cv::StereoSGBM sgbm(0, 64, 15), tests/dense_stereo_test.cpp:61-65), entirely in integers.  The arithmetic is stated in
// include/ssba.h; tests/sgbm_reference.py restates it in numpy and the device equals it to the bit.
//
// Volumes are [row][computable column][disparity] in 16 bits, the disparity fastest, so the lanes of a wave read one pixel's D
// values in one coalesced access.  Five launches on the caller's stream:
//     k_sgbm_hcost   one work-group per row (and chunk of it): the row's pre-filtered and raw signals of both images with their
//                    half-sample minima and maxima as twelve byte arrays in LDS (no pre-filtered image in HBM), then one lane per
//                    (x, d): the Birchfield-Tomasi pixel costs of the 2r + 1 columns around x, summed
//     k_sgbm_vcost   the box sum's vertical pass: one lane per (y, x, 4 disparities) adds 2r + 1 row sums -> C
//     k_sgbm_paths   one wave per path, lane = disparity (K = ceil(D / 64) consecutive disparities per lane).  The previous
//                    pixel's L stays in registers; min L(q) is an integer DPP wave reduction, L(q, d -+ 1) a DPP wave shift.  The
//                    addresses of a path are known ahead: the loads of the next four steps are issued before the current four
//                    are computed.  All five directions run in ONE launch and each writes an L volume of its own.
//     k_sgbm_select  one wave per pixel: S = the sum of the five L volumes, arg-min (smallest d on ties), uniqueness, sub-pixel
//     k_sgbm_lr      one work-group per row: the right view's map in LDS, one lane per right column looping over d with
//                    x = x2 + d (x grows with d, so "ties keep the larger x" is <=), then the check and both outputs
// S is summed from per-direction L volumes instead of being accumulated by one launch per direction.  The path kernel is bound
// by the latency of its W or `rows` dependent steps, not by bytes: one launch holds five times as many independent chains as a
// launch per direction would (2 rows + 3 W + 2 (rows - 1) waves), and the volumes cost 20 + 10 bytes per (pixel, d) against 46
// for a 32-bit S read and written five times.  The price is memory: six 16-bit volumes instead of one and a 32-bit one.
// No atomics; every element of every volume is written by exactly one lane of one launch: two runs give the same bits.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/ssba.h"
#include "ssba_pool.h"
#include "ssba_sgbm.h"

namespace ssba {

void set_last_error(const std::string &s);      // ssba_api.hip

constexpr int SG_THREADS = 256, SG_WAVES = SG_THREADS / 64;
constexpr int SG_INF = 0x3fffffff;              // "no such disparity": survives + P1 + P2 in 32 bits
constexpr int SG_MAX_COLS = 5461;               // twelve byte signals of a row in 64 KiB of LDS
constexpr int SG_PREFETCH = 4;
constexpr uint16_t SG_NO_WINNER = 0xffff;
constexpr uint32_t SG_MAX_CHUNK = 65535;        // the pairs of a chunk are a grid's y or z dimension

struct SgbmVolumes {
    uint16_t *L[5];
};

template <int CTRL, int ROW_MASK> static __device__ __forceinline__ int sg_dpp(int v, int old) {
    return __builtin_amdgcn_update_dpp(old, v, CTRL, ROW_MASK, 0xf, false);
}
// the wave reductions of ssba_device.h on integers: row shifts, row_bcast:15 / :31, the result in lane 63
static __device__ __forceinline__ int sg_wave_min(int v) {
    v = min(v, sg_dpp<0x111, 0xf>(v, v));
    v = min(v, sg_dpp<0x112, 0xf>(v, v));
    v = min(v, sg_dpp<0x114, 0xf>(v, v));
    v = min(v, sg_dpp<0x118, 0xf>(v, v));
    v = min(v, sg_dpp<0x142, 0xa>(v, v));
    v = min(v, sg_dpp<0x143, 0xc>(v, v));
    return __builtin_amdgcn_readlane(v, 63);
}
static __device__ __forceinline__ int sg_wave_max(int v) {
    v = max(v, sg_dpp<0x111, 0xf>(v, v));
    v = max(v, sg_dpp<0x112, 0xf>(v, v));
    v = max(v, sg_dpp<0x114, 0xf>(v, v));
    v = max(v, sg_dpp<0x118, 0xf>(v, v));
    v = max(v, sg_dpp<0x142, 0xa>(v, v));
    v = max(v, sg_dpp<0x143, 0xc>(v, v));
    return __builtin_amdgcn_readlane(v, 63);
}
static __device__ __forceinline__ int sg_from_lane_below(int v) { return sg_dpp<0x138, 0xf>(v, SG_INF); }    // wave_shr:1
static __device__ __forceinline__ int sg_from_lane_above(int v) { return sg_dpp<0x130, 0xf>(v, SG_INF); }    // wave_shl:1

// the K values of one pixel that this lane holds (d = lane * K + k, counted from min_disparity); 0 past D
template <int K> static __device__ __forceinline__ void sg_load(const uint16_t *__restrict__ px, int lane, int D, int *out) {
    if constexpr (K == 1) {
        out[0] = lane < D ? (int)px[lane] : 0;
    } else if constexpr (K == 2) {
        const uint32_t w = 2 * lane < D ? *reinterpret_cast<const uint32_t *>(px + 2 * lane) : 0u;
        out[0] = (int)(w & 0xffffu);
        out[1] = (int)(w >> 16);
    } else if constexpr (K == 4) {
        const uint2 w = 4 * lane < D ? *reinterpret_cast<const uint2 *>(px + 4 * lane) : make_uint2(0u, 0u);
        out[0] = (int)(w.x & 0xffffu);
        out[1] = (int)(w.x >> 16);
        out[2] = (int)(w.y & 0xffffu);
        out[3] = (int)(w.y >> 16);
    } else {
#pragma unroll
        for (int k = 0; k < K; ++k) out[k] = lane * K + k < D ? (int)px[lane * K + k] : 0;
    }
}

template <int K> static __device__ __forceinline__ void sg_store(uint16_t *__restrict__ px, int lane, int D, const int *v) {
    if constexpr (K == 2) {
        if (2 * lane < D) *reinterpret_cast<uint32_t *>(px + 2 * lane) = (uint32_t)v[0] | ((uint32_t)v[1] << 16);
    } else if constexpr (K == 4) {
        if (4 * lane < D) *reinterpret_cast<uint2 *>(px + 4 * lane) = make_uint2((uint32_t)v[0] | ((uint32_t)v[1] << 16), (uint32_t)v[2] | ((uint32_t)v[3] << 16));
    } else {
#pragma unroll
        for (int k = 0; k < K; ++k)
            if (lane * K + k < D) px[lane * K + k] = (uint16_t)v[k];
    }
}

static __device__ __forceinline__ int sg_bt(int a, int amin, int amax, int b, int bmin, int bmax) {
    const int c0 = max(0, max(a - bmax, bmin - a)), c1 = max(0, max(b - amax, amin - b));
    return min(c0, c1);
}

// hsum[y][xi][d] = sum_{i=-r..r} c(clamp(x + i), y, d).  LDS: sig[(4 signals x {value, min, max})][cols] bytes.
static __device__ __forceinline__ void sg_hcost_body(uint8_t *sig, const uint8_t *left, const uint8_t *right,
                                                     uint16_t *hsum, SgbmPlan p, int per_chunk) {
    const int y = blockIdx.y, cols = p.cols, rows = p.rows;
    const int ym = y > 0 ? y - 1 : 1, yp = y + 1 < rows ? y + 1 : rows - 2;
    for (int x = threadIdx.x; x < cols; x += SG_THREADS) {
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const uint8_t *__restrict__ I = q ? right : left;
            const uint8_t *__restrict__ r0 = I + (size_t)ym * cols, *__restrict__ r1 = I + (size_t)y * cols, *__restrict__ r2 = I + (size_t)yp * cols;
            int g = 0;
            if (x > 0 && x < cols - 1) g = ((int)r0[x + 1] - (int)r0[x - 1]) + 2 * ((int)r1[x + 1] - (int)r1[x - 1]) + ((int)r2[x + 1] - (int)r2[x - 1]);
            sig[(size_t)(3 * q) * cols + x] = (uint8_t)(min(max(g, -p.cap), p.cap) + p.cap);
            sig[(size_t)(3 * (2 + q)) * cols + x] = r1[x];
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 4 * cols; i += SG_THREADS) {
        const int s = i / cols, x = i - s * cols;
        uint8_t *v = sig + (size_t)(3 * s) * cols;
        const int a = v[x], lo = (a + (int)v[max(x - 1, 0)]) >> 1, hi = (a + (int)v[min(x + 1, cols - 1)]) >> 1;
        v[cols + x] = (uint8_t)min(a, min(lo, hi));
        v[2 * cols + x] = (uint8_t)max(a, max(lo, hi));
    }
    __syncthreads();
    const uint8_t *Pl = sig, *Pr = sig + 3 * cols, *Il = sig + 6 * cols, *Ir = sig + 9 * cols;
    const int total = p.W * p.D, begin = blockIdx.x * per_chunk, end = min(total, begin + per_chunk);
    uint16_t *__restrict__ out = hsum + (size_t)y * total;
    for (int e = begin + threadIdx.x; e < end; e += SG_THREADS) {
        const int xi = e / p.D, d = e - xi * p.D;
        int sum = 0;
        for (int i = -p.r; i <= p.r; ++i) {
            const int xa = min(max(p.maxD + xi + i, p.maxD), cols - 1), xb = xa - (p.min_d + d);      // xb >= 1
            sum += sg_bt(Pl[xa], Pl[cols + xa], Pl[2 * cols + xa], Pr[xb], Pr[cols + xb], Pr[2 * cols + xb]) +
                   (sg_bt(Il[xa], Il[cols + xa], Il[2 * cols + xa], Ir[xb], Ir[cols + xb], Ir[2 * cols + xb]) >> 2);
        }
        out[e] = (uint16_t)sum;
    }
}

__global__ __launch_bounds__(SG_THREADS) void k_sgbm_hcost(const uint8_t *__restrict__ left, const uint8_t *__restrict__ right, uint16_t *__restrict__ hsum,
                                                          SgbmPlan p, int per_chunk) {
    extern __shared__ uint8_t sig[];
    sg_hcost_body(sig, left, right, hsum, p, per_chunk);
}

// C[y][xi][d] = sum_{j=-r..r} hsum[clamp(y + j)][xi][d]; four disparities per lane (D is a multiple of 16)
static __device__ __forceinline__ void sg_vcost_body(const uint16_t *hsum, uint16_t *C, SgbmPlan p) {
    const size_t row4 = (size_t)p.W * p.D / 4, i = (size_t)blockIdx.x * SG_THREADS + threadIdx.x;
    if (i >= row4 * p.rows) return;
    const int y = (int)(i / row4);
    const size_t rem = i - (size_t)y * row4;
    uint32_t s0 = 0, s1 = 0, s2 = 0, s3 = 0;
    for (int j = -p.r; j <= p.r; ++j) {
        const int yy = min(max(y + j, 0), p.rows - 1);
        const uint2 w = reinterpret_cast<const uint2 *>(hsum)[(size_t)yy * row4 + rem];
        s0 += w.x & 0xffffu;
        s1 += w.x >> 16;
        s2 += w.y & 0xffffu;
        s3 += w.y >> 16;
    }
    reinterpret_cast<uint2 *>(C)[i] = make_uint2(s0 | (s1 << 16), s2 | (s3 << 16));
}

__global__ __launch_bounds__(SG_THREADS) void k_sgbm_vcost(const uint16_t *__restrict__ hsum, uint16_t *__restrict__ C, SgbmPlan p) {
    sg_vcost_body(hsum, C, p);
}

// One wave per path.  Chains in order: rows from the left (predecessor x - 1), rows from the right (x + 1), W columns downwards,
// W + rows - 1 diagonals down-right (predecessor (x - 1, y - 1): they start in row 0 or in the first computable column), as
// many down-left.  L = C where the predecessor lies outside, which is C + min(0, P1, P1, P2) - 0 from an all-zero predecessor.
template <int K>
static __device__ __forceinline__ void sg_paths_body(const uint16_t *C, SgbmVolumes vol, SgbmPlan p, int nchains) {
    const int lane = threadIdx.x & 63;
    int c = blockIdx.x * SG_WAVES + (threadIdx.x >> 6);
    if (c >= nchains) return;       // a whole wave
    const int W = p.W, rows = p.rows, D = p.D, nd = W + rows - 1;
    int dir, x0, y0, dx, dy, n;
    if (c < rows) { dir = 0; x0 = 0; y0 = c; dx = 1; dy = 0; n = W; }
    else if ((c -= rows) < rows) { dir = 1; x0 = W - 1; y0 = c; dx = -1; dy = 0; n = W; }
    else if ((c -= rows) < W) { dir = 3; x0 = c; y0 = 0; dx = 0; dy = 1; n = rows; }
    else if ((c -= W) < nd) { dir = 2; x0 = c < W ? c : 0; y0 = c < W ? 0 : c - W + 1; dx = 1; dy = 1; n = min(W - x0, rows - y0); }
    else { c -= nd; dir = 4; x0 = c < W ? c : W - 1; y0 = c < W ? 0 : c - W + 1; dx = -1; dy = 1; n = min(x0 + 1, rows - y0); }
    const long long off = ((long long)y0 * W + x0) * D, stride = ((long long)dy * W + dx) * D;
    const uint16_t *__restrict__ src = C + off;
    uint16_t *__restrict__ dst = vol.L[dir] + off;
    int prev[K], cur[SG_PREFETCH][K], nxt[SG_PREFETCH][K];
#pragma unroll
    for (int k = 0; k < K; ++k) prev[k] = lane * K + k < D ? 0 : SG_INF;
#pragma unroll
    for (int u = 0; u < SG_PREFETCH; ++u)
        if (u < n) sg_load<K>(src + u * stride, lane, D, cur[u]);
    for (int base = 0; base < n; base += SG_PREFETCH) {
#pragma unroll
        for (int u = 0; u < SG_PREFETCH; ++u)
            if (base + SG_PREFETCH + u < n) sg_load<K>(src + (base + SG_PREFETCH + u) * stride, lane, D, nxt[u]);
#pragma unroll
        for (int u = 0; u < SG_PREFETCH; ++u) {
            if (base + u >= n) break;       // the same for every lane
            int m = prev[0];
#pragma unroll
            for (int k = 1; k < K; ++k) m = min(m, prev[k]);
            m = sg_wave_min(m);
            const int below = sg_from_lane_below(prev[K - 1]), above = sg_from_lane_above(prev[0]);
            int now[K];
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const int lo = k == 0 ? below : prev[k > 0 ? k - 1 : 0], hi = k == K - 1 ? above : prev[k + 1 < K ? k + 1 : K - 1];
                const int best = min(min(prev[k], min(lo, hi) + p.P1), m + p.P2);
                now[k] = lane * K + k < D ? cur[u][k] + best - m : SG_INF;
            }
            sg_store<K>(dst + (base + u) * stride, lane, D, now);
#pragma unroll
            for (int k = 0; k < K; ++k) prev[k] = now[k];
        }
#pragma unroll
        for (int u = 0; u < SG_PREFETCH; ++u)
#pragma unroll
            for (int k = 0; k < K; ++k) cur[u][k] = nxt[u][k];
    }
}

template <int K>
__global__ __launch_bounds__(SG_THREADS) void k_sgbm_paths(const uint16_t *__restrict__ C, SgbmVolumes vol, SgbmPlan p, int nchains) {
    sg_paths_body<K>(C, vol, p, nchains);
}

// One wave per pixel.  winner: the disparity (min_disparity included) or SG_NO_WINNER where uniqueness fails.
template <int K>
static __device__ __forceinline__ void sg_select_body(SgbmVolumes vol, uint16_t *winner, int *smin_out,
                                                      int16_t *disp16_out, SgbmPlan p) {
    const int lane = threadIdx.x & 63;
    const size_t px = (size_t)blockIdx.x * SG_WAVES + (threadIdx.x >> 6);
    if (px >= (size_t)p.rows * p.W) return;     // a whole wave
    const int D = p.D;
    int S[K];
#pragma unroll
    for (int k = 0; k < K; ++k) S[k] = 0;
#pragma unroll
    for (int q = 0; q < 5; ++q) {
        int v[K];
        sg_load<K>(vol.L[q] + px * D, lane, D, v);
#pragma unroll
        for (int k = 0; k < K; ++k) S[k] += v[k];
    }
    // S < 5 * 65536 and d < 256: the smallest (S, d) pair in one integer
    int key = INT_MAX;
#pragma unroll
    for (int k = 0; k < K; ++k)
        if (lane * K + k < D) key = min(key, (S[k] << 9) | (lane * K + k));
    key = sg_wave_min(key);
    const int smin = key >> 9, best = key & 511;
    int rival = 0, sm = 0, sp = 0;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int d = lane * K + k;
        if (d < D) {
            if (abs(d - best) > 1 && S[k] * (100 - p.uniq) < smin * 100) rival = 1;
            if (d == best - 1) sm = S[k];
            if (d == best + 1) sp = S[k];
        }
    }
    rival = sg_wave_max(rival);
    sm = sg_wave_max(sm);
    sp = sg_wave_max(sp);
    if (lane == 0) {
        int d16 = 16 * (best + p.min_d);
        if (best > 0 && best < D - 1) {
            const int den = max(sm + sp - 2 * smin, 1);
            d16 += ((sm - sp) * 16 + den) / (2 * den);      // C's division truncates
        }
        winner[px] = rival ? SG_NO_WINNER : (uint16_t)(best + p.min_d);
        smin_out[px] = smin;
        disp16_out[px] = (int16_t)d16;
    }
}

template <int K>
__global__ __launch_bounds__(SG_THREADS) void k_sgbm_select(SgbmVolumes vol, uint16_t *__restrict__ winner, int *__restrict__ smin_out,
                                                           int16_t *__restrict__ disp16_out, SgbmPlan p) {
    sg_select_body<K>(vol, winner, smin_out, disp16_out, p);
}

// One work-group per row.  LDS: disp2[cols] as int16.
static __device__ __forceinline__ void sg_lr_body(int16_t *disp2, const uint16_t *winner, const int *smin,
                                                  const int16_t *disp16_w, int16_t *disp16_out, double *disparity_out,
                                                  SgbmPlan p) {
    const int y = blockIdx.x, cols = p.cols, W = p.W;
    const uint16_t *__restrict__ win = winner + (size_t)y * W;
    const int *__restrict__ cost = smin + (size_t)y * W;
    if (p.lr >= 0) {
        for (int x2 = threadIdx.x; x2 < cols; x2 += SG_THREADS) {
            int best = INT_MAX, bd = p.min_d - 1;
            for (int d = p.min_d; d < p.maxD; ++d) {
                const int xi = x2 + d - p.maxD;
                if (xi >= 0 && xi < W && (int)win[xi] == d && cost[xi] <= best) { best = cost[xi]; bd = d; }
            }
            disp2[x2] = (int16_t)bd;
        }
        __syncthreads();
    }
    const int invalid = (p.min_d - 1) * 16;
    for (int x = threadIdx.x; x < cols; x += SG_THREADS) {
        int v = invalid;
        bool ok = false;
        if (x >= p.maxD) {
            const int xi = x - p.maxD;
            ok = win[xi] != SG_NO_WINNER;
            v = disp16_w[(size_t)y * W + xi];
            if (ok && p.lr >= 0) {
                const int lo = v >> 4, hi = (v + 15) >> 4, a = x - lo, b = x - hi;
                const bool bad_a = a >= 0 && a < cols && disp2[a] >= p.min_d && abs(disp2[a] - lo) > p.lr;
                const bool bad_b = b >= 0 && b < cols && disp2[b] >= p.min_d && abs(disp2[b] - hi) > p.lr;
                ok = !(bad_a && bad_b);
            }
            if (!ok) v = invalid;
        }
        const size_t i = (size_t)y * cols + x;
        if (disp16_out) disp16_out[i] = (int16_t)v;
        if (disparity_out) disparity_out[i] = ok ? (double)v / 16.0 : __builtin_nan("");
    }
}

__global__ __launch_bounds__(SG_THREADS) void k_sgbm_lr(const uint16_t *__restrict__ winner, const int *__restrict__ smin, const int16_t *__restrict__ disp16_w,
                                                       int16_t *__restrict__ disp16_out, double *__restrict__ disparity_out, SgbmPlan p) {
    extern __shared__ int16_t disp2[];
    sg_lr_body(disp2, winner, smin, disp16_w, disp16_out, disparity_out, p);
}

// The five kernels over the pairs of a chunk (ssba_stereo_sgbm_batch, ssba_image_sequence_create): the pair is the grid's last
// dimension, images, volumes, per-pixel arrays and outputs are pair-major with one stride each, so a work-group's base pointers
// follow from its block index (wave-uniform) and the bodies above run unchanged: member k's bits are the solo call's.
struct SgbmStrides {
    size_t img, vol, px, out;       // elements between two pairs: input images, volumes, winner / smin / disp16_w, outputs
};

static __device__ __forceinline__ SgbmVolumes sg_pair_volumes(SgbmVolumes vol, size_t off) {
    SgbmVolumes v;
#pragma unroll
    for (int q = 0; q < 5; ++q) v.L[q] = vol.L[q] + off;
    return v;
}

__global__ __launch_bounds__(SG_THREADS) void k_sgbm_hcost_batch(const uint8_t *__restrict__ left, const uint8_t *__restrict__ right,
                                                                uint16_t *__restrict__ hsum, SgbmPlan p, int per_chunk, SgbmStrides st) {
    extern __shared__ uint8_t sig[];
    const size_t pair = blockIdx.z;
    sg_hcost_body(sig, left + pair * st.img, right + pair * st.img, hsum + pair * st.vol, p, per_chunk);
}

__global__ __launch_bounds__(SG_THREADS) void k_sgbm_vcost_batch(const uint16_t *__restrict__ hsum, uint16_t *__restrict__ C, SgbmPlan p, SgbmStrides st) {
    const size_t off = (size_t)blockIdx.y * st.vol;
    sg_vcost_body(hsum + off, C + off, p);
}

template <int K>
__global__ __launch_bounds__(SG_THREADS) void k_sgbm_paths_batch(const uint16_t *__restrict__ C, SgbmVolumes vol, SgbmPlan p, int nchains, SgbmStrides st) {
    const size_t off = (size_t)blockIdx.y * st.vol;
    sg_paths_body<K>(C + off, sg_pair_volumes(vol, off), p, nchains);
}

template <int K>
__global__ __launch_bounds__(SG_THREADS) void k_sgbm_select_batch(SgbmVolumes vol, uint16_t *__restrict__ winner, int *__restrict__ smin_out,
                                                                 int16_t *__restrict__ disp16_out, SgbmPlan p, SgbmStrides st) {
    const size_t pair = blockIdx.y;
    sg_select_body<K>(sg_pair_volumes(vol, pair * st.vol), winner + pair * st.px, smin_out + pair * st.px, disp16_out + pair * st.px, p);
}

__global__ __launch_bounds__(SG_THREADS) void k_sgbm_lr_batch(const uint16_t *__restrict__ winner, const int *__restrict__ smin,
                                                             const int16_t *__restrict__ disp16_w, int16_t *__restrict__ disp16_out,
                                                             double *__restrict__ disparity_out, SgbmPlan p, SgbmStrides st) {
    extern __shared__ int16_t disp2[];
    const size_t pair = blockIdx.y;
    sg_lr_body(disp2, winner + pair * st.px, smin + pair * st.px, disp16_w + pair * st.px, disp16_out ? disp16_out + pair * st.out : nullptr,
               disparity_out ? disparity_out + pair * st.out : nullptr, p);
}

static int sg_refuse(const char *call, int status, const char *what) {
    set_last_error(std::string(call) + ": " + what);
    return status;
}

int sgbm_check(const char *call, uint32_t rows, uint32_t cols, const ssba_sgbm_params *q, SgbmPlan *plan) {
    if (!q) return sg_refuse(call, SSBA_ERR_INVALID_ARGUMENT, "NULL matcher parameters");
    const int D = q->num_disparities, bs = q->block_size;
    if (q->min_disparity < 0) return sg_refuse(call, SSBA_ERR_INVALID_ARGUMENT, "min_disparity must not be negative");
    if (D < 16 || D > 256 || D % 16) return sg_refuse(call, SSBA_ERR_INVALID_ARGUMENT, "num_disparities must be a multiple of 16 in 16 ... 256");
    if (bs < 1 || bs > 15 || bs % 2 == 0) return sg_refuse(call, SSBA_ERR_INVALID_ARGUMENT, "block_size must be odd in 1 ... 15");
    if (q->uniqueness_ratio < 0 || q->uniqueness_ratio > 100) return sg_refuse(call, SSBA_ERR_INVALID_ARGUMENT, "uniqueness_ratio must be in 0 ... 100");
    if (q->pre_filter_cap > 127) return sg_refuse(call, SSBA_ERR_INVALID_ARGUMENT, "pre_filter_cap above 127: the filtered image no longer fits 8 bits");
    if (q->full_dp) return sg_refuse(call, SSBA_ERR_INVALID_ARGUMENT, "the eight-direction mode (full_dp) is not built");
    if (rows < 2) return sg_refuse(call, SSBA_ERR_INVALID_ARGUMENT, "the pre-filter reflects rows: at least 2");
    const long long maxD = (long long)q->min_disparity + D;
    if ((long long)cols <= maxD) return sg_refuse(call, SSBA_ERR_INVALID_ARGUMENT, "no computable column: cols must exceed min_disparity + num_disparities");
    if (maxD > 2047) return sg_refuse(call, SSBA_ERR_INVALID_ARGUMENT, "min_disparity + num_disparities above 2047: disp16 no longer fits 16 bits");
    const int cap = (q->pre_filter_cap > 15 ? q->pre_filter_cap : 15) | 1;
    const int P1 = q->p1 > 0 ? q->p1 : 2, p2 = q->p2 > 0 ? q->p2 : 5;
    const long long P2 = p2 > P1 + 1 ? p2 : (long long)P1 + 1;
    if ((long long)(2 * cap + 63) * bs * bs + P2 > 65535) return sg_refuse(call, SSBA_ERR_INVALID_ARGUMENT, "block cost plus P2 exceeds 16 bits");
    if (q->speckle_window_size || q->speckle_range) return sg_refuse(call, SSBA_ERR_UNSUPPORTED, "the speckle filter is not built (speckle_window_size and speckle_range must be 0)");
    if (cols > (uint32_t)SG_MAX_COLS || (unsigned long long)rows * (cols - maxD) * D >= (1ull << 31))
        return sg_refuse(call, SSBA_ERR_UNSUPPORTED, "image too large (at most 5461 columns and 2^31 volume entries)");
    *plan = SgbmPlan{(int)rows, (int)cols, (int)(cols - maxD), D, q->min_disparity, (int)maxD, bs / 2, cap, P1, (int)P2, q->uniqueness_ratio, q->disp12_max_diff};
    return SSBA_OK;
}

template <class T> static hipError_t sg_alloc(std::vector<void *> *temps, T **out, size_t n) {
    void *ptr = nullptr;
    const hipError_t e = pool_malloc(&ptr, n * sizeof(T));
    if (e != hipSuccess) return e;
    temps->push_back(ptr);
    *out = (T *)ptr;
    return hipSuccess;
}

#define SG_TRY(expr)                      \
    do {                                  \
        const hipError_t _e = (expr);     \
        if (_e != hipSuccess) return _e;  \
    } while (0)

hipError_t sgbm_enqueue(const SgbmPlan &p, const uint8_t *left, const uint8_t *right, int16_t *disp16, double *disparity, hipStream_t s,
                        std::vector<void *> *temps) {
    const size_t npx = (size_t)p.rows * p.W, nvol = npx * p.D;
    uint16_t *C = nullptr, *winner = nullptr;
    int *smin = nullptr;
    int16_t *d16w = nullptr;
    SgbmVolumes vol;
    SG_TRY(sg_alloc(temps, &C, nvol));
    for (int q = 0; q < 5; ++q) SG_TRY(sg_alloc(temps, &vol.L[q], nvol));
    SG_TRY(sg_alloc(temps, &winner, npx));
    SG_TRY(sg_alloc(temps, &smin, npx));
    SG_TRY(sg_alloc(temps, &d16w, npx));
    // the row sums live in the first L volume until the path kernel overwrites it
    const int total = p.W * p.D;
    int nchunk = (total + 8191) / 8192;
    nchunk = nchunk < 1 ? 1 : nchunk > 64 ? 64 : nchunk;
    const int per_chunk = ((total + nchunk - 1) / nchunk + SG_THREADS - 1) / SG_THREADS * SG_THREADS;
    hipLaunchKernelGGL(k_sgbm_hcost, dim3((total + per_chunk - 1) / per_chunk, p.rows), dim3(SG_THREADS), (size_t)12 * p.cols, s, left, right, vol.L[0], p, per_chunk);
    SG_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_sgbm_vcost, dim3((unsigned)((nvol / 4 + SG_THREADS - 1) / SG_THREADS)), dim3(SG_THREADS), 0, s, (const uint16_t *)vol.L[0], C, p);
    SG_TRY(hipGetLastError());
    const int nchains = 2 * p.rows + p.W + 2 * (p.W + p.rows - 1);
    const dim3 pgrid((nchains + SG_WAVES - 1) / SG_WAVES), sgrid((unsigned)((npx + SG_WAVES - 1) / SG_WAVES));
    switch ((p.D + 63) / 64) {
    case 1:
        hipLaunchKernelGGL(k_sgbm_paths<1>, pgrid, dim3(SG_THREADS), 0, s, (const uint16_t *)C, vol, p, nchains);
        hipLaunchKernelGGL(k_sgbm_select<1>, sgrid, dim3(SG_THREADS), 0, s, vol, winner, smin, d16w, p);
        break;
    case 2:
        hipLaunchKernelGGL(k_sgbm_paths<2>, pgrid, dim3(SG_THREADS), 0, s, (const uint16_t *)C, vol, p, nchains);
        hipLaunchKernelGGL(k_sgbm_select<2>, sgrid, dim3(SG_THREADS), 0, s, vol, winner, smin, d16w, p);
        break;
    case 3:
        hipLaunchKernelGGL(k_sgbm_paths<3>, pgrid, dim3(SG_THREADS), 0, s, (const uint16_t *)C, vol, p, nchains);
        hipLaunchKernelGGL(k_sgbm_select<3>, sgrid, dim3(SG_THREADS), 0, s, vol, winner, smin, d16w, p);
        break;
    default:
        hipLaunchKernelGGL(k_sgbm_paths<4>, pgrid, dim3(SG_THREADS), 0, s, (const uint16_t *)C, vol, p, nchains);
        hipLaunchKernelGGL(k_sgbm_select<4>, sgrid, dim3(SG_THREADS), 0, s, vol, winner, smin, d16w, p);
        break;
    }
    SG_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_sgbm_lr, dim3(p.rows), dim3(SG_THREADS), (size_t)2 * p.cols, s, (const uint16_t *)winner, (const int *)smin, (const int16_t *)d16w, disp16,
                       disparity, p);
    return hipGetLastError();
}

uint64_t sgbm_pair_bytes(const SgbmPlan &p) { return 12ull * (uint64_t)p.rows * (uint64_t)p.W * (uint64_t)p.D; }

int sgbm_chunk_pairs(const char *call, const SgbmPlan &p, uint32_t n, uint64_t workspace_bytes, uint32_t *pairs) {
    const uint64_t need = sgbm_pair_bytes(p), have = workspace_bytes ? workspace_bytes : SSBA_SGBM_DEFAULT_WORKSPACE_BYTES;
    if (have < need)
        return sg_refuse(call, SSBA_ERR_INVALID_ARGUMENT,
                         ("workspace_bytes " + std::to_string(have) + " is below the volumes of one pair: " + std::to_string(need) + " bytes needed").c_str());
    uint64_t fit = have / need;
    if (fit > n) fit = n;
    if (fit > SG_MAX_CHUNK) fit = SG_MAX_CHUNK;
    *pairs = (uint32_t)fit;
    return SSBA_OK;
}

hipError_t sgbm_enqueue_batch(const SgbmPlan &p, const uint8_t *left, const uint8_t *right, size_t img_stride, uint32_t n, uint32_t chunk_pairs,
                              int16_t *disp16, double *disparity, hipStream_t s, std::vector<void *> *temps) {
    const size_t npx = (size_t)p.rows * p.W, nvol = npx * p.D, m = chunk_pairs < n ? chunk_pairs : n;
    const SgbmStrides st = {img_stride, nvol, npx, (size_t)p.rows * p.cols};
    uint16_t *C = nullptr, *winner = nullptr;
    int *smin = nullptr;
    int16_t *d16w = nullptr;
    SgbmVolumes vol;
    SG_TRY(sg_alloc(temps, &C, m * nvol));
    for (int q = 0; q < 5; ++q) SG_TRY(sg_alloc(temps, &vol.L[q], m * nvol));
    SG_TRY(sg_alloc(temps, &winner, m * npx));
    SG_TRY(sg_alloc(temps, &smin, m * npx));
    SG_TRY(sg_alloc(temps, &d16w, m * npx));
    // the launch shapes of sgbm_enqueue with the pair behind them; the chunks follow each other on `s` and share the volumes
    const int total = p.W * p.D;
    int nchunk = (total + 8191) / 8192;
    nchunk = nchunk < 1 ? 1 : nchunk > 64 ? 64 : nchunk;
    const int per_chunk = ((total + nchunk - 1) / nchunk + SG_THREADS - 1) / SG_THREADS * SG_THREADS;
    const int nchains = 2 * p.rows + p.W + 2 * (p.W + p.rows - 1);
    for (uint32_t first = 0; first < n; first += (uint32_t)m) {
        const unsigned c = (unsigned)(n - first < m ? n - first : m);
        const uint8_t *l = left + first * st.img, *r = right + first * st.img;
        int16_t *o16 = disp16 ? disp16 + first * st.out : nullptr;
        double *od = disparity ? disparity + first * st.out : nullptr;
        hipLaunchKernelGGL(k_sgbm_hcost_batch, dim3((total + per_chunk - 1) / per_chunk, p.rows, c), dim3(SG_THREADS), (size_t)12 * p.cols, s, l, r, vol.L[0], p,
                           per_chunk, st);
        SG_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_sgbm_vcost_batch, dim3((unsigned)((nvol / 4 + SG_THREADS - 1) / SG_THREADS), c), dim3(SG_THREADS), 0, s, (const uint16_t *)vol.L[0], C, p,
                           st);
        SG_TRY(hipGetLastError());
        const dim3 pgrid((nchains + SG_WAVES - 1) / SG_WAVES, c), sgrid((unsigned)((npx + SG_WAVES - 1) / SG_WAVES), c);
        switch ((p.D + 63) / 64) {
        case 1:
            hipLaunchKernelGGL(k_sgbm_paths_batch<1>, pgrid, dim3(SG_THREADS), 0, s, (const uint16_t *)C, vol, p, nchains, st);
            hipLaunchKernelGGL(k_sgbm_select_batch<1>, sgrid, dim3(SG_THREADS), 0, s, vol, winner, smin, d16w, p, st);
            break;
        case 2:
            hipLaunchKernelGGL(k_sgbm_paths_batch<2>, pgrid, dim3(SG_THREADS), 0, s, (const uint16_t *)C, vol, p, nchains, st);
            hipLaunchKernelGGL(k_sgbm_select_batch<2>, sgrid, dim3(SG_THREADS), 0, s, vol, winner, smin, d16w, p, st);
            break;
        case 3:
            hipLaunchKernelGGL(k_sgbm_paths_batch<3>, pgrid, dim3(SG_THREADS), 0, s, (const uint16_t *)C, vol, p, nchains, st);
            hipLaunchKernelGGL(k_sgbm_select_batch<3>, sgrid, dim3(SG_THREADS), 0, s, vol, winner, smin, d16w, p, st);
            break;
        default:
            hipLaunchKernelGGL(k_sgbm_paths_batch<4>, pgrid, dim3(SG_THREADS), 0, s, (const uint16_t *)C, vol, p, nchains, st);
            hipLaunchKernelGGL(k_sgbm_select_batch<4>, sgrid, dim3(SG_THREADS), 0, s, vol, winner, smin, d16w, p, st);
            break;
        }
        SG_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_sgbm_lr_batch, dim3(p.rows, c), dim3(SG_THREADS), (size_t)2 * p.cols, s, (const uint16_t *)winner, (const int *)smin,
                           (const int16_t *)d16w, o16, od, p, st);
        SG_TRY(hipGetLastError());
    }
    return hipSuccess;
}

static hipError_t sg_run_batch(const SgbmPlan &p, const uint8_t *left, const uint8_t *right, uint32_t n, uint32_t chunk_pairs, int16_t *disp16_out,
                               double *disparity_out, hipStream_t s, std::vector<void *> *temps) {
    const size_t npix = (size_t)p.rows * p.cols, all = npix * n;
    uint8_t *dl = nullptr, *dr = nullptr;
    int16_t *d16 = nullptr;
    double *dd = nullptr;
    SG_TRY(sg_alloc(temps, &dl, all));
    SG_TRY(sg_alloc(temps, &dr, all));
    if (disp16_out) SG_TRY(sg_alloc(temps, &d16, all));
    if (disparity_out) SG_TRY(sg_alloc(temps, &dd, all));
    SG_TRY(hipMemcpyAsync(dl, left, all, hipMemcpyHostToDevice, s));
    SG_TRY(hipMemcpyAsync(dr, right, all, hipMemcpyHostToDevice, s));
    SG_TRY(sgbm_enqueue_batch(p, dl, dr, npix, n, chunk_pairs, d16, dd, s, temps));
    if (disp16_out) SG_TRY(hipMemcpyAsync(disp16_out, d16, all * sizeof(int16_t), hipMemcpyDeviceToHost, s));
    if (disparity_out) SG_TRY(hipMemcpyAsync(disparity_out, dd, all * sizeof(double), hipMemcpyDeviceToHost, s));
    return hipStreamSynchronize(s);
}

static hipError_t sg_run(const SgbmPlan &p, const uint8_t *left, const uint8_t *right, int16_t *disp16_out, double *disparity_out, hipStream_t s,
                         std::vector<void *> *temps) {
    const size_t n = (size_t)p.rows * p.cols;
    uint8_t *dl = nullptr, *dr = nullptr;
    int16_t *d16 = nullptr;
    double *dd = nullptr;
    SG_TRY(sg_alloc(temps, &dl, n));
    SG_TRY(sg_alloc(temps, &dr, n));
    if (disp16_out) SG_TRY(sg_alloc(temps, &d16, n));
    if (disparity_out) SG_TRY(sg_alloc(temps, &dd, n));
    SG_TRY(hipMemcpyAsync(dl, left, n, hipMemcpyHostToDevice, s));
    SG_TRY(hipMemcpyAsync(dr, right, n, hipMemcpyHostToDevice, s));
    SG_TRY(sgbm_enqueue(p, dl, dr, d16, dd, s, temps));
    if (disp16_out) SG_TRY(hipMemcpyAsync(disp16_out, d16, n * sizeof(int16_t), hipMemcpyDeviceToHost, s));
    if (disparity_out) SG_TRY(hipMemcpyAsync(disparity_out, dd, n * sizeof(double), hipMemcpyDeviceToHost, s));
    return hipStreamSynchronize(s);
}

}  // namespace ssba

using namespace ssba;

extern "C" {

void ssba_sgbm_default_params(ssba_sgbm_params *params) {
    if (!params) return;
    *params = ssba_sgbm_params{};
    params->min_disparity = 0;
    params->num_disparities = 64;
    params->block_size = 15;
}

int ssba_stereo_sgbm(const uint8_t *left, const uint8_t *right, uint32_t rows, uint32_t cols, const ssba_sgbm_params *params, int device,
                     int16_t *disp16_out, double *disparity_out) {
    const char *call = "ssba_stereo_sgbm";
    if (!left || !right) return sg_refuse(call, SSBA_ERR_INVALID_ARGUMENT, "NULL image");
    SgbmPlan plan;
    if (const int rc = sgbm_check(call, rows, cols, params, &plan)) return rc;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return sg_refuse(call, SSBA_ERR_NO_DEVICE, "hipGetDeviceCount found no device");
    if (device < 0 && hipGetDevice(&device) != hipSuccess) return SSBA_ERR_NO_DEVICE;
    if (device >= n) return sg_refuse(call, SSBA_ERR_INVALID_ARGUMENT, "no such device");
    if (hipSetDevice(device) != hipSuccess) return sg_refuse(call, SSBA_ERR_HIP, "hipSetDevice failed");
    hipStream_t s = nullptr;
    if (pool_stream_acquire(&s) != hipSuccess) return sg_refuse(call, SSBA_ERR_HIP, "no stream");
    std::vector<void *> temps;
    const hipError_t e = sg_run(plan, left, right, disp16_out, disparity_out, s, &temps);
    hipStreamSynchronize(s);
    for (void *t : temps) pool_free(t);
    pool_stream_release(s);
    if (e != hipSuccess) return sg_refuse(call, SSBA_ERR_HIP, hipGetErrorString(e));
    return SSBA_OK;
}

int ssba_stereo_sgbm_batch(const uint8_t *left, const uint8_t *right, uint32_t n, uint32_t rows, uint32_t cols, const ssba_sgbm_params *params,
                           uint64_t workspace_bytes, int device, int16_t *disp16_out, double *disparity_out) {
    const char *call = "ssba_stereo_sgbm_batch";
    if (!left || !right) return sg_refuse(call, SSBA_ERR_INVALID_ARGUMENT, "NULL image");
    SgbmPlan plan;
    if (const int rc = sgbm_check(call, rows, cols, params, &plan)) return rc;
    if (n == 0) return sg_refuse(call, SSBA_ERR_INVALID_ARGUMENT, "n = 0");
    uint32_t chunk_pairs = 0;
    if (const int rc = sgbm_chunk_pairs(call, plan, n, workspace_bytes, &chunk_pairs)) return rc;
    int nd = 0;
    if (hipGetDeviceCount(&nd) != hipSuccess || nd <= 0) return sg_refuse(call, SSBA_ERR_NO_DEVICE, "hipGetDeviceCount found no device");
    if (device < 0 && hipGetDevice(&device) != hipSuccess) return SSBA_ERR_NO_DEVICE;
    if (device >= nd) return sg_refuse(call, SSBA_ERR_INVALID_ARGUMENT, "no such device");
    if (hipSetDevice(device) != hipSuccess) return sg_refuse(call, SSBA_ERR_HIP, "hipSetDevice failed");
    hipStream_t s = nullptr;
    if (pool_stream_acquire(&s) != hipSuccess) return sg_refuse(call, SSBA_ERR_HIP, "no stream");
    std::vector<void *> temps;
    const hipError_t e = sg_run_batch(plan, left, right, n, chunk_pairs, disp16_out, disparity_out, s, &temps);
    hipStreamSynchronize(s);
    for (void *t : temps) pool_free(t);
    pool_stream_release(s);
    if (e != hipSuccess) return sg_refuse(call, SSBA_ERR_HIP, hipGetErrorString(e));
    return SSBA_OK;
}

}  // extern "C"
