// libssba_tracks.so: sparse stereo feature tracks from raw frames (include/ssba_tracks.h states the arithmetic; the numpy
// statement is tests/tracks_reference.py).  Everything is integer arithmetic, and every position in an output comes from a
// prefix sum, so the results do not depend on scheduling.  The image (or the pair) is a grid dimension of every kernel: the
// number of launches does not depend on the number of frames.
//
//   k_tr_score      ring scores of every pixel of every image                      grid (cols / 64, rows / 4, images)
//   k_tr_nms        3 x 3 suppression, one 256-bin score histogram per image       grid (cols / 64, rows / 4, images)
//   k_tr_select     the cut score from the histogram, row-major compaction         grid (images), one work-group walks its image
//   k_tr_describe   31 x 31 patch -> 27 x 27 box sums in LDS -> 256 bits           grid (max_features, images)
//   k_tr_best       best train index per query under the gate, both directions     grid (queries / 64, pairs, 2)
//   k_tr_stereo     cross-check, disparity, survivors compacted in keypoint order  grid (frames)
//   k_tr_best       the same kernel over the F - 1 pairs of consecutive survivors
//   k_tr_link       ids: one work-group walks the frames                           grid (1)
//   k_tr_prune      short tracks out, ids renumbered, observations written         grid (1)
// ssba_track_sequence_subpixel puts two launches in front of k_tr_prune:
//   k_tr_anchor     per id the survivor slot that issued it                        grid (max_features / 256, frames)
//   k_tr_refine     one wave per survivor: the anchor's 15 x 15 template placed    grid (max_features / 4, frames)
//                   in the left image (2-D), then in the right image (x only)
// and ssba_track_refine runs the same placement (rf_solve) over a list of items: k_tr_refine_items, grid (items / 4).
// A stream (ssba_track_stream_push) runs the kernels up to k_tr_stereo and k_tr_best on one pair, then
//   k_ts_link       the frame's ids against the retained previous survivors         grid (1)
//   k_ts_carry      one wave per survivor: the anchor patch inherited or cut        grid (max_features / 4)
//   k_ts_refine     k_tr_refine with the template from the patch store              grid (max_features / 4)
//   k_ts_emit       the push outputs compacted, the frame's ring entry              grid (1)
// and ssba_track_stream_window is one launch, k_ts_window: k_tr_link and k_tr_prune on the ring's stored links, grid (1).
// A stream with odometry enabled (ssba_track_stream_enable_odometry) adds four launches to a push, ssba_tracks_odometry.h:
//   k_od_match, k_od_align, k_od_score, k_od_solve: the matches to the frame before triangulated, the 3-point RANSAC, the
//   two-view Levenberg-Marquardt refinement and the chained pose, which comes down in the push's one copy.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <cmath>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/ssba_tracks.h"
#include "ssba_brief_pattern.h"
#include "ssba_pool.h"

namespace ssba {
namespace {

constexpr int TR_BORDER = SSBA_TRACK_BORDER;
constexpr int TR_WORDS = SSBA_TRACK_DESC_WORDS;
constexpr uint32_t TR_NONE = 0xffffffffu;     // packed key (distance << 16) | index of "no train entry passed the gate"
constexpr int TR_BLOCK = 1024;                // the scanning kernels: 16 waves, 4 items per thread cover SSBA_TRACK_MAX_FEATURES
constexpr int TR_ITEMS = 4;
constexpr int TR_SPLIT = 4;                   // k_tr_best: the lanes that share a query, each takes every fourth train entry
constexpr int TR_QUERIES = 64;                // queries per work-group
constexpr int TR_THREADS = TR_QUERIES * TR_SPLIT;
constexpr int TR_TILE = 512;                  // train descriptors staged per step: 16 KiB + 2 KiB of positions
constexpr int TR_PATCH = 2 * TR_BORDER + 1;   // 31
constexpr int TR_BOXES = 2 * SSBA_BRIEF_RADIUS + 1;   // 27

static_assert(TR_BLOCK * TR_ITEMS == SSBA_TRACK_MAX_FEATURES, "one pass of the scanning kernels covers every keypoint slot");
static_assert(SSBA_BRIEF_PAIRS == 256 && SSBA_BRIEF_RADIUS + 2 == TR_BORDER, "pattern and border belong together");

__constant__ int8_t c_brief[SSBA_BRIEF_PAIRS][4] = {SSBA_BRIEF_PATTERN_ROWS};

struct TrackGate {
    int kind, max_dy, max_disparity, radius;
};

// exclusive prefix sum of one value per thread over a work-group of TR_BLOCK threads; *total is the sum.  `part` holds one
// entry per wave and is free again when the call returns.
__device__ __forceinline__ uint32_t tr_block_exscan(uint32_t v, uint32_t *part, uint32_t *total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t up = __shfl_up(inc, d, 64);
        if (lane >= d) inc += up;
    }
    if (lane == 63) part[wave] = inc;
    __syncthreads();
    uint32_t before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < TR_BLOCK / 64; ++w) {
        const uint32_t p = part[w];
        before += w < wave ? p : 0u;
        all += p;
    }
    __syncthreads();
    *total = all;
    return before + inc - v;
}

// ---- detector ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_tr_score(const uint8_t *__restrict__ images, uint8_t *__restrict__ score, int *__restrict__ hist, int rows,
                                                  int cols, int threshold) {
    const int img = blockIdx.z;
    if (blockIdx.x == 0 && blockIdx.y == 0) hist[img * 256 + threadIdx.y * 64 + threadIdx.x] = 0;      // k_tr_nms adds into it
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= cols || y >= rows) return;
    const size_t base = (size_t)img * rows * cols;
    int s = 0;
    if (x >= TR_BORDER && x < cols - TR_BORDER && y >= TR_BORDER && y < rows - TR_BORDER) {
        const uint8_t *p = images + base + (size_t)y * cols + x;
        const int c = p[0];
        const int dx[16] = {0, 1, 2, 3, 3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1};
        const int dy[16] = {-3, -3, -2, -1, 0, 1, 2, 3, 3, 3, 2, 1, 0, -1, -2, -3};
        int d[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) d[i] = (int)p[dy[i] * cols + dx[i]] - c;
        int bright = -255, dark = -255;
#pragma unroll
        for (int a = 0; a < 16; ++a) {
            int lo = 255, hi = -255;
#pragma unroll
            for (int k = 0; k < 9; ++k) {
                lo = min(lo, d[(a + k) & 15]);
                hi = max(hi, d[(a + k) & 15]);
            }
            bright = max(bright, lo);
            dark = max(dark, -hi);
        }
        s = max(0, max(bright, dark));
        if (s <= threshold) s = 0;
    }
    score[base + (size_t)y * cols + x] = (uint8_t)s;
}

__global__ __launch_bounds__(256) void k_tr_nms(const uint8_t *__restrict__ score, uint8_t *__restrict__ kept, int *__restrict__ hist, int rows, int cols) {
    __shared__ int bins[256];
    const int img = blockIdx.z, t = threadIdx.y * 64 + threadIdx.x;
    bins[t] = 0;
    __syncthreads();
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x < cols && y < rows) {
        const size_t base = (size_t)img * rows * cols;
        const uint8_t *p = score + base + (size_t)y * cols + x;
        const int s = p[0];
        bool keep = s > 0;           // s > 0 only inside the border, where all eight neighbours exist
        if (keep) {
#pragma unroll
            for (int j = -1; j <= 1; ++j)
#pragma unroll
                for (int i = -1; i <= 1; ++i) {
                    if (i == 0 && j == 0) continue;
                    const int q = p[j * cols + i];
                    const bool before = j < 0 || (j == 0 && i < 0);      // q precedes p in row-major order
                    keep = keep && (s > q || (s == q && !before));
                }
        }
        kept[base + (size_t)y * cols + x] = keep ? (uint8_t)s : (uint8_t)0;
        if (keep) atomicAdd(&bins[s], 1);                                  // counts: the order of the additions does not matter
    }
    __syncthreads();
    if (bins[t]) atomicAdd(&hist[img * 256 + t], bins[t]);
}

// One work-group per image.  The cut score T is the largest score with count(s >= T) >= max_features (0: everything is kept);
// every s > T is kept and the first `quota` pixels with s == T in row-major order.  The work-group walks the image in chunks of
// TR_BLOCK * TR_ITEMS pixels; one scan per chunk carries both counts, (s > T) in the upper and (s == T) in the lower 16 bits.
__global__ __launch_bounds__(TR_BLOCK) void k_tr_select(const uint8_t *__restrict__ kept, const int *__restrict__ hist, int rows, int cols, int max_features,
                                                        uint32_t *__restrict__ count, uint16_t *__restrict__ xy, uint8_t *__restrict__ score_out) {
    __shared__ uint32_t part[TR_BLOCK / 64];
    __shared__ int cut[2];
    const int img = blockIdx.x;
    if (threadIdx.x == 0) {
        int above = 0, T = 0, quota = 0;
        for (int s = 255; s >= 1; --s) {
            const int h = hist[img * 256 + s];
            if (above + h >= max_features) {
                T = s;
                quota = max_features - above;
                break;
            }
            above += h;
        }
        cut[0] = T;
        cut[1] = quota;
    }
    __syncthreads();
    const int T = cut[0];
    const uint32_t quota = (uint32_t)cut[1];
    const size_t npix = (size_t)rows * cols;
    const uint8_t *im = kept + (size_t)img * npix;
    uint16_t *oxy = xy + (size_t)img * max_features * 2;
    uint8_t *osc = score_out + (size_t)img * max_features;
    uint32_t run_gt = 0, run_eq = 0;
    for (size_t chunk = 0; chunk < npix; chunk += (size_t)TR_BLOCK * TR_ITEMS) {
        const size_t first = chunk + (size_t)threadIdx.x * TR_ITEMS;
        int s[TR_ITEMS];
        uint32_t mine = 0;
#pragma unroll
        for (int i = 0; i < TR_ITEMS; ++i) {
            s[i] = first + i < npix ? (int)im[first + i] : 0;
            if (s[i] > T) mine += 1u << 16;
            else if (T > 0 && s[i] == T) mine += 1u;
        }
        uint32_t total;
        const uint32_t before = tr_block_exscan(mine, part, &total);
        uint32_t gt = run_gt + (before >> 16), eq = run_eq + (before & 0xffffu);
#pragma unroll
        for (int i = 0; i < TR_ITEMS; ++i) {
            const bool is_gt = s[i] > T, is_eq = T > 0 && s[i] == T;
            if (is_gt || (is_eq && eq < quota)) {
                const uint32_t pos = gt + min(eq, quota);
                if (pos < (uint32_t)max_features) {              // holds by construction; the store stays inside the image's slots
                    const size_t px = first + i;
                    oxy[2 * pos] = (uint16_t)(px % cols);
                    oxy[2 * pos + 1] = (uint16_t)(px / cols);
                    osc[pos] = (uint8_t)s[i];
                }
            }
            gt += is_gt;
            eq += is_eq;
        }
        run_gt += total >> 16;
        run_eq += total & 0xffffu;
    }
    if (threadIdx.x == 0) count[img] = min(run_gt + min(run_eq, quota), (uint32_t)max_features);
}

// One work-group per keypoint slot: the 31 x 31 patch, its 27 x 27 box sums, one bit per thread, one ballot per wave.
__global__ __launch_bounds__(256) void k_tr_describe(const uint8_t *__restrict__ images, int rows, int cols, int max_features, const uint32_t *__restrict__ count,
                                                     const uint16_t *__restrict__ xy, uint32_t *__restrict__ desc) {
    __shared__ uint8_t patch[TR_PATCH * TR_PATCH];
    __shared__ uint16_t box[TR_BOXES * TR_BOXES];
    const int img = blockIdx.y, k = blockIdx.x, t = threadIdx.x;
    if ((uint32_t)k >= count[img]) return;
    const size_t slot = (size_t)img * max_features + k;
    const int x = xy[2 * slot], y = xy[2 * slot + 1];
    if (x < TR_BORDER || x >= cols - TR_BORDER || y < TR_BORDER || y >= rows - TR_BORDER) return;      // never: k_tr_score keeps the border
    const uint8_t *im = images + (size_t)img * rows * cols;
    for (int i = t; i < TR_PATCH * TR_PATCH; i += 256) {
        const int py = i / TR_PATCH, px = i - py * TR_PATCH;
        patch[i] = im[(size_t)(y - TR_BORDER + py) * cols + (x - TR_BORDER + px)];
    }
    __syncthreads();
    for (int i = t; i < TR_BOXES * TR_BOXES; i += 256) {
        const int by = i / TR_BOXES, bx = i - by * TR_BOXES;
        int sum = 0;
#pragma unroll
        for (int j = 0; j < 5; ++j)
#pragma unroll
            for (int l = 0; l < 5; ++l) sum += patch[(by + j) * TR_PATCH + bx + l];
        box[i] = (uint16_t)sum;          // at most 25 * 255
    }
    __syncthreads();
    const int a = (c_brief[t][1] + SSBA_BRIEF_RADIUS) * TR_BOXES + c_brief[t][0] + SSBA_BRIEF_RADIUS;
    const int b = (c_brief[t][3] + SSBA_BRIEF_RADIUS) * TR_BOXES + c_brief[t][2] + SSBA_BRIEF_RADIUS;
    const unsigned long long bits = __ballot(box[a] < box[b]);
    if ((t & 63) == 0) {
        desc[slot * TR_WORDS + (t >> 6) * 2] = (uint32_t)bits;
        desc[slot * TR_WORDS + (t >> 6) * 2 + 1] = (uint32_t)(bits >> 32);
    }
}

// ---- matcher ----------------------------------------------------------------------------------------------------------------
// Pair p matches set A = slots [p * stride, p * stride + count_a[p]) of desc_a / xy_a against set B likewise.  blockIdx.z = 0:
// the queries are A and the train side B, best_ab[p * stride + a] = the packed key of a's best b; blockIdx.z = 1: the roles
// swapped, into best_ba.  The train side passes through LDS in tiles of TR_TILE descriptors.  TR_SPLIT neighbouring lanes share a
// query and take every TR_SPLIT-th entry of the tile: a wave reads TR_SPLIT consecutive entries per step (distinct banks, each
// broadcast to the lanes of its part), 16 bytes at a time, and the lanes' packed keys meet in two shuffles.
struct MatchSets {
    const uint32_t *desc_a, *desc_b;
    const uint16_t *xy_a, *xy_b;
    const uint32_t *count_a, *count_b;
    uint32_t *best_ab, *best_ba;
    uint32_t stride;
};

__device__ __forceinline__ bool tr_gate(const TrackGate g, int xa, int ya, int xb, int yb) {
    if (g.kind == SSBA_TRACK_GATE_STEREO) return abs(ya - yb) < g.max_dy && xa - xb > 0 && xa - xb <= g.max_disparity;
    if (g.kind == SSBA_TRACK_GATE_TEMPORAL && g.radius > 0) return abs(xa - xb) <= g.radius && abs(ya - yb) <= g.radius;
    return true;
}

__global__ __launch_bounds__(TR_THREADS) void k_tr_best(MatchSets m, TrackGate g) {
    __shared__ uint4 tile[TR_TILE * 2];
    __shared__ uint32_t tile_xy[TR_TILE];
    const int pair = blockIdx.y;
    const bool swapped = blockIdx.z != 0;
    const size_t off = (size_t)pair * m.stride;
    const uint32_t nq = min(swapped ? m.count_b[pair] : m.count_a[pair], m.stride);
    const uint32_t nt = min(swapped ? m.count_a[pair] : m.count_b[pair], m.stride);
    const uint32_t q = blockIdx.x * TR_QUERIES + threadIdx.x / TR_SPLIT, part = threadIdx.x % TR_SPLIT;
    if (blockIdx.x * TR_QUERIES >= nq) return;            // the whole work-group leaves together
    const uint32_t *qd = (swapped ? m.desc_b : m.desc_a) + off * TR_WORDS;
    const uint16_t *qxy = (swapped ? m.xy_b : m.xy_a) + off * 2;
    const uint4 *td = (const uint4 *)((swapped ? m.desc_a : m.desc_b) + off * TR_WORDS);
    const uint32_t *txy = (const uint32_t *)((swapped ? m.xy_a : m.xy_b) + off * 2);
    uint32_t *best = (swapped ? m.best_ba : m.best_ab) + off;
    const bool live = q < nq;
    uint4 d0 = make_uint4(0, 0, 0, 0), d1 = d0;
    int qx = 0, qy = 0;
    if (live) {
        const uint4 *src = (const uint4 *)(qd + (size_t)q * TR_WORDS);
        d0 = src[0];
        d1 = src[1];
        qx = qxy[2 * q];
        qy = qxy[2 * q + 1];
    }
    uint32_t key = TR_NONE;
    for (uint32_t t0 = 0; t0 < nt; t0 += TR_TILE) {
        const uint32_t n = min((uint32_t)TR_TILE, nt - t0);
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < 2 * n; i += TR_THREADS) tile[i] = td[2 * (size_t)t0 + i];
        for (uint32_t i = threadIdx.x; i < n; i += TR_THREADS) tile_xy[i] = txy[t0 + i];
        __syncthreads();
#pragma unroll 2
        for (uint32_t j = part; j < n; j += TR_SPLIT) {
            const uint4 e0 = tile[2 * j], e1 = tile[2 * j + 1];
            const uint32_t p = tile_xy[j];
            const int tx = p & 0xffffu, ty = p >> 16;
            const uint32_t dist = __popc(d0.x ^ e0.x) + __popc(d0.y ^ e0.y) + __popc(d0.z ^ e0.z) + __popc(d0.w ^ e0.w) + __popc(d1.x ^ e1.x) +
                                  __popc(d1.y ^ e1.y) + __popc(d1.z ^ e1.z) + __popc(d1.w ^ e1.w);
            const bool pass = swapped ? tr_gate(g, tx, ty, qx, qy) : tr_gate(g, qx, qy, tx, ty);
            key = min(key, pass ? (dist << 16) | (t0 + j) : TR_NONE);      // the smallest index wins a tie
        }
    }
    static_assert(TR_SPLIT == 4, "two shuffles join four lanes");
    key = min(key, (uint32_t)__shfl_xor((int)key, 1, 64));
    key = min(key, (uint32_t)__shfl_xor((int)key, 2, 64));
    if (live && part == 0) best[q] = key;
}

// (a, b) is a match when each is the other's best and the distance is within max_hamming
__device__ __forceinline__ bool tr_mutual(const uint32_t *best_ab, const uint32_t *best_ba, uint32_t a, uint32_t nb, int max_hamming, uint32_t *b_out) {
    const uint32_t key = best_ab[a];
    if (key == TR_NONE || (int)(key >> 16) > max_hamming) return false;
    const uint32_t b = key & 0xffffu;
    if (b >= nb) return false;
    const uint32_t back = best_ba[b];
    if (back == TR_NONE || (back & 0xffffu) != a) return false;
    *b_out = b;
    return true;
}

__global__ __launch_bounds__(256) void k_tr_crosscheck(const uint32_t *__restrict__ best_ab, const uint32_t *__restrict__ best_ba, uint32_t na, uint32_t nb,
                                                       int max_hamming, int32_t *__restrict__ match_a, int32_t *__restrict__ dist_a) {
    const uint32_t a = blockIdx.x * 256 + threadIdx.x;
    if (a >= na) return;
    uint32_t b = 0;
    const bool ok = tr_mutual(best_ab, best_ba, a, nb, max_hamming, &b);
    match_a[a] = ok ? (int32_t)b : -1;
    dist_a[a] = ok ? (int32_t)(best_ab[a] >> 16) : -1;
}

// ---- survivors, ids, observations -------------------------------------------------------------------------------------------
// Frame f: left keypoints are image f of the feature arrays, right keypoints image frames + f.  A survivor carries its
// disparity in sixteenths of a pixel, whichever source it has.
struct Survivors {
    uint32_t *count;          // frames
    uint32_t *desc;           // frames * stride * 8
    uint16_t *xy;             // frames * stride * 2
    int32_t *d16;             // frames * stride
};

__global__ __launch_bounds__(TR_BLOCK) void k_tr_stereo(const uint32_t *__restrict__ count, const uint16_t *__restrict__ xy, const uint32_t *__restrict__ desc,
                                                        const uint32_t *__restrict__ best_lr, const uint32_t *__restrict__ best_rl,
                                                        const int16_t *__restrict__ disp16, int frames, int rows, int cols, uint32_t stride, int max_hamming,
                                                        Survivors out) {
    __shared__ uint32_t part[TR_BLOCK / 64];
    const int f = blockIdx.x;
    const uint32_t nl = min(count[f], stride), nr = disp16 ? 0u : min(count[frames + f], stride);
    const size_t lo = (size_t)f * stride, ro = (size_t)(frames + f) * stride;
    int d16[TR_ITEMS];
    uint32_t mine = 0;
#pragma unroll
    for (int i = 0; i < TR_ITEMS; ++i) {
        const uint32_t a = threadIdx.x * TR_ITEMS + i;
        d16[i] = 0;
        if (a < nl) {
            const int x = xy[2 * (lo + a)], y = xy[2 * (lo + a) + 1];
            if (disp16) {
                if (x < cols && y < rows) d16[i] = disp16[((size_t)f * rows + y) * cols + x];
            } else {
                uint32_t b = 0;
                if (tr_mutual(best_lr + lo, best_rl + lo, a, nr, max_hamming, &b)) d16[i] = 16 * (x - (int)xy[2 * (ro + b)]);
            }
        }
        mine += d16[i] > 0;
    }
    uint32_t total;
    uint32_t pos = tr_block_exscan(mine, part, &total);
#pragma unroll
    for (int i = 0; i < TR_ITEMS; ++i) {
        if (d16[i] <= 0) continue;
        const uint32_t a = threadIdx.x * TR_ITEMS + i;
        const size_t src = lo + a, dst = lo + pos;
        if (pos < stride) {
            const uint4 *s = (const uint4 *)(desc + src * TR_WORDS);
            uint4 *d = (uint4 *)(out.desc + dst * TR_WORDS);
            d[0] = s[0];
            d[1] = s[1];
            out.xy[2 * dst] = xy[2 * src];
            out.xy[2 * dst + 1] = xy[2 * src + 1];
            out.d16[dst] = d16[i];
        }
        ++pos;
    }
    if (threadIdx.x == 0) out.count[f] = min(total, stride);
}

// One work-group walks the frames.  id[f * stride + j] of survivor j of frame f; length[id] counts its observations (every id
// occurs at most once per frame, because a cross-checked match is one to one, so the thread that owns the survivor adds alone).
__global__ __launch_bounds__(TR_BLOCK) void k_tr_link(const uint32_t *__restrict__ surv_count, const uint32_t *__restrict__ best_pn, const uint32_t *__restrict__ best_np,
                                                      int frames, uint32_t stride, int max_hamming, uint32_t *__restrict__ id, uint32_t *__restrict__ length,
                                                      uint32_t *__restrict__ num_ids) {
    __shared__ uint32_t part[TR_BLOCK / 64];
    for (size_t i = threadIdx.x; i < (size_t)frames * stride; i += TR_BLOCK) length[i] = 0;
    __syncthreads();
    uint32_t next = 0;
    for (int f = 0; f < frames; ++f) {
        const uint32_t n = min(surv_count[f], stride), np = f ? min(surv_count[f - 1], stride) : 0u;
        const size_t cur = (size_t)f * stride, prev = (size_t)(f ? f - 1 : 0) * stride;
        uint32_t inherited[TR_ITEMS], fresh = 0;
#pragma unroll
        for (int i = 0; i < TR_ITEMS; ++i) {
            const uint32_t j = threadIdx.x * TR_ITEMS + i;
            inherited[i] = TR_NONE;
            if (j >= n) continue;
            uint32_t a = 0;
            // pair f - 1 has A = the survivors of frame f - 1 and B = those of frame f: j is a B entry
            if (f && tr_mutual(best_np + prev, best_pn + prev, j, np, max_hamming, &a)) inherited[i] = id[prev + a];
            fresh += inherited[i] == TR_NONE;
        }
        uint32_t total;
        uint32_t pos = next + tr_block_exscan(fresh, part, &total);
#pragma unroll
        for (int i = 0; i < TR_ITEMS; ++i) {
            const uint32_t j = threadIdx.x * TR_ITEMS + i;
            if (j >= n) continue;
            const uint32_t mine = inherited[i] == TR_NONE ? pos++ : inherited[i];
            id[cur + j] = mine;
            if (mine < (uint32_t)frames * stride) length[mine] += 1;
        }
        next += total;
        __syncthreads();          // frame f's ids are read by frame f + 1 of this same work-group
    }
    if (threadIdx.x == 0) *num_ids = next;
}

// The same work-group shape: new ids = a running prefix over (length >= min_track_length) in id order, which is the order of
// first appearance; then the kept observations of every frame in keypoint order.  refined: NULL, or (u, v, d) in 1/256 pixel
// per survivor slot from k_tr_refine, which has also set the id of every survivor it dropped to TR_NONE.
__global__ __launch_bounds__(TR_BLOCK) void k_tr_prune(const uint32_t *__restrict__ surv_count, const uint16_t *__restrict__ surv_xy, const int32_t *__restrict__ surv_d16,
                                                       const uint32_t *__restrict__ id, const uint32_t *__restrict__ length, const uint32_t *__restrict__ num_ids,
                                                       int frames, uint32_t stride, int min_track_length, const int32_t *__restrict__ refined,
                                                       uint32_t *__restrict__ new_id, uint32_t *__restrict__ state_start, uint32_t *__restrict__ point_id,
                                                       double *__restrict__ uvd, uint32_t *__restrict__ totals) {
    __shared__ uint32_t part[TR_BLOCK / 64];
    const uint32_t ids = min(*num_ids, (uint32_t)frames * stride);
    uint32_t run = 0;
    for (uint32_t chunk = 0; chunk < ids; chunk += TR_BLOCK * TR_ITEMS) {
        uint32_t keep[TR_ITEMS], mine = 0;
#pragma unroll
        for (int i = 0; i < TR_ITEMS; ++i) {
            const uint32_t t = chunk + threadIdx.x * TR_ITEMS + i;
            keep[i] = t < ids && length[t] >= (uint32_t)min_track_length;
            mine += keep[i];
        }
        uint32_t total;
        uint32_t pos = run + tr_block_exscan(mine, part, &total);
#pragma unroll
        for (int i = 0; i < TR_ITEMS; ++i) {
            const uint32_t t = chunk + threadIdx.x * TR_ITEMS + i;
            if (t < ids) new_id[t] = keep[i] ? pos++ : TR_NONE;
        }
        run += total;
    }
    __syncthreads();
    uint32_t written = 0;
    for (int f = 0; f < frames; ++f) {
        const uint32_t n = min(surv_count[f], stride);
        const size_t cur = (size_t)f * stride;
        uint32_t renamed[TR_ITEMS], mine = 0;
#pragma unroll
        for (int i = 0; i < TR_ITEMS; ++i) {
            const uint32_t j = threadIdx.x * TR_ITEMS + i;
            renamed[i] = TR_NONE;
            if (j < n && id[cur + j] < ids) renamed[i] = new_id[id[cur + j]];
            mine += renamed[i] != TR_NONE;
        }
        uint32_t total;
        uint32_t pos = written + tr_block_exscan(mine, part, &total);
        if (threadIdx.x == 0) state_start[f] = written;
#pragma unroll
        for (int i = 0; i < TR_ITEMS; ++i) {
            if (renamed[i] == TR_NONE) continue;
            const uint32_t j = threadIdx.x * TR_ITEMS + i;
            point_id[pos] = renamed[i];                       // pos < frames * stride: at most one observation per survivor slot
            if (refined) {
#pragma unroll
                for (int c = 0; c < 3; ++c) uvd[3 * (size_t)pos + c] = (double)refined[3 * (cur + j) + c] / 256.0;
            } else {
                uvd[3 * (size_t)pos] = (double)surv_xy[2 * (cur + j)];
                uvd[3 * (size_t)pos + 1] = (double)surv_xy[2 * (cur + j) + 1];
                uvd[3 * (size_t)pos + 2] = (double)surv_d16[cur + j] / 16.0;
            }
            ++pos;
        }
        written += total;
    }
    if (threadIdx.x == 0) {
        state_start[frames] = written;
        totals[0] = written;
        totals[1] = run;
    }
}

// ---- sub-pixel refinement ---------------------------------------------------------------------------------------------------
// One wave places one 15 x 15 template.  Lane l owns window pixels l, l + 64, l + 128, l + 192 (< 225) and keeps their T, gx, gy
// in registers.  Every tap an evaluation can read lies within max_shift + 8 pixels of the start, so that neighbourhood of the
// target is staged in LDS once, (16 + 2 max_shift)^2 bytes in rows of RF_TILE, and the dependent evaluations read LDS only.
// The sums are integers and meet in xor butterflies, so every lane holds the same step and the control flow is wave-uniform.
constexpr int RF_RADIUS = 7;
constexpr int RF_SIDE = 2 * RF_RADIUS + 1;           // 15
constexpr int RF_PIXELS = RF_SIDE * RF_SIDE;         // 225
constexpr int RF_PER_LANE = 4;
constexpr int RF_TILE = 32;                          // 16 + 2 * 8, the largest max_shift
constexpr int RF_WAVES = 4;
constexpr int RF_ITEM = 7;

static_assert(RF_PER_LANE * 64 >= RF_PIXELS, "the lanes of a wave cover the window");

struct RefineTemplate {
    int T[RF_PER_LANE], gx[RF_PER_LANE], gy[RF_PER_LANE];
};

struct RefineResult {
    int x, y, status;
    uint32_t sad;
};

// sums modulo 2^32: a signed total is the cast of the result
__device__ __forceinline__ uint32_t rf_wave_sum(uint32_t v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += (uint32_t)__shfl_xor((int)v, d, 64);
    return v;
}

__device__ __forceinline__ long long rf_wave_sum64(long long v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, d, 64), hi = (uint32_t)__shfl_xor((int)(v >> 32), d, 64);
        v += (long long)(((unsigned long long)hi << 32) | lo);
    }
    return v;
}

// false: the 17 x 17 support of the anchor leaves its image (nothing is read)
__device__ __forceinline__ bool rf_template(const uint8_t *__restrict__ A, int rows, int cols, int ax, int ay, int lane, RefineTemplate *t) {
    if (ax < RF_RADIUS + 1 || ay < RF_RADIUS + 1 || ax >= cols - RF_RADIUS - 1 || ay >= rows - RF_RADIUS - 1) return false;
#pragma unroll
    for (int m = 0; m < RF_PER_LANE; ++m) {
        const int k = lane + 64 * m;
        t->T[m] = t->gx[m] = t->gy[m] = 0;
        if (k < RF_PIXELS) {
            const int j = k / RF_SIDE - RF_RADIUS, i = k % RF_SIDE - RF_RADIUS;
            const uint8_t *p = A + (size_t)(ay + j) * cols + (ax + i);
            t->T[m] = p[0];
            t->gx[m] = (int)p[1] - (int)p[-1];
            t->gy[m] = (int)p[cols] - (int)p[-cols];
        }
    }
    return true;
}

// a tap of the window at (px, py) falls outside the image
__device__ __forceinline__ bool rf_leaves(int px, int py, int rows, int cols) {
    const int cx = px >> 8, cy = py >> 8;
    return cx < RF_RADIUS || cy < RF_RADIUS || cx >= cols - RF_RADIUS - 1 || cy >= rows - RF_RADIUS - 1;
}

// The only floating point of the library before the outputs: IEEE doubles, every product rounded before the subtraction.
__device__ __forceinline__ void rf_step(int H11, int H12, int H22, long long det, long long bx, long long by, int mode, double *dx, double *dy) {
#pragma clang fp contract(off)
    if (mode) {
        *dx = rint((double)bx / ((double)H11 * 128.0));
        *dy = 0.0;
        return;
    }
    const double scale = (double)det * 128.0;
    const double nx = (double)H22 * (double)bx - (double)H12 * (double)by;
    const double ny = (double)H11 * (double)by - (double)H12 * (double)bx;
    *dx = rint(nx / scale);
    *dy = rint(ny / scale);
}

// The position of template t in image B, started at (x0, y0) in 1/256 pixel; mode 1: x only.  Every thread of the work-group
// calls it together, because the staging is fenced by two barriers; a wave with live == false only keeps them company and gets
// {x0, y0, OK, 0}.  `tile` is the wave's own RF_TILE * RF_TILE bytes.
__device__ __forceinline__ RefineResult rf_solve(uint8_t *tile, bool live, const RefineTemplate &t, const uint8_t *__restrict__ B, int rows, int cols, int x0,
                                                 int y0, int mode, const ssba_track_refine_params rp, int lane) {
    RefineResult r = {x0, y0, SSBA_TRACK_REFINE_OK, 0u};
    if (live && rf_leaves(x0, y0, rows, cols)) {
        r.status = SSBA_TRACK_REFINE_EDGE;
        live = false;
    }
    const int side = 16 + 2 * rp.max_shift, ox = (x0 >> 8) - rp.max_shift - RF_RADIUS, oy = (y0 >> 8) - rp.max_shift - RF_RADIUS;
    if (live)
        for (int k = lane; k < side * side; k += 64) {
            const int ty = k / side, tx = k - ty * side;
            const int sx = min(max(ox + tx, 0), cols - 1), sy = min(max(oy + ty, 0), rows - 1);      // a clamped byte is never a tap
            tile[ty * RF_TILE + tx] = B[(size_t)sy * cols + sx];
        }
    __syncthreads();
    if (live) {
        int h11 = 0, h12 = 0, h22 = 0;
#pragma unroll
        for (int m = 0; m < RF_PER_LANE; ++m) {
            const int gx = t.gx[m], gy = mode ? 0 : t.gy[m];
            h11 += gx * gx;
            h12 += gx * gy;
            h22 += gy * gy;
        }
        const int H11 = (int)rf_wave_sum((uint32_t)h11), H12 = (int)rf_wave_sum((uint32_t)h12), H22 = (int)rf_wave_sum((uint32_t)h22);      // |H| < 2^26
        const long long det = (long long)H11 * H22 - (long long)H12 * H12;
        const bool flat = mode ? H11 <= 0 : det <= 0;
        int px = x0, py = y0, status = SSBA_TRACK_REFINE_ITERATIONS;
        uint32_t sad = 0;
        for (int it = 0; it < rp.iterations; ++it) {
            if (rf_leaves(px, py, rows, cols)) {
                status = SSBA_TRACK_REFINE_EDGE;
                break;
            }
            if (flat) {
                status = SSBA_TRACK_REFINE_FLAT;
                break;
            }
            long long bx = 0, by = 0;
            uint32_t sabs = 0;
#pragma unroll
            for (int m = 0; m < RF_PER_LANE; ++m) {
                const int k = lane + 64 * m;
                if (k < RF_PIXELS) {
                    const int j = k / RF_SIDE - RF_RADIUS, i = k % RF_SIDE - RF_RADIUS;
                    const int X = px + 256 * i, Y = py + 256 * j, fx = X & 255, fy = Y & 255;
                    // |p - start| <= 256 max_shift (the FAR test of the step before): 0 <= column, row and column + 1, row + 1 < side
                    const uint8_t *q = tile + ((Y >> 8) - oy) * RF_TILE + ((X >> 8) - ox);
                    const int S = (256 - fx) * (256 - fy) * q[0] + fx * (256 - fy) * q[1] + (256 - fx) * fy * q[RF_TILE] + fx * fy * q[RF_TILE + 1];
                    const int e = S - 65536 * t.T[m];
                    bx += (long long)t.gx[m] * e;
                    if (!mode) by += (long long)t.gy[m] * e;
                    sabs += (uint32_t)abs(e);
                }
            }
            bx = rf_wave_sum64(bx);
            by = rf_wave_sum64(by);
            sad = rf_wave_sum(sabs) >> 16;                      // the sum is below 225 * 255 * 65536 < 2^32
            double dx, dy;
            rf_step(H11, H12, H22, det, bx, by, mode, &dx, &dy);
            if (!(fabs(dx) < 1e9 && fabs(dy) < 1e9)) {          // far beyond any max_shift; below, the step is an exact int
                status = SSBA_TRACK_REFINE_FAR;
                break;
            }
            const int sx = (int)dx, sy = (int)dy;
            px -= sx;
            py -= sy;
            if (max(abs(px - x0), abs(py - y0)) > 256 * rp.max_shift) {
                status = SSBA_TRACK_REFINE_FAR;
                break;
            }
            if (max(abs(sx), abs(sy)) <= 1) {
                status = SSBA_TRACK_REFINE_OK;
                break;
            }
        }
        if (status == SSBA_TRACK_REFINE_OK && rp.max_sad > 0 && sad > (uint32_t)rp.max_sad) status = SSBA_TRACK_REFINE_SAD;
        r.status = status;
        r.sad = sad;
        if (status == SSBA_TRACK_REFINE_OK) {
            r.x = px;
            r.y = py;
        }
    }
    __syncthreads();          // the tile is free for the next call
    return r;
}

// ssba_track_refine: item k = anchor image, ax, ay, target image, x0, y0, mode; the host has checked the image indices and the mode
__global__ __launch_bounds__(64 * RF_WAVES) void k_tr_refine_items(const uint8_t *__restrict__ images, int rows, int cols, const int32_t *__restrict__ items,
                                                                    uint32_t num_items, ssba_track_refine_params rp, int32_t *__restrict__ xy,
                                                                    int32_t *__restrict__ status, uint32_t *__restrict__ sad) {
    __shared__ uint8_t tiles[RF_WAVES][RF_TILE * RF_TILE];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t k = blockIdx.x * RF_WAVES + wave;
    const bool live = k < num_items;
    int it[RF_ITEM] = {0, 0, 0, 0, 0, 0, 0};
    if (live)
#pragma unroll
        for (int c = 0; c < RF_ITEM; ++c) it[c] = items[(size_t)k * RF_ITEM + c];
    const size_t npix = (size_t)rows * cols;
    RefineTemplate t = {};
    const bool inside = live && rf_template(images + (size_t)it[0] * npix, rows, cols, it[1], it[2], lane, &t);
    RefineResult r = rf_solve(tiles[wave], inside, t, images + (size_t)it[3] * npix, rows, cols, it[4], it[5], it[6], rp, lane);
    if (live && lane == 0) {
        xy[2 * (size_t)k] = r.x;
        xy[2 * (size_t)k + 1] = r.y;
        status[k] = inside ? r.status : SSBA_TRACK_REFINE_EDGE;
        sad[k] = r.sad;
    }
}

// anchor[id] = the survivor slot f * stride + j that issued the id: the survivor that inherited none (k_tr_link's test)
__global__ __launch_bounds__(256) void k_tr_anchor(const uint32_t *__restrict__ surv_count, const uint32_t *__restrict__ best_pn, const uint32_t *__restrict__ best_np,
                                                   const uint32_t *__restrict__ id, int frames, uint32_t stride, int max_hamming, uint32_t *__restrict__ anchor,
                                                   uint32_t *__restrict__ dropped) {
    const int f = blockIdx.y;
    const uint32_t j = blockIdx.x * 256 + threadIdx.x;
    if (f == 0 && j == 0) *dropped = 0;           // k_tr_refine counts into it
    if (j >= min(surv_count[f], stride)) return;
    const uint32_t np = f ? min(surv_count[f - 1], stride) : 0u;
    const size_t cur = (size_t)f * stride, prev = (size_t)(f ? f - 1 : 0) * stride;
    uint32_t a = 0;
    if (f && tr_mutual(best_np + prev, best_pn + prev, j, np, max_hamming, &a)) return;
    const uint32_t mine = id[cur + j];
    if (mine < (uint32_t)frames * stride) anchor[mine] = (uint32_t)(cur + j);
}

// Survivor j of frame f against the template of its id's anchor: the left position in 2-D from the keypoint (the anchor itself
// keeps its pixel), then with right images the right position in x only on the refined row, d = x_left - x_right.  A survivor
// whose status is not OK is dropped: its id slot is masked for k_tr_prune and its track is one shorter (integer atomics, the
// order does not matter).  refined[slot] = (u, v, d) in 1/256 pixel.
__global__ __launch_bounds__(64 * RF_WAVES) void k_tr_refine(const uint8_t *__restrict__ images, int frames, int rows, int cols, int has_right,
                                                              const uint32_t *__restrict__ surv_count, const uint16_t *__restrict__ surv_xy,
                                                              const int32_t *__restrict__ surv_d16, const uint32_t *__restrict__ anchor, uint32_t stride,
                                                              ssba_track_refine_params rp, uint32_t *id, uint32_t *length, int32_t *__restrict__ refined,
                                                              uint32_t *dropped) {
    __shared__ uint8_t tiles[RF_WAVES][RF_TILE * RF_TILE];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int f = blockIdx.y;
    const uint32_t n = min(surv_count[f], stride), j = blockIdx.x * RF_WAVES + wave;
    if (blockIdx.x * RF_WAVES >= n) return;          // the whole work-group leaves together
    const size_t npix = (size_t)rows * cols, cur = (size_t)f * stride, slots = (size_t)frames * stride;
    bool live = j < n;
    uint32_t mine = TR_NONE, a = 0;
    if (live) {
        mine = id[cur + j];
        live = mine < slots;
        if (live) a = anchor[mine];
        live = live && a < slots;                    // holds: every id has the slot that issued it
    }
    int x = 0, y = 0, d16 = 0, ax = 0, ay = 0;
    if (live) {
        x = surv_xy[2 * (cur + j)];
        y = surv_xy[2 * (cur + j) + 1];
        d16 = surv_d16[cur + j];
        ax = surv_xy[2 * (size_t)a];
        ay = surv_xy[2 * (size_t)a + 1];
    }
    RefineTemplate t = {};
    const bool inside = live && rf_template(images + (size_t)(a / stride) * npix, rows, cols, ax, ay, lane, &t);      // holds: keypoints keep 15 pixels
    const bool self = a == cur + j;
    const RefineResult l = rf_solve(tiles[wave], inside && !self, t, images + (size_t)f * npix, rows, cols, 256 * x, 256 * y, 0, rp, lane);
    int status = inside ? l.status : SSBA_TRACK_REFINE_EDGE, dq8 = 16 * d16;
    const bool pair = has_right && inside && status == SSBA_TRACK_REFINE_OK;
    const RefineResult r = rf_solve(tiles[wave], pair, t, images + (size_t)(has_right ? frames + f : f) * npix, rows, cols, l.x - 16 * d16, l.y, 1, rp, lane);
    if (pair) {
        status = r.status;
        dq8 = l.x - r.x;
        if (status == SSBA_TRACK_REFINE_OK && dq8 <= 0) status = SSBA_TRACK_REFINE_DISPARITY;
    }
    if (live && lane == 0) {
        refined[3 * (cur + j)] = l.x;
        refined[3 * (cur + j) + 1] = l.y;
        refined[3 * (cur + j) + 2] = dq8;
        if (status != SSBA_TRACK_REFINE_OK) {
            id[cur + j] = TR_NONE;
            atomicSub(&length[mine], 1u);
            atomicAdd(dropped, 1u);
        }
    }
}

// ---- the stream -------------------------------------------------------------------------------------------------------------
// One frame against the state a stream keeps on the device (include/ssba_tracks.h, "Streaming"; the numpy statement is
// tests/tracks_stream_reference.py).  The survivors of the previous and of the current frame are two buffers that swap roles;
// the ring holds one entry per survivor slot for each of the last `window` frames.
constexpr int TS_SIDE = 2 * RF_RADIUS + 3;           // 17: the template and the ring of pixels its gradients read
constexpr int TS_PATCH = TS_SIDE * TS_SIDE;          // 289
constexpr int TS_PATCH_WORDS = (TS_PATCH + 3) / 4;   // a patch starts on a word, so that an inherited one is copied in words
constexpr int TS_PATCH_STRIDE = 4 * TS_PATCH_WORDS;

static_assert(RF_RADIUS + 1 <= TR_BORDER, "the patch of a keypoint lies inside its image");

struct StreamEntry {
    uint32_t id;              // as issued
    uint32_t from;            // the slot of the frame before that the id was inherited from, TR_NONE: the id was issued here
    uint32_t kept;            // 0: the refinement dropped the observation
    int32_t v[3];             // whole pixel: x, y, d16; refined: u, v, d in 1/256 pixel
};

// an entry's observation as k_tr_prune writes it: q8 / 256.0, or (x, y, d16 / 16.0)
__device__ __forceinline__ void ts_uvd(const int32_t *v, bool refined, double *__restrict__ out) {
    out[0] = refined ? (double)v[0] / 256.0 : (double)v[0];
    out[1] = refined ? (double)v[1] / 256.0 : (double)v[1];
    out[2] = refined ? (double)v[2] / 256.0 : (double)v[2] / 16.0;
}

// k_tr_link for one frame: B = the current survivors, A = those of the frame before (np = 0 on the first push).  The fresh ids
// start at *next_id, which is the stream's running id.
__global__ __launch_bounds__(TR_BLOCK) void k_ts_link(const uint32_t *__restrict__ cur_count, const uint32_t *__restrict__ prev_count, int has_prev,
                                                      const uint32_t *__restrict__ best_pn, const uint32_t *__restrict__ best_np,
                                                      const uint32_t *__restrict__ prev_id, uint32_t stride, int max_hamming, uint32_t *__restrict__ cur_id,
                                                      uint32_t *__restrict__ from, uint32_t *next_id) {
    __shared__ uint32_t part[TR_BLOCK / 64];
    const uint32_t n = min(*cur_count, stride), np = has_prev ? min(*prev_count, stride) : 0u;
    const uint32_t next = *next_id;
    uint32_t inherited[TR_ITEMS], src[TR_ITEMS], fresh = 0;
#pragma unroll
    for (int i = 0; i < TR_ITEMS; ++i) {
        const uint32_t j = threadIdx.x * TR_ITEMS + i;
        inherited[i] = src[i] = TR_NONE;
        if (j >= n) continue;
        uint32_t a = 0;
        if (np && tr_mutual(best_np, best_pn, j, np, max_hamming, &a)) {
            inherited[i] = prev_id[a];
            src[i] = a;
        }
        fresh += src[i] == TR_NONE;
    }
    uint32_t total;
    uint32_t pos = next + tr_block_exscan(fresh, part, &total);       // its barriers stand between every read of *next_id and the write below
#pragma unroll
    for (int i = 0; i < TR_ITEMS; ++i) {
        const uint32_t j = threadIdx.x * TR_ITEMS + i;
        if (j >= n) continue;
        cur_id[j] = src[i] == TR_NONE ? pos++ : inherited[i];
        from[j] = src[i];
    }
    if (threadIdx.x == 0) *next_id = next + total;
}

// One wave per survivor: the anchor patch of its track.  An inheriting survivor copies its predecessor's, a fresh one cuts its
// own from the left image.
__global__ __launch_bounds__(64 * RF_WAVES) void k_ts_carry(const uint8_t *__restrict__ left, int rows, int cols, const uint32_t *__restrict__ cur_count,
                                                             const uint32_t *__restrict__ prev_count, const uint16_t *__restrict__ xy,
                                                             const uint32_t *__restrict__ from, uint32_t stride, const uint8_t *__restrict__ prev_patch,
                                                             uint8_t *__restrict__ cur_patch) {
    const int lane = threadIdx.x & 63;
    const uint32_t j = blockIdx.x * RF_WAVES + (threadIdx.x >> 6);
    if (j >= min(*cur_count, stride)) return;
    const uint32_t src = from[j];
    uint8_t *dst = cur_patch + (size_t)j * TS_PATCH_STRIDE;
    if (src != TR_NONE) {
        if (src >= min(*prev_count, stride)) return;                  // never: a link names a survivor of the frame before
        const uint32_t *s = (const uint32_t *)(prev_patch + (size_t)src * TS_PATCH_STRIDE);
        for (int k = lane; k < TS_PATCH_WORDS; k += 64) ((uint32_t *)dst)[k] = s[k];
        return;
    }
    const int x = xy[2 * j], y = xy[2 * j + 1];
    // Holds: keypoints keep 15 pixels.  Where rf_template would answer EDGE for such an anchor, a patch of zeros is stored, which
    // k_ts_refine finds FLAT: the observations of such a track would be dropped either way, under another status.
    const bool inside = x >= RF_RADIUS + 1 && y >= RF_RADIUS + 1 && x < cols - RF_RADIUS - 1 && y < rows - RF_RADIUS - 1;
    for (int k = lane; k < TS_PATCH; k += 64) {
        const int py = k / TS_SIDE, px = k - py * TS_SIDE;
        dst[k] = inside ? left[(size_t)(y - RF_RADIUS - 1 + py) * cols + (x - RF_RADIUS - 1 + px)] : (uint8_t)0;
    }
}

// rf_template from a stored patch: the same T, gx, gy as from the image the patch was cut from
__device__ __forceinline__ void ts_template(const uint8_t *__restrict__ P, int lane, RefineTemplate *t) {
#pragma unroll
    for (int m = 0; m < RF_PER_LANE; ++m) {
        const int k = lane + 64 * m;
        t->T[m] = t->gx[m] = t->gy[m] = 0;
        if (k < RF_PIXELS) {
            const uint8_t *p = P + (k / RF_SIDE + 1) * TS_SIDE + (k % RF_SIDE + 1);
            t->T[m] = p[0];
            t->gx[m] = (int)p[1] - (int)p[-1];
            t->gy[m] = (int)p[TS_SIDE] - (int)p[-TS_SIDE];
        }
    }
}

// k_tr_refine for one frame with the template from the patch store: images = the left image, then the right one when there is one
__global__ __launch_bounds__(64 * RF_WAVES) void k_ts_refine(const uint8_t *__restrict__ images, int rows, int cols, int has_right,
                                                              const uint32_t *__restrict__ cur_count, const uint16_t *__restrict__ xy,
                                                              const int32_t *__restrict__ d16s, const uint32_t *__restrict__ from,
                                                              const uint8_t *__restrict__ patch, uint32_t stride, ssba_track_refine_params rp,
                                                              int32_t *__restrict__ refined, int32_t *__restrict__ status_out) {
    __shared__ uint8_t tiles[RF_WAVES][RF_TILE * RF_TILE];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t n = min(*cur_count, stride), j = blockIdx.x * RF_WAVES + wave;
    if (blockIdx.x * RF_WAVES >= n) return;          // the whole work-group leaves together
    const size_t npix = (size_t)rows * cols;
    const bool live = j < n;
    int x = 0, y = 0, d16 = 0;
    bool self = false;
    RefineTemplate t = {};
    if (live) {
        x = xy[2 * j];
        y = xy[2 * j + 1];
        d16 = d16s[j];
        self = from[j] == TR_NONE;
        ts_template(patch + (size_t)j * TS_PATCH_STRIDE, lane, &t);
    }
    const RefineResult l = rf_solve(tiles[wave], live && !self, t, images, rows, cols, 256 * x, 256 * y, 0, rp, lane);
    int status = l.status, dq8 = 16 * d16;
    const bool pair = has_right && live && status == SSBA_TRACK_REFINE_OK;
    const RefineResult r = rf_solve(tiles[wave], pair, t, images + (has_right ? npix : 0), rows, cols, l.x - 16 * d16, l.y, 1, rp, lane);
    if (pair) {
        status = r.status;
        dq8 = l.x - r.x;
        if (status == SSBA_TRACK_REFINE_OK && dq8 <= 0) status = SSBA_TRACK_REFINE_DISPARITY;
    }
    if (live && lane == 0) {
        refined[3 * j] = l.x;
        refined[3 * j + 1] = l.y;
        refined[3 * j + 2] = dq8;
        status_out[j] = status;
    }
}

// The frame's ring entry, and its kept survivors compacted into the push outputs: out_scalars = kept, dropped, the running id.
// refined / status: NULL for whole-pixel observations.
__global__ __launch_bounds__(TR_BLOCK) void k_ts_emit(const uint32_t *__restrict__ cur_count, const uint16_t *__restrict__ xy, const int32_t *__restrict__ d16s,
                                                      const uint32_t *__restrict__ cur_id, const uint32_t *__restrict__ from,
                                                      const int32_t *__restrict__ refined, const int32_t *__restrict__ status, uint32_t stride,
                                                      const uint32_t *__restrict__ next_id, StreamEntry *__restrict__ entries, uint32_t *__restrict__ entry_count,
                                                      uint32_t *__restrict__ out_scalars, double *__restrict__ out_uvd, uint32_t *__restrict__ out_id) {
    __shared__ uint32_t part[TR_BLOCK / 64];
    const uint32_t n = min(*cur_count, stride);
    StreamEntry e[TR_ITEMS];
    uint32_t mine = 0;
#pragma unroll
    for (int i = 0; i < TR_ITEMS; ++i) {
        const uint32_t j = threadIdx.x * TR_ITEMS + i;
        e[i].kept = 0;
        if (j >= n) continue;
        e[i].id = cur_id[j];
        e[i].from = from[j];
        e[i].kept = status ? status[j] == SSBA_TRACK_REFINE_OK : 1;
        if (refined) {
#pragma unroll
            for (int c = 0; c < 3; ++c) e[i].v[c] = refined[3 * j + c];
        } else {
            e[i].v[0] = xy[2 * j];
            e[i].v[1] = xy[2 * j + 1];
            e[i].v[2] = d16s[j];
        }
        entries[j] = e[i];
        mine += e[i].kept;
    }
    uint32_t total;
    uint32_t pos = tr_block_exscan(mine, part, &total);
#pragma unroll
    for (int i = 0; i < TR_ITEMS; ++i) {
        if (!e[i].kept) continue;
        if (pos < stride) {                          // holds: at most one observation per survivor slot
            out_id[pos] = e[i].id;
            ts_uvd(e[i].v, refined != nullptr, out_uvd + 3 * (size_t)pos);
        }
        ++pos;
    }
    if (threadIdx.x == 0) {
        *entry_count = n;
        out_scalars[0] = total;
        out_scalars[1] = n - total;
        out_scalars[2] = *next_id;
    }
}

// k_tr_link and k_tr_prune on stored links: one work-group walks the `frames` ring entries from ring slot `first` on (the ring
// has `ring` slots and wraps).  A survivor of the walk's first frame starts a track whatever it inherited before the window.
__global__ __launch_bounds__(TR_BLOCK) void k_ts_window(const StreamEntry *__restrict__ entries, const uint32_t *__restrict__ entry_count, uint32_t ring,
                                                        uint32_t first, int frames, uint32_t stride, int min_track_length, int refined, uint32_t *local,
                                                        uint32_t *length, uint32_t *new_id, uint32_t *__restrict__ state_start, uint32_t *__restrict__ point_id,
                                                        double *__restrict__ uvd, uint32_t *__restrict__ totals) {
    __shared__ uint32_t part[TR_BLOCK / 64];
    const uint32_t slots = (uint32_t)frames * stride;
    for (uint32_t i = threadIdx.x; i < slots; i += TR_BLOCK) length[i] = 0;
    __syncthreads();
    uint32_t next = 0, np = 0;
    for (int f = 0; f < frames; ++f) {
        const uint32_t r = (first + f) % ring, n = min(entry_count[r], stride);
        const StreamEntry *in = entries + (size_t)r * stride;
        const size_t cur = (size_t)f * stride, prev = (size_t)(f ? f - 1 : 0) * stride;
        uint32_t inherited[TR_ITEMS], kept[TR_ITEMS], fresh = 0;
#pragma unroll
        for (int i = 0; i < TR_ITEMS; ++i) {
            const uint32_t j = threadIdx.x * TR_ITEMS + i;
            inherited[i] = TR_NONE;
            kept[i] = 0;
            if (j >= n) continue;
            const uint32_t src = in[j].from;
            kept[i] = in[j].kept;
            if (f && src < np) inherited[i] = local[prev + src];
            fresh += inherited[i] == TR_NONE;
        }
        uint32_t total;
        uint32_t pos = next + tr_block_exscan(fresh, part, &total);
#pragma unroll
        for (int i = 0; i < TR_ITEMS; ++i) {
            const uint32_t j = threadIdx.x * TR_ITEMS + i;
            if (j >= n) continue;
            const uint32_t mine = inherited[i] == TR_NONE ? pos++ : inherited[i];
            local[cur + j] = mine;
            if (kept[i] && mine < slots) length[mine] += 1;      // a link is one to one: the thread that owns the survivor adds alone
        }
        next += total;
        np = n;
        __syncthreads();          // frame f's local ids are read by frame f + 1 of this same work-group
    }
    const uint32_t ids = min(next, slots);
    uint32_t run = 0;
    for (uint32_t chunk = 0; chunk < ids; chunk += TR_BLOCK * TR_ITEMS) {
        uint32_t keep[TR_ITEMS], mine = 0;
#pragma unroll
        for (int i = 0; i < TR_ITEMS; ++i) {
            const uint32_t t = chunk + threadIdx.x * TR_ITEMS + i;
            keep[i] = t < ids && length[t] >= (uint32_t)min_track_length;
            mine += keep[i];
        }
        uint32_t total;
        uint32_t pos = run + tr_block_exscan(mine, part, &total);
#pragma unroll
        for (int i = 0; i < TR_ITEMS; ++i) {
            const uint32_t t = chunk + threadIdx.x * TR_ITEMS + i;
            if (t < ids) new_id[t] = keep[i] ? pos++ : TR_NONE;
        }
        run += total;
    }
    __syncthreads();
    uint32_t written = 0;
    for (int f = 0; f < frames; ++f) {
        const uint32_t r = (first + f) % ring, n = min(entry_count[r], stride);
        const StreamEntry *in = entries + (size_t)r * stride;
        const size_t cur = (size_t)f * stride;
        uint32_t renamed[TR_ITEMS], mine = 0;
#pragma unroll
        for (int i = 0; i < TR_ITEMS; ++i) {
            const uint32_t j = threadIdx.x * TR_ITEMS + i;
            renamed[i] = TR_NONE;
            if (j < n && in[j].kept && local[cur + j] < ids) renamed[i] = new_id[local[cur + j]];
            mine += renamed[i] != TR_NONE;
        }
        uint32_t total;
        uint32_t pos = written + tr_block_exscan(mine, part, &total);
        if (threadIdx.x == 0) state_start[f] = written;
#pragma unroll
        for (int i = 0; i < TR_ITEMS; ++i) {
            if (renamed[i] == TR_NONE) continue;
            const uint32_t j = threadIdx.x * TR_ITEMS + i;
            point_id[pos] = renamed[i];                           // pos < frames * stride: at most one observation per survivor slot
            ts_uvd(in[j].v, refined != 0, uvd + 3 * (size_t)pos);
            ++pos;
        }
        written += total;
    }
    if (threadIdx.x == 0) {
        state_start[frames] = written;
        totals[0] = written;
        totals[1] = run;
    }
}

}  // namespace
}  // namespace ssba

#include "ssba_tracks_odometry.h"      // k_od_match ... k_od_solve: a pose with every push (uses the scan and ts_uvd above)

namespace ssba {
namespace {

// ---- host -------------------------------------------------------------------------------------------------------------------
std::mutex g_error_mutex;
std::string g_error;
thread_local std::string t_error_copy;

int tr_refuse(const char *call, int status, const std::string &what) {
    std::lock_guard<std::mutex> lock(g_error_mutex);
    g_error = std::string(call) + ": " + what;
    return status;
}

#define TR_TRY(expr)                      \
    do {                                  \
        const hipError_t _e = (expr);     \
        if (_e != hipSuccess) return _e;  \
    } while (0)

template <class T> hipError_t tr_alloc(std::vector<void *> *temps, T **out, size_t n) {
    void *ptr = nullptr;
    const hipError_t e = pool_malloc(&ptr, (n ? n : 1) * sizeof(T));
    if (e != hipSuccess) return e;
    temps->push_back(ptr);
    *out = (T *)ptr;
    return hipSuccess;
}

int tr_check_params(const char *call, const ssba_track_params *p) {
    if (!p) return tr_refuse(call, SSBA_ERR_INVALID_ARGUMENT, "NULL parameters");
    if (p->max_features < 1 || p->max_features > SSBA_TRACK_MAX_FEATURES) return tr_refuse(call, SSBA_ERR_INVALID_ARGUMENT, "max_features must be in 1 ... 4096");
    if (p->fast_threshold < 0 || p->fast_threshold > 254) return tr_refuse(call, SSBA_ERR_INVALID_ARGUMENT, "fast_threshold must be in 0 ... 254");
    if (p->max_hamming < 0 || p->max_hamming > 256) return tr_refuse(call, SSBA_ERR_INVALID_ARGUMENT, "max_hamming must be in 0 ... 256");
    if (p->stereo_max_dy < 0 || p->max_disparity < 0 || p->temporal_radius < 0)
        return tr_refuse(call, SSBA_ERR_INVALID_ARGUMENT, "stereo_max_dy, max_disparity and temporal_radius must not be negative");
    if (p->min_track_length < 1) return tr_refuse(call, SSBA_ERR_INVALID_ARGUMENT, "min_track_length must be at least 1");
    return SSBA_OK;
}

int tr_check_refine_params(const char *call, const ssba_track_refine_params *p) {
    if (!p) return tr_refuse(call, SSBA_ERR_INVALID_ARGUMENT, "NULL refine parameters");
    if (p->iterations < 1 || p->iterations > 64) return tr_refuse(call, SSBA_ERR_INVALID_ARGUMENT, "iterations must be in 1 ... 64");
    if (p->max_shift < 1 || p->max_shift > 8) return tr_refuse(call, SSBA_ERR_INVALID_ARGUMENT, "max_shift must be in 1 ... 8");
    if (p->max_sad < 0) return tr_refuse(call, SSBA_ERR_INVALID_ARGUMENT, "max_sad must not be negative");
    return SSBA_OK;
}

int tr_check_size(const char *call, uint32_t rows, uint32_t cols) {
    if (rows < 31 || cols < 31 || rows > 8192 || cols > 8192) return tr_refuse(call, SSBA_ERR_INVALID_ARGUMENT, "rows and cols must be in 31 ... 8192");
    return SSBA_OK;
}

int tr_open_device(const char *call, int device, hipStream_t *s) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return tr_refuse(call, SSBA_ERR_NO_DEVICE, "hipGetDeviceCount found no device");
    if (device < 0 && hipGetDevice(&device) != hipSuccess) return tr_refuse(call, SSBA_ERR_NO_DEVICE, "hipGetDevice failed");
    if (device >= n) return tr_refuse(call, SSBA_ERR_INVALID_ARGUMENT, "no such device");
    if (hipSetDevice(device) != hipSuccess) return tr_refuse(call, SSBA_ERR_HIP, "hipSetDevice failed");
    if (pool_stream_acquire(s) != hipSuccess) return tr_refuse(call, SSBA_ERR_HIP, "no stream");
    return SSBA_OK;
}

struct Features {
    uint32_t *count = nullptr;     // n
    uint16_t *xy = nullptr;        // n * max_features * 2
    uint8_t *score = nullptr;      // n * max_features
    uint32_t *desc = nullptr;      // n * max_features * 8
};

struct FeatureScratch {
    uint8_t *score = nullptr, *kept = nullptr;     // n * rows * cols each
    int *hist = nullptr;                           // n * 256
};

hipError_t tr_alloc_features(uint32_t n, int rows, int cols, const ssba_track_params &p, FeatureScratch *w, Features *f, std::vector<void *> *temps) {
    const size_t npix = (size_t)rows * cols, slots = (size_t)n * p.max_features;
    TR_TRY(tr_alloc(temps, &w->score, npix * n));
    TR_TRY(tr_alloc(temps, &w->kept, npix * n));
    TR_TRY(tr_alloc(temps, &w->hist, (size_t)n * 256));
    TR_TRY(tr_alloc(temps, &f->count, (size_t)n));
    TR_TRY(tr_alloc(temps, &f->xy, slots * 2));
    TR_TRY(tr_alloc(temps, &f->score, slots));
    return tr_alloc(temps, &f->desc, slots * TR_WORDS);
}

// four launches for n images already on the device
hipError_t tr_launch_features(const uint8_t *images, uint32_t n, int rows, int cols, const ssba_track_params &p, const FeatureScratch &w, const Features &f,
                              hipStream_t s) {
    const dim3 grid((cols + 63) / 64, (rows + 3) / 4, n), block(64, 4);
    hipLaunchKernelGGL(k_tr_score, grid, block, 0, s, images, w.score, w.hist, rows, cols, p.fast_threshold);
    TR_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_tr_nms, grid, block, 0, s, (const uint8_t *)w.score, w.kept, w.hist, rows, cols);
    TR_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_tr_select, dim3(n), dim3(TR_BLOCK), 0, s, (const uint8_t *)w.kept, (const int *)w.hist, rows, cols, p.max_features, f.count, f.xy, f.score);
    TR_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_tr_describe, dim3(p.max_features, n), dim3(256), 0, s, images, rows, cols, p.max_features, (const uint32_t *)f.count,
                       (const uint16_t *)f.xy, f.desc);
    return hipGetLastError();
}

hipError_t tr_enqueue_features(const uint8_t *images, uint32_t n, int rows, int cols, const ssba_track_params &p, bool clear, Features *f, hipStream_t s,
                               std::vector<void *> *temps) {
    const size_t slots = (size_t)n * p.max_features;
    FeatureScratch w;
    TR_TRY(tr_alloc_features(n, rows, cols, p, &w, f, temps));
    if (clear) {       // a caller that downloads whole arrays gets zeros behind the counts
        TR_TRY(hipMemsetAsync(f->xy, 0, slots * 2 * sizeof(uint16_t), s));
        TR_TRY(hipMemsetAsync(f->score, 0, slots, s));
        TR_TRY(hipMemsetAsync(f->desc, 0, slots * TR_WORDS * sizeof(uint32_t), s));
    }
    return tr_launch_features(images, n, rows, cols, p, w, *f, s);
}

hipError_t tr_enqueue_best(const MatchSets &m, uint32_t pairs, const TrackGate &g, hipStream_t s) {
    if (!pairs) return hipSuccess;
    hipLaunchKernelGGL(k_tr_best, dim3((m.stride + TR_QUERIES - 1) / TR_QUERIES, pairs, 2), dim3(TR_THREADS), 0, s, m, g);
    return hipGetLastError();
}

hipError_t tr_run_features(const uint8_t *images, uint32_t n, uint32_t rows, uint32_t cols, const ssba_track_params &p, uint32_t *count, uint16_t *xy,
                           uint8_t *score, uint32_t *desc, hipStream_t s, std::vector<void *> *temps) {
    const size_t all = (size_t)rows * cols * n, slots = (size_t)n * p.max_features;
    uint8_t *dimg = nullptr;
    Features f;
    TR_TRY(tr_alloc(temps, &dimg, all));
    TR_TRY(hipMemcpyAsync(dimg, images, all, hipMemcpyHostToDevice, s));
    TR_TRY(tr_enqueue_features(dimg, n, (int)rows, (int)cols, p, true, &f, s, temps));
    TR_TRY(hipMemcpyAsync(count, f.count, n * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    TR_TRY(hipMemcpyAsync(xy, f.xy, slots * 2 * sizeof(uint16_t), hipMemcpyDeviceToHost, s));
    TR_TRY(hipMemcpyAsync(score, f.score, slots, hipMemcpyDeviceToHost, s));
    TR_TRY(hipMemcpyAsync(desc, f.desc, slots * TR_WORDS * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    return hipStreamSynchronize(s);
}

hipError_t tr_run_match(const uint32_t *desc_a, const uint16_t *xy_a, uint32_t na, const uint32_t *desc_b, const uint16_t *xy_b, uint32_t nb, const TrackGate &g,
                        int max_hamming, int32_t *match_a, int32_t *dist_a, hipStream_t s, std::vector<void *> *temps) {
    const uint32_t stride = na > nb ? na : nb;
    uint32_t *da = nullptr, *db = nullptr, *counts = nullptr, *best_ab = nullptr, *best_ba = nullptr;
    uint16_t *pa = nullptr, *pb = nullptr;
    int32_t *dm = nullptr, *dd = nullptr;
    TR_TRY(tr_alloc(temps, &da, (size_t)stride * TR_WORDS));
    TR_TRY(tr_alloc(temps, &db, (size_t)stride * TR_WORDS));
    TR_TRY(tr_alloc(temps, &pa, (size_t)stride * 2));
    TR_TRY(tr_alloc(temps, &pb, (size_t)stride * 2));
    TR_TRY(tr_alloc(temps, &counts, (size_t)2));
    TR_TRY(tr_alloc(temps, &best_ab, (size_t)stride));
    TR_TRY(tr_alloc(temps, &best_ba, (size_t)stride));
    TR_TRY(tr_alloc(temps, &dm, (size_t)na));
    TR_TRY(tr_alloc(temps, &dd, (size_t)na));
    const uint32_t host_counts[2] = {na, nb};
    TR_TRY(hipMemcpyAsync(counts, host_counts, sizeof host_counts, hipMemcpyHostToDevice, s));
    if (na) TR_TRY(hipMemcpyAsync(da, desc_a, (size_t)na * TR_WORDS * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    if (na) TR_TRY(hipMemcpyAsync(pa, xy_a, (size_t)na * 2 * sizeof(uint16_t), hipMemcpyHostToDevice, s));
    if (nb) TR_TRY(hipMemcpyAsync(db, desc_b, (size_t)nb * TR_WORDS * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    if (nb) TR_TRY(hipMemcpyAsync(pb, xy_b, (size_t)nb * 2 * sizeof(uint16_t), hipMemcpyHostToDevice, s));
    TR_TRY(hipStreamSynchronize(s));       // host_counts leaves scope with this frame; the copies above read pageable memory
    if (na) {
        const MatchSets m = {da, db, pa, pb, counts, counts + 1, best_ab, best_ba, stride};
        TR_TRY(tr_enqueue_best(m, 1, g, s));
        hipLaunchKernelGGL(k_tr_crosscheck, dim3((na + 255) / 256), dim3(256), 0, s, (const uint32_t *)best_ab, (const uint32_t *)best_ba, na, nb, max_hamming, dm, dd);
        TR_TRY(hipGetLastError());
        TR_TRY(hipMemcpyAsync(match_a, dm, (size_t)na * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        TR_TRY(hipMemcpyAsync(dist_a, dd, (size_t)na * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    }
    return hipStreamSynchronize(s);
}

struct SequenceOut {
    uint64_t capacity;
    uint32_t *state_start, *point_id;
    double *uvd;
    uint64_t *num_observations;
    uint32_t *num_points;
    uint64_t *num_dropped = nullptr;      // ssba_track_sequence_subpixel only
    uint32_t needed = 0;
    bool too_small = false;
};

// refine: NULL for whole-pixel observations, or the parameters of the two launches that put sub-pixel ones in front of k_tr_prune
hipError_t tr_run_sequence(const uint8_t *left, const uint8_t *right, const int16_t *disp16, uint32_t frames, uint32_t rows, uint32_t cols,
                           const ssba_track_params &p, const ssba_track_refine_params *refine, SequenceOut *o, hipStream_t s, std::vector<void *> *temps) {
    const size_t npix = (size_t)rows * cols, stack = npix * frames;
    const uint32_t n = right ? 2 * frames : frames, stride = (uint32_t)p.max_features;
    const size_t slots = (size_t)frames * stride;
    uint8_t *dimg = nullptr;
    int16_t *dd16 = nullptr;
    TR_TRY(tr_alloc(temps, &dimg, npix * n));
    TR_TRY(hipMemcpyAsync(dimg, left, stack, hipMemcpyHostToDevice, s));
    if (right) {
        TR_TRY(hipMemcpyAsync(dimg + stack, right, stack, hipMemcpyHostToDevice, s));
    } else {
        TR_TRY(tr_alloc(temps, &dd16, stack));
        TR_TRY(hipMemcpyAsync(dd16, disp16, stack * sizeof(int16_t), hipMemcpyHostToDevice, s));
    }
    Features f;
    TR_TRY(tr_enqueue_features(dimg, n, (int)rows, (int)cols, p, false, &f, s, temps));

    uint32_t *best_lr = nullptr, *best_rl = nullptr, *best_pn = nullptr, *best_np = nullptr, *id = nullptr, *length = nullptr, *new_id = nullptr, *scalars = nullptr;
    uint32_t *d_start = nullptr, *d_point = nullptr;
    double *d_uvd = nullptr;
    Survivors sv;
    TR_TRY(tr_alloc(temps, &best_lr, slots));
    TR_TRY(tr_alloc(temps, &best_rl, slots));
    TR_TRY(tr_alloc(temps, &best_pn, slots));
    TR_TRY(tr_alloc(temps, &best_np, slots));
    TR_TRY(tr_alloc(temps, &sv.count, (size_t)frames));
    TR_TRY(tr_alloc(temps, &sv.desc, slots * TR_WORDS));
    TR_TRY(tr_alloc(temps, &sv.xy, slots * 2));
    TR_TRY(tr_alloc(temps, &sv.d16, slots));
    TR_TRY(tr_alloc(temps, &id, slots));
    TR_TRY(tr_alloc(temps, &length, slots));
    TR_TRY(tr_alloc(temps, &new_id, slots));
    TR_TRY(tr_alloc(temps, &scalars, (size_t)4));                 // the number of ids; observations and points after pruning; dropped
    TR_TRY(tr_alloc(temps, &d_start, (size_t)frames + 1));
    TR_TRY(tr_alloc(temps, &d_point, slots));
    TR_TRY(tr_alloc(temps, &d_uvd, slots * 3));

    if (right) {      // left frame f is image f, right frame f image frames + f of the feature arrays
        const MatchSets m = {f.desc, f.desc + slots * TR_WORDS, f.xy, f.xy + slots * 2, f.count, f.count + frames, best_lr, best_rl, stride};
        TR_TRY(tr_enqueue_best(m, frames, TrackGate{SSBA_TRACK_GATE_STEREO, p.stereo_max_dy, p.max_disparity, 0}, s));
    }
    hipLaunchKernelGGL(k_tr_stereo, dim3(frames), dim3(TR_BLOCK), 0, s, (const uint32_t *)f.count, (const uint16_t *)f.xy, (const uint32_t *)f.desc,
                       (const uint32_t *)best_lr, (const uint32_t *)best_rl, (const int16_t *)dd16, (int)frames, (int)rows, (int)cols, stride, p.max_hamming, sv);
    TR_TRY(hipGetLastError());
    {                 // pair k: A = the survivors of frame k, B = those of frame k + 1
        const MatchSets m = {sv.desc, sv.desc + (size_t)stride * TR_WORDS, sv.xy, sv.xy + (size_t)stride * 2, sv.count, sv.count + 1, best_pn, best_np, stride};
        TR_TRY(tr_enqueue_best(m, frames - 1, TrackGate{SSBA_TRACK_GATE_TEMPORAL, 0, 0, p.temporal_radius}, s));
    }
    hipLaunchKernelGGL(k_tr_link, dim3(1), dim3(TR_BLOCK), 0, s, (const uint32_t *)sv.count, (const uint32_t *)best_pn, (const uint32_t *)best_np, (int)frames, stride,
                       p.max_hamming, id, length, scalars);
    TR_TRY(hipGetLastError());
    int32_t *refined = nullptr;
    if (refine) {
        uint32_t *anchor = nullptr;
        TR_TRY(tr_alloc(temps, &anchor, slots));
        TR_TRY(tr_alloc(temps, &refined, slots * 3));
        hipLaunchKernelGGL(k_tr_anchor, dim3((stride + 255) / 256, frames), dim3(256), 0, s, (const uint32_t *)sv.count, (const uint32_t *)best_pn,
                           (const uint32_t *)best_np, (const uint32_t *)id, (int)frames, stride, p.max_hamming, anchor, scalars + 3);
        TR_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_tr_refine, dim3((stride + RF_WAVES - 1) / RF_WAVES, frames), dim3(64 * RF_WAVES), 0, s, (const uint8_t *)dimg, (int)frames, (int)rows,
                           (int)cols, right ? 1 : 0, (const uint32_t *)sv.count, (const uint16_t *)sv.xy, (const int32_t *)sv.d16, (const uint32_t *)anchor, stride,
                           *refine, id, length, refined, scalars + 3);
        TR_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(k_tr_prune, dim3(1), dim3(TR_BLOCK), 0, s, (const uint32_t *)sv.count, (const uint16_t *)sv.xy, (const int32_t *)sv.d16, (const uint32_t *)id,
                       (const uint32_t *)length, (const uint32_t *)scalars, (int)frames, stride, p.min_track_length, (const int32_t *)refined, new_id, d_start, d_point,
                       d_uvd, scalars + 1);
    TR_TRY(hipGetLastError());
    uint32_t totals[3] = {0, 0, 0};
    TR_TRY(hipMemcpyAsync(totals, scalars + 1, (refine ? 3 : 2) * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    TR_TRY(hipStreamSynchronize(s));
    o->needed = totals[0];
    if ((uint64_t)totals[0] > o->capacity) {
        o->too_small = true;
        return hipSuccess;
    }
    TR_TRY(hipMemcpyAsync(o->state_start, d_start, ((size_t)frames + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    if (totals[0]) {
        TR_TRY(hipMemcpyAsync(o->point_id, d_point, (size_t)totals[0] * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        TR_TRY(hipMemcpyAsync(o->uvd, d_uvd, (size_t)totals[0] * 3 * sizeof(double), hipMemcpyDeviceToHost, s));
    }
    TR_TRY(hipStreamSynchronize(s));
    *o->num_observations = totals[0];
    *o->num_points = totals[1];
    if (o->num_dropped) *o->num_dropped = totals[2];
    return hipSuccess;
}

hipError_t tr_run_refine(const uint8_t *images, uint32_t n, uint32_t rows, uint32_t cols, const int32_t *items, uint32_t num_items,
                         const ssba_track_refine_params &rp, int32_t *xy, int32_t *status, uint32_t *sad, hipStream_t s, std::vector<void *> *temps) {
    const size_t all = (size_t)rows * cols * n;
    uint8_t *dimg = nullptr;
    int32_t *ditems = nullptr, *dxy = nullptr, *dstatus = nullptr;
    uint32_t *dsad = nullptr;
    TR_TRY(tr_alloc(temps, &dimg, all));
    TR_TRY(tr_alloc(temps, &ditems, (size_t)num_items * RF_ITEM));
    TR_TRY(tr_alloc(temps, &dxy, (size_t)num_items * 2));
    TR_TRY(tr_alloc(temps, &dstatus, (size_t)num_items));
    TR_TRY(tr_alloc(temps, &dsad, (size_t)num_items));
    TR_TRY(hipMemcpyAsync(dimg, images, all, hipMemcpyHostToDevice, s));
    TR_TRY(hipMemcpyAsync(ditems, items, (size_t)num_items * RF_ITEM * sizeof(int32_t), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_tr_refine_items, dim3((num_items + RF_WAVES - 1) / RF_WAVES), dim3(64 * RF_WAVES), 0, s, (const uint8_t *)dimg, (int)rows, (int)cols,
                       (const int32_t *)ditems, num_items, rp, dxy, dstatus, dsad);
    TR_TRY(hipGetLastError());
    TR_TRY(hipMemcpyAsync(xy, dxy, (size_t)num_items * 2 * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    TR_TRY(hipMemcpyAsync(status, dstatus, (size_t)num_items * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    TR_TRY(hipMemcpyAsync(sad, dsad, (size_t)num_items * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    return hipStreamSynchronize(s);
}

int tr_close(const char *call, hipError_t e, hipStream_t s, std::vector<void *> *temps) {
    (void)hipStreamSynchronize(s);
    for (void *t : *temps) pool_free(t);
    pool_stream_release(s);
    if (e != hipSuccess) return tr_refuse(call, SSBA_ERR_HIP, hipGetErrorString(e));
    return SSBA_OK;
}

}  // namespace
}  // namespace ssba

using namespace ssba;

// Everything a stream owns.  All of it is allocated by ssba_track_stream_create; a push and a window call allocate nothing.
struct ssba_track_stream {
    int device = 0;
    uint32_t rows = 0, cols = 0, window = 0;
    ssba_track_params p = {};
    bool refine = false;
    ssba_track_refine_params rp = {};
    hipStream_t s = nullptr;
    std::vector<void *> temps;
    uint8_t *stage_in = nullptr, *stage_out = nullptr;      // pinned: the frame going up, the push outputs coming down
    int source = 0;                                         // 0: nothing pushed yet, 1: right images, 2: disp16 maps
    uint64_t pushed = 0;
    uint32_t next_id = 0;                                   // the device's running id as of the last push
    int cur = 0;                                            // which of the two survivor sets the next push fills
    bool failed = false;                                    // a HIP call failed mid-push or mid-window: the device state is not the host's
    // the frame: left image, right image, disp16 map; its features (two images) and the matcher's keys
    uint8_t *images = nullptr;
    FeatureScratch scratch;
    Features f;
    uint32_t *best_lr = nullptr, *best_rl = nullptr, *best_pn = nullptr, *best_np = nullptr;
    // previous and current survivors
    Survivors sv[2] = {};
    uint32_t *id[2] = {nullptr, nullptr};
    uint8_t *patch[2] = {nullptr, nullptr};                 // refine only
    uint32_t *from = nullptr, *running_id = nullptr;
    int32_t *refined = nullptr, *status = nullptr;          // refine only
    uint8_t *out = nullptr;                                 // 4 uint32 scalars, max_features * 3 doubles, max_features ids
    // the ring and the window call's work arrays
    StreamEntry *entries = nullptr;
    uint32_t *entry_count = nullptr, *local = nullptr, *length = nullptr, *new_id = nullptr, *w_start = nullptr, *w_point = nullptr, *w_totals = nullptr;
    double *w_uvd = nullptr;
    // odometry (ssba_track_stream_enable_odometry): the rule, the work arrays, the kept flags and observations of the previous and
    // the current frame, first_pose on the device, the last push's pose block on the host
    bool odometry = false;
    OdRule od_rule = {};
    OdWork od = {};
    uint8_t *od_kept[2] = {nullptr, nullptr};
    double *od_uvd[2] = {nullptr, nullptr};
    double *od_first = nullptr;
    OdPose pose = {};
};

namespace {

constexpr size_t TS_OUT_SCALARS = 4 * sizeof(uint32_t);

size_t ts_out_bytes(uint32_t stride) { return TS_OUT_SCALARS + (size_t)stride * (3 * sizeof(double) + sizeof(uint32_t)); }

// with odometry the pose block follows the push outputs on the next multiple of 8 bytes
size_t ts_pose_at(uint32_t stride) { return (ts_out_bytes(stride) + 7) & ~(size_t)7; }

int od_check_params(const char *call, const ssba_track_odometry_params *p) {
    if (!p) return tr_refuse(call, SSBA_ERR_INVALID_ARGUMENT, "NULL odometry parameters");
    if (p->ransac_iterations < 1 || p->ransac_iterations > SSBA_TRACK_ODOMETRY_MAX)
        return tr_refuse(call, SSBA_ERR_INVALID_ARGUMENT, "ransac_iterations must be in 1 ... 4096");
    if (p->refine_iterations > SSBA_TRACK_ODOMETRY_MAX_REFINE) return tr_refuse(call, SSBA_ERR_INVALID_ARGUMENT, "refine_iterations must not exceed 1024");
    const double positive[5] = {p->ransac_threshold, p->observation_variance, p->camera.fu, p->camera.fv, p->camera.b};
    for (double v : positive)
        if (!(v > 0.0) || !std::isfinite(v))
            return tr_refuse(call, SSBA_ERR_INVALID_ARGUMENT, "ransac_threshold, observation_variance and the camera's fu, fv and b must be positive");
    if (!std::isfinite(p->camera.cu) || !std::isfinite(p->camera.cv)) return tr_refuse(call, SSBA_ERR_INVALID_ARGUMENT, "the camera's cu and cv must be finite");
    return SSBA_OK;
}

OdRule od_rule_of(const ssba_track_odometry_params &p) {
    return OdRule{Cam{p.camera.fu, p.camera.fv, p.camera.cu, p.camera.cv, p.camera.b}, p.ransac_iterations, p.refine_iterations, p.ransac_threshold,
                  1.0 / std::sqrt(p.observation_variance)};
}

hipError_t od_allocate(std::vector<void *> *t, const OdRule &rule, OdWork *w) {
    const size_t cap = SSBA_TRACK_ODOMETRY_MAX;
    TR_TRY(tr_alloc(t, &w->n, (size_t)1));
    for (double **a : {&w->obs0, &w->obs1, &w->pts0, &w->pts1, &w->x, &w->c, &w->scale}) TR_TRY(tr_alloc(t, a, cap * 3));
    TR_TRY(tr_alloc(t, &w->hyp, (size_t)rule.hypotheses * 12));
    TR_TRY(tr_alloc(t, &w->count, (size_t)rule.hypotheses));
    TR_TRY(tr_alloc(t, &w->inlier, cap));
    TR_TRY(tr_alloc(t, &w->index, cap));
    TR_TRY(tr_alloc(t, &w->cost_log, (size_t)rule.iterations + 1));
    TR_TRY(tr_alloc(t, &w->step_ok, (size_t)rule.iterations + 1));
    TR_TRY(tr_alloc(t, &w->chain, (size_t)12));
    return hipSuccess;
}

// the launches behind the match list: k_od_align and k_od_score (not for a stream's first push, mode 1), k_od_solve
hipError_t od_enqueue(const OdRule &rule, uint32_t frame, const OdWork &w, int mode, const double *first_pose, OdPose *out, hipStream_t s) {
    if (mode != 1) {
        hipLaunchKernelGGL(k_od_align, dim3((rule.hypotheses + 255) / 256), dim3(256), 0, s, rule, frame, w);
        TR_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_od_score, dim3((rule.hypotheses + 3) / 4), dim3(256), 0, s, rule, w);
        TR_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(k_od_solve, dim3(1), dim3(OD_BLOCK), 0, s, rule, w, mode, first_pose, out);
    return hipGetLastError();
}

void od_info(const OdPose &p, ssba_track_pose_info *info) {
    if (!info) return;
    *info = ssba_track_pose_info{p.status, p.num_matches, p.num_inliers, p.num_iterations, p.initial_cost, p.final_cost};
}

hipError_t od_enable(ssba_track_stream *st, const ssba_track_odometry_params &p) {
    const uint32_t stride = (uint32_t)st->p.max_features;
    const size_t bytes = ts_pose_at(stride) + sizeof(OdPose);
    std::vector<void *> *t = &st->temps;
    st->od_rule = od_rule_of(p);
    TR_TRY(od_allocate(t, st->od_rule, &st->od));
    for (int b = 0; b < 2; ++b) {
        TR_TRY(tr_alloc(t, &st->od_kept[b], (size_t)stride));
        TR_TRY(tr_alloc(t, &st->od_uvd[b], (size_t)stride * 3));
    }
    TR_TRY(tr_alloc(t, &st->od_first, (size_t)12));
    TR_TRY(tr_alloc(t, &st->out, bytes));            // the push output block with the pose block behind it; the old one is freed with the stream
    void *pinned = nullptr;
    TR_TRY(pool_host_malloc(&pinned, bytes));
    pool_host_free(st->stage_out);
    st->stage_out = (uint8_t *)pinned;
    memcpy(st->stage_out, p.first_pose, 12 * sizeof(double));
    TR_TRY(hipMemcpyAsync(st->od_first, st->stage_out, 12 * sizeof(double), hipMemcpyHostToDevice, st->s));
    return hipStreamSynchronize(st->s);
}

hipError_t od_run_relative(const OdRule &rule, uint32_t frame, uint32_t n, const double *uvd_prev, const double *uvd_cur, double *T_ransac, uint8_t *inlier,
                           double *cost_log, int32_t *step_ok, OdPose *pose, hipStream_t s, std::vector<void *> *temps) {
    OdWork w = {};
    OdPose *dpose = nullptr;
    double *dprev = nullptr, *dcur = nullptr;
    TR_TRY(od_allocate(temps, rule, &w));
    TR_TRY(tr_alloc(temps, &dpose, (size_t)1));
    TR_TRY(tr_alloc(temps, &dprev, (size_t)n * 3));
    TR_TRY(tr_alloc(temps, &dcur, (size_t)n * 3));
    if (n) {
        TR_TRY(hipMemcpyAsync(dprev, uvd_prev, (size_t)n * 3 * sizeof(double), hipMemcpyHostToDevice, s));
        TR_TRY(hipMemcpyAsync(dcur, uvd_cur, (size_t)n * 3 * sizeof(double), hipMemcpyHostToDevice, s));
    }
    hipLaunchKernelGGL(k_od_pairs, dim3(n ? (n + 255) / 256 : 1), dim3(256), 0, s, rule.cam, (const double *)dprev, (const double *)dcur, n, w);
    TR_TRY(hipGetLastError());
    TR_TRY(od_enqueue(rule, frame, w, 2, nullptr, dpose, s));
    TR_TRY(hipMemcpyAsync(pose, dpose, sizeof(OdPose), hipMemcpyDeviceToHost, s));
    if (inlier && n) TR_TRY(hipMemcpyAsync(inlier, w.inlier, (size_t)n, hipMemcpyDeviceToHost, s));
    if (cost_log) TR_TRY(hipMemcpyAsync(cost_log, w.cost_log, ((size_t)rule.iterations + 1) * sizeof(double), hipMemcpyDeviceToHost, s));
    if (step_ok) TR_TRY(hipMemcpyAsync(step_ok, w.step_ok, ((size_t)rule.iterations + 1) * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    TR_TRY(hipStreamSynchronize(s));
    if (T_ransac) memcpy(T_ransac, pose->T_ransac, 12 * sizeof(double));
    return hipSuccess;
}

hipError_t ts_allocate(ssba_track_stream *st) {
    const size_t npix = (size_t)st->rows * st->cols, stride = (size_t)st->p.max_features, slots = stride * st->window;
    std::vector<void *> *t = &st->temps;
    TR_TRY(tr_alloc(t, &st->images, 4 * npix));                      // left, right, then the int16 map on its even offset
    TR_TRY(tr_alloc_features(2, (int)st->rows, (int)st->cols, st->p, &st->scratch, &st->f, t));
    TR_TRY(tr_alloc(t, &st->best_lr, stride));
    TR_TRY(tr_alloc(t, &st->best_rl, stride));
    TR_TRY(tr_alloc(t, &st->best_pn, stride));
    TR_TRY(tr_alloc(t, &st->best_np, stride));
    for (int b = 0; b < 2; ++b) {
        TR_TRY(tr_alloc(t, &st->sv[b].count, (size_t)1));
        TR_TRY(tr_alloc(t, &st->sv[b].desc, stride * TR_WORDS));
        TR_TRY(tr_alloc(t, &st->sv[b].xy, stride * 2));
        TR_TRY(tr_alloc(t, &st->sv[b].d16, stride));
        TR_TRY(tr_alloc(t, &st->id[b], stride));
        if (st->refine) TR_TRY(tr_alloc(t, &st->patch[b], stride * TS_PATCH_STRIDE));
    }
    TR_TRY(tr_alloc(t, &st->from, stride));
    TR_TRY(tr_alloc(t, &st->running_id, (size_t)1));
    if (st->refine) {
        TR_TRY(tr_alloc(t, &st->refined, stride * 3));
        TR_TRY(tr_alloc(t, &st->status, stride));
    }
    TR_TRY(tr_alloc(t, &st->out, ts_out_bytes((uint32_t)stride)));
    TR_TRY(tr_alloc(t, &st->entries, slots));
    TR_TRY(tr_alloc(t, &st->entry_count, (size_t)st->window));
    TR_TRY(tr_alloc(t, &st->local, slots));
    TR_TRY(tr_alloc(t, &st->length, slots));
    TR_TRY(tr_alloc(t, &st->new_id, slots));
    TR_TRY(tr_alloc(t, &st->w_start, (size_t)st->window + 1));
    TR_TRY(tr_alloc(t, &st->w_point, slots));
    TR_TRY(tr_alloc(t, &st->w_uvd, slots * 3));
    TR_TRY(tr_alloc(t, &st->w_totals, (size_t)2));
    void *pinned = nullptr;
    TR_TRY(pool_host_malloc(&pinned, 3 * npix + 1));
    st->stage_in = (uint8_t *)pinned;
    TR_TRY(pool_host_malloc(&pinned, ts_out_bytes((uint32_t)stride)));
    st->stage_out = (uint8_t *)pinned;
    TR_TRY(hipMemsetAsync(st->running_id, 0, sizeof(uint32_t), st->s));
    return hipStreamSynchronize(st->s);
}

void ts_free(ssba_track_stream *st) {
    if (st->s) (void)hipStreamSynchronize(st->s);
    for (void *t : st->temps) pool_free(t);
    pool_host_free(st->stage_in);
    pool_host_free(st->stage_out);
    if (st->s) pool_stream_release(st->s);
    delete st;
}

// The launches of a push: 4 for the features, k_tr_best left-right with right images, k_tr_stereo, k_tr_best against the frame
// before (not on the first push), k_ts_link, with refinement k_ts_carry and k_ts_refine, k_ts_emit.
hipError_t ts_push(ssba_track_stream *st, const uint8_t *left, const uint8_t *right, const int16_t *disp16, uint32_t *scalars) {
    const size_t npix = (size_t)st->rows * st->cols, map_at = (npix + 1) & ~(size_t)1;
    const uint32_t stride = (uint32_t)st->p.max_features;
    const int rows = (int)st->rows, cols = (int)st->cols;
    const ssba_track_params &p = st->p;
    hipStream_t s = st->s;
    const int16_t *dd16 = nullptr;
    memcpy(st->stage_in, left, npix);
    if (right) {
        memcpy(st->stage_in + npix, right, npix);
        TR_TRY(hipMemcpyAsync(st->images, st->stage_in, 2 * npix, hipMemcpyHostToDevice, s));
    } else {
        memcpy(st->stage_in + map_at, disp16, npix * sizeof(int16_t));
        TR_TRY(hipMemcpyAsync(st->images, st->stage_in, npix, hipMemcpyHostToDevice, s));
        TR_TRY(hipMemcpyAsync(st->images + 2 * npix, st->stage_in + map_at, npix * sizeof(int16_t), hipMemcpyHostToDevice, s));
        dd16 = (const int16_t *)(st->images + 2 * npix);
    }
    TR_TRY(tr_launch_features(st->images, right ? 2 : 1, rows, cols, p, st->scratch, st->f, s));
    if (right) {      // the pair is a two-image stack: left is image 0, right image 1 of the feature arrays
        const MatchSets m = {st->f.desc, st->f.desc + (size_t)stride * TR_WORDS, st->f.xy, st->f.xy + (size_t)stride * 2, st->f.count, st->f.count + 1,
                             st->best_lr, st->best_rl, stride};
        TR_TRY(tr_enqueue_best(m, 1, TrackGate{SSBA_TRACK_GATE_STEREO, p.stereo_max_dy, p.max_disparity, 0}, s));
    }
    const Survivors &now = st->sv[st->cur], &before = st->sv[st->cur ^ 1];
    hipLaunchKernelGGL(k_tr_stereo, dim3(1), dim3(TR_BLOCK), 0, s, (const uint32_t *)st->f.count, (const uint16_t *)st->f.xy, (const uint32_t *)st->f.desc,
                       (const uint32_t *)st->best_lr, (const uint32_t *)st->best_rl, dd16, 1, rows, cols, stride, p.max_hamming, now);
    TR_TRY(hipGetLastError());
    const int has_prev = st->pushed > 0;
    if (has_prev) {   // A = the survivors of the frame before, B = those of this frame
        const MatchSets m = {before.desc, now.desc, before.xy, now.xy, before.count, now.count, st->best_pn, st->best_np, stride};
        TR_TRY(tr_enqueue_best(m, 1, TrackGate{SSBA_TRACK_GATE_TEMPORAL, 0, 0, p.temporal_radius}, s));
    }
    hipLaunchKernelGGL(k_ts_link, dim3(1), dim3(TR_BLOCK), 0, s, (const uint32_t *)now.count, (const uint32_t *)before.count, has_prev,
                       (const uint32_t *)st->best_pn, (const uint32_t *)st->best_np, (const uint32_t *)st->id[st->cur ^ 1], stride, p.max_hamming, st->id[st->cur],
                       st->from, st->running_id);
    TR_TRY(hipGetLastError());
    if (st->refine) {
        const dim3 grid((stride + RF_WAVES - 1) / RF_WAVES), block(64 * RF_WAVES);
        hipLaunchKernelGGL(k_ts_carry, grid, block, 0, s, (const uint8_t *)st->images, rows, cols, (const uint32_t *)now.count, (const uint32_t *)before.count,
                           (const uint16_t *)now.xy, (const uint32_t *)st->from, stride, (const uint8_t *)st->patch[st->cur ^ 1], st->patch[st->cur]);
        TR_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_ts_refine, grid, block, 0, s, (const uint8_t *)st->images, rows, cols, right ? 1 : 0, (const uint32_t *)now.count,
                           (const uint16_t *)now.xy, (const int32_t *)now.d16, (const uint32_t *)st->from, (const uint8_t *)st->patch[st->cur], stride, st->rp,
                           st->refined, st->status);
        TR_TRY(hipGetLastError());
    }
    const uint32_t slot = (uint32_t)(st->pushed % st->window);
    hipLaunchKernelGGL(k_ts_emit, dim3(1), dim3(TR_BLOCK), 0, s, (const uint32_t *)now.count, (const uint16_t *)now.xy, (const int32_t *)now.d16,
                       (const uint32_t *)st->id[st->cur], (const uint32_t *)st->from, (const int32_t *)st->refined, (const int32_t *)st->status, stride,
                       (const uint32_t *)st->running_id, st->entries + (size_t)slot * stride, st->entry_count + slot, (uint32_t *)st->out,
                       (double *)(st->out + TS_OUT_SCALARS), (uint32_t *)(st->out + TS_OUT_SCALARS + (size_t)stride * 3 * sizeof(double)));
    TR_TRY(hipGetLastError());
    if (st->odometry) {      // 4 launches more (2 on the first push); the pose block comes down in the same copy
        hipLaunchKernelGGL(k_od_match, dim3(1), dim3(TR_BLOCK), 0, s, st->od_rule.cam, (const uint32_t *)now.count, (const uint16_t *)now.xy,
                           (const int32_t *)now.d16, (const uint32_t *)st->from, (const int32_t *)st->refined, (const int32_t *)st->status, stride, has_prev,
                           (const uint8_t *)st->od_kept[st->cur ^ 1], (const double *)st->od_uvd[st->cur ^ 1], st->od_kept[st->cur], st->od_uvd[st->cur], st->od);
        TR_TRY(hipGetLastError());
        TR_TRY(od_enqueue(st->od_rule, (uint32_t)st->pushed, st->od, has_prev ? 0 : 1, st->od_first, (OdPose *)(st->out + ts_pose_at(stride)), s));
    }
    const size_t down = st->odometry ? ts_pose_at(stride) + sizeof(OdPose) : ts_out_bytes(stride);
    TR_TRY(hipMemcpyAsync(st->stage_out, st->out, down, hipMemcpyDeviceToHost, s));
    TR_TRY(hipStreamSynchronize(s));          // the one synchronisation of a push
    memcpy(scalars, st->stage_out, 3 * sizeof(uint32_t));
    if (st->odometry) memcpy(&st->pose, st->stage_out + ts_pose_at(stride), sizeof(OdPose));
    return hipSuccess;
}

// one launch whatever `frames`
hipError_t ts_window(ssba_track_stream *st, uint32_t frames, SequenceOut *o) {
    const uint32_t stride = (uint32_t)st->p.max_features, first = (uint32_t)((st->pushed - frames) % st->window);
    hipStream_t s = st->s;
    hipLaunchKernelGGL(k_ts_window, dim3(1), dim3(TR_BLOCK), 0, s, (const StreamEntry *)st->entries, (const uint32_t *)st->entry_count, st->window, first,
                       (int)frames, stride, st->p.min_track_length, st->refine ? 1 : 0, st->local, st->length, st->new_id, st->w_start, st->w_point, st->w_uvd,
                       st->w_totals);
    TR_TRY(hipGetLastError());
    uint32_t *totals = (uint32_t *)st->stage_out;
    TR_TRY(hipMemcpyAsync(totals, st->w_totals, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    TR_TRY(hipStreamSynchronize(s));
    o->needed = totals[0];
    if ((uint64_t)totals[0] > o->capacity) {
        o->too_small = true;
        return hipSuccess;
    }
    const uint32_t n = totals[0], points = totals[1];
    TR_TRY(hipMemcpyAsync(o->state_start, st->w_start, ((size_t)frames + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    if (n) {
        TR_TRY(hipMemcpyAsync(o->point_id, st->w_point, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        TR_TRY(hipMemcpyAsync(o->uvd, st->w_uvd, (size_t)n * 3 * sizeof(double), hipMemcpyDeviceToHost, s));
    }
    TR_TRY(hipStreamSynchronize(s));
    *o->num_observations = n;
    *o->num_points = points;
    return hipSuccess;
}

}  // namespace

extern "C" {

int ssba_track_stream_create(uint32_t rows, uint32_t cols, const ssba_track_params *params, const ssba_track_refine_params *refine_params, uint32_t window,
                             int device, ssba_track_stream **stream) {
    const char *call = "ssba_track_stream_create";
    if (!stream) return tr_refuse(call, SSBA_ERR_INVALID_ARGUMENT, "NULL stream");
    if (const int rc = tr_check_params(call, params)) return rc;
    if (refine_params)
        if (const int rc = tr_check_refine_params(call, refine_params)) return rc;
    if (const int rc = tr_check_size(call, rows, cols)) return rc;
    if (window < 1 || window > SSBA_TRACK_STREAM_MAX_WINDOW)
        return tr_refuse(call, SSBA_ERR_INVALID_ARGUMENT, "window must be in 1 ... " + std::to_string(SSBA_TRACK_STREAM_MAX_WINDOW));
    hipStream_t s = nullptr;
    if (const int rc = tr_open_device(call, device, &s)) return rc;
    ssba_track_stream *st = new ssba_track_stream;
    (void)hipGetDevice(&st->device);
    st->rows = rows;
    st->cols = cols;
    st->window = window;
    st->p = *params;
    st->refine = refine_params != nullptr;
    if (refine_params) st->rp = *refine_params;
    st->s = s;
    const hipError_t e = ts_allocate(st);
    if (e != hipSuccess) {
        ts_free(st);
        return tr_refuse(call, SSBA_ERR_HIP, hipGetErrorString(e));
    }
    *stream = st;
    return SSBA_OK;
}

int ssba_track_stream_push(ssba_track_stream *stream, const uint8_t *left, const uint8_t *right, const int16_t *disp16, uint32_t *track_id, double *uvd,
                           uint32_t *num_observations, uint32_t *num_dropped) {
    const char *call = "ssba_track_stream_push";
    if (!left) return tr_refuse(call, SSBA_ERR_INVALID_ARGUMENT, "NULL left image");
    if (!right == !disp16) return tr_refuse(call, SSBA_ERR_INVALID_ARGUMENT, "exactly one of right and disp16 must be given");
    if (!track_id || !uvd || !num_observations || !num_dropped) return tr_refuse(call, SSBA_ERR_INVALID_ARGUMENT, "NULL output");
    if (!stream) return tr_refuse(call, SSBA_ERR_INVALID_ARGUMENT, "NULL stream");
    if (stream->failed) return tr_refuse(call, SSBA_ERR_STATE, "an earlier call on this stream ended with a HIP error: destroy it");
    const int source = right ? 1 : 2;
    if (stream->source && stream->source != source)
        return tr_refuse(call, SSBA_ERR_INVALID_ARGUMENT, std::string("the stream's first push fixed its disparity source: ") + (source == 1 ? "disp16" : "right") + " must be given");
    const uint32_t stride = (uint32_t)stream->p.max_features;
    if (0xffffffffu - stream->next_id < stride)
        return tr_refuse(call, SSBA_ERR_STATE, "fewer than max_features ids are left below 2^32 - 1: " + std::to_string(stream->next_id) + " have been issued");
    if (hipSetDevice(stream->device) != hipSuccess) return tr_refuse(call, SSBA_ERR_HIP, "hipSetDevice failed");
    uint32_t scalars[3] = {0, 0, 0};
    const hipError_t e = ts_push(stream, left, right, disp16, scalars);
    if (e != hipSuccess) {
        stream->failed = true;          // the running id and the current survivor set may have advanced on the device
        (void)hipStreamSynchronize(stream->s);
        return tr_refuse(call, SSBA_ERR_HIP, hipGetErrorString(e));
    }
    const uint32_t n = scalars[0] < stride ? scalars[0] : stride;
    memcpy(uvd, stream->stage_out + TS_OUT_SCALARS, (size_t)n * 3 * sizeof(double));
    memcpy(track_id, stream->stage_out + TS_OUT_SCALARS + (size_t)stride * 3 * sizeof(double), (size_t)n * sizeof(uint32_t));
    *num_observations = n;
    *num_dropped = scalars[1];
    stream->next_id = scalars[2];
    stream->source = source;
    stream->pushed += 1;
    stream->cur ^= 1;
    return SSBA_OK;
}

int ssba_track_stream_window(ssba_track_stream *stream, uint32_t frames, uint64_t capacity, uint32_t *state_start, uint32_t *point_id, double *uvd,
                             uint64_t *num_observations, uint32_t *num_points) {
    const char *call = "ssba_track_stream_window";
    if (!state_start || !num_observations || !num_points || (capacity && (!point_id || !uvd))) return tr_refuse(call, SSBA_ERR_INVALID_ARGUMENT, "NULL output");
    if (frames < 1) return tr_refuse(call, SSBA_ERR_INVALID_ARGUMENT, "frames must be at least 1");
    if (!stream) return tr_refuse(call, SSBA_ERR_INVALID_ARGUMENT, "NULL stream");
    if (stream->failed) return tr_refuse(call, SSBA_ERR_STATE, "an earlier call on this stream ended with a HIP error: destroy it");
    if (frames > stream->window || frames > stream->pushed)
        return tr_refuse(call, SSBA_ERR_INVALID_ARGUMENT, "frames " + std::to_string(frames) + " exceeds the stream's window " + std::to_string(stream->window) +
                                                              " or the " + std::to_string(stream->pushed) + " frames pushed");
    if (hipSetDevice(stream->device) != hipSuccess) return tr_refuse(call, SSBA_ERR_HIP, "hipSetDevice failed");
    SequenceOut o = {capacity, state_start, point_id, uvd, num_observations, num_points};
    const hipError_t e = ts_window(stream, frames, &o);
    if (e != hipSuccess) {
        stream->failed = true;
        (void)hipStreamSynchronize(stream->s);
        return tr_refuse(call, SSBA_ERR_HIP, hipGetErrorString(e));
    }
    if (o.too_small)
        return tr_refuse(call, SSBA_ERR_INVALID_ARGUMENT, "capacity " + std::to_string(capacity) + " is below the " + std::to_string(o.needed) + " observations found");
    return SSBA_OK;
}

void ssba_track_stream_destroy(ssba_track_stream *stream) {
    if (!stream) return;
    (void)hipSetDevice(stream->device);
    ts_free(stream);
}

void ssba_track_default_odometry_params(ssba_track_odometry_params *params) {
    if (!params) return;
    *params = ssba_track_odometry_params{{0.0, 0.0, 0.0, 0.0, 0.0}, 400, 4.0, 20, 4.0, {0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1}};
}

int ssba_track_stream_enable_odometry(ssba_track_stream *stream, const ssba_track_odometry_params *params) {
    const char *call = "ssba_track_stream_enable_odometry";
    if (!stream) return tr_refuse(call, SSBA_ERR_INVALID_ARGUMENT, "NULL stream");
    if (const int rc = od_check_params(call, params)) return rc;
    if (stream->failed) return tr_refuse(call, SSBA_ERR_STATE, "an earlier call on this stream ended with a HIP error: destroy it");
    if (stream->pushed) return tr_refuse(call, SSBA_ERR_STATE, "odometry is enabled before the first push");
    if (stream->odometry) return tr_refuse(call, SSBA_ERR_STATE, "odometry is enabled already");
    if (hipSetDevice(stream->device) != hipSuccess) return tr_refuse(call, SSBA_ERR_HIP, "hipSetDevice failed");
    const hipError_t e = od_enable(stream, *params);
    if (e != hipSuccess) {
        stream->failed = true;
        (void)hipStreamSynchronize(stream->s);
        return tr_refuse(call, SSBA_ERR_HIP, hipGetErrorString(e));
    }
    stream->odometry = true;
    return SSBA_OK;
}

int ssba_track_stream_pose(ssba_track_stream *stream, double T_k_km1[12], double T_k_0[12], ssba_track_pose_info *info) {
    const char *call = "ssba_track_stream_pose";
    if (!stream) return tr_refuse(call, SSBA_ERR_INVALID_ARGUMENT, "NULL stream");
    if (!T_k_km1 || !T_k_0) return tr_refuse(call, SSBA_ERR_INVALID_ARGUMENT, "NULL output");
    if (!stream->odometry) return tr_refuse(call, SSBA_ERR_STATE, "the stream has no odometry: ssba_track_stream_enable_odometry comes before the first push");
    if (!stream->pushed) return tr_refuse(call, SSBA_ERR_STATE, "nothing has been pushed yet");
    if (stream->failed) return tr_refuse(call, SSBA_ERR_STATE, "an earlier call on this stream ended with a HIP error: destroy it");
    memcpy(T_k_km1, stream->pose.T_rel, 12 * sizeof(double));
    memcpy(T_k_0, stream->pose.T_abs, 12 * sizeof(double));
    od_info(stream->pose, info);
    return SSBA_OK;
}

int ssba_track_relative_pose(const ssba_track_odometry_params *params, uint32_t frame_index, uint32_t n, const double *uvd_prev, const double *uvd_cur,
                             int device, double *T_ransac, uint8_t *inlier, double *T, ssba_track_pose_info *info, double *cost_log, int32_t *step_ok) {
    const char *call = "ssba_track_relative_pose";
    if (const int rc = od_check_params(call, params)) return rc;
    if (n && (!uvd_prev || !uvd_cur)) return tr_refuse(call, SSBA_ERR_INVALID_ARGUMENT, "NULL observations");
    if (!T || !info) return tr_refuse(call, SSBA_ERR_INVALID_ARGUMENT, "NULL output");
    if (n > SSBA_TRACK_ODOMETRY_MAX) return tr_refuse(call, SSBA_ERR_INVALID_ARGUMENT, "n must not exceed 4096");
    hipStream_t s = nullptr;
    if (const int rc = tr_open_device(call, device, &s)) return rc;
    std::vector<void *> temps;
    OdPose pose = {};
    const hipError_t e = od_run_relative(od_rule_of(*params), frame_index, n, uvd_prev, uvd_cur, T_ransac, inlier, cost_log, step_ok, &pose, s, &temps);
    const int rc = tr_close(call, e, s, &temps);
    if (rc) return rc;
    memcpy(T, pose.T_rel, 12 * sizeof(double));
    od_info(pose, info);
    return SSBA_OK;
}

void ssba_track_default_params(ssba_track_params *params) {
    if (!params) return;
    *params = ssba_track_params{20, 1000, 5, 128, 64, 0, 2};
}

const char *ssba_track_last_error(void) {
    std::lock_guard<std::mutex> lock(g_error_mutex);
    t_error_copy = g_error;
    return t_error_copy.c_str();
}

int ssba_track_features(const uint8_t *images, uint32_t n, uint32_t rows, uint32_t cols, const ssba_track_params *params, int device, uint32_t *count,
                        uint16_t *xy, uint8_t *score, uint32_t *desc) {
    const char *call = "ssba_track_features";
    if (!images) return tr_refuse(call, SSBA_ERR_INVALID_ARGUMENT, "NULL image");
    if (!count || !xy || !score || !desc) return tr_refuse(call, SSBA_ERR_INVALID_ARGUMENT, "NULL output");
    if (const int rc = tr_check_params(call, params)) return rc;
    if (n < 1 || n > 65535) return tr_refuse(call, SSBA_ERR_INVALID_ARGUMENT, "n must be in 1 ... 65535");
    if (const int rc = tr_check_size(call, rows, cols)) return rc;
    hipStream_t s = nullptr;
    if (const int rc = tr_open_device(call, device, &s)) return rc;
    std::vector<void *> temps;
    const hipError_t e = tr_run_features(images, n, rows, cols, *params, count, xy, score, desc, s, &temps);
    return tr_close(call, e, s, &temps);
}

int ssba_track_match(const uint32_t *desc_a, const uint16_t *xy_a, uint32_t na, const uint32_t *desc_b, const uint16_t *xy_b, uint32_t nb, int gate,
                     const ssba_track_params *params, int device, int32_t *match_a, int32_t *dist_a) {
    const char *call = "ssba_track_match";
    if ((na && (!desc_a || !xy_a)) || (nb && (!desc_b || !xy_b))) return tr_refuse(call, SSBA_ERR_INVALID_ARGUMENT, "NULL descriptors or positions");
    if (na && (!match_a || !dist_a)) return tr_refuse(call, SSBA_ERR_INVALID_ARGUMENT, "NULL output");
    if (const int rc = tr_check_params(call, params)) return rc;
    if (gate != SSBA_TRACK_GATE_NONE && gate != SSBA_TRACK_GATE_STEREO && gate != SSBA_TRACK_GATE_TEMPORAL)
        return tr_refuse(call, SSBA_ERR_INVALID_ARGUMENT, "unknown gate");
    if (na > 65535 || nb > 65535) return tr_refuse(call, SSBA_ERR_INVALID_ARGUMENT, "na and nb must not exceed 65535 (the index half of the packed key)");
    hipStream_t s = nullptr;
    if (const int rc = tr_open_device(call, device, &s)) return rc;
    std::vector<void *> temps;
    const TrackGate g = {gate, params->stereo_max_dy, params->max_disparity, params->temporal_radius};
    const hipError_t e = tr_run_match(desc_a, xy_a, na, desc_b, xy_b, nb, g, params->max_hamming, match_a, dist_a, s, &temps);
    return tr_close(call, e, s, &temps);
}

int ssba_track_sequence(const uint8_t *left, const uint8_t *right, const int16_t *disp16, uint32_t frames, uint32_t rows, uint32_t cols,
                        const ssba_track_params *params, int device, uint64_t capacity, uint32_t *state_start, uint32_t *point_id, double *uvd,
                        uint64_t *num_observations, uint32_t *num_points) {
    const char *call = "ssba_track_sequence";
    if (!left) return tr_refuse(call, SSBA_ERR_INVALID_ARGUMENT, "NULL left images");
    if (!right == !disp16) return tr_refuse(call, SSBA_ERR_INVALID_ARGUMENT, "exactly one of right and disp16 must be given");
    if (!state_start || !num_observations || !num_points || (capacity && (!point_id || !uvd))) return tr_refuse(call, SSBA_ERR_INVALID_ARGUMENT, "NULL output");
    if (const int rc = tr_check_params(call, params)) return rc;
    if (frames < 1 || frames > 32767) return tr_refuse(call, SSBA_ERR_INVALID_ARGUMENT, "frames must be in 1 ... 32767");
    if (const int rc = tr_check_size(call, rows, cols)) return rc;
    hipStream_t s = nullptr;
    if (const int rc = tr_open_device(call, device, &s)) return rc;
    std::vector<void *> temps;
    SequenceOut o = {capacity, state_start, point_id, uvd, num_observations, num_points};
    const hipError_t e = tr_run_sequence(left, right, disp16, frames, rows, cols, *params, nullptr, &o, s, &temps);
    const int rc = tr_close(call, e, s, &temps);
    if (rc) return rc;
    if (o.too_small)
        return tr_refuse(call, SSBA_ERR_INVALID_ARGUMENT, "capacity " + std::to_string(capacity) + " is below the " + std::to_string(o.needed) + " observations found");
    return SSBA_OK;
}

void ssba_track_default_refine_params(ssba_track_refine_params *params) {
    if (!params) return;
    *params = ssba_track_refine_params{10, 4, 0};
}

int ssba_track_refine(const uint8_t *images, uint32_t n, uint32_t rows, uint32_t cols, const int32_t *items, uint32_t num_items,
                      const ssba_track_refine_params *refine_params, int device, int32_t *xy_q8, int32_t *status, uint32_t *sad) {
    const char *call = "ssba_track_refine";
    if (!images) return tr_refuse(call, SSBA_ERR_INVALID_ARGUMENT, "NULL image");
    if (num_items && !items) return tr_refuse(call, SSBA_ERR_INVALID_ARGUMENT, "NULL items");
    if (num_items && (!xy_q8 || !status || !sad)) return tr_refuse(call, SSBA_ERR_INVALID_ARGUMENT, "NULL output");
    if (const int rc = tr_check_refine_params(call, refine_params)) return rc;
    if (n < 1 || n > 65535) return tr_refuse(call, SSBA_ERR_INVALID_ARGUMENT, "n must be in 1 ... 65535");
    if (const int rc = tr_check_size(call, rows, cols)) return rc;
    for (uint32_t k = 0; k < num_items; ++k) {
        const int32_t *it = items + (size_t)k * RF_ITEM;
        if (it[0] < 0 || (uint32_t)it[0] >= n || it[3] < 0 || (uint32_t)it[3] >= n)
            return tr_refuse(call, SSBA_ERR_INVALID_ARGUMENT, "item " + std::to_string(k) + " names an image index outside 0 ... n - 1");
        if (it[6] != 0 && it[6] != 1) return tr_refuse(call, SSBA_ERR_INVALID_ARGUMENT, "item " + std::to_string(k) + " has an unknown mode");
    }
    if (!num_items) return SSBA_OK;
    hipStream_t s = nullptr;
    if (const int rc = tr_open_device(call, device, &s)) return rc;
    std::vector<void *> temps;
    const hipError_t e = tr_run_refine(images, n, rows, cols, items, num_items, *refine_params, xy_q8, status, sad, s, &temps);
    return tr_close(call, e, s, &temps);
}

int ssba_track_sequence_subpixel(const uint8_t *left, const uint8_t *right, const int16_t *disp16, uint32_t frames, uint32_t rows, uint32_t cols,
                                 const ssba_track_params *params, int device, uint64_t capacity, uint32_t *state_start, uint32_t *point_id, double *uvd,
                                 uint64_t *num_observations, uint32_t *num_points, const ssba_track_refine_params *refine_params, uint64_t *num_dropped) {
    const char *call = "ssba_track_sequence_subpixel";
    if (!left) return tr_refuse(call, SSBA_ERR_INVALID_ARGUMENT, "NULL left images");
    if (!right == !disp16) return tr_refuse(call, SSBA_ERR_INVALID_ARGUMENT, "exactly one of right and disp16 must be given");
    if (!state_start || !num_observations || !num_points || !num_dropped || (capacity && (!point_id || !uvd)))
        return tr_refuse(call, SSBA_ERR_INVALID_ARGUMENT, "NULL output");
    if (const int rc = tr_check_params(call, params)) return rc;
    if (const int rc = tr_check_refine_params(call, refine_params)) return rc;
    if (frames < 1 || frames > 32767) return tr_refuse(call, SSBA_ERR_INVALID_ARGUMENT, "frames must be in 1 ... 32767");
    if (const int rc = tr_check_size(call, rows, cols)) return rc;
    hipStream_t s = nullptr;
    if (const int rc = tr_open_device(call, device, &s)) return rc;
    std::vector<void *> temps;
    SequenceOut o = {capacity, state_start, point_id, uvd, num_observations, num_points, num_dropped};
    const hipError_t e = tr_run_sequence(left, right, disp16, frames, rows, cols, *params, refine_params, &o, s, &temps);
    const int rc = tr_close(call, e, s, &temps);
    if (rc) return rc;
    if (o.too_small)
        return tr_refuse(call, SSBA_ERR_INVALID_ARGUMENT, "capacity " + std::to_string(capacity) + " is below the " + std::to_string(o.needed) + " observations found");
    return SSBA_OK;
}

}  // extern "C"
