// The pre-processing of the reference's dense driver (tests/dense_stereo_test.cpp:52-72) on the device: cv::pyrDown on the 8-bit
// pair, convertTo(CV_64F, 1./255.), cv::Sobel, and the disparity map carried to the coarser levels; plus the coarse-to-fine
// solve over the levels (ssba_image_pyramid_align).  The arithmetic is stated in include/ssba.h; tests/pyramid_reference.py
// restates it in numpy.
//
// A pyramid of n levels is 2 n - 1 launches on its own stream:
//     k_pyr_down    per level > 0, both images (blockIdx.z): a work-group stages the (2 * 32 + 3) x (2 * 8 + 3) source bytes of
//                   its 32 x 8 destination tile in LDS, border reflected on the way in, and each lane forms its 5 x 5 sum in
//                   integers:  dst = (sum w_i w_j src + 128) >> 8
//     k_pyr_finish  per level, one lane per pixel: ref and track as double, the two Sobel images of the chosen source, and above
//                   disparity_level the disparity d_l[y][x] = d_{l-1}[2 y][2 x] / 2
// No atomics and no sums across lanes: two builds give the same bits.
//
// ssba_image_pyramid_create_stereo has no disparity map to upload: the right image of the reference instant is halved down to
// disparity_level by the same k_pyr_down (one more launch per level, on levels that only the matcher reads) and the semi-global
// matcher of ssba_sgbm.hip writes its double map straight into the level's disparity buffer, ahead of the k_pyr_finish that
// derives the next level from it.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../include/ssba.h"
#include "ssba_image_pyramid.h"
#include "ssba_pool.h"
#include "ssba_sgbm.h"

namespace ssba {

void set_last_error(const std::string &s);      // ssba_api.hip

constexpr int PYR_TW = 32, PYR_TH = 8, PYR_THREADS = PYR_TW * PYR_TH;
constexpr int PYR_SW = 2 * PYR_TW + 3, PYR_SH = 2 * PYR_TH + 3, PYR_STRIDE = PYR_SW + 1;
constexpr int PYR_MIN_SIDE = 8;

// BORDER_REFLECT_101: -1 -> 1, -2 -> 2, n -> n - 2, n + 1 -> n - 3.  Lanes of a partial tile ask for indices far outside; those
// values are never used and only have to stay inside the image.
static __device__ __forceinline__ int pyr_reflect(int i, int n) {
    if (i < 0) i = -i;
    if (i >= n) i = 2 * n - 2 - i;
    return min(max(i, 0), n - 1);
}

static __device__ __forceinline__ void pyr_down_body(uint8_t *tile, const uint8_t *src, uint8_t *dst, int srows, int scols,
                                                     int drows, int dcols) {
    const int x0 = blockIdx.x * PYR_TW, y0 = blockIdx.y * PYR_TH;
    for (int i = threadIdx.x; i < PYR_SH * PYR_SW; i += PYR_THREADS) {
        const int r = i / PYR_SW, c = i - r * PYR_SW;
        const int sy = pyr_reflect(2 * y0 - 2 + r, srows), sx = pyr_reflect(2 * x0 - 2 + c, scols);
        tile[r * PYR_STRIDE + c] = src[(size_t)sy * scols + sx];
    }
    __syncthreads();
    const int tx = threadIdx.x % PYR_TW, ty = threadIdx.x / PYR_TW;
    const int x = x0 + tx, y = y0 + ty;
    if (x >= dcols || y >= drows) return;
    const int w[5] = {1, 4, 6, 4, 1};
    int sum = 0;
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        const uint8_t *row = tile + (2 * ty + i) * PYR_STRIDE + 2 * tx;
        sum += w[i] * ((int)row[0] + 4 * (int)row[1] + 6 * (int)row[2] + 4 * (int)row[3] + (int)row[4]);
    }
    dst[(size_t)y * dcols + x] = (uint8_t)((sum + 128) >> 8);
}

__global__ __launch_bounds__(PYR_THREADS) void k_pyr_down(const uint8_t *__restrict__ src0, const uint8_t *__restrict__ src1,
                                                          uint8_t *__restrict__ dst0, uint8_t *__restrict__ dst1, int srows, int scols,
                                                          int drows, int dcols) {
    __shared__ uint8_t tile[PYR_SH * PYR_STRIDE];
    pyr_down_body(tile, blockIdx.z ? src1 : src0, blockIdx.z ? dst1 : dst0, srows, scols, drows, dcols);
}

// One level of a sequence: image blockIdx.z of a frame-major buffer, the strides in pixels of the two levels
__global__ __launch_bounds__(PYR_THREADS) void k_pyr_down_seq(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, int srows, int scols, int drows,
                                                              int dcols) {
    __shared__ uint8_t tile[PYR_SH * PYR_STRIDE];
    pyr_down_body(tile, src + (size_t)blockIdx.z * srows * scols, dst + (size_t)blockIdx.z * drows * dcols, srows, scols, drows, dcols);
}

// convertTo(CV_64F, 1. / 255.): the converted image is rounded before it is differenced, as convertTo stores it
static __device__ __forceinline__ double pyr_convert(uint8_t u) {
#pragma clang fp contract(off)
    const double k = 1.0 / 255.0;
    return (double)u * k;
}

// the two Sobel images of g at (x, y), border reflected
static __device__ __forceinline__ void pyr_sobel(const uint8_t *__restrict__ g, int x, int y, int rows, int cols, double scale, double *gx, double *gy) {
#pragma clang fp contract(off)
    const int xm = x > 0 ? x - 1 : 1, xp = x + 1 < cols ? x + 1 : cols - 2;
    const int ym = y > 0 ? y - 1 : 1, yp = y + 1 < rows ? y + 1 : rows - 2;
    const uint8_t *__restrict__ r0 = g + (size_t)ym * cols, *__restrict__ r1 = g + (size_t)y * cols, *__restrict__ r2 = g + (size_t)yp * cols;
    const double a00 = pyr_convert(r0[xm]), a01 = pyr_convert(r0[x]), a02 = pyr_convert(r0[xp]);
    const double a10 = pyr_convert(r1[xm]), a12 = pyr_convert(r1[xp]);
    const double a20 = pyr_convert(r2[xm]), a21 = pyr_convert(r2[x]), a22 = pyr_convert(r2[xp]);
    // the summation order of synth.sobel: (first row + 2 * middle row) + last row, then the scale
    *gx = scale * (((a02 - a00) + 2.0 * (a12 - a10)) + (a22 - a20));
    *gy = scale * (((a20 - a00) + 2.0 * (a21 - a01)) + (a22 - a02));
}

// d_l[y][x] = d_{l-1}[2 y][2 x] / 2
static __device__ __forceinline__ double pyr_disp_down(const double *__restrict__ disp_src, int x, int y, int src_cols) {
    return disp_src[(size_t)(2 * y) * src_cols + 2 * x] / 2.0;
}

// disp_dst = nullptr below and at disparity_level; disp_src is the finer level's map, src_cols wide
__global__ __launch_bounds__(PYR_THREADS) void k_pyr_finish(const uint8_t *__restrict__ u0, const uint8_t *__restrict__ u1, double *__restrict__ ref,
                                                            double *__restrict__ track, double *__restrict__ gradx, double *__restrict__ grady, int rows,
                                                            int cols, int gradient_source, double scale, const double *__restrict__ disp_src,
                                                            double *__restrict__ disp_dst, int src_cols) {
    const int x = blockIdx.x * PYR_TW + threadIdx.x % PYR_TW, y = blockIdx.y * PYR_TH + threadIdx.x / PYR_TW;
    if (x >= cols || y >= rows) return;
    const size_t i = (size_t)y * cols + x;
    ref[i] = pyr_convert(u0[i]);
    track[i] = pyr_convert(u1[i]);
    double gx, gy;
    pyr_sobel(gradient_source == SSBA_GRADIENT_OF_TRACKED ? u1 : u0, x, y, rows, cols, scale, &gx, &gy);
    gradx[i] = gx;
    grady[i] = gy;
    if (disp_dst) disp_dst[i] = pyr_disp_down(disp_src, x, y, src_cols);
}

// One level of a sequence, frame blockIdx.z: the frame's double image and its two Sobel images, once for both of its roles (the
// tracked image of pair z - 1, the reference image of pair z), and for z < npairs above disparity_level pair z's disparity map.
// u8, img, gradx, grady and disp_dst are frame-major with rows * cols between frames, disp_src with src_rows * src_cols.
__global__ __launch_bounds__(PYR_THREADS) void k_pyr_finish_seq(const uint8_t *__restrict__ u8, double *__restrict__ img, double *__restrict__ gradx,
                                                                double *__restrict__ grady, int rows, int cols, double scale, int npairs,
                                                                const double *__restrict__ disp_src, double *__restrict__ disp_dst, int src_rows,
                                                                int src_cols) {
    const int x = blockIdx.x * PYR_TW + threadIdx.x % PYR_TW, y = blockIdx.y * PYR_TH + threadIdx.x / PYR_TW;
    if (x >= cols || y >= rows) return;
    const size_t npix = (size_t)rows * cols, f = blockIdx.z, i = f * npix + (size_t)y * cols + x;
    const uint8_t *__restrict__ u = u8 + f * npix;
    img[i] = pyr_convert(u[(size_t)y * cols + x]);
    double gx, gy;
    pyr_sobel(u, x, y, rows, cols, scale, &gx, &gy);
    gradx[i] = gx;
    grady[i] = gy;
    if (disp_dst && (int)f < npairs) disp_dst[i] = pyr_disp_down(disp_src + f * (size_t)src_rows * src_cols, x, y, src_cols);
}

template <class T>
static hipError_t pyr_alloc(ssba_image_pyramid *pyr, T **out, size_t n) {
    void *p = nullptr;
    const hipError_t e = pool_malloc(&p, n * sizeof(T));
    if (e != hipSuccess) return e;
    pyr->allocs.push_back(p);
    *out = (T *)p;
    return hipSuccess;
}

static void pyr_free(ssba_image_pyramid *pyr) {
    hipSetDevice(pyr->device);
    if (pyr->stream) hipStreamSynchronize(pyr->stream);
    for (void *a : pyr->allocs) pool_free(a);
    if (pyr->stream) pool_stream_release(pyr->stream);
    delete pyr;
}

#define PYR_HIP(expr)                                                                                  \
    do {                                                                                               \
        hipError_t _e = (expr);                                                                        \
        if (_e != hipSuccess) {                                                                        \
            set_last_error(std::string("ssba_image_pyramid: ") + #expr + ": " + hipGetErrorString(_e)); \
            return SSBA_ERR_HIP;                                                                       \
        }                                                                                              \
    } while (0)

// disparity: the caller's map at disparity_level, or nullptr with right_u8 and the matcher's plan for that level
static int pyr_build(ssba_image_pyramid *pyr, const uint8_t *ref_u8, const uint8_t *track_u8, const double *disparity, const uint8_t *right_u8,
                     const SgbmPlan *plan, char *stage, std::vector<void *> *temps) {
    const int n = (int)pyr->lv.size(), dl = pyr->disparity_level;
    std::vector<uint8_t *> right(right_u8 ? dl + 1 : 0, nullptr);
    for (size_t l = 0; l < right.size(); ++l) {      // the right levels and the matcher's volumes are released when the build is complete
        void *ptr = nullptr;
        PYR_HIP(pool_malloc(&ptr, (size_t)pyr->lv[l].rows * pyr->lv[l].cols));
        temps->push_back(ptr);
        right[l] = (uint8_t *)ptr;
    }
    for (int l = 0; l < n; ++l) {
        ssba_image_pyramid::Level &L = pyr->lv[l];
        const size_t npix = (size_t)L.rows * L.cols;
        for (int q = 0; q < 2; ++q) PYR_HIP(pyr_alloc(pyr, &L.u8[q], npix));
        for (int q = 0; q < 4; ++q) PYR_HIP(pyr_alloc(pyr, &L.img[q], npix));
        if (l >= dl) PYR_HIP(pyr_alloc(pyr, &L.disp, npix));
    }
    const size_t n0 = (size_t)pyr->lv[0].rows * pyr->lv[0].cols, nd = (size_t)pyr->lv[dl].rows * pyr->lv[dl].cols;
    memcpy(stage, ref_u8, n0);
    memcpy(stage + n0, track_u8, n0);
    const size_t od = (2 * n0 + 255) / 256 * 256;
    if (disparity) memcpy(stage + od, disparity, nd * sizeof(double));
    else memcpy(stage + od, right_u8, n0);
    hipStream_t s = pyr->stream;
    PYR_HIP(hipMemcpyAsync(pyr->lv[0].u8[0], stage, n0, hipMemcpyHostToDevice, s));
    PYR_HIP(hipMemcpyAsync(pyr->lv[0].u8[1], stage + n0, n0, hipMemcpyHostToDevice, s));
    if (disparity) PYR_HIP(hipMemcpyAsync(pyr->lv[dl].disp, stage + od, nd * sizeof(double), hipMemcpyHostToDevice, s));
    else PYR_HIP(hipMemcpyAsync(right[0], stage + od, n0, hipMemcpyHostToDevice, s));
    for (int l = 0; l < n; ++l) {
        const ssba_image_pyramid::Level &L = pyr->lv[l];
        const dim3 grid((L.cols + PYR_TW - 1) / PYR_TW, (L.rows + PYR_TH - 1) / PYR_TH, 1);
        if (l > 0) {
            const ssba_image_pyramid::Level &F = pyr->lv[l - 1];
            hipLaunchKernelGGL(k_pyr_down, dim3(grid.x, grid.y, 2), dim3(PYR_THREADS), 0, s, (const uint8_t *)F.u8[0], (const uint8_t *)F.u8[1], L.u8[0],
                               L.u8[1], F.rows, F.cols, L.rows, L.cols);
            PYR_HIP(hipGetLastError());
            if (l < (int)right.size()) {
                hipLaunchKernelGGL(k_pyr_down, dim3(grid.x, grid.y, 1), dim3(PYR_THREADS), 0, s, (const uint8_t *)right[l - 1], (const uint8_t *)right[l - 1],
                                   right[l], right[l], F.rows, F.cols, L.rows, L.cols);
                PYR_HIP(hipGetLastError());
            }
        }
        if (l == dl && !disparity) PYR_HIP(sgbm_enqueue(*plan, L.u8[0], right[dl], nullptr, L.disp, s, temps));
        const bool derive = l > dl;
        hipLaunchKernelGGL(k_pyr_finish, grid, dim3(PYR_THREADS), 0, s, (const uint8_t *)L.u8[0], (const uint8_t *)L.u8[1], L.img[0], L.img[1], L.img[2],
                           L.img[3], L.rows, L.cols, pyr->gradient_source, pyr->gradient_scale, derive ? (const double *)pyr->lv[l - 1].disp : nullptr,
                           derive ? L.disp : nullptr, derive ? pyr->lv[l - 1].cols : 0);
        PYR_HIP(hipGetLastError());
    }
    PYR_HIP(hipStreamSynchronize(s));
    return SSBA_OK;
}

static int pyr_invalid(const char *call, const char *what) {
    set_last_error(std::string(call) + ": " + what);
    return SSBA_ERR_INVALID_ARGUMENT;
}

// ssba_image_pyramid_create (disparity) and ssba_image_pyramid_create_stereo (right_u8 and params)
static int pyr_create(const char *call, const uint8_t *ref_u8, const uint8_t *track_u8, const double *disparity, const uint8_t *right_u8,
                      const ssba_sgbm_params *params, uint32_t rows, uint32_t cols, uint32_t levels, uint32_t disparity_level, int gradient_source,
                      double gradient_scale, int device, ssba_image_pyramid **out) {
    if (!out) return pyr_invalid(call, "NULL output");
    *out = nullptr;
    if (!ref_u8 || !track_u8 || (!disparity && !right_u8)) return pyr_invalid(call, "NULL array");
    if (levels == 0) return pyr_invalid(call, "levels = 0");
    if (disparity_level >= levels) return pyr_invalid(call, "disparity_level must be below levels");
    if (gradient_source != SSBA_GRADIENT_OF_REFERENCE && gradient_source != SSBA_GRADIENT_OF_TRACKED) return pyr_invalid(call, "unknown gradient source");
    if (!std::isfinite(gradient_scale) || gradient_scale == 0.0) return pyr_invalid(call, "gradient_scale must be finite and not zero");
    if (levels > 31 || (rows >> (levels - 1)) < (uint32_t)PYR_MIN_SIDE || (cols >> (levels - 1)) < (uint32_t)PYR_MIN_SIDE)
        return pyr_invalid(call, "every level needs at least 8 rows and 8 columns");
    if ((uint64_t)rows * cols >= (1ull << 31)) {
        set_last_error(std::string(call) + ": image too large for the 32-bit pixel references of this build");
        return SSBA_ERR_UNSUPPORTED;
    }
    SgbmPlan plan{};
    if (!disparity)
        if (const int rc = sgbm_check(call, rows >> disparity_level, cols >> disparity_level, params, &plan)) return rc;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
        set_last_error(std::string(call) + ": hipGetDeviceCount found no device");
        return SSBA_ERR_NO_DEVICE;
    }
    if (device < 0 && hipGetDevice(&device) != hipSuccess) return SSBA_ERR_NO_DEVICE;
    if (device >= n) return pyr_invalid(call, "no such device");
    PYR_HIP(hipSetDevice(device));
    ssba_image_pyramid *pyr = new ssba_image_pyramid();
    pyr->device = device;
    pyr->disparity_level = (int)disparity_level;
    pyr->gradient_source = gradient_source;
    pyr->gradient_scale = gradient_scale;
    pyr->lv.resize(levels);
    for (uint32_t l = 0; l < levels; ++l) { pyr->lv[l].rows = (int)(rows >> l); pyr->lv[l].cols = (int)(cols >> l); }
    int rc = SSBA_OK;
    void *stage = nullptr;
    std::vector<void *> temps;
    const size_t n0 = (size_t)rows * cols, nd = (size_t)pyr->lv[disparity_level].rows * pyr->lv[disparity_level].cols;
    const size_t tail = disparity ? nd * sizeof(double) : n0;
    if (pool_stream_acquire(&pyr->stream) != hipSuccess || pool_host_malloc(&stage, (2 * n0 + 255) / 256 * 256 + tail) != hipSuccess) {
        set_last_error(std::string(call) + ": no stream or no pinned staging memory");
        rc = SSBA_ERR_HIP;
    } else {
        rc = pyr_build(pyr, ref_u8, track_u8, disparity, right_u8, &plan, (char *)stage, &temps);
    }
    if (stage) { if (pyr->stream) hipStreamSynchronize(pyr->stream); pool_host_free(stage); }
    for (void *t : temps) pool_free(t);
    if (rc) { pyr_free(pyr); return rc; }
    *out = pyr;
    return SSBA_OK;
}

template <class T>
static hipError_t seq_alloc(ssba_image_sequence *seq, T **out, size_t n) {
    void *p = nullptr;
    const hipError_t e = pool_malloc(&p, n * sizeof(T));
    if (e != hipSuccess) return e;
    seq->allocs.push_back(p);
    *out = (T *)p;
    return hipSuccess;
}

static void seq_free(ssba_image_sequence *seq) {
    hipSetDevice(seq->device);
    if (seq->stream) hipStreamSynchronize(seq->stream);
    for (ssba_image_pyramid *p : seq->pairs) delete p;
    for (void *a : seq->allocs) pool_free(a);
    if (seq->stream) pool_stream_release(seq->stream);
    delete seq;
}

// The build of a sequence: 2 levels + 4 launches while the pairs fit one matcher chunk (levels - 1 k_pyr_down_seq, the five
// matcher kernels per chunk, levels k_pyr_finish_seq), one copy up and one synchronisation.
static int seq_build(ssba_image_sequence *seq, const uint8_t *left, const uint8_t *right, uint32_t frames, uint32_t rows, uint32_t cols, uint32_t levels,
                     uint32_t dl, const SgbmPlan &plan, uint32_t chunk_pairs, int gradient_source, double gradient_scale, char *stage,
                     std::vector<void *> *temps) {
    const uint32_t npairs = frames - 1;
    const size_t n0 = (size_t)rows * cols;
    std::vector<uint8_t *> u8(levels, nullptr);
    std::vector<double *> img(levels, nullptr), gx(levels, nullptr), gy(levels, nullptr), disp(levels, nullptr);
    for (uint32_t l = 0; l < levels; ++l) {
        const size_t npix = (size_t)(rows >> l) * (cols >> l);
        PYR_HIP(seq_alloc(seq, &u8[l], npix * (frames + (l <= dl ? npairs : 0))));
        PYR_HIP(seq_alloc(seq, &img[l], npix * frames));
        PYR_HIP(seq_alloc(seq, &gx[l], npix * frames));
        PYR_HIP(seq_alloc(seq, &gy[l], npix * frames));
        if (l >= dl) PYR_HIP(seq_alloc(seq, &disp[l], npix * npairs));
    }
    memcpy(stage, left, n0 * frames);
    memcpy(stage + n0 * frames, right, n0 * npairs);
    hipStream_t s = seq->stream;
    PYR_HIP(hipMemcpyAsync(u8[0], stage, n0 * (frames + npairs), hipMemcpyHostToDevice, s));
    for (uint32_t l = 0; l < levels; ++l) {
        const int r = (int)(rows >> l), c = (int)(cols >> l);
        const size_t npix = (size_t)r * c;
        const dim3 grid((c + PYR_TW - 1) / PYR_TW, (r + PYR_TH - 1) / PYR_TH, 1);
        if (l > 0) {
            hipLaunchKernelGGL(k_pyr_down_seq, dim3(grid.x, grid.y, frames + (l <= dl ? npairs : 0)), dim3(PYR_THREADS), 0, s, (const uint8_t *)u8[l - 1], u8[l],
                               (int)(rows >> (l - 1)), (int)(cols >> (l - 1)), r, c);
            PYR_HIP(hipGetLastError());
        }
        if (l == dl) PYR_HIP(sgbm_enqueue_batch(plan, u8[l], u8[l] + npix * frames, npix, npairs, chunk_pairs, nullptr, disp[l], s, temps));
        const bool derive = l > dl;
        hipLaunchKernelGGL(k_pyr_finish_seq, dim3(grid.x, grid.y, frames), dim3(PYR_THREADS), 0, s, (const uint8_t *)u8[l], img[l], gx[l], gy[l], r, c, gradient_scale,
                           (int)npairs, derive ? (const double *)disp[l - 1] : nullptr, derive ? disp[l] : nullptr, derive ? (int)(rows >> (l - 1)) : 0,
                           derive ? (int)(cols >> (l - 1)) : 0);
        PYR_HIP(hipGetLastError());
    }
    for (uint32_t k = 0; k < npairs; ++k) {
        ssba_image_pyramid *pyr = new ssba_image_pyramid();
        seq->pairs.push_back(pyr);
        pyr->borrowed = true;
        pyr->device = seq->device;
        pyr->stream = s;
        pyr->disparity_level = (int)dl;
        pyr->gradient_source = gradient_source;
        pyr->gradient_scale = gradient_scale;
        pyr->lv.resize(levels);
        const size_t g = gradient_source == SSBA_GRADIENT_OF_TRACKED ? k + 1 : k;
        for (uint32_t l = 0; l < levels; ++l) {
            ssba_image_pyramid::Level &L = pyr->lv[l];
            L.rows = (int)(rows >> l);
            L.cols = (int)(cols >> l);
            const size_t npix = (size_t)L.rows * L.cols;
            L.u8[0] = u8[l] + npix * k;
            L.u8[1] = u8[l] + npix * (k + 1);
            L.img[0] = img[l] + npix * k;
            L.img[1] = img[l] + npix * (k + 1);
            L.img[2] = gx[l] + npix * g;
            L.img[3] = gy[l] + npix * g;
            L.disp = l >= dl ? disp[l] + npix * k : nullptr;
        }
    }
    PYR_HIP(hipStreamSynchronize(s));
    return SSBA_OK;
}

}  // namespace ssba

using namespace ssba;

extern "C" {

int ssba_image_pyramid_create(const uint8_t *ref_u8, const uint8_t *track_u8, const double *disparity, uint32_t rows, uint32_t cols,
                              uint32_t levels, uint32_t disparity_level, int gradient_source, double gradient_scale, int device,
                              ssba_image_pyramid **out) {
    if (out) *out = nullptr;
    if (!disparity) return pyr_invalid("ssba_image_pyramid_create", "NULL array");
    return pyr_create("ssba_image_pyramid_create", ref_u8, track_u8, disparity, nullptr, nullptr, rows, cols, levels, disparity_level, gradient_source,
                      gradient_scale, device, out);
}

int ssba_image_pyramid_create_stereo(const uint8_t *ref_left_u8, const uint8_t *ref_right_u8, const uint8_t *track_u8, uint32_t rows, uint32_t cols,
                                     uint32_t levels, uint32_t disparity_level, const ssba_sgbm_params *params, int gradient_source,
                                     double gradient_scale, int device, ssba_image_pyramid **out) {
    if (out) *out = nullptr;
    if (!ref_right_u8) return pyr_invalid("ssba_image_pyramid_create_stereo", "NULL array");
    return pyr_create("ssba_image_pyramid_create_stereo", ref_left_u8, track_u8, nullptr, ref_right_u8, params, rows, cols, levels, disparity_level,
                      gradient_source, gradient_scale, device, out);
}

int ssba_image_pyramid_destroy(ssba_image_pyramid *pyr) {
    if (!pyr) return pyr_invalid("ssba_image_pyramid_destroy", "NULL pyramid");
    if (pyr->borrowed) return pyr_invalid("ssba_image_pyramid_destroy", "the pyramid is borrowed from an image sequence and ends with it (ssba_image_sequence_destroy)");
    pyr_free(pyr);
    return SSBA_OK;
}

int ssba_image_sequence_create(const uint8_t *left, const uint8_t *right, uint32_t frames, uint32_t rows, uint32_t cols, uint32_t levels,
                               uint32_t disparity_level, const ssba_sgbm_params *params, uint64_t workspace_bytes, int gradient_source,
                               double gradient_scale, int device, ssba_image_sequence **out) {
    const char *call = "ssba_image_sequence_create";
    if (!out) return pyr_invalid(call, "NULL output");
    *out = nullptr;
    if (!left || !right) return pyr_invalid(call, "NULL array");
    if (frames < 2) return pyr_invalid(call, "a sequence needs at least 2 frames");
    if (levels == 0) return pyr_invalid(call, "levels = 0");
    if (disparity_level >= levels) return pyr_invalid(call, "disparity_level must be below levels");
    if (gradient_source != SSBA_GRADIENT_OF_REFERENCE && gradient_source != SSBA_GRADIENT_OF_TRACKED) return pyr_invalid(call, "unknown gradient source");
    if (!std::isfinite(gradient_scale) || gradient_scale == 0.0) return pyr_invalid(call, "gradient_scale must be finite and not zero");
    if (levels > 31 || (rows >> (levels - 1)) < (uint32_t)PYR_MIN_SIDE || (cols >> (levels - 1)) < (uint32_t)PYR_MIN_SIDE)
        return pyr_invalid(call, "every level needs at least 8 rows and 8 columns");
    if ((uint64_t)rows * cols >= (1ull << 31)) {
        set_last_error(std::string(call) + ": image too large for the 32-bit pixel references of this build");
        return SSBA_ERR_UNSUPPORTED;
    }
    if (frames > 32768) return pyr_invalid(call, "at most 32768 frames (the 2 frames - 1 images of a level are one grid dimension)");
    SgbmPlan plan{};
    if (const int rc = sgbm_check(call, rows >> disparity_level, cols >> disparity_level, params, &plan)) return rc;
    uint32_t chunk_pairs = 0;
    if (const int rc = sgbm_chunk_pairs(call, plan, frames - 1, workspace_bytes, &chunk_pairs)) return rc;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
        set_last_error(std::string(call) + ": hipGetDeviceCount found no device");
        return SSBA_ERR_NO_DEVICE;
    }
    if (device < 0 && hipGetDevice(&device) != hipSuccess) return SSBA_ERR_NO_DEVICE;
    if (device >= n) return pyr_invalid(call, "no such device");
    PYR_HIP(hipSetDevice(device));
    ssba_image_sequence *seq = new ssba_image_sequence();
    seq->device = device;
    int rc = SSBA_OK;
    void *stage = nullptr;
    std::vector<void *> temps;
    if (pool_stream_acquire(&seq->stream) != hipSuccess || pool_host_malloc(&stage, (size_t)rows * cols * (2 * (size_t)frames - 1)) != hipSuccess) {
        set_last_error(std::string(call) + ": no stream or no pinned staging memory");
        rc = SSBA_ERR_HIP;
    } else {
        rc = seq_build(seq, left, right, frames, rows, cols, levels, disparity_level, plan, chunk_pairs, gradient_source, gradient_scale, (char *)stage, &temps);
    }
    if (stage) { if (seq->stream) hipStreamSynchronize(seq->stream); pool_host_free(stage); }
    for (void *t : temps) pool_free(t);
    if (rc) { seq_free(seq); return rc; }
    *out = seq;
    return SSBA_OK;
}

int ssba_image_sequence_pyramid(ssba_image_sequence *seq, uint32_t k, ssba_image_pyramid **out) {
    const char *call = "ssba_image_sequence_pyramid";
    if (out) *out = nullptr;
    if (!seq || !out) return pyr_invalid(call, "NULL argument");
    if (k >= seq->pairs.size()) return pyr_invalid(call, ("no such pair: the sequence has " + std::to_string(seq->pairs.size())).c_str());
    *out = seq->pairs[k];
    return SSBA_OK;
}

int ssba_image_sequence_destroy(ssba_image_sequence *seq) {
    if (!seq) return pyr_invalid("ssba_image_sequence_destroy", "NULL sequence");
    seq_free(seq);
    return SSBA_OK;
}

int ssba_image_pyramid_level(ssba_image_pyramid *pyr, uint32_t level, uint32_t *rows, uint32_t *cols, uint8_t *ref_u8, uint8_t *track_u8,
                             double *ref, double *track, double *gradx, double *grady, double *disparity) {
    const char *call = "ssba_image_pyramid_level";
    if (!pyr) return pyr_invalid(call, "NULL pyramid");
    if (level >= pyr->lv.size()) return pyr_invalid(call, "no such level");
    if (disparity && (int)level < pyr->disparity_level) return pyr_invalid(call, "levels finer than disparity_level have no disparity map");
    const ssba_image_pyramid::Level &L = pyr->lv[level];
    if (rows) *rows = (uint32_t)L.rows;
    if (cols) *cols = (uint32_t)L.cols;
    const size_t npix = (size_t)L.rows * L.cols;
    PYR_HIP(hipSetDevice(pyr->device));
    if (ref_u8) PYR_HIP(hipMemcpyAsync(ref_u8, L.u8[0], npix, hipMemcpyDeviceToHost, pyr->stream));
    if (track_u8) PYR_HIP(hipMemcpyAsync(track_u8, L.u8[1], npix, hipMemcpyDeviceToHost, pyr->stream));
    double *dst[5] = {ref, track, gradx, grady, disparity};
    const double *src[5] = {L.img[0], L.img[1], L.img[2], L.img[3], L.disp};
    for (int q = 0; q < 5; ++q)
        if (dst[q]) PYR_HIP(hipMemcpyAsync(dst[q], src[q], npix * sizeof(double), hipMemcpyDeviceToHost, pyr->stream));
    PYR_HIP(hipStreamSynchronize(pyr->stream));
    return SSBA_OK;
}

// the loss of every level's handle: one width for all levels, intensities do not scale with the level
int ssba_image_pyramid_set_huber_loss(ssba_image_pyramid *pyr, double a) {
    if (!pyr) return pyr_invalid("ssba_image_pyramid_set_huber_loss", "NULL pyramid");
    pyr->huber_a = a > 0.0 ? a : 0.0;
    return SSBA_OK;
}

// Per-level set-up shared by ssba_image_pyramid_align and ssba_image_pyramid_align_batch: the map the handle's blocks come from
// (the caller's at disparity_level, the level's derived map in `derived` above it) and the finalized handle on the level, with
// camera0 scaled to it.  Levels above disparity_level hold their derived disparities constant (free, they absorb the motion and
// the pose does not move).
static int pyr_level_handle(ssba_image_pyramid *pyr, const ssba_camera *camera0, int l, double *pose, double *disparity, std::vector<double> &derived,
                            int interpolation, int disparities_constant, ssba_problem **out) {
    *out = nullptr;
    const ssba_image_pyramid::Level &L = pyr->lv[l];
    const bool base = l == pyr->disparity_level;
    const double s = ldexp(1.0, -l);       // pyrDown samples at even pixels: u_l = u / 2^l exactly
    const ssba_camera cam = {camera0->fu * s, camera0->fv * s, camera0->cu * s, camera0->cv * s, camera0->b};
    double *map = disparity;
    int rc;
    if (!base) {
        derived.resize((size_t)L.rows * L.cols);
        if ((rc = ssba_image_pyramid_level(pyr, (uint32_t)l, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, derived.data()))) return rc;
        map = derived.data();
    }
    ssba_problem *h = nullptr;
    if ((rc = ssba_create(&cam, pyr->device, &h))) return rc;
    if ((rc = ssba_add_image_level(h, pyr, (uint32_t)l, pose, map, interpolation)) || (rc = ssba_set_huber_loss(h, pyr->huber_a)) ||
        (rc = ssba_set_disparity_blocks_constant(h, base ? (disparities_constant != 0) : 1)) || (rc = ssba_finalize(h))) {
        const std::string msg = ssba_last_error();
        ssba_destroy(h);
        set_last_error(msg);
        return rc;
    }
    *out = h;
    return SSBA_OK;
}

// Coarse to fine: the reference's main from :94 on, once per level, the pose carried down.
int ssba_image_pyramid_align(ssba_image_pyramid *pyr, const ssba_camera *camera0, double *pose, double *disparity, uint32_t coarsest_level,
                             int interpolation, int disparities_constant, const ssba_options *options, ssba_summary *summaries) {
    const char *call = "ssba_image_pyramid_align";
    if (!pyr || !camera0 || !pose || !disparity || !options) return pyr_invalid(call, "NULL argument");
    if (coarsest_level >= pyr->lv.size()) return pyr_invalid(call, "no such level");
    if ((int)coarsest_level < pyr->disparity_level) return pyr_invalid(call, "coarsest_level is finer than disparity_level: no disparity map there");
    if (interpolation != SSBA_IMAGE_NEAREST && interpolation != SSBA_IMAGE_BILINEAR) return pyr_invalid(call, "unknown interpolation");
    if (options->trust_region_strategy_type != 0) {
        set_last_error(std::string(call) + ": image blocks are solved with Levenberg-Marquardt only (DOGLEG asked for)");
        return SSBA_ERR_UNSUPPORTED;
    }
    std::vector<double> derived;
    for (int l = (int)coarsest_level; l >= pyr->disparity_level; --l) {
        ssba_problem *h = nullptr;
        ssba_summary sum;
        memset(&sum, 0, sizeof sum);
        int rc = pyr_level_handle(pyr, camera0, l, pose, disparity, derived, interpolation, disparities_constant, &h);
        if (!rc) rc = ssba_solve(h, options, &sum);
        const std::string msg = rc ? std::string(ssba_last_error()) : std::string();
        if (h) ssba_destroy(h);
        if (rc) { set_last_error(std::string(call) + ": level " + std::to_string(l) + ": " + msg); }
        if (summaries && (rc == SSBA_OK || rc == SSBA_ERR_NUMERICAL_FAILURE)) summaries[coarsest_level - (uint32_t)l] = sum;
        if (rc) return rc;      // an unusable solution left the pose (and the map) as they were before this level
    }
    return SSBA_OK;
}

// The same over n pyramids in lockstep: per level one handle per pyramid still in the run and one ssba_image_solve_batch.
int ssba_image_pyramid_align_batch(ssba_image_pyramid **pyramids, uint32_t n, const ssba_camera *camera0, double *poses, double **disparities,
                                   uint32_t coarsest_level, int interpolation, int disparities_constant, const ssba_options *options,
                                   ssba_summary *summaries, int *statuses) {
    const char *call = "ssba_image_pyramid_align_batch";
    if (!pyramids || !camera0 || !poses || !disparities || !options) return pyr_invalid(call, "NULL argument");
    if (n == 0) return pyr_invalid(call, "n = 0");
    if (n > SSBA_IMAGE_BATCH_MAX) return pyr_invalid(call, "n is above SSBA_IMAGE_BATCH_MAX");
    for (uint32_t k = 0; k < n; ++k) {
        const std::string who = "pyramid " + std::to_string(k);
        if (!pyramids[k] || !disparities[k]) return pyr_invalid(call, (who + ": NULL pyramid or disparity map").c_str());
        if (pyramids[k]->device != pyramids[0]->device) return pyr_invalid(call, (who + " lives on a different device than pyramid 0").c_str());
        if (pyramids[k]->disparity_level != pyramids[0]->disparity_level) return pyr_invalid(call, (who + " has a different disparity_level than pyramid 0").c_str());
        if (coarsest_level >= pyramids[k]->lv.size()) return pyr_invalid(call, (who + " has no such level (coarsest_level)").c_str());
    }
    const int dl = pyramids[0]->disparity_level;
    if ((int)coarsest_level < dl) return pyr_invalid(call, "coarsest_level is finer than disparity_level: no disparity map there");
    if (interpolation != SSBA_IMAGE_NEAREST && interpolation != SSBA_IMAGE_BILINEAR) return pyr_invalid(call, "unknown interpolation");
    if (options->trust_region_strategy_type != 0) {
        set_last_error(std::string(call) + ": image blocks are solved with Levenberg-Marquardt only (DOGLEG asked for)");
        return SSBA_ERR_UNSUPPORTED;
    }
    const uint32_t levels = coarsest_level - (uint32_t)dl + 1;
    if (summaries) memset(summaries, 0, sizeof(ssba_summary) * (size_t)n * levels);
    std::vector<int> status(n, SSBA_OK);
    std::vector<std::vector<double>> derived(n);
    std::vector<uint32_t> who;
    std::vector<ssba_problem *> hs;
    std::vector<ssba_summary> sums;
    std::vector<int> sts;
    int fatal = SSBA_OK;
    std::string fatal_msg;
    for (int l = (int)coarsest_level; l >= dl && !fatal; --l) {
        who.clear(); hs.clear();
        for (uint32_t k = 0; k < n; ++k) {
            if (status[k]) continue;       // dropped out at a coarser level: its pose stays the last usable one
            ssba_problem *h = nullptr;
            const int rc = pyr_level_handle(pyramids[k], camera0, l, poses + (size_t)k * 12, disparities[k], derived[k], interpolation, disparities_constant, &h);
            if (rc) { status[k] = rc; continue; }
            who.push_back(k); hs.push_back(h);
        }
        if (hs.empty()) break;
        constexpr int UNSET = INT32_MIN;
        sums.assign(hs.size(), ssba_summary{});
        sts.assign(hs.size(), UNSET);
        const int rc = ssba_image_solve_batch(hs.data(), (uint32_t)hs.size(), options, 0, sums.data(), sts.data());
        if (rc && sts[0] == UNSET) {       // the batch itself failed (not a member's solve): nothing more can run
            fatal = rc;
            fatal_msg = std::string(call) + ": level " + std::to_string(l) + ": " + ssba_last_error();
        }
        for (size_t q = 0; q < hs.size(); ++q) {
            ssba_destroy(hs[q]);
            if (fatal) continue;
            const uint32_t k = who[q];
            if (summaries && (sts[q] == SSBA_OK || sts[q] == SSBA_ERR_NUMERICAL_FAILURE)) summaries[(size_t)k * levels + (coarsest_level - (uint32_t)l)] = sums[q];
            status[k] = sts[q];
        }
    }
    if (fatal) { set_last_error(fatal_msg); return fatal; }
    int first = SSBA_OK;
    for (uint32_t k = 0; k < n; ++k) {
        if (statuses) statuses[k] = status[k];
        if (status[k] && !first) {
            first = status[k];
            set_last_error(std::string(call) + ": pyramid " + std::to_string(k) + " ended without a usable solution or could not be set up at one level");
        }
    }
    return first;
}

}  // extern "C"
