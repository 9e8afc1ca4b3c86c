// The 6 x 6 pose block in packed upper storage and its Cholesky solve, shared by the layouts whose reduced system is one such
// block per free pose: pose-only (ssba_kernels.hip) and dense photometric alignment (ssba_image.hip).
#pragma once
#include "ssba_device.h"

namespace ssba {

static __device__ __forceinline__ int tri21(int r, int c) {   // packed upper index, r <= c
    return r * 6 - (r * (r - 1)) / 2 + (c - r);
}

// 6 x 6 Cholesky of the packed upper triangle A (tri21 order), then x = -A^-1 g; false on a non-positive or non-finite pivot
static __device__ __forceinline__ bool po_solve6(const double A[21], const double g[6], double x[6]) {
    double Lw[6][6];
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        double v = A[tri21(j, j)];
#pragma unroll
        for (int q = 0; q < j; ++q) v -= Lw[j][q] * Lw[j][q];
        if (!(v > 0.0) || !isfinite(v)) return false;
        const double piv = sqrt(v), ip = 1.0 / piv;
        Lw[j][j] = piv;
#pragma unroll
        for (int i = j + 1; i < 6; ++i) {
            double w = A[tri21(j, i)];
#pragma unroll
            for (int q = 0; q < j; ++q) w -= Lw[i][q] * Lw[j][q];
            Lw[i][j] = w * ip;
        }
    }
    double y[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        double v = -g[i];
#pragma unroll
        for (int q = 0; q < i; ++q) v -= Lw[i][q] * y[q];
        y[i] = v / Lw[i][i];
    }
#pragma unroll
    for (int i = 5; i >= 0; --i) {
        double v = y[i];
#pragma unroll
        for (int q = i + 1; q < 6; ++q) v -= Lw[q][i] * x[q];
        x[i] = v / Lw[i][i];
    }
    return true;
}

}  // namespace ssba
