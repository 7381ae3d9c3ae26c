// occ_tile_walk.h -- the tile walk the occupancy kernels share (occ_loss_kernels.h, occ_lovasz_kernels.h): 256 threads, tiles of
// T x T columns x TD depth cells, 256 voxels per step; channels-last rows go through LDS in contiguous runs.
#pragma once
#include "rt.h"

#define FBBEV_OCCL_THREADS 256

__device__ __forceinline__ int occl_min(int a, int b) { return a < b ? a : b; }
__device__ __forceinline__ int occl_max(int a, int b) { return a > b ? a : b; }
__device__ __forceinline__ bool occl_finite(float x) { return fabsf(x) < __builtin_inff(); }      // false for NaN

struct occl_tile {
    int b, h0, w0, d0, THe, TWe, TDe, nvox;
    long long base;
};
__device__ __forceinline__ occl_tile occl_tile_of(int tile, int T, int TD, int nth, int ntw, int ntd, int H, int W, int D, long long sb,
                                                  long long sh, long long sw, long long sd) {
    occl_tile q;
    unsigned int r = (unsigned int)tile;
    const int id = (int)(r % (unsigned int)ntd); r /= (unsigned int)ntd;
    const int iw = (int)(r % (unsigned int)ntw); r /= (unsigned int)ntw;
    const int ih = (int)(r % (unsigned int)nth);
    q.b = (int)(r / (unsigned int)nth);
    q.h0 = ih * T; q.w0 = iw * T; q.d0 = id * TD;
    q.THe = occl_min(T, H - q.h0); q.TWe = occl_min(T, W - q.w0); q.TDe = occl_min(TD, D - q.d0);
    q.nvox = q.THe * q.TWe * q.TDe;
    q.base = (long long)q.b * sb + (long long)q.h0 * sh + (long long)q.w0 * sw + (long long)q.d0 * sd;
    return q;
}

// channels-last: the voxels [v0, v1) of the tile as contiguous runs of floats (a row, fixed h, or a column, fixed h and w, of the tile),
// copied between global memory and the LDS rows; TO_LDS: global -> LDS, else LDS -> global
template <bool TO_LDS>
__device__ __forceinline__ void occl_copy_runs(float* g, float* stage, const occl_tile& q, int v0, int v1, int C, int row_runs,
                                               long long sh, long long sw, int t) {
    const int rv = row_runs ? q.TWe * q.TDe : q.TDe;
    for (int run = v0 / rv; run * rv < v1; ++run) {
        const int lo = occl_max(v0, run * rv), hi = occl_min(v1, (run + 1) * rv);
        const int th = row_runs ? run : run / q.TWe, tw = row_runs ? 0 : run % q.TWe;
        float* src = g + q.base + (long long)th * sh + (long long)tw * sw + (long long)(lo - run * rv) * C;
        float* dst = stage + (lo - v0) * C;
        const int len = (hi - lo) * C;
        if (TO_LDS) {
            for (int f = t; f < len; f += 4 * FBBEV_OCCL_THREADS) {          // four loads requested before the first LDS store
                const int f1 = f + FBBEV_OCCL_THREADS, f2 = f1 + FBBEV_OCCL_THREADS, f3 = f2 + FBBEV_OCCL_THREADS;
                const float x0 = src[f];
                const float x1 = f1 < len ? src[f1] : 0.f, x2 = f2 < len ? src[f2] : 0.f, x3 = f3 < len ? src[f3] : 0.f;
                dst[f] = x0;
                if (f1 < len) dst[f1] = x1;
                if (f2 < len) dst[f2] = x2;
                if (f3 < len) dst[f3] = x3;
            }
        } else {
            for (int f = t; f < len; f += FBBEV_OCCL_THREADS) src[f] = dst[f];
        }
    }
}
