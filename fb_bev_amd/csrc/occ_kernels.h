// occ_kernels.h -- occupancy class map and mIoU confusion matrix in one pass over the head's logits.
// Replaces the inference tail of the reference (fbocc.py:539-554: fix_void slice, softmax, argmax, permute / flip / rot90 / permute)
// and the scoring of a frame (occ_metrics.py:80-105 hist_info / compute_mIoU bincount, :122-164 add_batch masks and the range ring).
//
// Softmax is monotone, so the class is taken from the logits: the lowest index among the maxima of logits[c0:], and 0 when any of
// them is NaN or +inf (the softmax row is then all NaN and its argmax is 0).  The reference's axis shuffle is an H <-> W transpose:
// classes[b, w, h, d] = class(logits[b, :, h, w, d]).
//
// A workgroup of 256 threads owns a tile of TH x TW columns x TD depth cells (<= 4096 voxels) and walks tiles with a grid stride.
//   pass 1, input order (h, w, d), 256 voxels per step: a voxel's class goes into the LDS tile as a byte at [w][h][d].
//           Channels-last logits (a voxel's C floats contiguous) are staged through LDS in contiguous runs, one dword per lane, and a
//           lane then reads its voxel's row at a stride of C words; every other stride pattern is read straight from global memory,
//           which is coalesced for class planes (lanes walk d, then w).
//   pass 2, output order (w, h, d): the tile leaves as runs of TH * D contiguous bytes per w, four bytes per lane where D % 4 == 0 and
//           the pointers are 4-byte aligned.  Labels and masks live in the output order, so scoring happens here: key = gt * n + pred
//           for a counted voxel.  A wave first aggregates: ballot per distinct key and ONE LDS add of the population count while a key
//           still covers 8 lanes or more (real frames: almost every visible voxel is (free, free)); the remaining lanes add 1 each.
// The workgroup's private n x n table is added to `hist` at the end, non-zero bins only.  Integer adds only: exact and run-to-run stable.
#pragma once
#include "rt.h"

#define FBBEV_OCC_THREADS 256
#define FBBEV_OCC_TILE_VOXELS 4096

__device__ __forceinline__ int occ_min(int a, int b) { return a < b ? a : b; }
__device__ __forceinline__ int occ_max(int a, int b) { return a > b ? a : b; }

// one add per distinct key of the wave while keys are popular, then one add per remaining lane; every lane of the wave calls it
__device__ __forceinline__ void occ_hist_add(int* table, int key, int lane) {
    unsigned long long todo = __ballot(key >= 0);
    while (todo) {
        const int leader = __ffsll((long long)todo) - 1;
        const int k = __shfl(key, leader, 64);
        const unsigned long long same = __ballot(key == k);
        const int cnt = __popcll(same);
        if (cnt < 8) {
            if ((todo >> lane) & 1ull) atomicAdd(&table[key], 1);
            break;
        }
        if (lane == leader) atomicAdd(&table[k], cnt);
        todo &= ~same;
    }
}

// lowest index among the maxima of x[0..n), 0 when one of them is NaN or +inf.  `ld(j)` returns element j.
template <class Load>
__device__ __forceinline__ int occ_argmax(int n, Load ld) {
    const float inf = __builtin_inff();
    float best = ld(0);
    int idx = 0;
    bool bad = !(best < inf);
    int j = 1;
    for (; j + 4 <= n; j += 4) {                 // four independent loads in flight
        const float a = ld(j), b = ld(j + 1), c = ld(j + 2), d = ld(j + 3);
        bad = bad || !(a < inf) || !(b < inf) || !(c < inf) || !(d < inf);
        if (a > best) { best = a; idx = j; }
        if (b > best) { best = b; idx = j + 1; }
        if (c > best) { best = c; idx = j + 2; }
        if (d > best) { best = d; idx = j + 3; }
    }
    for (; j < n; ++j) {
        const float a = ld(j);
        bad = bad || !(a < inf);
        if (a > best) { best = a; idx = j; }
    }
    return bad ? 0 : idx;
}

// STAGED: channels-last (sc == 1, sd == C), through LDS; VEC4: pass 2 moves four bytes per lane
template <bool STAGED, bool VEC4>
__global__ void __launch_bounds__(FBBEV_OCC_THREADS)
k_occ_classes(const float* __restrict__ logits, long long sb, long long sc, long long sh, long long sw, long long sd,
              int C, int c0, int H, int W, int D,
              int T, int TD,                          // tile: T x T columns x TD depth cells, <= FBBEV_OCC_TILE_VOXELS voxels
              int nth, int ntw, int ntd, int ntiles,  // tiles along h, w, d; all of them (batch included)
              int row_runs,                           // STAGED: 1 when a tile row (fixed h) is one contiguous run (TD == D, sw == D * C)
              unsigned char* __restrict__ classes, const unsigned char* __restrict__ gt, const unsigned char* __restrict__ mask,
              const unsigned char* __restrict__ column_mask, int* __restrict__ hist) {
    const int n = C - c0;
    float* stage = fbbev_dyn_lds_f32();                                             // staged: 256 voxels x C floats
    int* table = reinterpret_cast<int*>(stage + (STAGED ? FBBEV_OCC_THREADS * C : 0));   // n x n
    unsigned char* cls = reinterpret_cast<unsigned char*>(table + n * n);           // the tile's classes, [w][h][d]
    const int t = threadIdx.x, lane = t & 63;
    const bool score = hist != nullptr;
    if (score) {
        for (int i = t; i < n * n; i += FBBEV_OCC_THREADS) table[i] = 0;
    }
    __syncthreads();

    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        unsigned int r = (unsigned int)tile;
        const int id = (int)(r % (unsigned int)ntd); r /= (unsigned int)ntd;
        const int iw = (int)(r % (unsigned int)ntw); r /= (unsigned int)ntw;
        const int ih = (int)(r % (unsigned int)nth);
        const int b = (int)(r / (unsigned int)nth);
        const int h0 = ih * T, w0 = iw * T, d0 = id * TD;
        const int THe = occ_min(T, H - h0), TWe = occ_min(T, W - w0), TDe = occ_min(TD, D - d0);
        const int nvox = THe * TWe * TDe;
        const long long base = (long long)b * sb + (long long)h0 * sh + (long long)w0 * sw + (long long)d0 * sd;

        // ---- pass 1: classes of the tile, 256 voxels (input order: h, w, d) per step
        for (int v0 = 0; v0 < nvox; v0 += FBBEV_OCC_THREADS) {
            const int v1 = occ_min(v0 + FBBEV_OCC_THREADS, nvox);
            if (STAGED) {
                // the voxels [v0, v1) as contiguous runs of floats: a row (fixed h) or a column (fixed h, w) of the tile
                const int rv = row_runs ? TWe * TDe : TDe;
                for (int run = v0 / rv; run * rv < v1; ++run) {
                    const int lo = occ_max(v0, run * rv), hi = occ_min(v1, (run + 1) * rv);
                    const int th = row_runs ? run : run / TWe, tw = row_runs ? 0 : run % TWe;
                    const float* src = logits + base + (long long)th * sh + (long long)tw * sw + (long long)(lo - run * rv) * C;
                    float* dst = stage + (lo - v0) * C;
                    const int len = (hi - lo) * C;
                    for (int f = t; f < len; f += 4 * FBBEV_OCC_THREADS) {          // four loads requested before the first LDS store
                        const int f1 = f + FBBEV_OCC_THREADS, f2 = f1 + FBBEV_OCC_THREADS, f3 = f2 + FBBEV_OCC_THREADS;
                        const float x0 = src[f];
                        const float x1 = f1 < len ? src[f1] : 0.f, x2 = f2 < len ? src[f2] : 0.f, x3 = f3 < len ? src[f3] : 0.f;
                        dst[f] = x0;
                        if (f1 < len) dst[f1] = x1;
                        if (f2 < len) dst[f2] = x2;
                        if (f3 < len) dst[f3] = x3;
                    }
                }
                __syncthreads();
            }
            const int v = v0 + t;
            if (v < v1) {
                const int th = v / (TWe * TDe), rr = v - th * (TWe * TDe);
                const int tw = rr / TDe, td = rr - tw * TDe;
                int c;
                if (STAGED) {
                    const float* row = stage + t * C + c0;
                    c = occ_argmax(n, [&](int j) { return row[j]; });
                } else {
                    const float* p = logits + base + (long long)th * sh + (long long)tw * sw + (long long)td * sd + (long long)c0 * sc;
                    c = occ_argmax(n, [&](int j) { return p[(long long)j * sc]; });
                }
                cls[(tw * THe + th) * TDe + td] = (unsigned char)c;
            }
            if (STAGED) __syncthreads();
        }
        __syncthreads();

        // ---- pass 2: the tile in output order (w, h, d); scoring
        constexpr int step = VEC4 ? 4 : 1;
        const int colbytes = THe * TDe;
        for (int q0 = 0; q0 < nvox; q0 += FBBEV_OCC_THREADS * step) {
            const int q = q0 + t * step;
            const bool live = q < nvox;
            int tw = 0, th = 0, td = 0;
            long long o = 0;
            unsigned int pred4 = 0, gt4 = 0xffffffffu, m4 = 0;
            if (live) {
                tw = q / colbytes;
                const int rr = q - tw * colbytes;
                th = rr / TDe;
                td = rr - th * TDe;
                o = (((long long)b * W + (w0 + tw)) * H + (h0 + th)) * D + (d0 + td);
                if (VEC4) {
                    pred4 = *reinterpret_cast<const unsigned int*>(cls + q);
                    *reinterpret_cast<unsigned int*>(classes + o) = pred4;
                } else {
                    pred4 = cls[q];
                    classes[o] = (unsigned char)pred4;
                }
                if (score) {
                    const bool col = column_mask ? column_mask[(long long)(w0 + tw) * H + (h0 + th)] != 0 : true;
                    if (col) {
                        if (VEC4) {
                            gt4 = *reinterpret_cast<const unsigned int*>(gt + o);
                            m4 = mask ? *reinterpret_cast<const unsigned int*>(mask + o) : 0x01010101u;
                        } else {
                            gt4 = 0xffffff00u | gt[o];
                            m4 = mask ? mask[o] : 1u;
                        }
                    }
                }
            }
            if (score) {
                for (int e = 0; e < step; ++e) {
                    const int g = (int)((gt4 >> (8 * e)) & 0xffu), p = (int)((pred4 >> (8 * e)) & 0xffu);
                    const bool counted = g < n && ((m4 >> (8 * e)) & 0xffu) != 0;
                    occ_hist_add(table, counted ? g * n + p : -1, lane);
                }
            }
        }
        __syncthreads();
    }

    if (score) {
        for (int i = t; i < n * n; i += FBBEV_OCC_THREADS) {
            const int cnt = table[i];
            if (cnt) atomicAdd(&hist[i], cnt);
        }
    }
}
