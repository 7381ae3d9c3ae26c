// depth_loss_kernels.h -- the depth supervision loss of CM_DepthNet from one pass each way.
// Replaces get_downsampled_gt_depth + get_depth_loss (depth_net.py:396-450 of the reference): the view / permute copy of gt, the
// == 0 / full_like / where passes, the min, the int64 one-hot, the permuted copy of the depth distribution, binary_cross_entropy
// over every element, the mask multiply and the two reductions -- and autograd's mirror of all that.
//   gt (BN, H, W) f32, probs (BN, D, h, w) f32, h = H / ds, w = W / ds, both contiguous.  Per cell of ds x ds pixels:
//     m      = min over the cell of (x == 0 ? 1e5 : x)          NaN wins, as in torch.min
//     bins   = (m - bin0) / step                                one IEEE subtraction, one IEEE division
//     label  = 0 <= bins < D + 1 ? (int)bins - 1 : -1           -1 = background (bin 0 included)
//     cell   = sum_d -max(d == label ? logf(p_d) : log1pf(-p_d), -100)      foreground cells only
// k_depth_loss_fwd: one workgroup per (image, cell row); the ds image rows of a cell row are contiguous in memory.  The cell row is
// walked in chunks of `cc` cells (cc * ds <= FBBEV_DL_COLS columns):
//   a. a thread owns columns (four adjacent ones with 16-byte loads) and takes their minimum down the ds rows: consecutive lanes
//      read consecutive addresses, the ds loads of a thread are independent;
//   b. the column minima go through LDS, a thread per cell takes the minimum of its ds columns, bins it, stores the label to
//      global memory and to LDS;
//   c. the D rows of cc probabilities of the chunk are read with consecutive lanes on consecutive cells, four independent loads
//      per thread and step (a wave per depth row with one dependent load per row measured 59 us per call at the shipped shape,
//      profiles/r21_depth_loss.md has the present figure); a thread adds the terms of its elements in a register.
// The workgroup's sum (a fixed tree over the 256 threads) and its foreground count go to the workspace as record blockIdx.x;
// k_depth_loss_reduce (one workgroup) adds the records in a fixed order, floats in double, and rounds once.  No atomics: the
// bits depend on the shape and the inputs alone.  The grid is NOT capped: BN * h workgroups (< 2^31 is checked by the launcher).
// k_depth_loss_grad: a thread per element of grad_probs, torch's binary_cross_entropy backward; every element is written.
#pragma once
#include "rt.h"

#define FBBEV_DL_THREADS 256
#define FBBEV_DL_COLS 4096                                       // columns of a chunk: 16 KiB of column minima in LDS
#define FBBEV_DL_MAX_D 4096                                      // keeps D * cc below 2^31 and a thread's fp32 chain short

// min(m, x) in which a NaN wins and stays (torch.min): once m is NaN both comparisons are false for every later x
__device__ __forceinline__ float dl_min(float m, float x) { return (x < m || x != x) ? x : m; }
__device__ __forceinline__ float dl_mask(float x) { return x == 0.0f ? 1e5f : x; }      // -0.0 == 0.0: masked as well

template <bool V4>
__global__ void __launch_bounds__(FBBEV_DL_THREADS)
k_depth_loss_fwd(const float* __restrict__ gt, int H, int W, int ds, int h, int w, int cc, const float* __restrict__ probs, int D,
                 float bin0, float step, int* __restrict__ labels, float* __restrict__ part_f, int* __restrict__ part_i) {
    float* colmin = fbbev_dyn_lds_f32();                                   // FBBEV_DL_COLS column minima of the chunk
    int* lab = reinterpret_cast<int*>(colmin + FBBEV_DL_COLS);             // FBBEV_DL_COLS labels of the chunk (cc <= FBBEV_DL_COLS)
    float* red = colmin + 2 * FBBEV_DL_COLS;                               // 256 words: the reductions at the end
    const int t = threadIdx.x;
    const int n = blockIdx.x / h, r = blockIdx.x - n * h;
    const float* rows = gt + ((long long)n * H + (long long)r * ds) * W;   // ds rows of W floats
    const float dmax = (float)(D + 1);
    float acc = 0.f;
    int cnt = 0;

    for (int c0 = 0; c0 < w; c0 += cc) {
        const int nc = w - c0 < cc ? w - c0 : cc;                          // cells of this chunk
        const int col0 = c0 * ds, ncol = nc * ds;                          // its columns
        // ---- a. column minima
        if (V4) {                                                          // W % 4 == 0, col0 % 4 == 0, gt 16-byte aligned => ncol % 4 == 0
            for (int q = t; q < ncol / 4; q += FBBEV_DL_THREADS) {
                const float* p = rows + col0 + 4 * q;
                float m0 = __builtin_inff(), m1 = m0, m2 = m0, m3 = m0;
#pragma unroll 4
                for (int y = 0; y < ds; ++y) {
                    const fbbev_v4f v = fbbev_gld_v4f(p + (long long)y * W);
                    m0 = dl_min(m0, dl_mask(v[0]));
                    m1 = dl_min(m1, dl_mask(v[1]));
                    m2 = dl_min(m2, dl_mask(v[2]));
                    m3 = dl_min(m3, dl_mask(v[3]));
                }
                colmin[4 * q] = m0; colmin[4 * q + 1] = m1; colmin[4 * q + 2] = m2; colmin[4 * q + 3] = m3;
            }
        } else {
            for (int c = t; c < ncol; c += FBBEV_DL_THREADS) {
                const float* p = rows + col0 + c;
                float m = __builtin_inff();
#pragma unroll 4
                for (int y = 0; y < ds; ++y) m = dl_min(m, dl_mask(p[(long long)y * W]));
                colmin[c] = m;
            }
        }
        __syncthreads();
        // ---- b. the chunk's labels
        for (int j = t; j < nc; j += FBBEV_DL_THREADS) {
            float m = colmin[j * ds];
            for (int x = 1; x < ds; ++x) m = dl_min(m, colmin[j * ds + x]);
            const float bins = fbbev_div(fbbev_sub(m, bin0), step);
            int label = -1;
            if (bins >= 0.0f && bins < dmax) label = (int)bins - 1;        // NaN fails both comparisons
            lab[j] = label;
            labels[((long long)n * h + r) * w + c0 + j] = label;
            cnt += label >= 0 ? 1 : 0;
        }
        __syncthreads();
        // ---- c. the terms of the chunk's foreground cells
        if (probs) {
            const float* prow = probs + (((long long)n * D) * h + r) * w + c0;      // + d * h * w + j
            const long long plane = (long long)h * w;
            const int items = D * nc;                                      // element i = d * nc + j; below 2^24
            // four elements per thread and step: the loads are unconditional (a tail index is clamped, a background cell's value is
            // dropped), so that all four are in flight before the first logarithm
            for (int i0 = t; i0 < items; i0 += 4 * FBBEV_DL_THREADS) {
                float p[4];
                int lb[4], dd[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int i = i0 + u * FBBEV_DL_THREADS;
                    const int ic = i < items ? i : items - 1;
                    const int d = ic / nc, j = ic - d * nc;
                    p[u] = prow[d * plane + j];
                    lb[u] = i < items ? lab[j] : -1;
                    dd[u] = d;
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    if (lb[u] >= 0) {
                        const float l = dd[u] == lb[u] ? logf(p[u]) : log1pf(-p[u]);
                        acc += -(l < -100.f ? -100.f : l);                 // the clamp lets a NaN through
                    }
                }
            }
        }
        __syncthreads();                                                   // lab and colmin are rewritten by the next chunk
    }

    // ---- the workgroup's record: a fixed tree over the threads
    red[t] = acc;
    __syncthreads();
    for (int s = FBBEV_DL_THREADS / 2; s > 0; s >>= 1) {
        if (t < s) red[t] += red[t + s];
        __syncthreads();
    }
    if (t == 0) part_f[blockIdx.x] = red[0];
    __syncthreads();
    int* redi = reinterpret_cast<int*>(red);
    redi[t] = cnt;
    __syncthreads();
    for (int s = FBBEV_DL_THREADS / 2; s > 0; s >>= 1) {
        if (t < s) redi[t] += redi[t + s];
        __syncthreads();
    }
    if (t == 0) part_i[blockIdx.x] = redi[0];
}

// one workgroup: thread t adds records t, t + 256, ... in ascending order (floats in double), the 256 thread sums go through a fixed
// tree (still in double) and the total is rounded once.  out_f = {bce_sum, bce_sum / max(count, 1)}, out_i = {count}.
__global__ void __launch_bounds__(FBBEV_DL_THREADS)
k_depth_loss_reduce(const float* __restrict__ part_f, const int* __restrict__ part_i, int nrec, float* __restrict__ out_f,
                    int* __restrict__ out_i) {
    double* sums = reinterpret_cast<double*>(fbbev_dyn_lds_f32());         // 256 doubles, then 256 ints
    int* cnts = reinterpret_cast<int*>(sums + FBBEV_DL_THREADS);
    const int t = threadIdx.x;
    double s = 0.0;
    int c = 0;
    for (int i = t; i < nrec; i += FBBEV_DL_THREADS) {
        s += (double)part_f[i];
        c += part_i[i];
    }
    sums[t] = s;
    cnts[t] = c;
    __syncthreads();
    for (int k = FBBEV_DL_THREADS / 2; k > 0; k >>= 1) {
        if (t < k) { sums[t] += sums[t + k]; cnts[t] += cnts[t + k]; }
        __syncthreads();
    }
    if (t == 0) {
        const double S = sums[0];
        const int C = cnts[0];
        const float total = (float)S;
        out_f[0] = total;
        out_f[1] = fbbev_div(total, (float)(C > 1 ? C : 1));
        out_i[0] = C;
    }
}

// grad_probs (BN, D, h, w), a thread per element: torch's binary_cross_entropy backward times the mean's 1 / max(count, 1),
//   grad_loss / max(count, 1) * (p - [d == label]) / max((1 - p) p, 1e-12f)
// for a foreground cell, an exact 0 for a background cell.  count and grad_loss are read from device memory.
__global__ void __launch_bounds__(FBBEV_DL_THREADS)
k_depth_loss_grad(const float* __restrict__ probs, const int* __restrict__ labels, const int* __restrict__ out_i,
                  const float* __restrict__ grad_loss, unsigned int D, unsigned int hw, unsigned int total,
                  float* __restrict__ grad_probs) {
    const unsigned int i = blockIdx.x * (unsigned int)FBBEV_DL_THREADS + threadIdx.x;       // total < 2^31: no overflow
    if (i >= total) return;
    const unsigned int plane = i / hw, cell = i - plane * hw;              // plane = n * D + d
    const unsigned int n = plane / D, d = plane - n * D;
    const int label = labels[n * hw + cell];
    float g = 0.f;
    if (label >= 0) {
        const int count = out_i[0];
        const float scale = grad_loss[0] / (float)(count > 1 ? count : 1);
        const float p = probs[i];
        const float tgt = (int)d == label ? 1.f : 0.f;
        const float den = (1.f - p) * p;
        g = scale * (p - tgt) / (den > 1e-12f ? den : 1e-12f);
    }
    grad_probs[i] = g;
}
