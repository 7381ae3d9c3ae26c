// occ_loss_kernels.h -- the voxel losses of the occupancy head from one pass over the logits, forward and backward.
// Replaces the full-size passes of CustomFocalLoss / CE_ssc_loss (focal_loss.py:13-54,191-286, semkitti.py:167-182), sem_scal_loss
// (semkitti.py:111-164) and geo_scal_loss (semkitti.py:78-107): each of them is a function of a handful of sums over the voxels of
// per-voxel functions of one softmax row and one label.  With x = nan_to_num(logits, 0, 0, 0), p = softmax(x), t the label,
// m = (t != 255), e = empty_idx:
//   P[c] = sum m p[c]    N[c] = sum m [t == c] p[c]    Q[c] = sum m [t != c] (1 - p[c])    G = sum m (1 - p[e])
//   CLS  = sum m w[t] (-log p[t])                                      (cross entropy)
//   CLS  = sum m r[h, w] sum_c w[c] f(x[c], [t == c])                  (focal: f = the sigmoid focal term)
//   cnt[c] = sum m [t == c]    n_valid = sum m
// Labels are 0..C-1 or 255; what a label in C..254 yields is unspecified (no access leaves its bounds: such a voxel is counted in
// n_valid, P, Q and G, matches no class and adds nothing to a cross-entropy CLS).
// k_occ_loss_stats leaves one record of these per workgroup, k_occ_loss_reduce adds the records in ascending workgroup order (floats in
// double, rounded once), k_occ_loss_grad turns the gradient with respect to the sums into the gradient with respect to the logits.
// No atomics anywhere: the bits depend on the shape alone.
//
// The walk is k_occ_classes': 256 threads, tiles of T x T columns x TD depth cells, a grid stride over the tiles, 256 voxels per step.
//   step, part A (a thread per voxel): the voxel's row of C logits lies in LDS (channels-last rows are staged there in contiguous
//       runs; every other stride pattern is read from global memory, coalesced for class planes); the thread cleans it, takes the CLS
//       term, and overwrites it with the softmax row p.  A thread's row starts at word t * C: no bank conflicts for an odd C (the
//       shipped 19), 2-way at C = 18 and up to 32-way at C = 32 -- correct, not fast.
//   step, part B (a thread per class and voxel subset): thread j owns class j % C and the voxels j / C, j / C + 256 / C, ... of the
//       step and adds p[c] into P / N / Q / G / cnt held in REGISTERS: no accumulator is indexed by a label, so nothing goes to scratch
//       and nothing needs an atomic.  Lanes read consecutive LDS words.
// At the end the 256 / C partial sums of a class are added in ascending order, CLS goes through a fixed tree.
#pragma once
#include "rt.h"
#include "occ_tile_walk.h"

#define FBBEV_OCCL_MAX_BLOCKS 1024

__device__ __forceinline__ float occl_softplus(float x) { return fmaxf(x, 0.f) + log1pf(expf(-fabsf(x))); }
__device__ __forceinline__ float occl_pow(float b, float g) { return g == 2.f ? b * b : powf(b, g); }
// sigmoid focal term of CustomFocalLoss.forward for one logit: y ? alpha (1-s)^gamma softplus(-x) : (1-alpha) s^gamma softplus(x)
__device__ __forceinline__ float occl_focal(float x, bool y, float gamma, float alpha) {
    const float s = 1.f / (1.f + expf(-x));
    return y ? alpha * occl_pow(1.f - s, gamma) * occl_softplus(-x) : (1.f - alpha) * occl_pow(s, gamma) * occl_softplus(x);
}
// its derivative in x
__device__ __forceinline__ float occl_focal_dx(float x, bool y, float gamma, float alpha) {
    const float s = 1.f / (1.f + expf(-x));
    return y ? -alpha * occl_pow(1.f - s, gamma) * (gamma * s * occl_softplus(-x) + (1.f - s))
             : (1.f - alpha) * occl_pow(s, gamma) * (gamma * (1.f - s) * occl_softplus(x) + s);
}

// record of a workgroup in the workspace: floats [block][3C + 4] = P, N, Q, G, CLS, 0, 0; then ints [block][C + 1] = cnt, n_valid
template <bool STAGED>
__global__ void __launch_bounds__(FBBEV_OCCL_THREADS)
k_occ_loss_stats(const float* __restrict__ logits, long long sb, long long sc, long long sh, long long sw, long long sd,
                 int C, int H, int W, int D, int T, int TD, int nth, int ntw, int ntd, int ntiles, int row_runs,
                 const unsigned char* __restrict__ labels, const float* __restrict__ class_weight, const float* __restrict__ plane_weight,
                 int empty_idx, int focal, float gamma, float alpha, float* __restrict__ part_f, int* __restrict__ part_i) {
    float* stage = fbbev_dyn_lds_f32();                                    // 256 rows of C floats: x, then p
    float* red = stage + FBBEV_OCCL_THREADS * C;                           // 256 floats: the reductions at the end
    float* wts = red + FBBEV_OCCL_THREADS;                                 // C class weights
    int* lab = reinterpret_cast<int*>(wts + C);                            // 256 labels of the step, 255 = not counted
    const int t = threadIdx.x;
    const int parts = FBBEV_OCCL_THREADS / C;                              // voxel subsets per class in part B
    const int myc = t % C, mypart = t / C;
    const bool classed = mypart < parts;
    for (int i = t; i < C; i += FBBEV_OCCL_THREADS) wts[i] = class_weight ? class_weight[i] : 1.f;
    float aP = 0.f, aN = 0.f, aQ = 0.f, aG = 0.f, aCLS = 0.f;
    int aCnt = 0, aValid = 0;
    __syncthreads();

    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        int tile_v = tile;                                                 // the tile's fields live in vector registers: with ~30 kernel
        fbbev_opaque(tile_v);                                              // arguments the scalar file would overflow
        const occl_tile q = occl_tile_of(tile_v, T, TD, nth, ntw, ntd, H, W, D, sb, sh, sw, sd);
        for (int v0 = 0; v0 < q.nvox; v0 += FBBEV_OCCL_THREADS) {
            const int v1 = occl_min(v0 + FBBEV_OCCL_THREADS, q.nvox);
            if (STAGED) {
                occl_copy_runs<true>(const_cast<float*>(logits), stage, q, v0, v1, C, row_runs, sh, sw, t);
                __syncthreads();
            }
            // ---- part A: this thread's voxel
            const int v = v0 + t;
            int label = 255;
            float* row = stage + t * C;
            if (v < v1) {
                const int th = v / (q.TWe * q.TDe), rr = v - th * (q.TWe * q.TDe);
                const int tw = rr / q.TDe, td = rr - tw * q.TDe;
                label = labels[(((long long)q.b * H + (q.h0 + th)) * W + (q.w0 + tw)) * D + (q.d0 + td)];
                if (label != 255) {
                    const float* px = logits + q.base + (long long)th * sh + (long long)tw * sw + (long long)td * sd;
                    float mx = -__builtin_inff(), fsum = 0.f;
                    for (int c = 0; c < C; ++c) {
                        float x = STAGED ? row[c] : px[(long long)c * sc];
                        x = occl_finite(x) ? x : 0.f;
                        row[c] = x;
                        mx = fmaxf(mx, x);
                        if (focal) fsum += wts[c] * occl_focal(x, c == label, gamma, alpha);
                    }
                    const float xt = label < C ? row[label] : 0.f;
                    float sum = 0.f;
                    for (int c = 0; c < C; ++c) {
                        const float ex = expf(row[c] - mx);
                        row[c] = ex;
                        sum += ex;
                    }
                    const float inv = 1.f / sum;
                    for (int c = 0; c < C; ++c) row[c] *= inv;
                    if (focal) aCLS += plane_weight[(long long)(q.h0 + th) * W + (q.w0 + tw)] * fsum;
                    else if (label < C) aCLS += wts[label] * ((mx + logf(sum)) - xt);
                }
            }
            lab[t] = label;
            __syncthreads();
            // ---- part B: this thread's class over its voxels of the step
            if (classed) {
                for (int u = mypart; u < v1 - v0; u += parts) {
                    const int l = lab[u];
                    if (l == 255) continue;
                    const float p = stage[u * C + myc], np = 1.f - p;
                    aP += p;
                    if (l == myc) { aN += p; ++aCnt; } else aQ += np;
                    if (myc == empty_idx) aG += np;
                    ++aValid;
                }
            }
            __syncthreads();
        }
    }

    // ---- the workgroup's record: the partial sums of a class in ascending order of the voxel subset
    float* rec_f = part_f + (long long)blockIdx.x * (3 * C + 4);
    int* rec_i = part_i + (long long)blockIdx.x * (C + 1);
    for (int k = 0; k < 4; ++k) {
        red[t] = k == 0 ? aP : (k == 1 ? aN : (k == 2 ? aQ : aG));
        __syncthreads();
        if (t < C && (k < 3 || t == empty_idx)) {
            float s = 0.f;
            for (int j = 0; j < parts; ++j) s += red[j * C + t];
            rec_f[k < 3 ? k * C + t : 3 * C] = s;
        }
        __syncthreads();
    }
    int* redi = reinterpret_cast<int*>(red);
    redi[t] = aCnt;
    __syncthreads();
    if (t < C) {
        int s = 0;
        for (int j = 0; j < parts; ++j) s += redi[j * C + t];
        rec_i[t] = s;
    }
    __syncthreads();
    redi[t] = aValid;
    __syncthreads();
    if (t == 0) {
        int s = 0;
        for (int j = 0; j < parts; ++j) s += redi[j * C];
        rec_i[C] = s;
    }
    __syncthreads();
    red[t] = aCLS;
    __syncthreads();
    for (int s = FBBEV_OCCL_THREADS / 2; s > 0; s >>= 1) {
        if (t < s) red[t] += red[t + s];
        __syncthreads();
    }
    if (t == 0) {
        rec_f[3 * C + 1] = red[0];
        rec_f[3 * C + 2] = 0.f;
        rec_f[3 * C + 3] = 0.f;
    }
}

// one workgroup: the records in ascending workgroup order; floats in double and rounded once, ints in int32.  A statistic is one
// thread's chain of additions; the records come through LDS in chunks of FBBEV_OCCL_REDUCE_CHUNK, copied by the whole workgroup with
// four loads in flight per thread (a thread that read its 1024 records from global memory one after the other took longer than the
// pass over the logits).
#define FBBEV_OCCL_REDUCE_CHUNK 64
__device__ __forceinline__ void occl_copy_words(const int* __restrict__ src, int* dst, int len, int t) {
    for (int f = t; f < len; f += 4 * FBBEV_OCCL_THREADS) {
        const int f1 = f + FBBEV_OCCL_THREADS, f2 = f1 + FBBEV_OCCL_THREADS, f3 = f2 + FBBEV_OCCL_THREADS;
        const int x0 = src[f];
        const int x1 = f1 < len ? src[f1] : 0, x2 = f2 < len ? src[f2] : 0, x3 = f3 < len ? src[f3] : 0;
        dst[f] = x0;
        if (f1 < len) dst[f1] = x1;
        if (f2 < len) dst[f2] = x2;
        if (f3 < len) dst[f3] = x3;
    }
}
__global__ void __launch_bounds__(FBBEV_OCCL_THREADS)
k_occ_loss_reduce(const float* __restrict__ part_f, const int* __restrict__ part_i, int nblocks, int C, float* __restrict__ stats_f,
                  int* __restrict__ stats_i) {
    const int nf = 3 * C + 4, ni = C + 1, t = threadIdx.x;                 // nf + ni <= 133 threads hold a statistic each
    float* buf_f = fbbev_dyn_lds_f32();                                    // CHUNK records of floats, then CHUNK records of ints
    int* buf_i = reinterpret_cast<int*>(buf_f + FBBEV_OCCL_REDUCE_CHUNK * nf);
    double sf = 0.0;
    int si = 0;
    for (int b0 = 0; b0 < nblocks; b0 += FBBEV_OCCL_REDUCE_CHUNK) {
        const int nb = occl_min(FBBEV_OCCL_REDUCE_CHUNK, nblocks - b0);
        occl_copy_words(reinterpret_cast<const int*>(part_f) + (long long)b0 * nf, reinterpret_cast<int*>(buf_f), nb * nf, t);
        occl_copy_words(part_i + (long long)b0 * ni, buf_i, nb * ni, t);
        __syncthreads();
        if (t < nf) {
            for (int j = 0; j < nb; ++j) sf += (double)buf_f[j * nf + t];
        } else if (t < nf + ni) {
            for (int j = 0; j < nb; ++j) si += buf_i[j * ni + (t - nf)];
        }
        __syncthreads();
    }
    if (t < nf) stats_f[t] = (float)sf;
    else if (t < nf + ni) stats_i[t - nf] = si;
}

// grad_logits (the logits' strides) from grad_stats (3C + 4 floats in device memory, laid out as stats_f): with
//   g_c = m (gP[c] + [t == c] gN[c] - [t != c] gQ[c]) - [c == e] m gG
//   grad x[j] = p[j] (g_j - sum_c g_c p[c]) + the CLS term;  0 where the input was not finite, 0 for a voxel that is not counted
template <bool STAGED>
__global__ void __launch_bounds__(FBBEV_OCCL_THREADS)
k_occ_loss_grad(const float* __restrict__ logits, long long sb, long long sc, long long sh, long long sw, long long sd,
                int C, int H, int W, int D, int T, int TD, int nth, int ntw, int ntd, int ntiles, int row_runs,
                const unsigned char* __restrict__ labels, const float* __restrict__ class_weight, const float* __restrict__ plane_weight,
                int empty_idx, int focal, float gamma, float alpha, const float* __restrict__ grad_stats, float* __restrict__ grad_logits) {
    float* stage = fbbev_dyn_lds_f32();                                    // 256 rows of C floats: x, then grad x
    float* wts = stage + FBBEV_OCCL_THREADS * C;                           // C class weights
    float* gs = wts + C;                                                   // 3C + 4: gP, gN, gQ, gG, gCLS
    const int t = threadIdx.x;
    for (int i = t; i < C; i += FBBEV_OCCL_THREADS) wts[i] = class_weight ? class_weight[i] : 1.f;
    for (int i = t; i < 3 * C + 4; i += FBBEV_OCCL_THREADS) gs[i] = grad_stats[i];
    __syncthreads();
    const float gG = gs[3 * C], gCLS = gs[3 * C + 1];

    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        int tile_v = tile;                                                 // the tile's fields live in vector registers: with ~30 kernel
        fbbev_opaque(tile_v);                                              // arguments the scalar file would overflow
        const occl_tile q = occl_tile_of(tile_v, T, TD, nth, ntw, ntd, H, W, D, sb, sh, sw, sd);
        for (int v0 = 0; v0 < q.nvox; v0 += FBBEV_OCCL_THREADS) {
            const int v1 = occl_min(v0 + FBBEV_OCCL_THREADS, q.nvox);
            if (STAGED) {
                occl_copy_runs<true>(const_cast<float*>(logits), stage, q, v0, v1, C, row_runs, sh, sw, t);
                __syncthreads();
            }
            const int v = v0 + t;
            float* row = stage + t * C;
            if (v < v1) {
                const int th = v / (q.TWe * q.TDe), rr = v - th * (q.TWe * q.TDe);
                const int tw = rr / q.TDe, td = rr - tw * q.TDe;
                const long long at = q.base + (long long)th * sh + (long long)tw * sw + (long long)td * sd;
                const int label = labels[(((long long)q.b * H + (q.h0 + th)) * W + (q.w0 + tw)) * D + (q.d0 + td)];
                if (label == 255) {
                    for (int c = 0; c < C; ++c) {
                        if (STAGED) row[c] = 0.f;
                        else grad_logits[at + (long long)c * sc] = 0.f;
                    }
                } else {
                    unsigned int fin = 0;                                  // bit c: logit c was finite
                    float mx = -__builtin_inff();
                    for (int c = 0; c < C; ++c) {
                        float x = STAGED ? row[c] : logits[at + (long long)c * sc];
                        if (occl_finite(x)) fin |= 1u << c;
                        else x = 0.f;
                        row[c] = x;
                        mx = fmaxf(mx, x);
                    }
                    float sum = 0.f;
                    for (int c = 0; c < C; ++c) sum += expf(row[c] - mx);
                    const float inv = 1.f / sum;
                    float dot = 0.f;
                    for (int c = 0; c < C; ++c) {
                        const float g = gs[c] + (c == label ? gs[C + c] : -gs[2 * C + c]) - (c == empty_idx ? gG : 0.f);
                        dot += g * (expf(row[c] - mx) * inv);
                    }
                    const float cls = focal ? gCLS * plane_weight[(long long)(q.h0 + th) * W + (q.w0 + tw)]
                                            : (label < C ? gCLS * wts[label] : 0.f);
                    for (int c = 0; c < C; ++c) {
                        const float x = row[c], p = expf(x - mx) * inv;
                        const float g = gs[c] + (c == label ? gs[C + c] : -gs[2 * C + c]) - (c == empty_idx ? gG : 0.f);
                        float gx = p * (g - dot);
                        if (focal) gx += cls * wts[c] * occl_focal_dx(x, c == label, gamma, alpha);
                        else gx += cls * (p - (c == label ? 1.f : 0.f));
                        gx = ((fin >> c) & 1u) ? gx : 0.f;
                        if (STAGED) row[c] = gx;
                        else grad_logits[at + (long long)c * sc] = gx;
                    }
                }
            }
            if (STAGED) {
                __syncthreads();
                occl_copy_runs<false>(grad_logits, stage, q, v0, v1, C, row_runs, sh, sw, t);
                __syncthreads();
            }
        }
    }
}
