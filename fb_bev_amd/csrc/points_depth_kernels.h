// points_depth_kernels.h -- a LiDAR sweep to multi-view depth maps as a z-buffer.
// Replaces PointToMultiViewDepth (mmdet3d/datasets/pipelines/loading.py:876-966 of the reference), a CPU pipeline step: per camera a
// matmul, a division, a second matmul, a round, six comparisons, an argsort of `pixel_rank + depth / 100`, a first-of-run mask and a
// scatter -- and the (N, H, W) map through the loader and over PCIe.  Here a point and a camera cost one projection and one integer
// atomic; no sort and no key.
//   points (sum P, stride) f32 rows, the first three columns are read; offsets (B + 1) int32: sample b owns rows
//   offsets[b] .. offsets[b + 1] - 1.  M = lidar2img[b, n] (4, 4), R = post_rots[b, n] (3, 3), T = post_trans[b, n] (3).
//   Per (point p, camera n), every step ONE correctly rounded fp32 operation, in this order (the association of fbbev.h):
//     c_i = fmaf(M[i][2], p.z, fmaf(M[i][1], p.y, M[i][0] * p.x)) + M[i][3]          i = 0, 1, 2
//     (u, v, z) = (c_0 / c_2, c_1 / c_2, c_2)
//     q_i = fmaf(R[i][2], z, fmaf(R[i][1], v, R[i][0] * u)) + T[i]
//     x = rintf(q_0 / ds), y = rintf(q_1 / ds)                                       half to even, as torch.round
//     kept = x >= 0 && x < w && y >= 0 && y < h && q_2 < hi && q_2 >= lo              on floats: -0.0 is pixel 0, NaN and inf fail
// k_points_depth_splat: a kept point does atomicMax(word[((b N + n) h + y) w + x], ~bits(q_2)) on an unsigned plane that the
// launcher zeroed through the runtime.  lo > 0 (checked by the launcher), so a kept depth is positive and finite: its bits order as
// the floats do, ~bits orders them inversely, and no kept depth maps to 0, which stays "no return".  The atomic's result is not used
// (the no-return form), integer max is order-independent: the plane's bits depend on the inputs alone.
// Grid: (b, n, chunk) in blockIdx.x, `chunks` workgroups per (b, n), capped at FBBEV_PD_MAX_CHUNKS by the launcher; a thread walks
// the sample's points chunk * 256 + t, + chunks * 256, ...: threads past the sample's count exit, a sample longer than the grid
// loops.  The matrices of a workgroup are uniform (one (b, n) per workgroup).  Consecutive lanes read consecutive point rows.
// k_points_depth_resolve: the plane to f32 in place, word ? ~word : 0 on the bits (0 is +0.0f); 16-byte accesses over the aligned
// body, scalar words before and behind it.  Grid-stride, capped by the launcher.
#pragma once
#include "rt.h"

#define FBBEV_PD_THREADS 256
#define FBBEV_PD_MAX_CHUNKS 64                                   // workgroups per (sample, camera): 16384 points per pass
#define FBBEV_PD_RESOLVE_BLOCKS 2048                             // cap of the resolve grid

__device__ __forceinline__ unsigned int pd_bits(float x) { unsigned int u; __builtin_memcpy(&u, &x, 4); return u; }
// one row of a 3 x 3 product plus its translation: the chain stated above
__device__ __forceinline__ float pd_row(const float* __restrict__ m, float a, float b, float c, float t) {
    return fbbev_add(fmaf(m[2], c, fmaf(m[1], b, fbbev_mul(m[0], a))), t);
}

__global__ void __launch_bounds__(FBBEV_PD_THREADS)
k_points_depth_splat(const float* __restrict__ points, int stride, const int* __restrict__ offsets, int N, int chunks,
                     const float* __restrict__ lidar2img, const float* __restrict__ post_rots, const float* __restrict__ post_trans,
                     float ds, int h, int w, float lo, float hi, unsigned int* __restrict__ plane) {
    const unsigned int bn = blockIdx.x / (unsigned int)chunks, chunk = blockIdx.x - bn * (unsigned int)chunks;
    const unsigned int b = bn / (unsigned int)N;
    const long long first = offsets[b], count = (long long)offsets[b + 1] - first;
    const float* M = lidar2img + (size_t)bn * 16;
    const float* R = post_rots + (size_t)bn * 9;
    const float* T = post_trans + (size_t)bn * 3;
    unsigned int* map = plane + (size_t)bn * h * w;
    const float fw = (float)w, fh = (float)h;                    // h * w < 2^24: exact
    const long long step = (long long)chunks * FBBEV_PD_THREADS;
    for (long long i = (long long)chunk * FBBEV_PD_THREADS + threadIdx.x; i < count; i += step) {
        const float* p = points + (first + i) * stride;
        const float px = p[0], py = p[1], pz = p[2];
        const float c0 = pd_row(M, px, py, pz, M[3]);
        const float c1 = pd_row(M + 4, px, py, pz, M[7]);
        const float c2 = pd_row(M + 8, px, py, pz, M[11]);
        const float u = fbbev_div(c0, c2), v = fbbev_div(c1, c2);
        const float q0 = pd_row(R, u, v, c2, T[0]);
        const float q1 = pd_row(R + 3, u, v, c2, T[1]);
        const float q2 = pd_row(R + 6, u, v, c2, T[2]);
        const float x = rintf(fbbev_div(q0, ds)), y = rintf(fbbev_div(q1, ds));
        if (x >= 0.0f && x < fw && y >= 0.0f && y < fh && q2 < hi && q2 >= lo)
            atomicMax(map + (size_t)((int)y * w + (int)x), ~pd_bits(q2));
    }
}

// n words at `plane`; head = the words in front of the first 16-byte boundary (0..3, at most n), nv = the 16-byte groups behind them
__global__ void __launch_bounds__(FBBEV_PD_THREADS)
k_points_depth_resolve(unsigned int* __restrict__ plane, long long n, int head, long long nv) {
    const long long g = (long long)blockIdx.x * FBBEV_PD_THREADS + threadIdx.x;
    const long long total = (long long)gridDim.x * FBBEV_PD_THREADS;
    fbbev_v4u* body = reinterpret_cast<fbbev_v4u*>(plane + head);
    for (long long j = g; j < nv; j += total) {
        fbbev_v4u v = body[j];
        v[0] = v[0] ? ~v[0] : 0u;
        v[1] = v[1] ? ~v[1] : 0u;
        v[2] = v[2] ? ~v[2] : 0u;
        v[3] = v[3] ? ~v[3] : 0u;
        body[j] = v;
    }
    if (g < head) {
        const unsigned int v = plane[g];
        plane[g] = v ? ~v : 0u;
    }
    const long long tail = head + 4 * nv + g;                    // at most three words
    if (g < 4 && tail < n) {
        const unsigned int v = plane[tail];
        plane[tail] = v ? ~v : 0u;
    }
}
