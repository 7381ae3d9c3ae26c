// Deterministic mode (include/fbbev.h, FBBEV_FLAG_DETERMINISTIC): the depth-distribution gradient of the DA backward without float
// atomics.  The unit kernels' DET instantiations (k_da_bwd_unit_planes<., ., true>, k_da_cross_attn_bwd_unit<., ., true>) STORE
// the per-(camera, sample, query, anchor) sum of d loss / d depth weight over the heads (a fixed-order sum) into a (Ncam, B, Q, Za)
// buffer instead of pushing it to the four taps of the query's bin plane.  Then:
//   k_da_taps_absmax   max |sum| of the call as float bits (atomicMax on bits of non-negative floats: any order, same word)
//   k_da_taps_i64      every tap, wgt * sum in fp32 exactly as the atomic form computes it, added as 64-bit fixed point
//                      (integer adds: any completion order gives the same bits)
//   k_i64_to_f32_add   the fixed-point planes back to fp32, added to grad_pred_depth
// Scale: 2^s with s = 61 - e - kq, max |sum| < 2^e, Q * Za <= 2^kq.  A tap weight is in [0, 1] and one (query, anchor) puts at most
// one tap on a word, so no word's sum of |adds| reaches 2^61: no overflow, and the resolution is 2^-(61 - kq) of max |sum|
// (2^-43 at a 200 x 200 grid with 4 anchors) -- finer than the fp32 rounding of any word within 2^-19 of the largest.
// A non-finite sum poisons the whole gradient with NaN (the atomic form would poison the words it touches).
#pragma once
#include "rt.h"
#include "da_fused_kernels.h"
#include "fixed_point.h"


// exponent of the fixed-point scale from the max |sum| bits; false when there is nothing to add or the maximum is not finite
__host__ __device__ inline bool fbbev_det_scale_exp(unsigned int gbits, int kq, int& s) {
    if (gbits == 0u || gbits >= 0x7f800000u) return false;
    const int ex = (int)(gbits >> 23);                       // biased exponent: max |sum| < 2^(ex - 126) (denormals: 2^-126)
    const int e = ex == 0 ? -126 : ex - 126;
    s = 61 - e - kq;
    return true;
}

__global__ void __launch_bounds__(256)
k_da_taps_absmax(const float* __restrict__ dsum, long long n, unsigned int* __restrict__ gmax_bits) {
    float m = 0.f;
    bool bad = false;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const float a = fabsf(dsum[i]);
        bad = bad || !(a < __builtin_inff());
        m = fmaxf(m, a);
    }
    if (bad) m = __builtin_inff();
    unsigned int gb;
    __builtin_memcpy(&gb, &m, 4);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned int t = (unsigned int)__shfl_xor((int)gb, o, 64);
        gb = t > gb ? t : gb;
    }
    // one atomic per workgroup: thousands of same-word atomics (one per wave) serialised to ~100 us at configs[2]
    __shared__ unsigned int wmax[4];
    if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = gb;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned int m4 = wmax[0];
        for (int w = 1; w < 4; ++w) m4 = wmax[w] > m4 ? wmax[w] : m4;
        if (m4 != 0u) atomicMax(gmax_bits, m4);
    }
}

// one thread per (camera, sample, query, anchor) of the sums; taps on the (B*Ncam, DC, H0, W0) fixed-point planes
__global__ void __launch_bounds__(256)
k_da_taps_i64(const float* __restrict__ dsum, const float* __restrict__ ref_cam, const float* __restrict__ qdepth, int B, int Ncam,
              int Q, int Za, int DC, int H0, int W0, float d0, float dstep, int kq, const unsigned int* __restrict__ gmax_bits,
              unsigned long long* __restrict__ acc) {
    const long long n = (long long)Ncam * B * Q * Za;
    int s;
    if (!fbbev_det_scale_exp(*gmax_bits, kq, s)) return;
    const double sc = __builtin_ldexp(1.0, s);
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const float d = dsum[i];
        if (d == 0.f) continue;
        const long long cbq = i / Za, cb = cbq / Q;
        const int b = (int)(cb % B), cam = (int)(cb / B);
        float fb = floorf(__fdiv_rn(__fsub_rn(qdepth[i], d0), dstep));
        fb = fminf(fmaxf(fb, 0.f), (float)(DC - 1));
        int off[4];
        float wgt[4];
        fbbev_daf_plane_corners(ref_cam[i * 2], ref_cam[i * 2 + 1], H0, W0, off, wgt);
        unsigned long long* plane = acc + (((long long)b * Ncam + cam) * DC + (int)fb) * (long long)(H0 * W0);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (wgt[k] == 0.f) continue;
            const long long v = (long long)__builtin_rint((double)(wgt[k] * d) * sc);
            fbbev_atomic_add_u64(plane + off[k], (unsigned long long)v);
        }
    }
}

__global__ void __launch_bounds__(256)
k_i64_to_f32_add(const unsigned long long* __restrict__ acc, long long n, int kq, const unsigned int* __restrict__ gmax_bits,
                 float* __restrict__ out) {
    const unsigned int gb = *gmax_bits;
    int s = 0;
    const bool ok = fbbev_det_scale_exp(gb, kq, s);
    if (!ok && gb == 0u) return;                             // every sum was zero: nothing was added
    const double inv = __builtin_ldexp(1.0, -s);
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256)
        out[i] = ok ? out[i] + (float)((double)(long long)acc[i] * inv) : __builtin_nanf("");
}

// ---- split-K partials summed in chunk order (k_conv3d_wgrad_ndhwc<., true>): out[i] += part[0][i] + part[1][i] + ...
__global__ void __launch_bounds__(256)
k_sum_chunks_add(const float* __restrict__ part, int n_chunks, long long n, float* __restrict__ out) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        float s = 0.f;
        for (int c = 0; c < n_chunks; ++c) s += part[(long long)c * n + i];
        out[i] += s;
    }
}

// the per-head sums of k_da_cross_attn_bwd<., true> (Ncam, B, Q, M, Za) -> the taps' (Ncam, B, Q, Za) input, heads added in order
__global__ void __launch_bounds__(256)
k_da_head_sum(const float* __restrict__ per_head, long long n_cbq, int M, int Za, float* __restrict__ dsum) {
    const long long n = n_cbq * Za;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const long long cbq = i / Za;
        const int z = (int)(i - cbq * Za);
        float t = 0.f;
        for (int m = 0; m < M; ++m) t += per_head[(cbq * M + m) * Za + z];
        dsum[i] = t;
    }
}
