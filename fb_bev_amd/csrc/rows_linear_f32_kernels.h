// rows_linear_f32_kernels.h -- y = x W^T + b (+ ReLU | + residual -> LayerNorm) for the (B*Q, C) row tensors of the backward
// projection on the FP32 MFMA (v_mfma_f32_16x16x4_f32): the exact-fp32 route beside the split-operand kernels of
// rows_linear_kernels.h.  Every output element is ONE chain of fp32 fmaf's over the input channels in a fixed order that
// depends on in_features only (the arithmetic contract of fbbev_rows_linear_f32 in include/fbbev.h), so a host program can
// reproduce every bit.  The fp32 MFMA runs at 1/16 of the bf16 rate and the x3 form spends 3 bf16 MFMAs per product: about 5x the
// matrix work of k_rows_linear_x3 -- this route is for defined arithmetic, not for speed.
//
// Shape (as k_rows_linear_x3): workgroup = 4 waves x 2 16-row tiles (128 rows) x one 128-wide chunk of the outputs; K is walked
// in chunks of 128 channels = 8 k-blocks of 16.  The weight is read as nn.Linear stores it (row-major (O, I) fp32) and staged
// through LDS in A-operand order [out tile][k-block][lane][4]: lane (g, j) of k-block kb holds W[16 mt + j][16 kb + 4 g + 0..3], one
// ds_read_b128 at consecutive addresses per lane (conflict-free), 8 KB per 16 outputs, 64 KB for a full chunk (two workgroups per
// CU).  The rows are read straight into registers: lane (g, j) loads channels 16 kb + 4 g + 0..3 of row j as one float4.
//
// Order of the chain: MFMA e of k-block kb takes component e of both float4s, i.e. lane group g supplies channel 16 kb + 4 g + e
// as the instruction's k = g, and the instruction adds its four products in ascending k.  So the channels are consumed as
//     for kb: for e in 0..3: for g in 0..3: 16 kb + 4 g + e            (fbbev_rows_linear_f32_order below)
// No shuffles, no split-K, the accumulator carried across the K chunks.  Channels beyond I multiply zeros on both sides.
#pragma once
#include "rt.h"
#include "rows_linear_kernels.h"

#define FBBEV_RLF_TILE_FLOATS (8 * 64 * 4)                // floats of one 16-output tile of one K chunk: [8 k-blocks][lane][4]

// the order above, host side: order[t] = channel consumed at step t; returns the number of steps (= I)
static inline int fbbev_rows_linear_f32_order(int I, int* order) {
    int n = 0;
    for (int kb = 0; 16 * kb < I; ++kb)
        for (int e = 0; e < 4; ++e)
            for (int g = 0; g < 4; ++g) {
                const int c = 16 * kb + 4 * g + e;
                if (c < I) order[n++] = c;
            }
    return n;
}

// W[o0 .., c0 ..] (row-major, pitch I) -> LDS in A-operand order, zeros outside the matrix; U pieces per thread requested before the
// first is stored (the pattern of fbbev_stage_v4u).  A piece = 4 consecutive channels of one output, and piece i goes to LDS piece i:
// i = ((mt * 8 + kb) * 4 + g) * 16 + j, so a wave's 64 stores cover 1 KB of consecutive addresses (conflict-free; with the channel quad
// fastest -- the coalesced order of the global side -- the 32 lanes of one weight row hit the same four banks).  The global side then
// reads 64-byte runs of 16 weight rows per wave, the pattern of the row loads; the weight is small and stays in L2.
template <int U>
__device__ __forceinline__ void fbbev_rlf_stage(float* __restrict__ wl, const float* __restrict__ w, int I, int O, int o0, int c0,
                                                int nmt, int nkb) {
    const int n = nmt * 512;
    for (int i0 = threadIdx.x; i0 < n; i0 += 256 * U) {
        fbbev_v4f t[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int i = i0 + 256 * u, kb = (i >> 6) & 7;
            const int o = o0 + 16 * (i >> 9) + (i & 15), c = c0 + 16 * kb + 4 * ((i >> 4) & 3);
            const bool ok = i < n && o < O && c < I;                                      // I % 4 == 0: a piece is all in or all out
            t[u] = *reinterpret_cast<const fbbev_v4f*>(w + (ok ? (long long)o * I + c : 0));   // (clamped: unconditional loads)
            t[u] = ok ? t[u] : fbbev_v4f{0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int i = i0 + 256 * u;
            if (i < n && ((i >> 6) & 7) < nkb) *reinterpret_cast<fbbev_v4f*>(wl + 4 * i) = t[u];
        }
    }
}

// `res` and `out` are NOT __restrict__: fbbev_rows_linear_f32_ln allows residual == out (an element is read, then written, by one
// thread, and the stored value depends on the loaded one)
template <bool LN>
__global__ void __launch_bounds__(256, 2)
k_rows_linear_f32(const float* __restrict__ x, long long ldx, const float* __restrict__ w, const float* __restrict__ bias,
                  float* out, long long ldo, long long rows, int I, int O, int relu, int n_kc, int n_oc, int RT,
                  const float* __restrict__ addend, long long ld_add, long long add_period,
                  const float* res, long long ld_res, const float* __restrict__ ln_w, const float* __restrict__ ln_b, float ln_eps) {
    constexpr int NT = 2;
    float* wl = fbbev_dyn_lds_f32();                                                      // [nmt][FBBEV_RLF_TILE_FLOATS]
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int g = lane >> 4, j = lane & 15;
    const int oc = (int)(blockIdx.x % n_oc);              // the output chunks of one row tile are neighbours: its rows stay in L2
    const long long rt0 = (long long)(blockIdx.x / n_oc) * RT;
    const int o0 = oc * 128;
    const int nmt = (O - o0 >= 128) ? 8 : (O - o0 + 15) / 16;                             // 16-output tiles of this chunk
    // RT consecutive 128-row tiles per workgroup when the whole K fits one chunk (the weight is staged once); RT = 1 otherwise
    for (int ri = 0; ri < RT; ++ri) {
        const long long r0 = ((rt0 + ri) * 4 + wave) * (16 * NT);
        if ((rt0 + ri) * 4 * 16 * NT >= rows) break;                                      // uniform
        fbbev_v4f acc[8][NT];
#pragma unroll
        for (int mt = 0; mt < 8; ++mt)
#pragma unroll
            for (int t = 0; t < NT; ++t) acc[mt][t] = fbbev_v4f{0.f, 0.f, 0.f, 0.f};
        long long ra[NT];                                                                 // row of the addend (x + addend[row % period])
#pragma unroll
        for (int t = 0; t < NT; ++t) {                                                    // (once per row tile and lane; a 32-bit path beside it costs the scalar budget)
            const long long r = r0 + 16 * t + j;
            ra[t] = addend ? r % add_period : 0;
        }
        for (int kc = 0; kc < n_kc; ++kc) {
            const int c0 = kc * 128;
            const int nkb = (I - c0 >= 128) ? 8 : (I - c0 + 15) / 16;                     // k-blocks of this chunk
            // the chunk's row pieces first (into registers): they are in flight while the weight is staged
            fbbev_v4f xb[8][NT];
#pragma unroll
            for (int kb = 0; kb < 8; ++kb) {
                const int c = c0 + 16 * kb + 4 * g;
                if (kb >= nkb) {                                                          // uniform: nothing is requested beyond the input width
#pragma unroll
                    for (int t = 0; t < NT; ++t) xb[kb][t] = fbbev_v4f{0.f, 0.f, 0.f, 0.f};
                    continue;
                }
#pragma unroll
                for (int t = 0; t < NT; ++t) {
                    const long long r = r0 + 16 * t + j;
                    // (clamped; I % 4 == 0: a piece is all in or all out.  What a clamped lane holds is dealt with below:
                    // rows beyond `rows` are never stored, channels beyond I are zeroed in front of their MFMAs -- kept as 16 lane masks
                    // across the weight staging the predicates cost 32 scalar registers)
                    fbbev_v4f v = *reinterpret_cast<const fbbev_v4f*>(x + ((r < rows && c < I) ? r * ldx + c : 0));
                    if (addend)                                                           // uniform: x + addend[row % period] (query + query_pos)
                        v = v + *reinterpret_cast<const fbbev_v4f*>(addend + ((r < rows && c < I) ? ra[t] * ld_add + c : 0));
                    xb[kb][t] = v;
                }
            }
            if (n_kc > 1 || ri == 0) {
                if (kc || ri) __syncthreads();                                            // the previous chunk's weight is done with
                fbbev_rlf_stage<4>(wl, w, I, O, o0, c0, nmt, nkb);
                __syncthreads();
            }
#pragma unroll
            for (int kb = 0; kb < 8; ++kb) {
                if (kb >= nkb) break;                                                     // uniform: no k-block beyond the input width
                if (c0 + 16 * kb + 16 > I) {                                              // uniform: the last k-block of I % 16 == 8 -- the channels
#pragma unroll                                                                            // beyond I multiply zeros (the weight's are zeros in LDS)
                    for (int t = 0; t < NT; ++t) xb[kb][t] = g < 2 ? xb[kb][t] : fbbev_v4f{0.f, 0.f, 0.f, 0.f};
                }
#pragma unroll
                for (int mt = 0; mt < 8; ++mt) {
                    if (mt >= nmt) break;                                                 // uniform
                    const fbbev_v4f a = *reinterpret_cast<const fbbev_v4f*>(wl + ((mt * 8 + kb) * 64 + lane) * 4);
#pragma unroll
                    for (int e = 0; e < 4; ++e)
#pragma unroll
                        for (int t = 0; t < NT; ++t) acc[mt][t] = fbbev_mfma_f32_16x16x4(a[e], xb[kb][t][e], acc[mt][t]);
                }
            }
        }
        // accumulator register r of tile (mt, t) = output 16 mt + 4 g + r of row j: four consecutive outputs, one 16-byte access
        if constexpr (LN) {
            // LayerNorm epilogue, the arithmetic of k_rows_linear_x3<., true> (n_oc == 1: the workgroup holds whole output rows): two-pass
            // statistics, a row's O values live in the 4 lanes (g = 0..3, same j) of its row tile.  Bias / residual / LayerNorm pieces
            // requested together, unconditionally, at clamped addresses.
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                // an offset the compiler cannot see through: the bias / LayerNorm pieces are loop-invariant, and hoisted out of the row-tile
                // loop their 96 registers sat on top of the accumulators and row pieces of the MFMA phase (spills)
                int zo = 0;
                fbbev_opaque(zo);
                const long long r = r0 + 16 * t + j;
                const bool live = r < rows;
                fbbev_v4f v[8], pb[8], pr[8];
#pragma unroll
                for (int mt = 0; mt < 8; ++mt) {
                    const int o = 16 * mt + 4 * g, oc_ = (mt < nmt && o < O) ? o : 0;
                    pb[mt] = bias ? *reinterpret_cast<const fbbev_v4f*>(bias + oc_ + zo) : fbbev_v4f{0.f, 0.f, 0.f, 0.f};
                    pr[mt] = res ? *reinterpret_cast<const fbbev_v4f*>(res + (live ? r : 0) * ld_res + oc_) : fbbev_v4f{0.f, 0.f, 0.f, 0.f};
                }
                float s = 0.f;
#pragma unroll
                for (int mt = 0; mt < 8; ++mt) {
                    const int o = 16 * mt + 4 * g;
                    v[mt] = fbbev_v4f{0.f, 0.f, 0.f, 0.f};
                    if (mt < nmt && o < O) {
                        v[mt] = acc[mt][t];
                        if (bias) v[mt] = v[mt] + pb[mt];
                        if (res && live) v[mt] = v[mt] + pr[mt];
                        s += (v[mt][0] + v[mt][1]) + (v[mt][2] + v[mt][3]);
                    }
                }
                s += __shfl_xor(s, 16, 64); s += __shfl_xor(s, 32, 64);
                const float mean = s / (float)O;
                float q = 0.f;
#pragma unroll
                for (int mt = 0; mt < 8; ++mt) {
                    const int o = 16 * mt + 4 * g;
                    if (mt < nmt && o < O) {
                        v[mt] = v[mt] - fbbev_v4f{mean, mean, mean, mean};
                        q += (v[mt][0] * v[mt][0] + v[mt][1] * v[mt][1]) + (v[mt][2] * v[mt][2] + v[mt][3] * v[mt][3]);
                    }
                }
                q += __shfl_xor(q, 16, 64); q += __shfl_xor(q, 32, 64);
                const float inv = 1.0f / sqrtf(q / (float)O + ln_eps);
#pragma unroll
                for (int mt = 0; mt < 8; ++mt) {                                           // (pb / pr are free: the LayerNorm pieces take their place)
                    const int o = 16 * mt + 4 * g, oc_ = (mt < nmt && o < O) ? o : 0;
                    pb[mt] = *reinterpret_cast<const fbbev_v4f*>(ln_w + oc_ + zo);
                    pr[mt] = *reinterpret_cast<const fbbev_v4f*>(ln_b + oc_ + zo);
                }
#pragma unroll
                for (int mt = 0; mt < 8; ++mt) {
                    const int o = 16 * mt + 4 * g;
                    if (mt < nmt && o < O && live) {
                        const fbbev_v4f w4 = pb[mt], b4 = pr[mt];
                        fbbev_v4f y;
#pragma unroll
                        for (int e = 0; e < 4; ++e) y[e] = v[mt][e] * inv * w4[e] + b4[e];
                        fbbev_st(reinterpret_cast<fbbev_v4f*>(out + r * ldo + o), y);
                    }
                }
            }
        } else {
            fbbev_v4f pbias[8];                                                           // (requested together, clamped)
#pragma unroll
            for (int mt = 0; mt < 8; ++mt) {
                const int o = o0 + 16 * mt + 4 * g;
                pbias[mt] = bias ? *reinterpret_cast<const fbbev_v4f*>(bias + ((mt < nmt && o < O) ? o : 0)) : fbbev_v4f{0.f, 0.f, 0.f, 0.f};
            }
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const long long r = r0 + 16 * t + j;
                if (r >= rows) continue;
#pragma unroll
                for (int mt = 0; mt < 8; ++mt) {
                    const int o = o0 + 16 * mt + 4 * g;
                    if (mt >= nmt || o >= O) continue;                                    // O % 4 == 0: a group is all in or all out
                    fbbev_v4f v = acc[mt][t];
                    if (bias) v = v + pbias[mt];
                    if (relu) v = fbbev_v4f{fmaxf(v[0], 0.f), fmaxf(v[1], 0.f), fmaxf(v[2], 0.f), fmaxf(v[3], 0.f)};
                    fbbev_st(reinterpret_cast<fbbev_v4f*>(out + r * ldo + o), v);
                }
            }
        }
    }
}
