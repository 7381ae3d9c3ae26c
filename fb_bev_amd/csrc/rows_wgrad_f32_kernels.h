// rows_wgrad_f32_kernels.h -- weight and bias gradient of a row-wise linear layer in EXACT fp32 on the FP32 MFMA
// (v_mfma_f32_16x16x4_f32): the training side of the exact-fp32 route of rows_linear_f32_kernels.h, beside the split-operand
// kernel of wgrad_kernels.h.
//     gW (O, I) = gy^T x = sum over the R rows of gy[r, :]^T x[r, :],        gb (O) = sum over the rows of gy[r, :]
// Arithmetic contract (fbbev_rows_wgrad_f32 in include/fbbev.h): the rows are cut into S slices of L rows (L a multiple of 4 that
// depends on (rows, I, O) only); inside a slice every element is ONE fmaf chain over the slice's rows in ascending order, and the S
// partial results are added in ascending slice order by a second kernel.  No atomics; a host program reproduces every bit.
//
// The reduction index of this product is the ROW, and the instruction wants A as A[lane % 16][lane / 16] and B as
// B[lane / 16][lane % 16]: for a 4-row step at r0 a lane's operands are gy[r0 + lane / 16][o0 + lane % 16] and
// x[r0 + lane / 16][i0 + lane % 16] -- four 64-byte row segments per load instruction, straight from the row-major tensors.  No
// LDS, no transpose, no barrier (k_rows_wgrad_x3 turns every 32-row step through LDS for its bf16 fragments).  The instruction adds
// its four products in ascending k with one rounding each, so an element's chain visits the rows in ascending order.
//
// Work item = one WAVE: (slice, 64-output chunk, 80-input chunk) -> up to 4 x 5 accumulator tiles of 16 x 16, 20 independent MFMAs per
// 4-row step (the dependent-MFMA latency never shows), fed by 4 + 5 dword loads.  A step's operands are selected and PINNED, its MFMAs
// issued, and only then is its slot requested again (FBBEV_WGF_DEPTH steps ahead): compile-time register slots, no copies between them,
// and every wait of the loop is s_waitcnt vmcnt(27 .. 35) -- the loads of the three following steps stay in flight under the MFMAs.
// A workgroup is four consecutive items.  The bias gradient is one more MFMA per output tile with a ones operand: fmaf(gy, 1, q) ==
// q + gy.  Rows beyond the slice and columns beyond the matrix are never requested (clamped addresses) and enter their MFMAs as zeros
// on both sides.
#pragma once
#include "rt.h"

#define FBBEV_WGF_TO 4          // 16-output tiles of a work item
#define FBBEV_WGF_TI 5          // 16-input tiles of a work item
#define FBBEV_WGF_DEPTH 4       // 4-row steps whose loads are outstanding
#define FBBEV_WGF_MIN_SLICE 64
#define FBBEV_WGF_MAX_SLICE 4096
#define FBBEV_WGF_ITEMS 1024    // work items aimed at: one wave per SIMD of the 256 CUs

// x must be COMPUTED here and no memory operation moves across (fbbev_pin of rt.h for one float; the CPU emulator build has no
// scheduler to bind)
#ifdef FBBEV_TEST_OVERRIDES
static inline void fbbev_wgf_pin(float&) {}
#else
__device__ __forceinline__ void fbbev_wgf_pin(float& x) { asm volatile("" : "+v"(x) : : "memory"); }
#endif

// rows per slice: a function of (rows, I, O) only -- part of the arithmetic contract
static inline long long fbbev_rows_wgrad_f32_slice(long long rows, int I, int O) {
    const long long tiles = (long long)((O + 16 * FBBEV_WGF_TO - 1) / (16 * FBBEV_WGF_TO)) * ((I + 16 * FBBEV_WGF_TI - 1) / (16 * FBBEV_WGF_TI));
    const long long want = tiles >= FBBEV_WGF_ITEMS ? 1 : FBBEV_WGF_ITEMS / tiles;
    long long L = ((rows + want - 1) / want + 3) / 4 * 4;
    if (L < FBBEV_WGF_MIN_SLICE) L = FBBEV_WGF_MIN_SLICE;
    if (L > FBBEV_WGF_MAX_SLICE) L = FBBEV_WGF_MAX_SLICE;
    return L;
}

// grid = ceil(n_items / 4) workgroups of 256 threads; item = (slice s, output chunk oc, input chunk ic), ic fastest.  Writes
// part_w[s][o][i] (dense (O, I) per slice) and, from the ic == 0 items when part_b is given, part_b[s][o].
template <int DEPTH>
__global__ void __launch_bounds__(256, 2)
k_rows_wgrad_f32(const float* __restrict__ gy, long long ldg, const float* __restrict__ x, long long ldx, long long rows, int O, int I,
                 int L, int n_oc, int n_ic, unsigned int n_items, float* __restrict__ part_w, float* __restrict__ part_b) {
    constexpr int TO = FBBEV_WGF_TO, TI = FBBEV_WGF_TI;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63, g = lane >> 4, j = lane & 15;
    const unsigned int item = blockIdx.x * 4u + (unsigned int)wave;                       // the launcher keeps n_items + 3 below 2^32
    if (item >= n_items) return;                                                          // a whole wave
    const int ic = (int)(item % (unsigned int)n_ic), oc = (int)((item / (unsigned int)n_ic) % (unsigned int)n_oc);
    const long long s = item / ((unsigned int)n_ic * (unsigned int)n_oc);
    const int o0 = oc * 16 * TO, i0 = ic * 16 * TI;
    const int nto = (O - o0 >= 16 * TO) ? TO : (O - o0 + 15) / 16, nti = (I - i0 >= 16 * TI) ? TI : (I - i0 + 15) / 16;
    const long long r_begin = s * L, r_end = r_begin + L < rows ? r_begin + L : rows;
    const int nsteps = (int)((r_end - r_begin + 3) / 4);
    const bool do_bias = part_b != nullptr && ic == 0;                                    // uniform
    // this lane's columns (clamped to 0 where the matrix ends: O % 8 == 0, a tile may be half outside)
    int co[TO], ci[TI];
    bool vo[TO], vi[TI];
#pragma unroll
    for (int t = 0; t < TO; ++t) { vo[t] = t < nto && o0 + 16 * t + j < O; co[t] = vo[t] ? o0 + 16 * t + j : 0; }
#pragma unroll
    for (int t = 0; t < TI; ++t) { vi[t] = t < nti && i0 + 16 * t + j < I; ci[t] = vi[t] ? i0 + 16 * t + j : 0; }
    float ga[DEPTH][TO], xa[DEPTH][TI];
    // the loads of step st into slot d; a row beyond the slice reads the slice's last row, a column beyond the matrix (or a tile beyond
    // the chunk) column 0 of its row -- always inside the tensors; what those lanes hold is replaced by zeros when the step is consumed.
    // (The row is clamped by arithmetic: with a predicate in the address the compiler built a branch around the loads of a step and
    // waited for each of them.)
    auto request = [&](int d, int st) {
        const long long r = r_begin + 4 * (long long)st + g, rc = r < r_end ? r : r_end - 1;
        const float* pg = gy + rc * ldg;
        const float* px = x + rc * ldx;
#pragma unroll
        for (int t = 0; t < TO; ++t) ga[d][t] = pg[co[t]];
#pragma unroll
        for (int t = 0; t < TI; ++t) xa[d][t] = px[ci[t]];
    };
    const fbbev_v4f zero4 = {0.f, 0.f, 0.f, 0.f};
    fbbev_v4f acc[TO][TI], accb[TO];
#pragma unroll
    for (int t = 0; t < TO; ++t) {
        accb[t] = zero4;
#pragma unroll
        for (int u = 0; u < TI; ++u) acc[t][u] = zero4;
    }
    // in slot order, fenced: the wait counts of the loop are derived from the issue order on BOTH ways into it -- with the prologue's
    // loads reordered (slot 0 last) every wait at the top of a trip became vmcnt(0)
#pragma unroll
    for (int d = 0; d < DEPTH; ++d) {
        request(d, d);
        fbbev_sched_fence();
    }
    // DEPTH steps per trip, slot = step % DEPTH at compile time; the steps of the last trip beyond nsteps multiply zeros (fmaf(0, 0, p) = p).
    // Order inside a step: select + pin the slot's values, MFMAs, request the slot again.  With the request in front of the MFMAs the
    // compiler hoisted it above the selects -- a fifth register group, rotated with v_mov's behind an s_waitcnt vmcnt(0) every trip; and
    // selects that are not pinned are all linearised to the top of the trip, which waits for the youngest slot there.
    for (int s0 = 0; s0 < nsteps; s0 += DEPTH) {
#pragma unroll
        for (int d = 0; d < DEPTH; ++d) {
            const int st = s0 + d;
            const bool okr = r_begin + 4 * (long long)st + g < r_end;
            float a[TO], b[TI];
#pragma unroll
            for (int t = 0; t < TO; ++t) a[t] = (okr && vo[t]) ? ga[d][t] : 0.f;
#pragma unroll
            for (int t = 0; t < TI; ++t) b[t] = (okr && vi[t]) ? xa[d][t] : 0.f;
#pragma unroll
            for (int t = 0; t < TO; ++t) fbbev_wgf_pin(a[t]);
#pragma unroll
            for (int t = 0; t < TI; ++t) fbbev_wgf_pin(b[t]);
            fbbev_sched_fence();
#pragma unroll
            for (int t = 0; t < TO; ++t) {
                if (t >= nto) break;                                                      // uniform
#pragma unroll
                for (int u = 0; u < TI; ++u) {
                    if (u >= nti) break;                                                  // uniform
                    acc[t][u] = fbbev_mfma_f32_16x16x4(a[t], b[u], acc[t][u]);
                }
                if (do_bias) accb[t] = fbbev_mfma_f32_16x16x4(a[t], 1.0f, accb[t]);
            }
            fbbev_sched_fence();
            request(d, st + DEPTH);
            fbbev_sched_fence();
        }
    }
    // accumulator register r of tile (t, u) = p_s[o0 + 16 t + 4 g + r][i0 + 16 u + j]
    float* pw = part_w + s * O * (long long)I;
#pragma unroll
    for (int t = 0; t < TO; ++t) {
        if (t >= nto) break;
#pragma unroll
        for (int u = 0; u < TI; ++u) {
            if (u >= nti) break;
            const int i = i0 + 16 * u + j;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int o = o0 + 16 * t + 4 * g + r;
                if (o < O && i < I) pw[(long long)o * I + i] = acc[t][u][r];
            }
        }
    }
    if (do_bias) {                                                                        // every column of the ones product holds q_s[o]
#pragma unroll
        for (int t = 0; t < TO; ++t) {
            if (t >= nto) break;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int o = o0 + 16 * t + 4 * g + r;
                if (j == 0 && o < O) part_b[s * O + o] = accb[t][r];
            }
        }
    }
}

// gw[idx] = p_0[idx] + p_1[idx] + ... + p_{S-1}[idx], plain fp32 adds in ascending slice order (one thread per element: the order is
// the contract), U partials requested together; gb[o] likewise from part_b.
template <int U>
__global__ void __launch_bounds__(256)
k_rows_wgrad_f32_reduce(const float* __restrict__ part_w, const float* __restrict__ part_b, int S, long long OI, int O,
                        float* __restrict__ gw, float* __restrict__ gb) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long total = OI + (gb ? O : 0);
    if (idx >= total) return;
    const float* src = idx < OI ? part_w + idx : part_b + (idx - OI);
    const long long stride = idx < OI ? OI : (long long)O;
    float r = src[0];
    for (int s0 = 1; s0 < S; s0 += U) {
        float v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) v[u] = src[(long long)(s0 + u < S ? s0 + u : S - 1) * stride];   // (clamped: unconditional loads)
#pragma unroll
        for (int u = 0; u < U; ++u)
            if (s0 + u < S) r = fbbev_add(r, v[u]);
    }
    if (idx < OI) gw[idx] = r; else gb[idx - OI] = r;
}
