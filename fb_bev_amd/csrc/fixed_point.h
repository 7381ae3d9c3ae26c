// 64-bit fixed-point accumulation for the deterministic mode (include/fbbev.h FBBEV_FLAG_DETERMINISTIC): integer adds give the same
// bits in any order, so a float-atomic scatter becomes order-independent once every add is quantised at one scale.
#pragma once
#include "rt.h"

#if defined(__HIP__)
__device__ __forceinline__ void fbbev_atomic_add_u64(unsigned long long* p, unsigned long long v) { atomicAdd(p, v); }
#else
inline void fbbev_atomic_add_u64(unsigned long long* p, unsigned long long v) { *p += v; }     // the CPU emulator: one fiber at a time
#endif

// ---- fixed-point scatter (deterministic forms of the value-gradient atomics: k_msda_bwd<., true, true>).  Workspace header
// (FBBEV_FIX_HDR bytes) in front of the (n words) 64-bit accumulator: words 0..2 max |factor| bits of up to three tensors whose
// product bounds every add, word 3 the scale exponent s, word 4 the state (1 ok, 0 nothing to add, -1 a non-finite factor).
// s = 61 - sum(e_i) - kq with max |factor_i| < 2^e_i and at most 2^kq adds per word: no word's sum of |adds| reaches 2^61.
#define FBBEV_FIX_HDR 256

__global__ void __launch_bounds__(64)
k_fix_scale(int n_factors, int kq, unsigned int* __restrict__ hdr) {
    if (threadIdx.x != 0) return;
    int esum = 0, state = 1;
    for (int k = 0; k < n_factors; ++k) {
        const unsigned int gb = hdr[k];
        if (gb >= 0x7f800000u) { state = -1; break; }
        if (gb == 0u) { state = state < 0 ? state : 0; continue; }
        const int ex = (int)(gb >> 23);
        esum += ex == 0 ? -126 : ex - 126;
    }
    reinterpret_cast<int*>(hdr)[3] = 61 - esum - kq;
    reinterpret_cast<int*>(hdr)[4] = state;
}

__device__ __forceinline__ void fbbev_fix_add(unsigned long long* acc, float v, double sc) {
    fbbev_atomic_add_u64(acc, (unsigned long long)(long long)__builtin_rint((double)v * sc));
}

// out[i] += acc[i] * 2^-s (state 0: untouched; state -1: NaN)
__global__ void __launch_bounds__(256)
k_fix_to_f32_add(const unsigned int* __restrict__ hdr, long long n, float* __restrict__ out) {
    const int state = reinterpret_cast<const int*>(hdr)[4];
    if (state == 0) return;
    const double inv = __builtin_ldexp(1.0, -reinterpret_cast<const int*>(hdr)[3]);
    const unsigned long long* acc = reinterpret_cast<const unsigned long long*>(reinterpret_cast<const char*>(hdr) + FBBEV_FIX_HDR);
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256)
        out[i] = state > 0 ? out[i] + (float)((double)(long long)acc[i] * inv) : __builtin_nanf("");
}

