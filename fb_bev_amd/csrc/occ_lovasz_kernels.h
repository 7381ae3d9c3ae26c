// occ_lovasz_kernels.h -- the Lovasz-softmax term of the occupancy head (classes = 'present', per_image = False) on the device, forward
// and backward.  Replaces lovasz_softmax.py:20-33,157-229: a full-size softmax, a (C, N) error matrix, one sort per class
// with an int64 permutation, a gather, two prefix sums and the Jaccard differences, all kept alive for autograd.
//
// For class c over the valid voxels (t != 255): f_i = [t_i == c], e_i = |f_i - p_i[c]|, G = sum f.  Sorted by e descending (ties by
// ascending voxel index), position k = 1..n, F_k = fg elements among the first k, U_k = G + k - F_k.  The reference's Jaccard value is
// J_k = 1 - (G - F_k) / U_k = k / U_k, so the Lovasz coefficient g_k = J_k - J_{k-1} is a closed form in integers:
//     fg element:  g_k = 1 / U_k                    bg element:  g_k = (G - F_k) / (U_k (U_k - 1))
// evaluated in double and rounded once to float (IEEE operations only: a host program reproduces every bit).  loss_c = sum_k e_(k) g_k,
// each product exact in double, added per chunk and then over the chunks in a fixed order.  The reference takes g as a constant, so
// with h[c, i] = -g (fg) or +g (bg) and s = upstream / n_present:  grad x[j] = s p[j] (h[j] - sum_c h[c] p[c]).
//
// Bounds: C in 2..32; B H W D < 2^26 (U (U - 1) < 2^53: the double arithmetic is exact where it has to be).
//
// Kernels, for a group of g classes c0 .. c0 + g - 1 (the launcher walks the classes in groups to bound the workspace):
//   k_occ_lovasz_keys     the tile walk of k_occ_loss_stats.  Per voxel: x = nan_to_num(logits), p = softmax(x); per class of the group
//                         one word at keys[class][voxel]: the bits of e (e in [0, 1]: 30 bits) with the fg flag in bit 31, or
//                         FBBEV_OCCLV_DROP for a voxel labelled 255.  It also clears coef and writes errors_out (0 where ignored).
//   per radix pass (3 x 10 bits or 4 x 8 bits of the key ONE - bits(e): ascending key = descending e), segment = class, all segments
//   n_valid long, chunks of FBBEV_OCCLV_TILE pairs, workgroup = (class, chunk) with the class as the slow index of the grid:
//     k_occ_lovasz_hist     count matrix row [class][chunk][digit]; the first pass reads the words in voxel order, drops the ignored ones
//                           (they take no rank) and counts the chunk's valid and fg voxels
//     k_occ_lovasz_colscan  a thread per (class, digit): the column becomes its exclusive prefix over the chunks, the total goes to
//                           tot[class][digit]; the first pass also adds the chunk counts: fg_count[c] = G, fg_count[C] = n_valid
//     k_occ_lovasz_scatter  stable ranking of the chunk's 4096 pairs with wave ballots on top of wave-private digit counters in LDS
//                           (k_sort_scatter_seg's scheme); (key, payload) pairs, payload = voxel index | fg << 31
//   k_occ_lovasz_fgsum    fg elements per chunk of the sorted order
//   k_occ_lovasz_coef     F_k from a block scan on top of the earlier chunks' counts (integer adds only), g_k, h stored at
//                         coef[class][voxel], the chunk's sum of e g in double
//   k_occ_lovasz_loss     one workgroup per class: the chunk sums in a fixed order, rounded once
//   k_occ_lovasz_grad     k_occ_loss_grad's structure: p recomputed, the voxel's C coefficients read from coef
// n_valid and G are read from device words; nothing synchronises with the host; no float atomics: the bits depend on the inputs alone.
// A class with G == 0 is skipped from the first scatter on (its coefficients stay 0, its loss is 0).
#pragma once
#include "rt.h"
#include "occ_tile_walk.h"

#define FBBEV_OCCLV_WAVES 4
#define FBBEV_OCCLV_NT (FBBEV_OCCLV_WAVES * 64)
#define FBBEV_OCCLV_ROUNDS 16
#define FBBEV_OCCLV_TILE (FBBEV_OCCLV_NT * FBBEV_OCCLV_ROUNDS)
#define FBBEV_OCCLV_MAX_RB 10
#define FBBEV_OCCLV_MAX_NB (1 << FBBEV_OCCLV_MAX_RB)
#define FBBEV_OCCLV_DROP 0xffffffffu          // a voxel labelled 255: no key has bit 30 set
#define FBBEV_OCCLV_ONE 0x3f800000u           // bits of 1.0f: key = ONE - bits(e) in [0, ONE]
#define FBBEV_OCCLV_MAX_BLOCKS 1024           // grid cap of the two tile walks (keys, gradient)

__device__ __forceinline__ unsigned int occlv_bits(float x) { unsigned int u; __builtin_memcpy(&u, &x, 4); return u; }
__device__ __forceinline__ float occlv_float(unsigned int u) { float x; __builtin_memcpy(&x, &u, 4); return x; }

// exclusive sum scan of one int per thread over the workgroup's WAVES wave64s; *total = the workgroup's sum; ldsw: WAVES ints of LDS
template <int WAVES>
__device__ __forceinline__ int occlv_block_excl_scan(int v, int* ldsw, int* total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int nbr = __shfl_up(inc, o, 64);
        if (lane >= o) inc += nbr;
    }
    if (lane == 63) ldsw[w] = inc;
    __syncthreads();
    int carry = 0, tot = 0;
#pragma unroll
    for (int i = 0; i < WAVES; ++i) {
        const int x = ldsw[i];
        if (i < w) carry += x;
        tot += x;
    }
    __syncthreads();
    *total = tot;
    return carry + inc - v;
}

__device__ __forceinline__ int occlv_wave_sum(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;                                                              // lane 0 holds the sum
}

// the workgroup's sum of one double per thread through a fixed tree; red: FBBEV_OCCLV_NT doubles of LDS; valid in thread 0
__device__ __forceinline__ double occlv_block_sum(double v, double* red) {
    const int t = threadIdx.x;
    red[t] = v;
    __syncthreads();
    for (int s = FBBEV_OCCLV_NT / 2; s > 0; s >>= 1) {
        if (t < s) red[t] += red[t + s];
        __syncthreads();
    }
    return red[0];
}

// ---------------------------------------------------------------------------------------------------------------- keys
// keys [g][nvox] words; coef and errors_out [C][nvox] floats (class planes in (b, h, w, d) order); the thread that owns a voxel writes
// its g words of each (a wave covers runs of TD, or of TW x TD at a whole depth, consecutive words of a plane)
template <bool STAGED>
__global__ void __launch_bounds__(FBBEV_OCCL_THREADS)
k_occ_lovasz_keys(const float* __restrict__ logits, long long sb, long long sc, long long sh, long long sw, long long sd,
                  int C, int H, int W, int D, int T, int TD, int nth, int ntw, int ntd, int ntiles, int row_runs,
                  const unsigned char* __restrict__ labels, int c0, int g, int nvox, unsigned int* __restrict__ keys,
                  float* __restrict__ coef, float* __restrict__ errors_out) {
    float* stage = fbbev_dyn_lds_f32();                                    // 256 rows of C floats: x, then p
    const int t = threadIdx.x;
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        int tile_v = tile;                                                 // the tile's fields live in vector registers
        fbbev_opaque(tile_v);
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
                const int flat = ((q.b * H + (q.h0 + th)) * W + (q.w0 + tw)) * D + (q.d0 + td);      // < nvox < 2^26
                const int label = labels[flat];
                if (label != 255) {
                    const float* px = logits + q.base + (long long)th * sh + (long long)tw * sw + (long long)td * sd;
                    float mx = -__builtin_inff();
                    for (int c = 0; c < C; ++c) {
                        float x = STAGED ? row[c] : px[(long long)c * sc];
                        x = occl_finite(x) ? x : 0.f;
                        row[c] = x;
                        mx = fmaxf(mx, x);
                    }
                    float sum = 0.f;
                    for (int c = 0; c < C; ++c) {
                        const float ex = expf(row[c] - mx);
                        row[c] = ex;
                        sum += ex;
                    }
                    const float inv = 1.f / sum;
                    for (int c = 0; c < C; ++c) row[c] *= inv;
                }
                for (int cl = 0; cl < g; ++cl) {
                    const int c = c0 + cl;
                    unsigned int word = FBBEV_OCCLV_DROP;
                    float e = 0.f;
                    if (label != 255) {
                        const bool fg = c == label;
                        e = fabsf((fg ? 1.f : 0.f) - row[c]);
                        word = occlv_bits(e) | (fg ? 0x80000000u : 0u);
                    }
                    keys[(long long)cl * nvox + flat] = word;
                    coef[(long long)c * nvox + flat] = 0.f;
                    if (errors_out) errors_out[(long long)c * nvox + flat] = e;
                }
            }
            if (STAGED) __syncthreads();                                   // the rows are staged again by the whole workgroup
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- radix passes
// count matrix row of workgroup (class, chunk).  FIRST: the words of the keys kernel in voxel order (n = nvox, the ignored ones are
// neither counted nor ranked) and cstat[class][chunk] = (valid, fg); later passes: the pairs the previous pass wrote (n = n_valid)
template <bool FIRST>
__global__ void __launch_bounds__(FBBEV_OCCLV_NT)
k_occ_lovasz_hist(const unsigned int* __restrict__ keys0, const uint2* __restrict__ pairs, int pass, int rb, int nvox, int cps, int C,
                  int c0, const int* __restrict__ fg_count, int* __restrict__ matrix, int2* __restrict__ cstat) {
    constexpr int NT = FBBEV_OCCLV_NT, PER = FBBEV_OCCLV_ROUNDS;
    __shared__ int cnt[FBBEV_OCCLV_MAX_NB];
    __shared__ int tally[2];
    const int nb = 1 << rb, shift = pass * rb, tid = threadIdx.x;
    const unsigned int dmask = (unsigned int)nb - 1u;
    const int cl = (int)blockIdx.x / cps, chunk = (int)blockIdx.x - cl * cps;
    if (!FIRST && fg_count[c0 + cl] == 0) return;
    const int n = FIRST ? nvox : fg_count[C];
    const int base = chunk * FBBEV_OCCLV_TILE;
    if (base >= n) return;                                                 // block-uniform
    for (int d = tid; d < nb; d += NT) cnt[d] = 0;
    if (tid < 2) tally[tid] = 0;
    __syncthreads();
    const long long seg = (long long)cl * nvox;
    unsigned int k[PER];
#pragma unroll
    for (int r = 0; r < PER; ++r) {                                        // all loads first: one memory round trip
        const int idx = base + tid + r * NT;
        if (FIRST) k[r] = idx < n ? keys0[seg + idx] : FBBEV_OCCLV_DROP;
        else k[r] = idx < n ? pairs[seg + idx].x : FBBEV_OCCLV_DROP;
    }
    int valid = 0, fg = 0;
#pragma unroll
    for (int r = 0; r < PER; ++r) {
        if (k[r] == FBBEV_OCCLV_DROP) continue;
        const unsigned int key = FIRST ? FBBEV_OCCLV_ONE - (k[r] & 0x7fffffffu) : k[r];
        atomicAdd(&cnt[(key >> shift) & dmask], 1);
        ++valid;
        fg += (int)(k[r] >> 31);
    }
    if (FIRST) {
        valid = occlv_wave_sum(valid);
        fg = occlv_wave_sum(fg);
        if ((tid & 63) == 0) { atomicAdd(&tally[0], valid); atomicAdd(&tally[1], fg); }
    }
    __syncthreads();
    for (int d = tid; d < nb; d += NT) matrix[((long long)cl * cps + chunk) * nb + d] = cnt[d];
    if (FIRST && tid == 0) cstat[blockIdx.x] = make_int2(tally[0], tally[1]);
}

// a thread per (class, digit): matrix[class][chunk][digit] becomes the count of the digit in the EARLIER chunks of the class,
// tot[class][digit] its count in all of them.  grid = g * nb / 256.  FIRST: the workgroup of a class's digits 0..255 also adds the chunk
// counts of the class: fg_count[c] = G[c], and (class c0 of the group) fg_count[C] = n_valid -- integer sums, any order gives the same.
template <bool FIRST>
__global__ void __launch_bounds__(256)
k_occ_lovasz_colscan(int rb, int cps, int C, int c0, int* __restrict__ fg_count, int* __restrict__ matrix, int* __restrict__ tot,
                     const int2* __restrict__ cstat) {
    __shared__ int tally[2];
    const int nb = 1 << rb, nblk = nb >> 8, tid = threadIdx.x;                // nb is 256 or 1024
    const int cl = (int)blockIdx.x / nblk, part = (int)blockIdx.x - cl * nblk, d = part * 256 + tid;
    int rows = cps;
    if (!FIRST) {
        if (fg_count[c0 + cl] == 0) return;
        rows = (fg_count[C] + FBBEV_OCCLV_TILE - 1) / FBBEV_OCCLV_TILE;
    }
    int* col = matrix + (long long)cl * cps * nb + d;
    int run = 0;
    constexpr int U = 8;                                                   // row loads in flight per thread
    for (int r = 0; r < rows; r += U) {
        int v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) v[u] = r + u < rows ? col[(long long)(r + u) * nb] : 0;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (r + u < rows) col[(long long)(r + u) * nb] = run;
            run += v[u];
        }
    }
    tot[cl * nb + d] = run;
    if (FIRST && part == 0) {
        if (tid < 2) tally[tid] = 0;
        __syncthreads();
        int valid = 0, fg = 0;
        for (int i = tid; i < cps; i += 256) {
            const int2 s = cstat[cl * cps + i];
            valid += s.x;
            fg += s.y;
        }
        valid = occlv_wave_sum(valid);
        fg = occlv_wave_sum(fg);
        if ((tid & 63) == 0) { atomicAdd(&tally[0], valid); atomicAdd(&tally[1], fg); }
        __syncthreads();
        if (tid == 0) {
            fg_count[c0 + cl] = tally[1];
            if (cl == 0) fg_count[C] = tally[0];
        }
    }
}

// one scatter pass of workgroup (class, chunk): FBBEV_OCCLV_TILE pairs ranked stably -- order = (chunk, wave, round, lane) = input order
template <bool FIRST>
__global__ void __launch_bounds__(FBBEV_OCCLV_NT)
k_occ_lovasz_scatter(const unsigned int* __restrict__ keys0, const uint2* __restrict__ pairs_in, int pass, int rb, int nvox, int cps,
                     int C, int c0, const int* __restrict__ fg_count, const int* __restrict__ matrix, const int* __restrict__ tot,
                     uint2* __restrict__ pairs_out) {
    constexpr int WAVES = FBBEV_OCCLV_WAVES, ROUNDS = FBBEV_OCCLV_ROUNDS, NT = FBBEV_OCCLV_NT, NBM = FBBEV_OCCLV_MAX_NB;
    __shared__ int cnt[WAVES][NBM];      // per-wave running digit counters, then (in place) each wave's first position of a digit
    __shared__ int pos0[NBM];            // position of this chunk's first key of a digit inside the class segment
    __shared__ int ldsw[WAVES];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int nb = 1 << rb, shift = pass * rb;
    const unsigned int dmask = (unsigned int)nb - 1u;
    const int cl = (int)blockIdx.x / cps, chunk = (int)blockIdx.x - cl * cps;
    if (fg_count[c0 + cl] == 0) return;                                    // an absent class: nothing to rank
    const int n = FIRST ? nvox : fg_count[C];
    const int chunk0 = chunk * FBBEV_OCCLV_TILE;
    if (chunk0 >= n) return;                                               // block-uniform
    const long long seg = (long long)cl * nvox;
    const int wave0 = chunk0 + wave * (64 * ROUNDS);
    unsigned int k[ROUNDS], v[ROUNDS];
    int lr[ROUNDS];
    const unsigned long long lt = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
#pragma unroll
    for (int r = 0; r < ROUNDS; ++r) {                                     // the wave's pairs first: one memory round trip
        const int idx = wave0 + r * 64 + lane;
        if (FIRST) {
            const unsigned int w = idx < n ? keys0[seg + idx] : FBBEV_OCCLV_DROP;
            k[r] = w == FBBEV_OCCLV_DROP ? FBBEV_OCCLV_DROP : FBBEV_OCCLV_ONE - (w & 0x7fffffffu);
            v[r] = (unsigned int)idx | (w & 0x80000000u);
        } else {
            uint2 kv = make_uint2(FBBEV_OCCLV_DROP, 0u);
            if (idx < n) kv = pairs_in[seg + idx];
            k[r] = kv.x;
            v[r] = kv.y;
        }
    }
    for (int i = tid; i < WAVES * NBM; i += NT) (&cnt[0][0])[i] = 0;
    {   // pos0[d] = keys of smaller digits in the whole class + keys of digit d in the earlier chunks; four digits per thread
        const int* row = matrix + ((long long)cl * cps + chunk) * nb;
        const int* all = tot + cl * nb;
        const int d0 = 4 * tid;
        int a[4], p[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            a[j] = d0 + j < nb ? all[d0 + j] : 0;
            p[j] = d0 + j < nb ? row[d0 + j] : 0;
        }
        int total;
        int run = occlv_block_excl_scan<WAVES>(a[0] + a[1] + a[2] + a[3], ldsw, &total);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (d0 + j < nb) pos0[d0 + j] = run + p[j];
            run += a[j];
        }
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < ROUNDS; ++r) {
        lr[r] = -1;
        if (wave0 + r * 64 >= n) continue;                                 // wave-uniform: nothing of the segment in this round
        const bool valid = k[r] != FBBEV_OCCLV_DROP;
        const unsigned int d = (k[r] >> shift) & dmask;
        unsigned long long mm = __ballot(valid ? 1 : 0);                   // wave-level match on the digit
#pragma unroll
        for (int bit = 0; bit < FBBEV_OCCLV_MAX_RB; ++bit) {
            if (bit < rb) {
                const unsigned long long bb = __ballot((int)((d >> bit) & 1u));
                mm &= ((d >> bit) & 1u) ? bb : ~bb;
            }
        }
        const int leader = valid ? (__ffsll((long long)mm) - 1) : lane;
        int prev = 0;
        if (valid && lane == leader) {
            prev = cnt[wave][d];
            cnt[wave][d] = prev + __popcll(mm);
        }
        prev = __shfl(prev, leader, 64);
        if (valid) lr[r] = prev + __popcll(mm & lt);
    }
    __syncthreads();
    for (int d = tid; d < nb; d += NT) {                                   // in place: count -> first position of the wave's keys of digit d
        int run = pos0[d];
#pragma unroll
        for (int w = 0; w < WAVES; ++w) { const int c = cnt[w][d]; cnt[w][d] = run; run += c; }
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < ROUNDS; ++r) {
        if (lr[r] >= 0) {
            const unsigned int d = (k[r] >> shift) & dmask;
            pairs_out[seg + cnt[wave][d] + lr[r]] = make_uint2(k[r], v[r]);       // < seg + n_valid
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- scan and scatter
// sfg[class][chunk] = fg elements among the chunk's pairs of the sorted order
__global__ void __launch_bounds__(FBBEV_OCCLV_NT)
k_occ_lovasz_fgsum(const uint2* __restrict__ pairs, int nvox, int cps, int C, int c0, const int* __restrict__ fg_count,
                   int* __restrict__ sfg) {
    constexpr int NT = FBBEV_OCCLV_NT, PER = FBBEV_OCCLV_ROUNDS;
    __shared__ int tally;
    const int tid = threadIdx.x;
    const int cl = (int)blockIdx.x / cps, chunk = (int)blockIdx.x - cl * cps;
    if (fg_count[c0 + cl] == 0) return;
    const int n = fg_count[C], base = chunk * FBBEV_OCCLV_TILE;
    if (base >= n) return;
    if (tid == 0) tally = 0;
    __syncthreads();
    const long long seg = (long long)cl * nvox;
    unsigned int v[PER];
#pragma unroll
    for (int r = 0; r < PER; ++r) {
        const int idx = base + tid + r * NT;
        v[r] = idx < n ? pairs[seg + idx].y : 0u;
    }
    int fg = 0;
#pragma unroll
    for (int r = 0; r < PER; ++r) fg += (int)(v[r] >> 31);
    fg = occlv_wave_sum(fg);
    if ((tid & 63) == 0) atomicAdd(&tally, fg);
    __syncthreads();
    if (tid == 0) sfg[blockIdx.x] = tally;
}

// workgroup (class, chunk) of the sorted order; a thread owns FBBEV_OCCLV_ROUNDS consecutive positions.  part[class][chunk] = the chunk's
// sum of e g: products exact in double, a thread's chain in position order, the threads through a fixed tree
__global__ void __launch_bounds__(FBBEV_OCCLV_NT)
k_occ_lovasz_coef(const uint2* __restrict__ pairs, int nvox, int cps, int C, int c0, const int* __restrict__ fg_count,
                  const int* __restrict__ sfg, float* __restrict__ coef, double* __restrict__ part) {
    constexpr int WAVES = FBBEV_OCCLV_WAVES, NT = FBBEV_OCCLV_NT, PER = FBBEV_OCCLV_ROUNDS;
    __shared__ int ldsw[WAVES];
    __shared__ double red[NT];
    const int tid = threadIdx.x;
    const int cl = (int)blockIdx.x / cps, chunk = (int)blockIdx.x - cl * cps;
    const int G = fg_count[c0 + cl];
    if (G == 0) return;
    const int n = fg_count[C], chunk0 = chunk * FBBEV_OCCLV_TILE;
    if (chunk0 >= n) return;
    const long long seg = (long long)cl * nvox;
    const int first = chunk0 + tid * PER;
    uint2 kv[PER];
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        kv[j] = make_uint2(0u, 0u);
        if (first + j < n) kv[j] = pairs[seg + first + j];
    }
    int before = 0;                                                        // fg elements of the earlier chunks
    for (int i = tid; i < chunk; i += NT) before += sfg[cl * cps + i];
    int carry, unused;
    (void)occlv_block_excl_scan<WAVES>(before, ldsw, &carry);
    int local = 0;
#pragma unroll
    for (int j = 0; j < PER; ++j) local += (int)(kv[j].y >> 31);
    int F = carry + occlv_block_excl_scan<WAVES>(local, ldsw, &unused);
    float* plane = coef + (long long)(c0 + cl) * nvox;
    double acc = 0.0;
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        if (first + j < n) {
            const int fg = (int)(kv[j].y >> 31);
            F += fg;
            const int U = G + (first + j + 1) - F;                        // <= n_valid + G < 2^27
            const float g = fg ? (float)(1.0 / (double)U) : (float)((double)(G - F) / ((double)U * (double)(U - 1)));
            const float e = occlv_float(FBBEV_OCCLV_ONE - kv[j].x);
            acc += (double)e * (double)g;
            plane[kv[j].y & 0x7fffffffu] = fg ? -g : g;
        }
    }
    const double sum = occlv_block_sum(acc, red);
    if (tid == 0) part[blockIdx.x] = sum;
}

// workgroup = class: thread t adds the chunk sums t, t + 256, ... in ascending order, the threads meet in a fixed tree; rounded once
__global__ void __launch_bounds__(FBBEV_OCCLV_NT)
k_occ_lovasz_loss(int cps, int C, int c0, const int* __restrict__ fg_count, const double* __restrict__ part, float* __restrict__ loss_c) {
    __shared__ double red[FBBEV_OCCLV_NT];
    const int tid = threadIdx.x, cl = (int)blockIdx.x;
    if (fg_count[c0 + cl] == 0) {                                          // block-uniform; the chunk sums of an absent class do not exist
        if (tid == 0) loss_c[c0 + cl] = 0.f;
        return;
    }
    const int rows = (fg_count[C] + FBBEV_OCCLV_TILE - 1) / FBBEV_OCCLV_TILE;
    double acc = 0.0;
    for (int i = tid; i < rows; i += FBBEV_OCCLV_NT) acc += part[cl * cps + i];
    const double sum = occlv_block_sum(acc, red);
    if (tid == 0) loss_c[c0 + cl] = (float)sum;
}

// ---------------------------------------------------------------------------------------------------------------- backward
// grad x[j] = s p[j] (h[j] - sum_c h[c] p[c]), h = coef (a constant, as the reference's Variable(lovasz_grad(...))), s = *scale;
// 0 where the logit was not finite and for a voxel labelled 255.  Every element of the (B, C, H, W, D) view is written.
template <bool STAGED>
__global__ void __launch_bounds__(FBBEV_OCCL_THREADS)
k_occ_lovasz_grad(const float* __restrict__ logits, long long sb, long long sc, long long sh, long long sw, long long sd,
                  int C, int H, int W, int D, int T, int TD, int nth, int ntw, int ntd, int ntiles, int row_runs,
                  const unsigned char* __restrict__ labels, const float* __restrict__ coef, int nvox, const float* __restrict__ scale,
                  float* __restrict__ grad_logits) {
    float* stage = fbbev_dyn_lds_f32();                                    // 256 rows of C floats: x, then grad x
    float* hs = stage + FBBEV_OCCL_THREADS * C;                            // 256 rows of C floats: the voxel's coefficients
    const int t = threadIdx.x;
    const float s = scale[0];
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        int tile_v = tile;
        fbbev_opaque(tile_v);
        const occl_tile q = occl_tile_of(tile_v, T, TD, nth, ntw, ntd, H, W, D, sb, sh, sw, sd);
        for (int v0 = 0; v0 < q.nvox; v0 += FBBEV_OCCL_THREADS) {
            const int v1 = occl_min(v0 + FBBEV_OCCL_THREADS, q.nvox);
            if (STAGED) {
                occl_copy_runs<true>(const_cast<float*>(logits), stage, q, v0, v1, C, row_runs, sh, sw, t);
                __syncthreads();
            }
            const int v = v0 + t;
            float* row = stage + t * C;
            float* h = hs + t * C;
            if (v < v1) {
                const int th = v / (q.TWe * q.TDe), rr = v - th * (q.TWe * q.TDe);
                const int tw = rr / q.TDe, td = rr - tw * q.TDe;
                const long long at = q.base + (long long)th * sh + (long long)tw * sw + (long long)td * sd;
                const int flat = ((q.b * H + (q.h0 + th)) * W + (q.w0 + tw)) * D + (q.d0 + td);
                const int label = labels[flat];
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
                        h[c] = coef[(long long)c * nvox + flat];
                    }
                    float sum = 0.f;
                    for (int c = 0; c < C; ++c) {
                        const float ex = expf(row[c] - mx);
                        row[c] = ex;
                        sum += ex;
                    }
                    const float inv = 1.f / sum;
                    float dot = 0.f;
                    for (int c = 0; c < C; ++c) {
                        const float p = row[c] * inv;
                        row[c] = p;
                        dot += h[c] * p;
                    }
                    for (int c = 0; c < C; ++c) {
                        float gx = s * (row[c] * (h[c] - dot));
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
